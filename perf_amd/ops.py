"""Tensor-level wrappers over the C ABI (include/perf_hip.h).

Every function takes contiguous CUDA tensors, allocates outputs/workspaces with torch's caching
allocator, and enqueues on torch's current stream.  Nothing here has a CPU fallback: a CPU tensor
or a missing libperf_hip.so raises.
"""
import ctypes
import math
import os
from typing import NamedTuple

import torch

from . import _lib
from ._lib import DTYPE_BF16, DTYPE_FP16
from .grid import GridConfig, MlpConfig

_T16 = {DTYPE_BF16: torch.bfloat16, DTYPE_FP16: torch.float16}
_CODE = {torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_FP16, 'bf16': DTYPE_BF16, 'fp16': DTYPE_FP16,
         DTYPE_BF16: DTYPE_BF16, DTYPE_FP16: DTYPE_FP16}


# ---- optional per-kernel timing with HIP events on the launch stream (used by bench.py) ------------------
_PROF = None


def start_kernel_timing():
    """Record a HIP event pair around every C-ABI launch until stop_kernel_timing()."""
    global _PROF
    _PROF = {}


def stop_kernel_timing():
    """-> {entry point: (n_launches, mean milliseconds)}; synchronises the device."""
    global _PROF
    prof, _PROF = _PROF, None
    torch.cuda.synchronize()
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in (prof or {}).items() if v}


def _call(name, *args, label=None):
    """label: the name the launch is timed under when it differs from the entry point (one entry point, two kinds of launch)."""
    if _PROF is None:
        return _lib.call(name, *args)
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    _lib.call(name, *args)
    b.record()
    _PROF.setdefault(label or name, []).append((a, b))


def dtype_code(d) -> int:
    return _CODE[d]


def torch_dtype(d):
    return _T16[dtype_code(d)]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.PerfError('perf_amd ops need CUDA (HIP) tensors; there is no CPU path')
    if not t.is_contiguous():
        raise _lib.PerfError('perf_amd ops need contiguous tensors')
    return ctypes.c_void_p(t.data_ptr())


def _nd(n_dev):
    """Device-side sample count (int64 tensor with one element, e.g. the `total` of exclusive_scan_i32) or None."""
    if n_dev is None:
        return None
    if n_dev.dtype != torch.int64 or not n_dev.is_cuda:
        raise _lib.PerfError('n_dev must be an int64 CUDA tensor')
    return ctypes.c_void_p(n_dev.data_ptr())


def _f32(t, name):
    if t.dtype != torch.float32:
        raise _lib.PerfError(f'{name} must be float32, got {t.dtype}')
    return t


def _aabb6(aabb):
    vals = [float(v) for v in (aabb.detach().cpu().tolist() if torch.is_tensor(aabb) else aabb)]
    if len(vals) != 6:
        raise _lib.PerfError('aabb must hold 6 values')
    return (ctypes.c_float * 6)(*vals)


# ---- parameters ----------------------------------------------------------------------------------
def cast_params(src: torch.Tensor, dtype, out: torch.Tensor = None) -> torch.Tensor:
    _f32(src, 'params')
    code = dtype_code(dtype)
    if out is None:
        out = torch.empty(src.numel(), dtype=_T16[code], device=src.device)
    _call('perf_cast_params', _p(src), _p(out), src.numel(), code, _stream())
    return out


def adam_step(p, m, v, g, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, w16=None, zero_grad=True):
    code = dtype_code(w16.dtype) if w16 is not None else 0
    _call('perf_adam_step', _p(_f32(p, 'p')), _p(_f32(m, 'm')), _p(_f32(v, 'v')), _p(_f32(g, 'g')), _p(w16),
              p.numel(), code, int(step), float(lr), float(beta1), float(beta2), float(eps), int(bool(zero_grad)),
              _stream())


def adam_step_dev(p, m, v, g, step_dev, lr_dev, beta1=0.9, beta2=0.999, eps=1e-8, w16=None, zero_grad=False, gate=None, clear_flag=None,
                  pair=None, rider=None):
    """gate: device int64 [1]; the update is skipped when it holds 0 (a batch without samples).  clear_flag (device int32 [1]): zeroed by
    the launch, taken or not -- how the overflow flag is consumed when the bookkeeping rode in the repair launch (field_bwd(book=...)).
    pair = (pair table, field, n_net): p is [network (n_net) | table] and the step keeps that field's half of the pair table current too."""
    code = dtype_code(w16.dtype) if w16 is not None else 0
    if rider is not None:
        # rider (rider_write(...)): the launch carries stage C of the step riders -- the next batch's offsets and write pass
        table, field, n_net = pair if pair is not None else (None, 0, 0)
        if w16 is None or (table is not None and (table.dtype != torch.int32 or table.numel() != p.numel() - n_net)):
            raise _lib.PerfError('adam_step_dev: a rider needs w16 (and pair = (int32 [entries, 2] pair table, field, n_net) of (n - n_net) / 2 entries)')
        _call('perf_adam_step_dev_riders', _p(_f32(p, 'p')), _p(_f32(m, 'm')), _p(_f32(v, 'v')), _p(_f32(g, 'g')), _p(w16),
              p.numel(), code, _p(step_dev), _p(lr_dev), _nd(gate), float(beta1), float(beta2), float(eps), int(bool(zero_grad)),
              _p(clear_flag), _p(table), int(field), int(n_net), ctypes.byref(rider), _stream())
        return
    if pair is not None:
        # (perf_adam_step_dev_pair: the same step, which also stores every table entry into its field's half of the pair table)
        table, field, n_net = pair
        if w16 is None or table.dtype != torch.int32 or table.numel() != p.numel() - n_net:
            raise _lib.PerfError('adam_step_dev: pair = (int32 [entries, 2] pair table, field, n_net) needs w16 and a pair table of (n - n_net) / 2 entries')
        _call('perf_adam_step_dev_pair', _p(_f32(p, 'p')), _p(_f32(m, 'm')), _p(_f32(v, 'v')), _p(_f32(g, 'g')), _p(w16),
              p.numel(), code, _p(step_dev), _p(lr_dev), _nd(gate), float(beta1), float(beta2), float(eps), int(bool(zero_grad)),
              _p(clear_flag), _p(table), int(field), int(n_net), _stream())
        return
    _call('perf_adam_step_dev', _p(_f32(p, 'p')), _p(_f32(m, 'm')), _p(_f32(v, 'v')), _p(_f32(g, 'g')), _p(w16),
          p.numel(), code, _p(step_dev), _p(lr_dev), _nd(gate), float(beta1), float(beta2), float(eps), int(bool(zero_grad)),
          _p(clear_flag), _stream())


class StepBook:
    """The arguments of step_bookkeeping, kept for a call that carries the bookkeeping in one of its own launches (field_bwd(book=...):
    perf_field_bwd_book).  done: set by the call that did it -- the optimizer then skips its own bookkeeping launch and lets Adam clear the
    overflow flag."""

    def __init__(self, step_dev=None, gate=None, counters=None, n_marched=None, n_kept=None, capacity=0, overflow=None, remote_flags=None,
                 eff_gate=None, schedule=None, overflow_redone=False):
        self.args = dict(step_dev=step_dev, gate=gate, counters=counters, n_marched=n_marched, n_kept=n_kept, capacity=capacity, overflow=overflow,
                         remote_flags=remote_flags, eff_gate=eff_gate, schedule=schedule, overflow_redone=overflow_redone)
        self.done = False

    def struct(self):
        a = self.args
        table, it, lr_out, ratio_out = a['schedule'] if a['schedule'] is not None else (None, None, None, None)
        for name in ('gate', 'counters', 'n_marched', 'n_kept', 'eff_gate'):
            _nd(a[name])                                   # (dtype / device checks of the int64 scalars)
        q = lambda t: None if t is None else _p(t).value
        return _lib.StepBook(q(a['step_dev']), q(a['gate']), q(a['counters']), q(a['n_marched']), q(a['n_kept']), int(a['capacity'] or 0),
                             q(a['overflow']), q(a['remote_flags']), q(a['eff_gate']), q(table), q(it), q(lr_out), q(ratio_out),
                             int(table.shape[0]) if table is not None else 0, int(bool(a['overflow_redone'])))

    def launch(self):
        """The stand-alone launch (perf_step_bookkeeping) with the same arguments."""
        step_bookkeeping(**self.args)


def step_bookkeeping(step_dev=None, gate=None, counters=None, n_marched=None, n_kept=None, capacity=0, overflow=None,
                     remote_flags=None, eff_gate=None, schedule=None, overflow_redone=False):
    """One launch (perf_step_bookkeeping): decides whether the optimizer step is TAKEN (samples present, no fixed-point
    overflow flag -- local int32 `overflow` or `remote_flags` (float32 [2] = {overflow, truncated} summed over the ranks of a
    data-parallel job, dp_slot_unpack) --, batch not truncated at `capacity`), advances step_dev and writes eff_gate
    (int64 [1]) accordingly, accumulates counters (int64 [8]).
    schedule = (table f32 [n, 2] = rows of (lr, distortion ramp), iter_dev int32 [1], lr_out f32 [1], ratio_out f32 [1] or None):
    the device-side schedule of a graph-replayed phase (see perf_step_bookkeeping).  overflow_redone: the flagged gradient was
    repaired in place (hashgrid_bwd_redo): count the event, take the step."""
    ref = next(t for t in (step_dev, counters, eff_gate) if t is not None)
    if not ref.is_cuda:
        raise _lib.PerfError('perf_amd ops need CUDA (HIP) tensors; there is no CPU path')
    table, it, lr_out, ratio_out = schedule if schedule is not None else (None, None, None, None)
    _call('perf_step_bookkeeping', _p(step_dev), _nd(gate), _nd(counters), _nd(n_marched), _nd(n_kept), int(capacity or 0),
          _p(overflow), _p(remote_flags), int(bool(overflow_redone)), _nd(eff_gate), _p(table), int(table.shape[0]) if table is not None else 0, _p(it),
          _p(lr_out), _p(ratio_out), _stream())


def step_counters(device):
    """Zeroed int64 [8] block of perf_step_bookkeeping: {marched, kept, steps, max marched of one batch, steps skipped for
    fixed-point overflow, steps skipped for truncation, 0, 0}."""
    return torch.zeros(_lib.STEP_COUNTERS, dtype=torch.int64, device=device)


# ---- positions -----------------------------------------------------------------------------------
def points_from_rays(rays_o, rays_d, ray_indices, t_starts, t_ends, aabb, n_dev=None):
    n = ray_indices.numel()
    if ray_indices.dtype != torch.int64:
        raise _lib.PerfError('ray_indices must be int64')
    x01 = torch.empty(n, 3, dtype=torch.float32, device=rays_o.device)
    sel = torch.empty(n, dtype=torch.uint8, device=rays_o.device)
    _call('perf_points_from_rays', _p(_f32(rays_o, 'rays_o')), _p(_f32(rays_d, 'rays_d')), _p(ray_indices),
              _p(_f32(t_starts, 't_starts')), _p(_f32(t_ends, 't_ends')), _aabb6(aabb), _p(x01), _p(sel), n, _nd(n_dev), _stream())
    return x01, sel


def points_normalize(x, aabb):
    x = _f32(x, 'x').reshape(-1, 3)
    n = x.shape[0]
    x01 = torch.empty(n, 3, dtype=torch.float32, device=x.device)
    sel = torch.empty(n, dtype=torch.uint8, device=x.device)
    _call('perf_points_normalize', _p(x), _aabb6(aabb), _p(x01), _p(sel), n, _stream())
    return x01, sel


# ---- hash grid -----------------------------------------------------------------------------------
def hashgrid_fwd(grid: GridConfig, x01, table16, n_dev=None):
    """x01 [n,3] f32, table16 [total*2] 16-bit -> feat [L, n, 2] 16-bit (level major).  n_dev (device int64 [1]): only the
    first min(n, n_dev) samples are encoded (n = capacity = level stride)."""
    n = x01.shape[0]
    feat = torch.empty(grid.n_levels, n, 2, dtype=table16.dtype, device=x01.device)
    d = grid.desc()
    _call('perf_hashgrid_fwd', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(table16), _p(feat), n, _nd(n_dev),
              dtype_code(table16.dtype), _stream())
    return feat


def hashgrid_fwd2(grid: GridConfig, x01, table16_a, table16_b):
    """Both tables (same geometry) at the same points -> (feat_a, feat_b), each [L, n, 2] 16-bit."""
    n = x01.shape[0]
    fa = torch.empty(grid.n_levels, n, 2, dtype=table16_a.dtype, device=x01.device)
    fb = torch.empty(grid.n_levels, n, 2, dtype=table16_a.dtype, device=x01.device)
    d = grid.desc()
    _call('perf_hashgrid_fwd2', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(table16_a), _p(table16_b), _p(fa), _p(fb), n,
          dtype_code(table16_a.dtype), _stream())
    return fa, fb


def pair_table(grid: GridConfig, device):
    """An (uninitialised) pair table of two fields over `grid` (include/perf_hip_pair.h): int32 [total, 2], entry e = {field 0's packed
    2 x 16-bit features, field 1's}."""
    return torch.empty(grid.total, 2, dtype=torch.int32, device=device)


def pair_fill(pair, field, table16, n_entries=None):
    """pair[:n_entries, field] = the first n_entries entries (pairs of 16-bit features) of table16; the other field's half stays."""
    n_entries = table16.numel() // 2 if n_entries is None else int(n_entries)
    if pair.dtype != torch.int32 or pair.numel() < 2 * n_entries or table16.numel() < 2 * n_entries:
        raise _lib.PerfError('pair_fill: pair must be int32 [>= n_entries, 2] and table16 hold 2 * n_entries features')
    dtype_code(table16.dtype)
    _call('perf_pair_fill', _p(pair), int(field), _p(table16), n_entries, _stream())
    return pair


def hashgrid_fwd_pair(grid: GridConfig, x01, pair, dtype, n_dev=None, out=None):
    """Both fields of a pair table at the same points -> (feat_a, feat_b), each [L, n, 2] of `dtype`, bit-identical to hashgrid_fwd on
    that field's own table.  n_dev as in hashgrid_fwd.  out: the two feature arrays to write into (rows beyond the count stay)."""
    n = x01.shape[0]
    code = dtype_code(dtype)
    if pair.dtype != torch.int32 or pair.numel() != 2 * grid.total:
        raise _lib.PerfError('hashgrid_fwd_pair: pair must be the int32 [total, 2] pair table of this grid')
    if out is not None:
        fa, fb = out
        if any(f.dtype != _T16[code] or f.shape != (grid.n_levels, n, 2) for f in out):
            raise _lib.PerfError('hashgrid_fwd_pair: out must be two [L, n, 2] arrays of the table dtype')
    else:
        fa = torch.empty(grid.n_levels, n, 2, dtype=_T16[code], device=x01.device)
        fb = torch.empty(grid.n_levels, n, 2, dtype=_T16[code], device=x01.device)
    d = grid.desc()
    _call('perf_hashgrid_fwd_pair', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(pair), _p(fa), _p(fb), n, _nd(n_dev), code, _stream())
    return fa, fb


def hashgrid_fwd_f32(grid: GridConfig, x01, table):
    n = x01.shape[0]
    feat = torch.empty(grid.n_levels, n, 2, dtype=torch.float32, device=x01.device)
    d = grid.desc()
    _call('perf_hashgrid_fwd_f32', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(_f32(table, 'table')), _p(feat), n, _stream())
    return feat


_OVERFLOW_FLAG = {}


def overflow_flag(device):
    """Device int32 that the fixed-point grid backward ORs with 1 when a field nears the int32 range."""
    key = str(device)
    if key not in _OVERFLOW_FLAG:
        _OVERFLOW_FLAG[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _OVERFLOW_FLAG[key]


def headroom_state(device):
    """Zeroed state block of the fixed-point headroom feedback (one per table that is trained, see perf_hashgrid_bwd)."""
    return torch.zeros(_lib.HEADROOM_STATE_WORDS, dtype=torch.int32, device=device)


def hashgrid_bwd(grid: GridConfig, x01, dfeat, out=None, accumulate=False, level_absmax=None, n_dev=None, use_codes=True,
                 hr_state=None, shifts=None, raw_fields=False):
    """dfeat [L, n, 2] f32 -> gradient table [total*2] f32.  `out` (a contiguous fp32 view, e.g. the grid
    part of a flat gradient) is overwritten, or added to when accumulate=True.  level_absmax (device, 16 floats
    from mlp_bwd) selects the packed fixed-point accumulation.  shifts (device int32 [24]): job-wide units of a
    data-parallel step (dp_units) instead of level_absmax / hr_state; raw_fields: `out` receives the int32 field pairs
    (same storage; view it as int32) for an integer reduce-scatter followed by fixed_unfix."""
    n = x01.shape[0]
    if out is None:
        out = torch.empty(grid.n_params, dtype=torch.float32, device=x01.device)
        accumulate = False
    d = grid.desc()
    fixed = level_absmax is not None or shifts is not None
    # (a workspace without room for the tile codes selects the position-streaming owners: use_codes=False, tests)
    ws_bytes = _lib.load().perf_hashgrid_bwd_workspace_bytes(ctypes.byref(d), n if use_codes else 0)
    ws = torch.empty(ws_bytes // 4 + 4, dtype=torch.float32, device=x01.device)
    flag = overflow_flag(x01.device) if fixed else None
    _call('perf_hashgrid_bwd', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(_f32(dfeat, 'dfeat')), _p(_f32(out, 'grad')),
              n, _nd(n_dev), int(bool(accumulate)), _p(level_absmax), _p(flag),
              _p(hr_state if (level_absmax is not None and shifts is None) else None), _p(shifts), int(bool(raw_fields)),
              None, _p(ws), ws_bytes, _stream())
    return out


def hashgrid_bwd_lines(grid: GridConfig, x01, dfeat, out=None, accumulate=False, level_absmax=None, n_dev=None, hr_state=None,
                       use_owners=True, use_codes=True):
    """hashgrid_bwd for the line-local table layouts ('line_local' / 'line_overlap'; perf_hashgrid_bwd_lines): dfeat [L, n, 2] f32 ->
    gradient table [total*2] f32, overwritten or added to (accumulate=True).  level_absmax selects the fixed-point accumulation, hr_state
    its headroom feedback.  'line_overlap': both storage copies of a shared vertex receive the vertex's gradient.  use_owners=False
    (tests): a workspace without room for the LDS owners selects the global-atomics scatter for every line-local level; use_codes=False:
    one without room for the tile codes, the position-streaming owners."""
    if grid.layout == 'tcnn':
        raise ValueError('hashgrid_bwd_lines takes line-local layouts; a tcnn-layout grid goes through hashgrid_bwd')
    n = x01.shape[0]
    if out is None:
        out = torch.empty(grid.n_params, dtype=torch.float32, device=x01.device)
        accumulate = False
    d = grid.desc()
    lib = _lib.load()
    ws_bytes = lib.perf_hashgrid_bwd_lines_workspace_bytes(ctypes.byref(d), n if use_codes else 0)
    if ws_bytes < 0:
        _lib.check(-1, 'perf_hashgrid_bwd_lines_workspace_bytes')
    if not use_owners:
        # the tcnn-rule levels' own minimum only: no room for the line-local owners
        pre = _lib.GridDesc.from_buffer_copy(d)
        pre.n_levels = int(grid.local.argmax()) if grid.local.any() else grid.n_levels
        pre.layout = _lib.LAYOUT_TCNN
        ws_bytes = lib.perf_hashgrid_bwd_workspace_bytes(ctypes.byref(pre), 0) if pre.n_levels > 0 else 0
    ws = torch.empty(ws_bytes // 4 + 4, dtype=torch.float32, device=x01.device)
    fixed = level_absmax is not None
    flag = overflow_flag(x01.device) if fixed else None
    _call('perf_hashgrid_bwd_lines', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(_f32(dfeat, 'dfeat')), _p(_f32(out, 'grad')),
          n, _nd(n_dev), int(bool(accumulate)), _p(level_absmax), _p(flag), _p(hr_state if fixed else None), None, 0,
          None, _p(ws), ws_bytes, _stream())
    return out


def hashgrid_bwd_redo_supported(grid: GridConfig) -> bool:
    """Grids whose levels all fit LDS owners (<= 255 hashed / 64 dense tiles of 16,384 entries; line-local levels: <= 255 tiles):
    PeRF's L16/T18 does."""
    for l in range(grid.n_levels):
        tiles = -(-int(grid.size[l]) // 16384)
        if tiles > (255 if grid.hashed[l] or grid.local[l] else 64):
            return False
    return True


def hashgrid_bwd_redo(grid: GridConfig, x01, dfeat, out, n_dev=None, hr_state=None):
    """The repair launch of a fixed-point hashgrid_bwd into the same `out`: a no-op dispatch unless that call raised the
    overflow flag, else the table gradient again with fp32 LDS accumulation (perf_hashgrid_bwd / perf_hashgrid_bwd_lines, redo_flag)."""
    d = grid.desc()
    _call('perf_hashgrid_bwd' if grid.layout == 'tcnn' else 'perf_hashgrid_bwd_lines', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(_f32(dfeat, 'dfeat')), _p(_f32(out, 'grad')),
          x01.shape[0], _nd(n_dev), 0, None, None, _p(hr_state), None, 0, _p(overflow_flag(x01.device)), None, 0, _stream(),
          label='perf_hashgrid_bwd(redo: predicated no-op)')
    return out


FIELD_BWD_ONE_CALL = True       # False: the three entry points one by one (tools/shim_step_profile.py --three-calls: the A/B of the host cost)


class Workspace:
    """Grow-only holder of ONE float32 scratch block; its owner (a network: NetworkWithInputEncoding) takes the block with it."""

    def __init__(self):
        self.block = None

    def get(self, nbytes, device):
        """A block of at least nbytes.  Grown geometrically: the operator-shim path calls with a different exact n every step -- a
        buffer per size would pin a pool of differently sized blocks and push the caching allocator into hipMalloc (measured: +0.3 ms
        per step); any buffer that is large enough serves (the library lays it out from n)."""
        ws = self.block
        if ws is None or ws.numel() * 4 < nbytes or ws.device != device:
            grown = max(nbytes, int(1.5 * ws.numel() * 4) if ws is not None else 0)
            ws = torch.empty(grown // 4 + 4, dtype=torch.float32, device=device)
            if not (ws.is_cuda and torch.cuda.is_current_stream_capturing()):   # (a block first made INSIDE a capture belongs to that graph's pool: not kept)
                self.block = ws
        return ws


def field_bwd(grid: GridConfig, mlp: MlpConfig, x01, w16_net, feat16, dout, sel=None, fixed=True, redo=True, hr_state=None, n_dev=None,
              grad=None, extra=0, book=None, ws=None, riders=None):
    """The whole backward of one field in ONE boundary call (perf_field_bwd: MLP backward -> grid backward -> predicated fp32 repair)
    -> flat fp32 gradient [network | grid (+ `extra` trailing slots)].  feat16: [L, n, 2] or an IndexedFeat.  ws (a Workspace): the
    holder of the call's scratch memory (MLP partials, tile codes, dfeat), grown on demand: consecutive backwards on one stream reuse
    it -- do not overlap two backwards with one holder on different streams.  ws=None: a block of this call's own.
    riders = (rider_draw(...) or None, rider_count(...) or None): stages A and B of the step riders in the grid backward's launches
    (perf_field_bwd_riders); needs the one-call path -- a per-launch timing pass cannot carry them."""
    index, stride = None, 0
    if isinstance(feat16, IndexedFeat):
        feat16, index = feat16.feat, feat16.index
        stride = feat16.shape[1]
    n = index.shape[0] if index is not None else feat16.shape[1]
    dev = x01.device
    n_all = mlp.n_params + grid.n_params
    if grad is None:
        grad = torch.empty(n_all + extra, dtype=torch.float32, device=dev)
    if riders is not None and (_PROF is not None or not FIELD_BWD_ONE_CALL):
        raise _lib.PerfError('field_bwd: riders need the one-call backward (no per-launch timing pass)')
    if _PROF is not None or not FIELD_BWD_ONE_CALL:
        # per-launch timing (start_kernel_timing: bench.py's `kernels` / `roofline` blocks): the same three entry points one by one,
        # so that each is bracketed by its own pair of events
        res = mlp_bwd(mlp, w16_net, IndexedFeat(feat16, index) if index is not None else feat16, dout, sel, want_absmax=fixed, n_dev=n_dev,
                      dw_out=grad[:mlp.n_params])
        hashgrid_bwd_into(grid, x01, res[0], grad[mlp.n_params:n_all], level_absmax=res[2] if fixed else None, n_dev=n_dev,
                          hr_state=hr_state if fixed else None)
        if fixed and redo:
            hashgrid_bwd_redo(grid, x01, res[0], grad[mlp.n_params:n_all], n_dev=n_dev, hr_state=hr_state)
        return grad
    gd, md = grid.desc(), mlp.desc()
    nbytes = _lib.load().perf_field_bwd_workspace_bytes(ctypes.byref(gd), ctypes.byref(md), n, None, None, None)
    if nbytes < 0:
        raise _lib.PerfError('perf_field_bwd_workspace_bytes: bad arguments')
    ws = (ws or Workspace()).get(nbytes, dev)
    with_book = (book is not None and fixed and redo and hr_state is not None and n > 0 and book.args['overflow'] is not None
                 and book.args['overflow'].data_ptr() == overflow_flag(dev).data_ptr())
    # book (a StepBook): the step's bookkeeping rides in the repair launch (perf_field_bwd_book) -- one launch per step fewer; the flag
    # stays for adam_step_dev(clear_flag=...)
    sb = book.struct() if with_book else None
    head = (ctypes.byref(gd), ctypes.byref(md), _p(_f32(x01, 'x01')), _p(w16_net), _p(feat16), _p(index), stride, _p(sel), _p(_f32(dout, 'dout')), _p(grad))
    flags = (int(bool(fixed)), int(bool(fixed and redo)))
    state = (_p(overflow_flag(dev)) if fixed else None, _p(hr_state) if fixed else None)
    tail = (_p(ws), ws.numel() * 4, n, _nd(n_dev), dtype_code(w16_net.dtype))
    if riders is not None:
        draw, count = riders
        _call('perf_field_bwd_riders', *head, *flags, *state, *tail, ctypes.byref(sb) if with_book else None,
              ctypes.byref(draw) if draw is not None else None, ctypes.byref(count) if count is not None else None, _stream())
    elif with_book:
        _call('perf_field_bwd_book', *head, *state, *tail, ctypes.byref(sb), _stream())
    else:
        _call('perf_field_bwd', *head, *flags, *state, *tail, _stream())
    if with_book:
        book.done = True
    return grad


def hashgrid_bwd_into(grid, x01, dfeat, out, level_absmax=None, n_dev=None, hr_state=None, shifts=None, raw_fields=False):
    if grid.layout != 'tcnn':
        if shifts is not None or raw_fields:
            raise ValueError(f'{grid.layout}: given units / raw fields (the data-parallel integer exchange) need the tcnn table layout')
        return hashgrid_bwd_lines(grid, x01, dfeat, out=out, accumulate=False, level_absmax=level_absmax, n_dev=n_dev, hr_state=hr_state)
    return hashgrid_bwd(grid, x01, dfeat, out=out, accumulate=False, level_absmax=level_absmax, n_dev=n_dev, hr_state=hr_state,
                        shifts=shifts, raw_fields=raw_fields)


# ---- job-wide fixed-point units of a data-parallel step -------------------------------------------------------------------
def dp_stats_pack(level_absmax, field_max_prev, n_dev, n, out=None):
    """-> int32 [PERF_DP_STATS]: this rank's block of the statistics every rank all-gathers before its grid backward."""
    if out is None:
        out = torch.empty(_lib.DP_STATS, dtype=torch.int32, device=level_absmax.device)
    _call('perf_dp_stats_pack', _p(level_absmax), _p(field_max_prev), _nd(n_dev), int(n), _p(out), _stream())
    return out


def dp_units(grid: GridConfig, stats_all, world, hr_state, shifts=None, n_total=None, margin_bits=0, want_total=True):
    """stats_all int32 [world, PERF_DP_STATS] -> (shifts int32 [24], n_total int64 [1]); applies the headroom feedback to hr_state.
    margin_bits: make the units that many bits coarser (lagged units of perf_amd/dp.py)."""
    dev = stats_all.device
    if shifts is None:
        shifts = torch.empty(_lib.MAX_LEVELS, dtype=torch.int32, device=dev)
    if n_total is None and want_total:
        n_total = torch.empty(1, dtype=torch.int64, device=dev)
    d = grid.desc()
    _call('perf_dp_units', ctypes.byref(d), _p(stats_all), int(world), _p(hr_state), _p(shifts), _nd(n_total), int(margin_bits), _stream())
    return shifts, n_total


def dp_slot_pack(level_absmax, field_max, n_dev, n, overflow, n_marched, capacity, rank, world, out):
    """This rank's slot of the small all-reduce (perf_dp_slot_pack); `out`: float32 [world * PERF_DP_SLOT], the other slots are zeroed."""
    _call('perf_dp_slot_pack', _p(level_absmax), _p(field_max), _nd(n_dev), int(n), _p(overflow), _nd(n_marched), int(capacity or 0),
          int(rank), int(world), _p(_f32(out, 'slots')), _stream())
    return out


def dp_slot_unpack(slots, world, stats_all=None, job_flags=None, n_total=None):
    """All-reduced slots -> stats_all (int32 [world, PERF_DP_STATS], optional), job_flags (float32 [2] = {overflow, truncated}
    summed over the ranks), n_total (int64 [1])."""
    _call('perf_dp_slot_unpack', _p(_f32(slots, 'slots')), int(world), _p(stats_all), _p(job_flags), _nd(n_total), _stream())
    return job_flags, n_total


def fixed_unfix(grid: GridConfig, fields, entry_lo, entry_hi, shifts, field_max=None, flag=None):
    """In place: int32 field pairs of table entries [entry_lo, entry_hi) (`fields`: a contiguous 4-byte tensor holding them)
    -> fp32 gradients; field_max int32 [24] receives the slice's largest |field| per level."""
    d = grid.desc()
    _call('perf_fixed_unfix', ctypes.byref(d), _p(fields), int(entry_lo), int(entry_hi), _p(shifts), _p(field_max), _p(flag), _stream())
    return fields


def hashgrid_corners(grid: GridConfig, x01):
    """-> int32 [L, n, 8] absolute table entries of the 8 corners (bit0 = x, bit1 = y, bit2 = z)."""
    n = x01.shape[0]
    idx = torch.empty(grid.n_levels, n, 8, dtype=torch.int32, device=x01.device)
    d = grid.desc()
    _call('perf_hashgrid_corners', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(idx), n, _stream())
    return idx


def hashgrid_bwd_input(grid: GridConfig, x01, dfeat, table):
    n = x01.shape[0]
    dx = torch.empty(n, 3, dtype=torch.float32, device=x01.device)
    d = grid.desc()
    _call('perf_hashgrid_bwd_input', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(_f32(dfeat, 'dfeat')),
              _p(_f32(table, 'table')), _p(dx), n, _stream())
    return dx


def hashgrid_bwd_bwd_input(grid: GridConfig, x01, dfeat, table, ggx, want_ddfeat=True, want_dx=True):
    """Backward of hashgrid_bwd_input w.r.t. (dfeat, x01) given ggx = dL/d(dx) [n,3] -> (d_dfeat [L,n,2] | None, d_x [n,3] | None)."""
    n = x01.shape[0]
    dd = torch.empty(grid.n_levels, n, 2, dtype=torch.float32, device=x01.device) if want_ddfeat else None
    dx = torch.empty(n, 3, dtype=torch.float32, device=x01.device) if want_dx else None
    d = grid.desc()
    _call('perf_hashgrid_bwd_bwd_input', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(_f32(dfeat, 'dfeat')), _p(_f32(table, 'table')),
          _p(_f32(ggx, 'ggx')), _p(dd), _p(dx), n, _stream())
    return dd, dx


def hashgrid_bwd_bwd_param(grid: GridConfig, x01, dfeat, ggx):
    """Backward of hashgrid_bwd_input w.r.t. the table given ggx -> grad_table [total*2] f32."""
    n = x01.shape[0]
    out = torch.empty(grid.n_params, dtype=torch.float32, device=x01.device)
    d = grid.desc()
    _call('perf_hashgrid_bwd_bwd_param', ctypes.byref(d), _p(_f32(x01, 'x01')), _p(_f32(dfeat, 'dfeat')), _p(_f32(ggx, 'ggx')), _p(out), n,
          _stream())
    return out


# ---- MLP -----------------------------------------------------------------------------------------
def mlp_fwd(mlp: MlpConfig, w16, feat16, sel=None, n_dev=None):
    """feat16: [L, n, 2], or an IndexedFeat (n = its index's length): the rows are read in place, no compacted copy is made
    (perf_mlp_fwd_rows; bit-identical to the forward on the materialised rows)."""
    if isinstance(feat16, IndexedFeat):
        feat, index = feat16.feat, feat16.index
        assert index.dtype == torch.int32 and index.is_contiguous() and feat.is_contiguous()
        n = index.shape[0]
        out = torch.empty(n, mlp.n_output_dims, dtype=torch.float32, device=feat.device)
        d = mlp.desc()
        _call('perf_mlp_fwd_rows', ctypes.byref(d), _p(w16), _p(feat), _p(index), feat.shape[1], _p(sel), _p(out), n, _nd(n_dev),
              dtype_code(w16.dtype), _stream())
        return out
    n = feat16.shape[1]
    out = torch.empty(n, mlp.n_output_dims, dtype=torch.float32, device=feat16.device)
    d = mlp.desc()
    _call('perf_mlp_fwd', ctypes.byref(d), _p(w16), _p(feat16), _p(sel), _p(out), n, _nd(n_dev), dtype_code(w16.dtype), _stream())
    return out


import os as _os
# perf_field_infer runs encode + MLP as one kernel up to this many rows (16-level grids); the library reads the same switch
FUSED_MAX_SAMPLES = int(_os.environ.get('PERF_FUSED_MAX_SAMPLES', '4096'))


def field_infer(grid: GridConfig, mlp: MlpConfig, x01, sel, w16, n_dev=None, want_features=False):
    """act(MLP(encode(x01))) * sel without gradient in one boundary call; w16 = the network's 16-bit working copy
    [MLP weights | table].  want_features: also return the level-major 16-bit features [L, n, 2] the result was computed from
    (-> (out, feat))."""
    n = x01.shape[0]
    n_net = mlp.n_params
    out = torch.empty(n, mlp.n_output_dims, dtype=torch.float32, device=x01.device)
    feat = torch.empty(grid.n_levels, n, 2, dtype=w16.dtype, device=x01.device) if want_features else None
    fused = n <= FUSED_MAX_SAMPLES and grid.n_levels <= 16 and grid.layout == 'tcnn'      # (perf_field_infer's own choice)
    if _PROF is not None and not fused:
        # per-kernel timing (bench.py): the same two kernels the boundary call launches, issued one by one so that each gets
        # its own event pair
        feat = hashgrid_fwd(grid, x01, w16[n_net:], n_dev=n_dev)
        out = mlp_fwd(mlp, w16[:n_net], feat, sel, n_dev=n_dev)
        return (out, feat) if want_features else out
    scratch = None if (fused or want_features) else torch.empty(grid.n_levels * n, dtype=torch.int32, device=x01.device)
    gd, md = grid.desc(), mlp.desc()
    _call('perf_field_infer', ctypes.byref(gd), ctypes.byref(md), _p(_f32(x01, 'x01')), _p(sel), _p(w16[n_net:]), _p(w16[:n_net]),
          _p(out), n, _nd(n_dev), _p(scratch), scratch.numel() * 4 if scratch is not None else 0, _p(feat), dtype_code(w16.dtype), _stream())
    return (out, feat) if want_features else out


def field_grad_x(grid: GridConfig, mlp: MlpConfig, x01, sel, w16, inv_extent=None, n_dev=None, want_sigma=True, out=None):
    """Density and its spatial gradient in one kernel (perf_field_grad_x): -> (sigma [n] or None, grad [n,3]) with
    grad = d(act(MLP(encode(x01)))[0] * sel) / dx in world units, inv_extent = the three factors 1 / (aabb_max - aabb_min) (None: 1,
    the gradient w.r.t. x01).  w16 = the 16-bit working copy [MLP weights | table] (what field_infer takes); no gradient is recorded.
    n_dev: rows at and beyond the device count are left untouched; out = (sigma, grad) buffers to write into."""
    n = x01.shape[0]
    n_net = mlp.n_params
    if out is not None:
        sigma, grad = out
    else:
        grad = torch.empty(n, 3, dtype=torch.float32, device=x01.device)
        sigma = torch.empty(n, dtype=torch.float32, device=x01.device) if want_sigma else None
    ie = None if inv_extent is None else (ctypes.c_float * 3)(*[float(v) for v in inv_extent])
    gd, md = grid.desc(), mlp.desc()
    _call('perf_field_grad_x', ctypes.byref(gd), ctypes.byref(md), _p(_f32(x01, 'x01')), _p(sel), _p(w16[n_net:]), _p(w16[:n_net]), ie,
          _p(grad), _p(sigma), n, _nd(n_dev), dtype_code(w16.dtype), _stream())
    return sigma, grad


def field_grad_x_bwd(grid: GridConfig, mlp: MlpConfig, x01, sel, w16, inv_extent=None, dsigma=None, dgrad=None, n_dev=None, grad=None,
                     ws=None):
    """Backward of field_grad_x with respect to the field's parameters (perf_field_grad_x_bwd, include/perf_hip_ext.h): given the
    upstream gradients dsigma [n] and dgrad [n,3] (either may be None, not both) -> flat fp32 gradient [network | grid] of
    sum(dsigma * sigma) + sum(dgrad * grad_x), OVERWRITTEN in full (all zeros for an empty or dead batch).  One kernel on the 16-bit
    working copy w16; the network part is deterministic, the table part is scattered with fp32 atomics (order-dependent in its last
    bits).  ws (a Workspace): the holder of the call's scratch memory -- a network's bwd_workspace, as for field_bwd."""
    n = x01.shape[0]
    n_net = mlp.n_params
    dev = x01.device
    if grad is None:
        grad = torch.empty(n_net + grid.n_params, dtype=torch.float32, device=dev)
    ie = None if inv_extent is None else (ctypes.c_float * 3)(*[float(v) for v in inv_extent])
    gd, md = grid.desc(), mlp.desc()
    nbytes = _lib.load().perf_field_grad_x_bwd_workspace_bytes(ctypes.byref(gd), ctypes.byref(md), n)
    if nbytes < 0:
        _lib.check(-1, 'perf_field_grad_x_bwd_workspace_bytes')
    block = (ws or Workspace()).get(nbytes, dev)
    _call('perf_field_grad_x_bwd', ctypes.byref(gd), ctypes.byref(md), _p(_f32(x01, 'x01')), _p(sel), _p(w16[n_net:]), _p(w16[:n_net]), ie,
          _p(None if dsigma is None else _f32(dsigma, 'dsigma')), _p(None if dgrad is None else _f32(dgrad, 'dgrad')), _p(grad), _p(block),
          block.numel() * 4, n, _nd(n_dev), dtype_code(w16.dtype), _stream())
    return grad


def sphere_net_params(n_levels: int) -> int:
    """Length of the flat fp32 network buffer of the sphere distance field (include/perf_hip_sphere.h: [W1 | b1 | W2 | b2 | w3 | b3])."""
    return 64 * (3 + 2 * n_levels) + 64 + 64 * 64 + 64 + 64 + 1


def sphere_field_fwd(grid: GridConfig, table, net, dirs, want_grad=True):
    """The sphere distance field in one kernel (perf_sphere_field_fwd, include/perf_hip_sphere.h): -> (raw [n], g [n,3] or None) with
    raw = -(MLP([u; enc(0.49 u + 0.49)])) and g = d raw / du, all fp32.  table: the fp32 grid table, net: the flat fp32 network buffer
    (sphere_net_params values), dirs: [n,3].  want_grad=False forms no gradient (the raw values are bit-identical).  No graph is
    recorded."""
    n = dirs.shape[0]
    if net.numel() != sphere_net_params(grid.n_levels) or table.numel() != grid.n_params:
        raise _lib.PerfError(f'sphere_field_fwd: net has {net.numel()} values, table {table.numel()}; the grid asks for '
                             f'{sphere_net_params(grid.n_levels)} and {grid.n_params}')
    raw = torch.empty(n, dtype=torch.float32, device=dirs.device)
    g = torch.empty(n, 3, dtype=torch.float32, device=dirs.device) if want_grad else None
    gd = grid.desc()
    _call('perf_sphere_field_fwd', ctypes.byref(gd), _p(_f32(table, 'table')), _p(_f32(net, 'net')), _p(_f32(dirs, 'dirs')), _p(raw), _p(g), n,
          _stream())
    return raw, g


def sphere_field_bwd(grid: GridConfig, table, net, dirs, draw=None, dgrad=None, grad=None, ws=None):
    """Backward of sphere_field_fwd with respect to the parameters (perf_sphere_field_bwd): given draw = dL/d raw [n] and dgrad = dL/dg
    [n,3] (either may be None, not both) -> flat fp32 gradient [network | table], OVERWRITTEN in full (zeros for an empty batch).  One
    kernel; the network part is deterministic, the table part is scattered with fp32 atomics (order-dependent in its last bits).
    ws (a Workspace): the holder of the call's scratch memory -- its owner is the field (SphereDistanceField.bwd_workspace)."""
    n = dirs.shape[0]
    n_net = sphere_net_params(grid.n_levels)
    dev = dirs.device
    if net.numel() != n_net or table.numel() != grid.n_params:
        raise _lib.PerfError(f'sphere_field_bwd: net has {net.numel()} values, table {table.numel()}; the grid asks for {n_net} and {grid.n_params}')
    if grad is None:
        grad = torch.empty(n_net + grid.n_params, dtype=torch.float32, device=dev)
    gd = grid.desc()
    nbytes = _lib.load().perf_sphere_field_bwd_workspace_bytes(ctypes.byref(gd), n)
    if nbytes < 0:
        _lib.check(-1, 'perf_sphere_field_bwd_workspace_bytes')
    block = (ws or Workspace()).get(nbytes, dev)
    _call('perf_sphere_field_bwd', ctypes.byref(gd), _p(_f32(table, 'table')), _p(_f32(net, 'net')), _p(_f32(dirs, 'dirs')),
          _p(None if draw is None else _f32(draw, 'draw')), _p(None if dgrad is None else _f32(dgrad, 'dgrad')), _p(grad), _p(block),
          block.numel() * 4, n, _stream())
    return grad


# ---- the joint predictor's alignment step (include/perf_hip_joint.h) -------------------------------------------------------------------
def _joint_dims(who, P, R, bias_d, bias_n, coords):
    if bias_d.shape != (P, 1, R, R) or bias_n.dim() != 4 or bias_n.shape[:2] != (P, 3) or bias_n.shape[2] != bias_n.shape[3]:
        raise _lib.PerfError(f'{who}: bias_d must be [{P}, 1, {R}, {R}] and bias_n [{P}, 3, Rn, Rn], got {tuple(bias_d.shape)} and {tuple(bias_n.shape)}')
    if coords.shape[0] != P or coords.shape[-1] != 2 or coords.numel() != P * coords.shape[1] * 2:
        raise _lib.PerfError(f'{who}: coords must be [{P}, B, 2] (or [{P}, B, 1, 2]), got {tuple(coords.shape)}')
    return coords.shape[1], bias_n.shape[2]


def joint_sample(sup, bias_d, bias_n, ref, coords, u=None):
    """The sampling of one alignment step in one kernel (perf_joint_sample): sup [P,7,R,R], bias_d [P,1,R,R], bias_n [P,3,Rn,Rn],
    ref [2,H,W] (panorama distance, mask), coords [P,B,2] or [P,B,1,2] in [-1,1] -> (u [P*B,3], rec [P*B, JOINT_RECORD]) with
    rec = [sd | db | sn (3) | nb (3) | pr | pm | 0 | 0].  u: None (the kernel forms the directions) or fp32 [P*B,3], the directions the
    caller formed from the same maps and coordinates: taken as they are and returned.  No graph is recorded."""
    if sup.dim() != 4 or sup.shape[1] != 7 or sup.shape[2] != sup.shape[3] or ref.dim() != 3 or ref.shape[0] != 2:
        raise _lib.PerfError(f'joint_sample: sup must be [P, 7, R, R] and ref [2, H, W], got {tuple(sup.shape)} and {tuple(ref.shape)}')
    P, R = sup.shape[0], sup.shape[2]
    B, Rn = _joint_dims('joint_sample', P, R, bias_d, bias_n, coords)
    if u is not None and u.shape != (P * B, 3):
        raise _lib.PerfError(f'joint_sample: u must be [{P * B}, 3], got {tuple(u.shape)}')
    given = u
    if u is None:
        u = torch.empty(P * B, 3, dtype=torch.float32, device=sup.device)
    rec = torch.empty(P * B, _lib.JOINT_RECORD, dtype=torch.float32, device=sup.device)
    _call('perf_joint_sample', _p(_f32(sup, 'sup')), _p(_f32(bias_d, 'bias_d')), _p(_f32(bias_n, 'bias_n')), _p(_f32(ref, 'ref')),
          _p(_f32(coords, 'coords')), _p(None if given is None else _f32(given, 'u')), P, B, R, Rn, ref.shape[1], ref.shape[2], _p(u), _p(rec),
          _stream())
    return u, rec


def joint_loss(rec, coords, scale, u, d, g, o, R, Rn, w_ref, w_reg, w_n, w_ntv=0.0, tv=None, gbias_d=None, gbias_n=None, ws=None):
    """The losses of one alignment step and the gradients the head owns (perf_joint_loss) -> (losses [JOINT_LOSSES] = [L_d, L_n, L_reg,
    L_ref, TV_d, TV_n, total, 0], dd [N] = d total/d d, dg [N,3] = d total/d g, dscale [P]); deterministic.  tv: two device floats
    (TV_d, TV_n) or None.  gbias_d [P,1,R,R], gbias_n [P,3,Rn,Rn] (both or neither): d total/d db and d total/d nb are scattered ON
    TOP of their contents with fp32 atomics (order-dependent in the last bits); None: the maps get nothing.  ws: a Workspace."""
    P = scale.numel()
    N = rec.shape[0]
    if P < 1 or N % P or coords.numel() != 2 * N or u.shape != (N, 3) or g.shape != (N, 3) or o.numel() != 3 * N or d.numel() != N:
        raise _lib.PerfError(f'joint_loss: {N} records do not go with scale {tuple(scale.shape)}, coords {tuple(coords.shape)}, u {tuple(u.shape)}, '
                             f'd {tuple(d.shape)}, g {tuple(g.shape)}, o {tuple(o.shape)}')
    if (gbias_d is None) != (gbias_n is None) or (gbias_d is not None and (gbias_d.shape != (P, 1, R, R) or gbias_n.shape != (P, 3, Rn, Rn))):
        raise _lib.PerfError('joint_loss: gbias_d [P,1,R,R] and gbias_n [P,3,Rn,Rn] come together, in these shapes')
    if tv is not None and tv.numel() != 2:
        raise _lib.PerfError('joint_loss: tv holds two values (TV_d, TV_n)')
    B = N // P
    dev = rec.device
    losses = torch.empty(_lib.JOINT_LOSSES, dtype=torch.float32, device=dev)
    dd = torch.empty(N, dtype=torch.float32, device=dev)
    dg = torch.empty(N, 3, dtype=torch.float32, device=dev)
    dscale = torch.empty(P, dtype=torch.float32, device=dev)
    nbytes = _lib.load().perf_joint_loss_workspace_bytes(P, B)
    if nbytes < 0:
        _lib.check(-1, 'perf_joint_loss_workspace_bytes')
    block = (ws or Workspace()).get(nbytes, dev)
    _call('perf_joint_loss', _p(_f32(rec, 'rec')), _p(_f32(coords, 'coords')), _p(_f32(scale, 'scale')), _p(_f32(u, 'u')), _p(_f32(d, 'd')),
          _p(_f32(g, 'g')), _p(_f32(o, 'o')), P, B, int(R), int(Rn), float(w_ref), float(w_reg), float(w_n), float(w_ntv),
          _p(None if tv is None else _f32(tv, 'tv')), _p(losses), _p(dd), _p(dg), _p(dscale),
          _p(None if gbias_d is None else _f32(gbias_d, 'gbias_d')), _p(None if gbias_n is None else _f32(gbias_n, 'gbias_n')), _p(block),
          block.numel() * 4, _stream())
    return losses, dd, dg, dscale


def joint_tv(m, weight=1.0, grad=None, value=None, ws=None):
    """Total variation of a map [n,C,H,W] with smooth-L1(beta=0.01) (perf_joint_tv) -> (value [1], the unweighted TV; grad [n,C,H,W] =
    weight * dTV/dm, WRITTEN in full, gather form: deterministic).  grad / value: buffers to write into (value: one float)."""
    if m.dim() != 4:
        raise _lib.PerfError(f'joint_tv: the map must be [n, C, H, W], got {tuple(m.shape)}')
    n, C, H, W = m.shape
    if grad is None:
        grad = torch.empty_like(m, memory_format=torch.contiguous_format)
    if value is None:
        value = torch.empty(1, dtype=torch.float32, device=m.device)
    if grad.shape != m.shape or value.numel() != 1:
        raise _lib.PerfError('joint_tv: grad has the map\'s shape and value one element')
    nbytes = _lib.load().perf_joint_tv_workspace_bytes(n, C, H, W)
    if nbytes < 0:
        _lib.check(-1, 'perf_joint_tv_workspace_bytes')
    block = (ws or Workspace()).get(nbytes, m.device)
    _call('perf_joint_tv', _p(_f32(m, 'map')), n, C, H, W, float(weight), _p(_f32(grad, 'grad')), _p(_f32(value, 'value')), _p(block),
          block.numel() * 4, _stream())
    return value, grad


# ---- what the mesh units' bindings share ------------------------------------------------------------------------------------------------
_ANYWHERE = 'anywhere'          # _dev_tensor's device for a tensor the library is not handed (K = 0 views): it may be on the host


def _dev_tensor(who, name, t, dtype, shape, device=None, any_dtype_if_empty=False):
    """The one check of a tensor the library reads or writes: t is a contiguous CUDA tensor of dtype (one, or a tuple of them) and shape,
    on `device` (the device of the tensor it must live with) when one is given.  A shape entry is a size, or a letter for a dimension
    left free, reported as in [V, 3]; a shape of None leaves all of them free.  None passes through: an optional argument.
    any_dtype_if_empty: an empty t stands for NULL in the call and may have any dtype."""
    if t is None:
        return None
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    ok = torch.is_tensor(t) and (t.dtype in dtypes or (any_dtype_if_empty and t.numel() == 0)) and t.is_contiguous()
    ok = ok and (device is _ANYWHERE or (t.is_cuda and device in (None, t.device)))
    if ok and shape is not None:
        ok = t.dim() == len(shape) and all(isinstance(s, str) or s == d for s, d in zip(shape, t.shape))
    if not ok:
        want = ' or '.join(str(d) for d in dtypes) + ('' if shape is None else f' [{", ".join(str(s) for s in shape)}]')
        where = 'tensor' if device is _ANYWHERE else 'CUDA tensor (there is no CPU path)' if device is None else f'CUDA tensor on {device} (there is no CPU path)'
        got = f'{t.dtype} {tuple(t.shape)} on {t.device}{"" if t.is_contiguous() else ", not contiguous"}' if torch.is_tensor(t) else type(t).__name__
        raise _lib.PerfError(f'{who}: {name} must be a contiguous {want} {where}, got {got}')
    return t


def _pn(t):
    """The pointer of t, NULL for None and for an empty tensor."""
    return _p(t) if t is not None and t.numel() else None


def _flag(who, name, flag, n, device):
    """The words the library reports into: new int64 [n] ones, or what the caller passed, which is the caller's to size: only that it
    is a tensor is checked here."""
    if flag is None:
        return torch.empty(n, dtype=torch.int64, device=device)
    if not torch.is_tensor(flag):
        raise _lib.PerfError(f'{who}: {name} must be an int64 [{n}] CUDA tensor, got {type(flag).__name__}')
    return flag


def _mesh_ws(query, sizes, ws, device):
    """The int64 workspace of at least perf_*_workspace_bytes(*sizes) bytes on device: ws itself when it serves, else a new one."""
    nbytes = getattr(_lib.load(), query)(*sizes)
    if nbytes < 0:
        _lib.check(-1, query)
    if ws is not None and not torch.is_tensor(ws):
        raise _lib.PerfError(f'{query}: ws must be an int64 CUDA tensor or None, got {type(ws).__name__}')
    if ws is None or ws.numel() * 8 < nbytes or ws.device != device:
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
    return ws


def _ws_args(who, ws):
    """The (pointer, bytes) of a workspace in a library call; whether it is the one the count made is the library's to judge, by its bytes."""
    if not torch.is_tensor(ws):
        raise _lib.PerfError(f'{who}: ws must be the int64 CUDA workspace of the count, got {type(ws).__name__}')
    return _p(ws), ws.numel() * 8


def _mask_u8(who, name, mask, shape, device=None):
    """A bool or uint8 mask of shape as the contiguous uint8 the library reads; a strided one is copied."""
    if torch.is_tensor(mask):
        mask = mask.contiguous()
    return _dev_tensor(who, name, mask, (torch.bool, torch.uint8), shape, device).view(torch.uint8)


def _box3(who, lo, hi):
    """The bounds of a box, three values each, as the float [3] arguments of the library."""
    lo3, hi3 = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo3) != 3 or len(hi3) != 3:
        raise _lib.PerfError(f'{who}: lo and hi hold three values each')
    return (ctypes.c_float * 3)(*lo3), (ctypes.c_float * 3)(*hi3)


def _faces(who, faces, n_vertices, device=None):
    """faces int32 [F, 3] over n_vertices vertices, as many as the library takes -> (n_vertices, F)."""
    faces = _dev_tensor(who, 'faces', faces, torch.int32, ('F', 3), device)
    n = int(n_vertices)
    if n < 0 or n > _lib.MESHCC_MAX_VERTICES:
        raise _lib.PerfError(f'{who}: {n} vertices are outside 0 .. 2^30')
    return n, int(faces.shape[0])


def _mesh_head(who, vertices, faces, max_faces=None):
    """The head of a mesh: vertices fp32 [V, 3] and faces int32 [F, 3] on one device, at most max_faces of them -> (vertices, V, F, the
    (vertices, V, faces, F) a library call begins with)."""
    vertices = _dev_tensor(who, 'vertices', vertices, torch.float32, ('V', 3))
    nv, f = _faces(who, faces, vertices.shape[0], vertices.device)
    if max_faces is not None and f > max_faces:
        raise _lib.PerfError(f'{who}: {f} faces are more than {"2^31 - 1" if max_faces == (1 << 31) - 1 else max_faces}')
    return vertices, nv, f, (_pn(vertices), nv, _pn(faces), f)


def _labelled_faces(who, faces, labels, name):
    """faces int32 [F, 3] and the vertices' labels int32 [V], on one device -> (V, F)."""
    labels = _dev_tensor(who, name, labels, torch.int32, ('V',))
    return _faces(who, faces, labels.numel(), labels.device)


def _centres(who, centres):
    """The views' centres fp32 [K, 3] -> (centres, K).  With no view they are not read: any [0, 3] tensor serves, on the host as well."""
    if not (torch.is_tensor(centres) and tuple(centres.shape) == (0, 3)):
        centres = _dev_tensor(who, 'centres', centres, torch.float32, ('K', 3))
    return centres, int(centres.shape[0])


def _views_table(who, views, sizes, device):
    """The views of meshvis_views against their host sizes -> the (views, sizes, K) of a library call.  With no view the table is not
    read and may be on the host."""
    k = len(sizes)
    views = _dev_tensor(who, 'views', views, torch.int32, (k, 16), device if k else _ANYWHERE)
    return _pn(views), (ctypes.c_int32 * (2 * k))(*[v for hw in sizes for v in hw]) if k else None, k


def _blend_args(who, n, device, views, sizes, map_pointers, tol, facing, power, select, fallback, fill):
    """The views' side of the blend of include/perf_hip_meshcolor.h over n vertices on device, checked -> its arguments in a library
    call, from the views to the fill."""
    table, flat, k = _views_table(who, views, sizes, device)
    map_pointers = _dev_tensor(who, 'map_pointers', map_pointers, torch.int64, (k,), device if k else _ANYWHERE)
    if select not in _lib.MESHCOLOR_SELECT:
        raise _lib.PerfError(f"{who}: select is 'blend' or 'best', got {select!r}")
    fallback = _dev_tensor(who, "the vertices' fallback", fallback, torch.float32, (n, 3), device)          # (named with the vertices, like their normals: a
    # row count that disagrees is refused here whichever of the two is wrong)
    fill3 = [float(v) for v in fill]
    if len(fill3) != 3:
        raise _lib.PerfError(f'{who}: fill holds three values')
    return (table, _pn(map_pointers), flat, k, float(tol), int(bool(facing)), int(power), _lib.MESHCOLOR_SELECT[select], _pn(fallback),
            (ctypes.c_float * 3)(*fill3))


def _filtered(vertices, n_vertices_kept, n_faces_kept, device):
    """What a filter writes -> ((kept vertices or None without vertices, kept faces, kept_vertex_index), the tail of its library call)."""
    nv, nf = int(n_vertices_kept), int(n_faces_kept)
    vertices_out = torch.empty(nv, 3, dtype=torch.float32, device=device) if vertices is not None else None
    index = torch.empty(nv, dtype=torch.int32, device=device)
    faces_out = torch.empty(nf, 3, dtype=torch.int32, device=device)
    return (vertices_out, faces_out, index), (_pn(vertices_out), _pn(index), nv, _pn(faces_out), nf)


# ---- surface nets on a dense lattice (include/perf_hip_mesh.h) -------------------------------------------------------------------------
def _mesh_cells(who, field):
    field = _dev_tensor(who, 'field', field, torch.float32, ('nx+1', 'ny+1', 'nz+1'))
    if min(field.shape) < 2:
        raise _lib.PerfError(f'{who}: the field must be [nx+1, ny+1, nz+1] corner values with at least one cell per axis, got {tuple(field.shape)}')
    return tuple(int(s) - 1 for s in field.shape)


def mesh_count(field, thr, ws=None):
    """Classify the cells of a lattice of fp32 corner values [nx+1, ny+1, nz+1] against thr (perf_mesh_count) -> (counts, ws): counts =
    int64 [2] ON THE DEVICE (vertices, triangles), ws = the int64 workspace that mesh_write needs (pass one back in to reuse it)."""
    nx, ny, nz = _mesh_cells('mesh_count', field)
    ws = _mesh_ws('perf_mesh_workspace_bytes', (nx, ny, nz), ws, field.device)
    counts = torch.empty(2, dtype=torch.int64, device=field.device)
    _call('perf_mesh_count', _p(field), nx, ny, nz, float(thr), *_ws_args('mesh_count', ws), _p(counts), _stream())
    return counts, ws


def mesh_write(field, thr, lo, hi, ws, n_vertices, n_faces):
    """The vertices [n_vertices, 3] fp32 and faces [n_faces, 3] int32 of the lattice mesh_count classified into ws (perf_mesh_write); the
    same field and thr.  lo, hi: the box's bounds, three values each.  The two counts are what the caller read from mesh_count's totals:
    smaller ones are refused."""
    nx, ny, nz = _mesh_cells('mesh_write', field)
    lo3, hi3 = _box3('mesh_write', lo, hi)
    vertices = torch.empty(int(n_vertices), 3, dtype=torch.float32, device=field.device)
    faces = torch.empty(int(n_faces), 3, dtype=torch.int32, device=field.device)
    _call('perf_mesh_write', _p(field), nx, ny, nz, float(thr), lo3, hi3, *_ws_args('mesh_write', ws), _pn(vertices), int(n_vertices), _pn(faces), int(n_faces), _stream())
    return vertices, faces


# ---- surface nets on the live bricks of a lattice (include/perf_hip_brickmesh.h) -------------------------------------------------------
def _brick_shape(who, shape):
    n = tuple(int(v) for v in shape)
    if len(n) != 3:
        raise _lib.PerfError(f'{who}: the lattice has three dimensions, got {shape!r}')
    return n


def _brick_occ(who, binaries):
    """binaries: bool or uint8 [..., R, R, R] -> (uint8 view, R)."""
    if not torch.is_tensor(binaries) or binaries.dim() < 3 or len(set(binaries.shape[-3:])) != 1 or binaries.numel() != binaries.shape[-1] ** 3:
        got = f'{binaries.dtype} {tuple(binaries.shape)}' if torch.is_tensor(binaries) else type(binaries).__name__
        raise _lib.PerfError(f'{who}: binaries must be bool or uint8 [R, R, R], got {got}')
    return _mask_u8(who, 'binaries', binaries, tuple(binaries.shape)), int(binaries.shape[-1])


def brickmesh_select(binaries, shape, ws=None):
    """Which 8^3 bricks of a lattice of `shape` cells touch a set cell of the occupancy grid (perf_brickmesh_select) -> (table int32
    [Bx, By, Bz]: slot or -1, n_live: int64 [1] ON THE DEVICE)."""
    n = _brick_shape('brickmesh_select', shape)
    occ, res = _brick_occ('brickmesh_select', binaries)
    ws = _mesh_ws('perf_brickmesh_workspace_bytes', (*n, 0), ws, occ.device)
    table = torch.empty(tuple(v // 8 for v in n), dtype=torch.int32, device=occ.device)
    n_live = torch.empty(1, dtype=torch.int64, device=occ.device)
    _call('perf_brickmesh_select', _p(occ), res, *n, _p(table), _p(n_live), *_ws_args('brickmesh_select', ws), _stream())
    return table, n_live


def brickmesh_list(table, n_bricks):
    """The ascending linear indices int32 [n_bricks] of the bricks a table holds (perf_brickmesh_list)."""
    table = _dev_tensor('brickmesh_list', 'table', table, torch.int32, ('Bx', 'By', 'Bz'))
    ids = torch.empty(int(n_bricks), dtype=torch.int32, device=table.device)
    _call('perf_brickmesh_list', _p(table), *(8 * int(s) for s in table.shape), _pn(ids), int(n_bricks), _stream())
    return ids


def brickmesh_corners(ids, first, m, shape, binaries):
    """The stored corners of the slots first .. first + m - 1 (perf_brickmesh_corners) -> (x01 fp32 [m * 512, 3], sel uint8 [m * 512]:
    strictly inside the box AND in a set occupancy cell, interior uint8 [m * 512]: strictly inside the box)."""
    n = _brick_shape('brickmesh_corners', shape)
    ids = _dev_tensor('brickmesh_corners', 'ids', ids, torch.int32, None, any_dtype_if_empty=True)
    occ, res = _brick_occ('brickmesh_corners', binaries)
    m = int(m)
    x01 = torch.empty(max(m, 0) * 512, 3, dtype=torch.float32, device=ids.device)
    sel = torch.empty(max(m, 0) * 512, dtype=torch.uint8, device=ids.device)
    interior = torch.empty_like(sel)
    _call('perf_brickmesh_corners', _pn(ids), ids.numel(), int(first), m, *n, _p(occ), res, _pn(x01), _pn(sel), _pn(interior), _stream())
    return x01, sel, interior


def _brick_set(who, values, ids, table, shape):
    """The stored corners, the ids and the table of a set of bricks -> (the lattice's cells, M, the (values, ids, table, M) of a library call)."""
    n = _brick_shape(who, shape)
    values = _dev_tensor(who, 'values', values, torch.float32, None, any_dtype_if_empty=True)
    ids = _dev_tensor(who, 'ids', ids, torch.int32, None, any_dtype_if_empty=True)
    table = _dev_tensor(who, 'table', table, torch.int32, None)
    m = int(ids.numel())
    if values.numel() != m * 512 or tuple(table.shape) != tuple(v // 8 for v in n):
        raise _lib.PerfError(f'{who}: values {tuple(values.shape)}, ids {tuple(ids.shape)} and table {tuple(table.shape)} do not describe bricks of a lattice of {n} cells')
    return n, m, (_pn(values), _pn(ids), _p(table), m)


def brickmesh_count(values, ids, table, shape, thr, fill, ws=None):
    """Classify the cells of the live bricks (perf_brickmesh_count) -> (counts, ws): counts = int64 [3] ON THE DEVICE (vertices, triangles,
    violations of the closure rule), ws = the int64 workspace brickmesh_write needs."""
    n, m, bricks = _brick_set('brickmesh_count', values, ids, table, shape)
    ws = _mesh_ws('perf_brickmesh_workspace_bytes', (*n, m), ws, table.device)
    counts = torch.empty(3, dtype=torch.int64, device=table.device)
    _call('perf_brickmesh_count', *bricks, *n, float(thr), float(fill), *_ws_args('brickmesh_count', ws), _p(counts), _stream())
    return counts, ws


def brickmesh_write(values, ids, table, shape, thr, fill, lo, hi, ws, n_vertices, n_faces):
    """The vertices [n_vertices, 3] fp32, faces [n_faces, 3] int32 and cells [n_vertices] int64 (each vertex's linear cell of the virtual
    lattice) of what brickmesh_count classified into ws (perf_brickmesh_write).  Counts below the counted totals are refused."""
    n, m, bricks = _brick_set('brickmesh_write', values, ids, table, shape)
    lo3, hi3 = _box3('brickmesh_write', lo, hi)
    nv, nf = int(n_vertices), int(n_faces)
    vertices = torch.empty(nv, 3, dtype=torch.float32, device=table.device)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=table.device)
    cells = torch.empty(nv, dtype=torch.int64, device=table.device)
    _call('perf_brickmesh_write', *bricks, *n, float(thr), float(fill), lo3, hi3, *_ws_args('brickmesh_write', ws), _pn(vertices), nv, _pn(faces), nf, _pn(cells), _stream())
    return vertices, faces, cells


# ---- connected components of a triangle mesh (include/perf_hip_meshcc.h) ---------------------------------------------------------------
def meshcc_label(faces, n_vertices, ws=None):
    """Label the connected components of faces int32 [F, 3] over n_vertices vertices (perf_meshcc_label) -> (vertex_component int32 [V],
    counts, ws): counts = int64 [2] ON THE DEVICE (C, the first face with an index outside [0, V) or -1)."""
    n, f = _faces('meshcc_label', faces, n_vertices)
    ws = _mesh_ws('perf_meshcc_workspace_bytes', (n, f), ws, faces.device)
    vertex_component = torch.empty(n, dtype=torch.int32, device=faces.device)
    counts = torch.empty(2, dtype=torch.int64, device=faces.device)
    _call('perf_meshcc_label', _pn(faces), f, n, _pn(vertex_component), _p(counts), *_ws_args('meshcc_label', ws), _stream())
    return vertex_component, counts, ws


def meshcc_stats(faces, vertex_component, n_components, vertices=None):
    """faces int64 [C], vertices int32 [C] and, with vertices fp32 [V, 3], signed volume float64 [C] (else None) of the components
    (perf_meshcc_stats)."""
    n, f = _labelled_faces('meshcc_stats', faces, vertex_component, 'vertex_component')
    vertices = _dev_tensor('meshcc_stats', 'vertices', vertices, torch.float32, (n, 3), faces.device)
    c = int(n_components)
    faces_per = torch.empty(c, dtype=torch.int64, device=faces.device)
    vertices_per = torch.empty(c, dtype=torch.int32, device=faces.device)
    volume = torch.empty(c, dtype=torch.float64, device=faces.device) if vertices is not None else None
    _call('perf_meshcc_stats', _pn(faces), f, _pn(vertices), n, _pn(vertex_component), c, _pn(faces_per), _pn(vertices_per), _pn(volume), _stream())
    return faces_per, vertices_per, volume


def meshcc_filter_count(faces, vertex_component, keep, ws=None):
    """Rank the vertices and faces of the components keep [C] selects (perf_meshcc_filter_count) -> (counts, ws): counts = int64 [2] ON
    THE DEVICE (kept vertices, kept faces), ws = the workspace meshcc_filter_write needs."""
    n, f = _labelled_faces('meshcc_filter_count', faces, vertex_component, 'vertex_component')
    k = _mask_u8('meshcc_filter_count', 'keep', keep, ('C',), faces.device)
    ws = _mesh_ws('perf_meshcc_workspace_bytes', (n, f), ws, faces.device)
    counts = torch.empty(2, dtype=torch.int64, device=faces.device)
    _call('perf_meshcc_filter_count', _pn(faces), f, _pn(vertex_component), n, _pn(k), k.numel(), *_ws_args('meshcc_filter_count', ws), _p(counts), _stream())
    return counts, ws


def meshcc_filter_write(faces, vertex_component, keep, ws, n_vertices_kept, n_faces_kept, vertices=None):
    """The kept faces int32 [F', 3] re-indexed, kept_vertex_index int32 [V'] and, with vertices, the kept vertices fp32 [V', 3] (else
    None) of what meshcc_filter_count ranked into ws (perf_meshcc_filter_write).  Counts below the counted totals are refused."""
    n, f = _labelled_faces('meshcc_filter_write', faces, vertex_component, 'vertex_component')
    k = _mask_u8('meshcc_filter_write', 'keep', keep, ('C',), faces.device)
    vertices = _dev_tensor('meshcc_filter_write', 'vertices', vertices, torch.float32, (n, 3), faces.device)
    out, tail = _filtered(vertices, n_vertices_kept, n_faces_kept, faces.device)
    _call('perf_meshcc_filter_write', _pn(faces), f, _pn(vertex_component), n, _pn(k), k.numel(), _pn(vertices), *_ws_args('meshcc_filter_write', ws), *tail, _stream())
    return out


# ---- cull the faces no registered panorama saw (include/perf_hip_meshvis.h) ------------------------------------------------------------
def meshvis_views(poses, maps):
    """The device array of perf_meshvis_view of K panoramas -> (views int32 [K, 16] on the device, centres fp32 [K, 3], sizes: the host
    (height, width) pairs, maps: the tensors the descriptors point into, to be kept alive with them).  poses: K [4, 4] or [3, 4]
    camera-to-world matrices, on any device (they are not read back); maps: K CUDA fp32 [H, W] masked distance maps, any sizes."""
    if len(poses) != len(maps):
        raise _lib.PerfError(f'meshvis_views: {len(poses)} poses and {len(maps)} maps')
    k = len(maps)
    if k > _lib.MESHVIS_MAX_VIEWS:
        raise _lib.PerfError(f'meshvis_views: {k} views are more than {_lib.MESHVIS_MAX_VIEWS} (a vertex has one bit per view in a 64-bit word)')
    for m in maps:
        if not torch.is_tensor(m) or not m.is_cuda:
            raise _lib.PerfError('meshvis_views: the distance maps must be CUDA tensors (there is no CPU path)')
        if m.dim() != 2 or m.shape[0] < 1 or m.shape[1] < 1 or m.shape[0] >= 1 << 31 or m.shape[1] >= 1 << 31:
            raise _lib.PerfError(f'meshvis_views: a distance map is [H, W] with both at least 1, got {tuple(m.shape)}')
    dev = maps[0].device if k else torch.device('cuda')
    maps = [_f32(m, 'distance_map') for m in maps]
    sizes = [(int(m.shape[0]), int(m.shape[1])) for m in maps]
    if k == 0:
        return torch.zeros(0, 16, dtype=torch.int32, device=dev), torch.zeros(0, 3, dtype=torch.float32, device=dev), sizes, maps
    pose = torch.stack([torch.as_tensor(p, dtype=torch.float32).to(dev)[:3, :4] for p in poses])            # [K, 3, 4]
    rt = pose[:, :, :3].transpose(1, 2).reshape(k, 9)
    centres = pose[:, :, 3].contiguous()
    tail = []
    for (h, w), m in zip(sizes, maps):
        ptr = m.data_ptr()
        tail.append([h, w] + [v - (1 << 32) if v >= 1 << 31 else v for v in (ptr & 0xffffffff, ptr >> 32)])          # (the words of the pointer, low first)
    tail = torch.tensor(tail, dtype=torch.int32).to(dev)
    views = torch.cat([rt.contiguous().view(torch.int32), centres.view(torch.int32), tail], dim=1).contiguous()
    return views, centres, sizes, maps


def meshvis_vertex_bits(vertices, views, sizes, tol, free_tol):
    """visible_bits, free_bits int64 [V] of vertices fp32 [V, 3] against the views of meshvis_views: ONE launch for all of them
    (perf_meshvis_vertex_bits)."""
    vertices = _dev_tensor('meshvis_vertex_bits', 'vertices', vertices, torch.float32, ('V', 3), any_dtype_if_empty=True)
    n = int(vertices.shape[0])
    table = _views_table('meshvis_vertex_bits', views, sizes, vertices.device)
    visible = torch.empty(n, dtype=torch.int64, device=vertices.device)
    free = torch.empty(n, dtype=torch.int64, device=vertices.device)
    _call('perf_meshvis_vertex_bits', _pn(vertices), n, *table, float(tol), float(free_tol), _pn(visible), _pn(free), _stream())
    return visible, free


def meshvis_face_keep(faces, vertices, visible_bits, free_bits, centres, facing=True, min_views=1, carve=False, flag=None):
    """face_keep uint8 [F] by the face rule of include/perf_hip_meshvis.h (perf_meshvis_face_keep) -> (face_keep, flag): flag = int64 [1]
    ON THE DEVICE, the smallest index of a face with an index outside [0, V) or -1 (an int64 [1] view to write it into may be passed)."""
    vertices, n, f, _ = _mesh_head('meshvis_face_keep', vertices, faces)
    visible_bits = _dev_tensor('meshvis_face_keep', 'visible_bits', visible_bits, torch.int64, (n,), faces.device)
    free_bits = _dev_tensor('meshvis_face_keep', 'free_bits', free_bits, torch.int64, (n,), faces.device)
    centres, k = _centres('meshvis_face_keep', centres)
    keep = torch.empty(f, dtype=torch.uint8, device=faces.device)
    flag = _flag('meshvis_face_keep', 'flag', flag, 1, faces.device)
    _call('perf_meshvis_face_keep', _pn(faces), f, _pn(vertices), n, _pn(visible_bits), _pn(free_bits), _pn(centres), k, int(bool(facing)), int(min_views),
          int(bool(carve)), _pn(keep), _p(flag), _stream())
    return keep, flag


def meshvis_filter_count(faces, n_vertices, face_keep, ws=None, counts=None):
    """Rank the faces face_keep [F] selects and the vertices they name (perf_meshvis_filter_count) -> (counts, ws): counts = int64 [2] ON
    THE DEVICE (kept vertices, kept faces; an int64 [2] view to write them into may be passed), ws = the workspace meshvis_filter_write
    needs."""
    n, f = _faces('meshvis_filter_count', faces, n_vertices)
    k = _mask_u8('meshvis_filter_count', 'face_keep', face_keep, (f,), faces.device)
    ws = _mesh_ws('perf_meshvis_workspace_bytes', (n, f), ws, faces.device)
    counts = _flag('meshvis_filter_count', 'counts', counts, 2, faces.device)
    _call('perf_meshvis_filter_count', _pn(faces), f, n, _pn(k), *_ws_args('meshvis_filter_count', ws), _p(counts), _stream())
    return counts, ws


def meshvis_filter_write(faces, n_vertices, face_keep, ws, n_vertices_kept, n_faces_kept, vertices=None):
    """The kept faces int32 [F', 3] re-indexed, kept_vertex_index int32 [V'] and, with vertices, the kept vertices fp32 [V', 3] (else
    None) of what meshvis_filter_count ranked into ws (perf_meshvis_filter_write).  Counts below the counted totals are refused."""
    n, f = _faces('meshvis_filter_write', faces, n_vertices)
    k = _mask_u8('meshvis_filter_write', 'face_keep', face_keep, (f,), faces.device)
    vertices = _dev_tensor('meshvis_filter_write', 'vertices', vertices, torch.float32, (n, 3), faces.device)
    out, tail = _filtered(vertices, n_vertices_kept, n_faces_kept, faces.device)
    _call('perf_meshvis_filter_write', _pn(faces), f, n, _pn(k), _pn(vertices), *_ws_args('meshvis_filter_write', ws), *tail, _stream())
    return out


# ---- simplify a mesh by vertex clustering (include/perf_hip_meshsimp.h) -----------------------------------------------------------------
def _simp_grid(who, lo, h, n):
    lo3, n3 = [float(v) for v in lo], [int(v) for v in n]
    if len(lo3) != 3 or len(n3) != 3:
        raise _lib.PerfError(f'{who}: lo and n hold three values each')
    if any(v < 1 or v > _lib.MESHSIMP_MAX_CELLS for v in n3):
        raise _lib.PerfError(f'{who}: {n3} cells per axis are outside 1 .. 2^21')
    return (ctypes.c_float * 3)(*lo3), float(h), n3


def meshsimp_bounds(vertices):
    """fp32 [6] ON THE DEVICE: the smallest x, y, z and the largest x, y, z among the finite coordinates of vertices fp32 [V, 3]
    (perf_meshsimp_bounds); (+inf x 3, -inf x 3) when there is none."""
    vertices = _dev_tensor('meshsimp_bounds', 'vertices', vertices, torch.float32, ('V', 3))
    bounds = torch.empty(6, dtype=torch.float32, device=vertices.device)
    _call('perf_meshsimp_bounds', _pn(vertices), vertices.shape[0], _p(bounds), _stream())
    return bounds


def meshsimp_cluster(vertices, lo, h, n, n_faces=0, ws=None, counts=None):
    """The clusters of vertices fp32 [V, 3] in the grid (lo [3], cell edge h, n [3] cells per axis) by the cell rule of
    include/perf_hip_meshsimp.h (perf_meshsimp_cluster) -> (vertex_cluster int32 [V], counts, ws): counts = int64 [2] ON THE DEVICE (C, the
    first vertex with a coordinate that is not finite or -1; an int64 [2] view to write them into may be passed).  n_faces: the faces the
    workspace is to serve as well (meshsimp_faces)."""
    vertices = _dev_tensor('meshsimp_cluster', 'vertices', vertices, torch.float32, ('V', 3))
    nv = int(vertices.shape[0])
    lo3, h, n3 = _simp_grid('meshsimp_cluster', lo, h, n)
    ws = _mesh_ws('perf_meshsimp_workspace_bytes', (nv, int(n_faces)), ws, vertices.device)
    vertex_cluster = torch.empty(nv, dtype=torch.int32, device=vertices.device)
    counts = _flag('meshsimp_cluster', 'counts', counts, 2, vertices.device)
    _call('perf_meshsimp_cluster', _pn(vertices), nv, int(n_faces), lo3, h, *n3, _pn(vertex_cluster), _p(counts), *_ws_args('meshsimp_cluster', ws), _stream())
    return vertex_cluster, counts, ws


def meshsimp_place(vertices, lo, h, n, vertex_cluster, n_clusters, placement='mean'):
    """(cluster_vertices fp32 [C, 3], representative int32 [C]) of the labelling meshsimp_cluster made of the SAME vertices and grid
    (perf_meshsimp_place).  placement: 'mean' or 'member'."""
    vertices = _dev_tensor('meshsimp_place', 'vertices', vertices, torch.float32, ('V', 3))
    nv = int(vertices.shape[0])
    lo3, h, n3 = _simp_grid('meshsimp_place', lo, h, n)
    vertex_cluster = _dev_tensor('meshsimp_place', 'vertex_cluster', vertex_cluster, torch.int32, (nv,), vertices.device)
    if placement not in _lib.MESHSIMP_PLACEMENT:
        raise _lib.PerfError(f"meshsimp_place: placement is 'mean' or 'member', got {placement!r}")
    c = int(n_clusters)
    out = torch.empty(c, 3, dtype=torch.float32, device=vertices.device)
    representative = torch.empty(c, dtype=torch.int32, device=vertices.device)
    scratch = torch.empty(c * (_lib.MESHSIMP_SCRATCH_BYTES // 8), dtype=torch.int64, device=vertices.device)
    _call('perf_meshsimp_place', _pn(vertices), nv, lo3, h, *n3, _pn(vertex_cluster), c, _lib.MESHSIMP_PLACEMENT[placement], _pn(out), _pn(representative),
          _pn(scratch), scratch.numel() * 8, _stream())
    return out, representative


def meshsimp_faces(faces, vertex_cluster, dedupe='oriented', ws=None, flag=None):
    """faces int32 [F, 3] through vertex_cluster int32 [V] (perf_meshsimp_faces) -> (remapped int32 [F, 3], face_keep uint8 [F], flag):
    a face is kept unless two of its cluster ids are equal or (dedupe 'oriented' / 'unoriented') a face with a smaller index has its
    triple up to rotation / as a set; flag = int64 [1] ON THE DEVICE, the smallest index of a face with an index outside [0, V) or -1 (an
    int64 [1] view to write it into may be passed)."""
    nv, f = _labelled_faces('meshsimp_faces', faces, vertex_cluster, 'vertex_cluster')
    if dedupe not in _lib.MESHSIMP_DEDUPE:
        raise _lib.PerfError(f"meshsimp_faces: dedupe is 'oriented', 'unoriented' or None, got {dedupe!r}")
    if f > _lib.MESHSIMP_MAX_FACES:
        raise _lib.PerfError(f'meshsimp_faces: {f} faces are more than 2^31 - 1')
    ws = _mesh_ws('perf_meshsimp_workspace_bytes', (nv, f), ws, faces.device)
    remapped = torch.empty(f, 3, dtype=torch.int32, device=faces.device)
    keep = torch.empty(f, dtype=torch.uint8, device=faces.device)
    flag = _flag('meshsimp_faces', 'flag', flag, 1, faces.device)
    _call('perf_meshsimp_faces', _pn(faces), f, _pn(vertex_cluster), nv, _lib.MESHSIMP_DEDUPE[dedupe], _pn(remapped), _pn(keep), _p(flag), *_ws_args('meshsimp_faces', ws),
          _stream())
    return remapped, keep, flag


# ---- quadric error placement of the clusters' vertices (include/perf_hip_meshquadric.h) ------------------------------------------------
def meshquadric_sums(vertices, faces, lo, h, n, vertex_cluster, n_clusters, flags=None):
    """Stage A of include/perf_hip_meshquadric.h (perf_meshquadric_sums) -> (acc int64 [C, 9], flags): per cluster the int64 fixed-point
    sums (2^-40) of its members' quadrics, qA xx, xy, xz, yy, yz, zz then qb x, y, z, by integer atomics: exact in any order.  flags =
    int64 [2] ON THE DEVICE: the smallest index of a face with an index outside [0, V) or -1, then the smallest index of a face the
    2^60 rule skipped or -1 (an int64 [2] view to write them into may be passed)."""
    vertices, nv, f, mesh = _mesh_head('meshquadric_sums', vertices, faces, _lib.MESHQUADRIC_MAX_FACES)
    lo3, h, n3 = _simp_grid('meshquadric_sums', lo, h, n)
    vertex_cluster = _dev_tensor('meshquadric_sums', 'vertex_cluster', vertex_cluster, torch.int32, (nv,), vertices.device)
    c = int(n_clusters)
    if c < 0 or c > nv:
        raise _lib.PerfError(f'meshquadric_sums: {c} clusters, the mesh has {nv} vertices')
    acc = torch.empty(c, _lib.MESHQUADRIC_TERMS, dtype=torch.int64, device=vertices.device)
    flags = _flag('meshquadric_sums', 'flags', _dev_tensor('meshquadric_sums', 'flags', flags, torch.int64, (2,), vertices.device), 2, vertices.device)
    _call('perf_meshquadric_sums', *mesh, lo3, h, *n3, _pn(vertex_cluster), c, _pn(acc), ctypes.c_void_p(flags.data_ptr()), ctypes.c_void_p(flags.data_ptr() + 8),
          _stream())
    return acc, flags


def meshquadric_place(vertices, lo, h, n, anchor, representative, acc):
    """Stage B of include/perf_hip_meshquadric.h (perf_meshquadric_place) -> cluster vertices fp32 [C, 3]: the minimiser of the cluster's
    summed quadric, regularised towards anchor fp32 [C, 3] (the 'mean' placement) and clamped to the cell of vertices[representative];
    anchor's row, bit for bit, where the cluster has no face or no solve."""
    vertices = _dev_tensor('meshquadric_place', 'vertices', vertices, torch.float32, ('V', 3))
    nv, dev = int(vertices.shape[0]), vertices.device
    lo3, h, n3 = _simp_grid('meshquadric_place', lo, h, n)
    acc = _dev_tensor('meshquadric_place', 'acc', acc, torch.int64, ('C', _lib.MESHQUADRIC_TERMS), dev)
    c = int(acc.shape[0])
    if c > nv:
        raise _lib.PerfError(f'meshquadric_place: acc must be an int64 [C, {_lib.MESHQUADRIC_TERMS}] tensor with C <= {nv} vertices')
    anchor = _dev_tensor('meshquadric_place', 'anchor', anchor, torch.float32, (c, 3), dev)
    representative = _dev_tensor('meshquadric_place', 'representative', representative, torch.int32, (c,), dev)
    out = torch.empty(c, 3, dtype=torch.float32, device=dev)
    _call('perf_meshquadric_place', _pn(vertices), nv, lo3, h, *n3, _pn(anchor), _pn(representative), _pn(acc), c, _pn(out), _stream())
    return out


# ---- colour a mesh from the registered panoramas; vertex normals from faces (include/perf_hip_meshcolor.h) -----------------------------
def meshcolor_normal_sums(vertices, faces, scale_log2, flag=None):
    """The faces' area-weighted normals (double, times 2^scale_log2, rounded to int64) summed at their vertices by integer atomics
    (perf_meshcolor_normal_sums) -> (acc int64 [V, 3], flag): flag = int64 [1] ON THE DEVICE, the smallest index of a face with an index
    outside [0, V) or -1 (an int64 [1] view to write it into may be passed)."""
    vertices, nv, f, mesh = _mesh_head('meshcolor_normal_sums', vertices, faces, _lib.MESHCOLOR_MAX_FACES)
    acc = torch.empty(nv, 3, dtype=torch.int64, device=vertices.device)
    flag = _flag('meshcolor_normal_sums', 'flag', flag, 1, vertices.device)
    _call('perf_meshcolor_normal_sums', *mesh, int(scale_log2), _pn(acc), _p(flag), _stream())
    return acc, flag


def meshcolor_normals(acc):
    """Unit normals fp32 [V, 3] of the sums of meshcolor_normal_sums, exactly 0 where a sum is (perf_meshcolor_normals)."""
    acc = _dev_tensor('meshcolor_normals', 'acc', acc, torch.int64, ('V', 3))
    n = int(acc.shape[0])
    normals = torch.empty(n, 3, dtype=torch.float32, device=acc.device)
    _call('perf_meshcolor_normals', _pn(acc), n, _pn(normals), _stream())
    return normals


def meshcolor_maps(color_maps, sizes):
    """The device array of the K colour maps' pointers -> (pointers int64 [K] on the device, maps: the tensors it points into, to be kept
    alive with it).  color_maps: K CUDA [H, W, 3], converted to fp32 when they are not; sizes: the (height, width) pairs of the views' distance maps (meshvis_views), which
    map k must have."""
    if len(color_maps) != len(sizes):
        raise _lib.PerfError(f'meshcolor_maps: {len(color_maps)} colour maps and {len(sizes)} views')
    maps = []
    for k, (m, hw) in enumerate(zip(color_maps, sizes)):
        if not torch.is_tensor(m) or not m.is_cuda:
            raise _lib.PerfError(f'meshcolor_maps: view {k}\'s color_map must be a CUDA tensor (there is no CPU path)')
        if m.dim() != 3 or m.shape[2] != 3 or tuple(m.shape[:2]) != tuple(hw):
            raise _lib.PerfError(f'meshcolor_maps: view {k}\'s color_map is {tuple(m.shape)}, its distance map {tuple(hw)}: a colour map is [H, W, 3] of its distance map\'s size')
        maps.append(m.float().contiguous())          # (both return m itself when it already is fp32 and contiguous)
    dev = maps[0].device if maps else torch.device('cuda')
    return torch.tensor([m.data_ptr() for m in maps], dtype=torch.int64).to(dev), maps


def meshcolor_blend(vertices, normals, views, sizes, map_pointers, tol, facing=True, power=2, select='blend', fallback=None, fill=(0.5, 0.5, 0.5)):
    """(colors fp32 [V, 3], weight fp32 [V], used_bits int64 [V], best_view int8 [V]) of vertices fp32 [V, 3] against the views of
    meshvis_views and the colour maps of meshcolor_maps by the rule of include/perf_hip_meshcolor.h: ONE launch for all views
    (perf_meshcolor_blend).  normals fp32 [V, 3] are read only with facing; fallback fp32 [V, 3] or None."""
    vertices = _dev_tensor('meshcolor_blend', 'vertices', vertices, torch.float32, ('V', 3))
    n, dev = int(vertices.shape[0]), vertices.device
    if facing and normals is None:
        raise _lib.PerfError('meshcolor_blend: facing needs normals')
    normals = _dev_tensor('meshcolor_blend', "the vertices' normals", normals, torch.float32, (n, 3), dev) if facing else None
    blend = _blend_args('meshcolor_blend', n, dev, views, sizes, map_pointers, tol, facing, power, select, fallback, fill)
    colors = torch.empty(n, 3, dtype=torch.float32, device=dev)
    weight = torch.empty(n, dtype=torch.float32, device=dev)
    used = torch.empty(n, dtype=torch.int64, device=dev)
    best = torch.empty(n, dtype=torch.int8, device=dev)
    _call('perf_meshcolor_blend', _pn(vertices), _pn(normals), n, *blend, _pn(colors), _pn(weight), _pn(used), _pn(best), _stream())
    return colors, weight, used, best


# ---- a texture atlas for a mesh: corner UVs, the texel -> point map, the fused bake (include/perf_hip_meshtex.h) ------------------------
def _tex_layout(who, n_faces, size, tile):
    s, t, f = int(size), int(tile), int(n_faces)
    if not _lib.MESHTEX_MIN_SIZE <= s <= _lib.MESHTEX_MAX_SIZE:
        raise _lib.PerfError(f'{who}: an atlas size of {s} is outside 64 .. 16384')
    if not _lib.MESHTEX_MIN_TILE <= t <= s:
        raise _lib.PerfError(f'{who}: a tile of {t} texels is outside 4 .. {s}')
    if f < 0 or f > 2 * (s // t) ** 2:
        raise _lib.PerfError(f'{who}: {f} faces are more than the {2 * (s // t) ** 2} an atlas of {s} with tiles of {t} holds')
    return s, t


def _tex_mesh(who, vertices, normals, faces, size, tile):
    """The head of a mesh in an atlas -> (vertices, V, S, the (vertices, V, normals, faces, F, S, T) a library call begins with)."""
    vertices, nv, f, (pv, _, pf, _) = _mesh_head(who, vertices, faces)
    s, t = _tex_layout(who, f, size, tile)
    normals = _dev_tensor(who, "the vertices' normals", normals, torch.float32, (nv, 3), vertices.device)
    return vertices, nv, s, (pv, nv, _pn(normals), pf, f, s, t)


def meshtex_uv(n_faces, size, tile, device='cuda'):
    """The corner UVs fp32 [F, 3, 2] of the atlas layout of include/perf_hip_meshtex.h (perf_meshtex_uv)."""
    f = int(n_faces)
    s, t = _tex_layout('meshtex_uv', f, size, tile)
    if torch.device(device).type != 'cuda':
        raise _lib.PerfError('meshtex_uv: device must be a CUDA device (there is no CPU path)')
    uv = torch.empty(f, 3, 2, dtype=torch.float32, device=device)
    _call('perf_meshtex_uv', f, s, t, _pn(uv), _stream())
    return uv


def meshtex_points(vertices, faces, size, tile, normals=None, flag=None):
    """The texels' points of the atlas (perf_meshtex_points) -> (points fp32 [S * S, 3], point_normals fp32 [S * S, 3], face_of int32
    [S * S], coverage uint8 [S * S], flag): normals fp32 [V, 3] are interpolated, None takes the faces' own; flag = int64 [1] ON THE DEVICE,
    the smallest index of a face with an index outside [0, V) or -1 (an int64 [1] view to write it into may be passed)."""
    vertices, nv, s, head = _tex_mesh('meshtex_points', vertices, normals, faces, size, tile)
    dev = vertices.device
    points = torch.empty(s * s, 3, dtype=torch.float32, device=dev)
    point_normals = torch.empty(s * s, 3, dtype=torch.float32, device=dev)
    face_of = torch.empty(s * s, dtype=torch.int32, device=dev)
    coverage = torch.empty(s * s, dtype=torch.uint8, device=dev)
    flag = _flag('meshtex_points', 'flag', flag, 1, dev)
    _call('perf_meshtex_points', *head, _p(points), _p(point_normals), _p(face_of), _p(coverage), _p(flag), _stream())
    return points, point_normals, face_of, coverage, flag


def meshtex_bake(vertices, faces, size, tile, views, sizes, map_pointers, tol, normals=None, facing=True, power=2, select='blend', fallback=None,
                 fill=(0.5, 0.5, 0.5), flag=None):
    """The fused bake (perf_meshtex_bake): the texels' points through the blend of include/perf_hip_meshcolor.h in ONE launch -> (image fp32
    [S, S, 3], weight fp32 [S, S], used_bits int64 [S, S], coverage uint8 [S, S], flag).  views, sizes, map_pointers: of meshvis_views and
    meshcolor_maps; normals, fallback: fp32 [V, 3] or None."""
    vertices, nv, s, head = _tex_mesh('meshtex_bake', vertices, normals, faces, size, tile)
    dev = vertices.device
    blend = _blend_args('meshtex_bake', nv, dev, views, sizes, map_pointers, tol, facing, power, select, fallback, fill)
    image = torch.empty(s, s, 3, dtype=torch.float32, device=dev)
    weight = torch.empty(s, s, dtype=torch.float32, device=dev)
    used = torch.empty(s, s, dtype=torch.int64, device=dev)
    coverage = torch.empty(s, s, dtype=torch.uint8, device=dev)
    flag = _flag('meshtex_bake', 'flag', flag, 1, dev)
    _call('perf_meshtex_bake', *head, *blend, _p(image), _p(weight), _p(used), _p(coverage), _p(flag), _stream())
    return image, weight, used, coverage, flag


# ---- rays against a mesh on a uniform grid: closest hit, any hit, segment occlusion (include/perf_hip_meshray.h) -------------------------
def _ray_box(who, origin, cell, dims):
    """(origin fp32 [3], cell fp32, dims int32 [3]) as the library takes them, and the number of cells."""
    o3, d3 = [float(v) for v in origin], [int(v) for v in dims]
    if len(o3) != 3 or len(d3) != 3:
        raise _lib.PerfError(f'{who}: origin and dims hold three values each')
    if any(v < 1 for v in d3) or d3[0] * d3[1] * d3[2] > _lib.MESHRAY_MAX_CELLS:
        raise _lib.PerfError(f'{who}: a grid of {d3} cells has a dimension below 1 or more than 2^24 cells')
    return ((ctypes.c_float * 3)(*o3), float(cell), (ctypes.c_int32 * 3)(*d3)), d3[0] * d3[1] * d3[2]


def _ray_grid(who, vertices, faces, origin, cell, dims, offsets, refs):
    """A mesh in its grid of face lists -> (vertices, V, the arguments a library call begins with, from the vertices to the number of
    references)."""
    vertices, nv, f, mesh = _mesh_head(who, vertices, faces, _lib.MESHRAY_MAX_FACES)
    box, n_cells = _ray_box(who, origin, cell, dims)
    offsets = _dev_tensor(who, 'offsets', offsets, torch.int32, (n_cells,), vertices.device)
    refs = _dev_tensor(who, 'refs', refs, torch.int32, ('R',), vertices.device)
    return vertices, nv, (*mesh, *box, _p(offsets), _pn(refs), int(refs.numel()))


def meshray_grid_count(vertices, faces, origin, cell, dims, flag=None):
    """How many faces each cell of the grid (origin [3], cell edge, dims [3]) lists, by the range rule of include/perf_hip_meshray.h
    (perf_meshray_grid_count) -> (counts int32 [nx * ny * nz], flag): flag = int64 [1] ON THE DEVICE, the smallest index of a face with an
    index outside [0, V) or a vertex that is not finite, or -1 (an int64 [1] view to write it into may be passed)."""
    vertices, nv, f, mesh = _mesh_head('meshray_grid_count', vertices, faces, _lib.MESHRAY_MAX_FACES)
    box, n_cells = _ray_box('meshray_grid_count', origin, cell, dims)
    counts = torch.empty(n_cells, dtype=torch.int32, device=vertices.device)
    flag = _flag('meshray_grid_count', 'flag', flag, 1, vertices.device)
    _call('perf_meshray_grid_count', *mesh, *box, _p(counts), _p(flag), _stream())
    return counts, flag


def meshray_grid_write(vertices, faces, origin, cell, dims, counts, offsets, n_refs):
    """refs int32 [n_refs]: the faces of every cell, cell c's at offsets[c] .. offsets[c] + its count, in no particular order
    (perf_meshray_grid_write).  counts: what meshray_grid_count returned, left 0; offsets: their exclusive scan; n_refs: its total."""
    vertices, nv, f, mesh = _mesh_head('meshray_grid_write', vertices, faces, _lib.MESHRAY_MAX_FACES)
    box, n_cells = _ray_box('meshray_grid_write', origin, cell, dims)
    counts = _dev_tensor('meshray_grid_write', 'counts', counts, torch.int32, (n_cells,), vertices.device)
    offsets = _dev_tensor('meshray_grid_write', 'offsets', offsets, torch.int32, (n_cells,), vertices.device)
    r = int(n_refs)
    refs = torch.empty(max(r, 0), dtype=torch.int32, device=vertices.device)
    _call('perf_meshray_grid_write', *mesh, *box, _p(counts), _p(offsets), r, _pn(refs), int(refs.numel()), _stream())
    return refs


def meshray_cast(vertices, faces, origin, cell, dims, offsets, refs, rays_o, rays_d, t_min=0.0, t_max=float('inf'), any_hit=False, uv=True):
    """The closest hit of every ray -> (t fp32 [N], face int32 [N], u, v fp32 [N] or None without uv), or with any_hit the uint8 [N] flag
    alone, by the rule of include/perf_hip_meshray.h over the grid meshray_grid_write made of the SAME mesh (perf_meshray_cast)."""
    vertices, nv, grid = _ray_grid('meshray_cast', vertices, faces, origin, cell, dims, offsets, refs)
    dev = vertices.device
    rays_o = _dev_tensor('meshray_cast', 'rays_o', rays_o, torch.float32, ('N', 3), dev)
    n = int(rays_o.shape[0])
    rays_d = _dev_tensor('meshray_cast', 'rays_d', rays_d, torch.float32, (n, 3), dev)
    hit = t = face = u = v = None
    if any_hit:
        hit = torch.empty(n, dtype=torch.uint8, device=dev)
    else:
        t, face = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        if uv:
            u, v = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    _call('perf_meshray_cast', *grid, _pn(rays_o), _pn(rays_d), n, float(t_min), float(t_max), int(bool(any_hit)), _pn(t), _pn(face), _pn(u), _pn(v), _pn(hit),
          _stream())
    return hit if any_hit else (t, face, u, v)


def meshray_occluded(vertices, faces, origin, cell, dims, offsets, refs, centres, mask_bits):
    """occluded_bits int64 [V]: bit k iff bit k of mask_bits is set and a face that does not name the vertex cuts the segment from the vertex
    to centres[k] (fp32 [K, 3], K <= 64) at a strict 0 < t < 1 (perf_meshray_occluded)."""
    vertices, nv, grid = _ray_grid('meshray_occluded', vertices, faces, origin, cell, dims, offsets, refs)
    centres, k = _centres('meshray_occluded', centres)
    if k > _lib.MESHRAY_MAX_VIEWS:
        raise _lib.PerfError(f'meshray_occluded: {k} views are more than {_lib.MESHRAY_MAX_VIEWS} (a vertex has one bit per view in a 64-bit word)')
    mask_bits = _dev_tensor('meshray_occluded', 'mask_bits', mask_bits, torch.int64, (nv,), vertices.device)
    out = torch.empty(nv, dtype=torch.int64, device=vertices.device)
    _call('perf_meshray_occluded', *grid, _pn(centres), k, _pn(mask_bits), _pn(out), _stream())
    return out


# ---- the closest point of a mesh to each query point, on the same grid (include/staged/perf_hip_meshnear.h) ------------------------------
def meshnear_query(vertices, faces, origin, cell, dims, offsets, refs, points, max_distance=float('inf'), uv=True):
    """The closest point of the mesh to every point -> (dist2 float64 [N], face int32 [N], u, v fp32 [N] or None without uv): the
    lexicographic minimum of (dist2, face index) over ALL faces by the rule of include/staged/perf_hip_meshnear.h, searched over the grid
    meshray_grid_write made of the SAME mesh; +inf, -1, 0, 0 for a point that is not finite, for a mesh without a valid face and beyond
    max_distance (perf_meshnear_query)."""
    vertices, nv, grid = _ray_grid('meshnear_query', vertices, faces, origin, cell, dims, offsets, refs)
    dev = vertices.device
    points = _dev_tensor('meshnear_query', 'points', points, torch.float32, ('N', 3), dev)
    n = int(points.shape[0])
    limit = float(max_distance)
    if not limit >= 0.0:
        raise _lib.PerfError(f'meshnear_query: max_distance ({max_distance}) is NaN or negative')
    dist2, face = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    u = v = None
    if uv:
        u, v = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    _call('perf_meshnear_query', *grid, _pn(points), n, limit, _pn(dist2), _pn(face), _pn(u), _pn(v), _stream())
    return dist2, face, u, v


def normal_composite(weights, grad, packed):
    """normal [R,3] = unit(sum_i w_i * (-grad_i / |grad_i|)) per ray, exactly zero for rays without samples (perf_normal_composite)."""
    R = packed.shape[0]
    out = torch.empty(R, 3, dtype=torch.float32, device=weights.device)
    _call('perf_normal_composite', _p(_f32(weights, 'weights')), _p(_f32(grad, 'grad')), _p(packed), R, _p(out), _stream())
    return out


class PairFeat(NamedTuple):
    """The two level-major feature arrays [L, n, 2] of one pair encode (hashgrid_fwd_pair): field 0's and field 1's, same samples."""
    a: torch.Tensor
    b: torch.Tensor


class IndexedFeat(NamedTuple):
    """Level-major features [L, n_src, 2] of MORE samples than the caller means, and the row of each sample it does mean
    (int32 [n]; rows past the live count are not read): what compact_prefix(index_features=True) hands to the gradient pass
    instead of a compacted copy (perf_mlp_bwd's feat_index)."""
    feat: torch.Tensor
    index: torch.Tensor

    def materialize(self):
        """The compacted copy after all ([L, n, 2]; rows past the live count repeat a valid row)."""
        return self.feat.index_select(1, self.index.long().clamp_(0, self.feat.shape[1] - 1))


def mlp_bwd(mlp: MlpConfig, w16, feat16, dout, sel=None, need_dfeat=True, want_absmax=False, n_dev=None, dw_out=None):
    """Returns (dfeat [L,n,2] f32 or None, dw [n_net_params] f32[, level_absmax [16] f32]).  dw_out: write the weight gradient
    there (e.g. the head of a flat [network | grid] gradient) instead of into a fresh tensor.  feat16: [L, n, 2] or an
    IndexedFeat (n = its index's length)."""
    index, stride = None, 0
    if isinstance(feat16, IndexedFeat):
        feat16, index = feat16.feat, feat16.index
        assert index.dtype == torch.int32 and index.is_contiguous() and feat16.is_contiguous()
        stride = feat16.shape[1]
    n = index.shape[0] if index is not None else feat16.shape[1]
    d = mlp.desc()
    lib = _lib.load()
    ws_bytes = lib.perf_mlp_bwd_workspace_bytes(ctypes.byref(d), n)
    ws = torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=feat16.device)
    dfeat = torch.empty(mlp.n_levels, n, 2, dtype=torch.float32, device=feat16.device) if need_dfeat else None
    dw = dw_out if dw_out is not None else torch.empty(mlp.n_params, dtype=torch.float32, device=feat16.device)
    amax = torch.empty(_lib.MAX_LEVELS, dtype=torch.float32, device=feat16.device) if want_absmax else None
    _call('perf_mlp_bwd', ctypes.byref(d), _p(w16), _p(feat16), _p(index), stride, _p(sel), _p(_f32(dout, 'dout')), _p(dfeat), _p(dw),
          _p(amax), _p(ws), ws.numel() * 4, n, _nd(n_dev), dtype_code(w16.dtype), _stream())
    return (dfeat, dw, amax) if want_absmax else (dfeat, dw)


# ---- rays ----------------------------------------------------------------------------------------
def pano_raygen(pose, height, width, row0=0, nrows=None, device='cuda'):
    nrows = height - row0 if nrows is None else nrows
    pose_h = (ctypes.c_float * 16)(*[float(v) for v in torch.as_tensor(pose).detach().cpu().reshape(-1).tolist()])
    o = torch.empty(nrows, width, 3, dtype=torch.float32, device=device)
    d = torch.empty(nrows, width, 3, dtype=torch.float32, device=device)
    _call('perf_pano_raygen', pose_h, height, width, row0, nrows, _p(o), _p(d), _stream())
    return o, d


def pano_raygen_dev(pose_dev, height, width, row0=0, nrows=None, out=None):
    """pano_raygen with the pose (float32 [4,4] or [12+]) in device memory; `out` = (o, d) preallocated [nrows*width,3] buffers
    (a captured hipGraph writes the same buffers on every replay)."""
    nrows = height - row0 if nrows is None else nrows
    dev = pose_dev.device
    if out is None:
        o = torch.empty(nrows, width, 3, dtype=torch.float32, device=dev)
        d = torch.empty(nrows, width, 3, dtype=torch.float32, device=dev)
    else:
        o, d = out
    _call('perf_pano_raygen_dev', _p(_f32(pose_dev, 'pose')), height, width, row0, nrows, _p(o), _p(d), _stream())
    return o, d


def _pose16(pose):
    vals = [float(v) for v in torch.as_tensor(pose).detach().cpu().reshape(-1).tolist()]
    if len(vals) not in (12, 16):
        raise _lib.PerfError(f'pose must be a [4,4] or [3,4] matrix, got {len(vals)} values')
    return (ctypes.c_float * 16)(*vals)


def _ray_bufs(out, nrows, width, dev):
    if out is None:
        return (torch.empty(nrows, width, 3, dtype=torch.float32, device=dev),
                torch.empty(nrows, width, 3, dtype=torch.float32, device=dev))
    o, d = out
    for t in (o, d):
        if _f32(t, 'rays').numel() < nrows * width * 3:
            raise _lib.PerfError(f'ray buffer of {t.numel()} floats for {nrows}x{width} rays')
    return o, d


def pers_raygen(pose, height, width, fovy, row0=0, nrows=None, device='cuda'):
    """gen_pers_rays / cam_rays_cam_space (utils/camera_utils.py:60-80, 237-241) for rows [row0, row0+nrows) of a height x width
    perspective frame of vertical field of view fovy (radians): -> (o, d) [nrows, width, 3].  pose [4,4] or [3,4] on any device."""
    nrows = height - row0 if nrows is None else nrows
    o, d = _ray_bufs(None, nrows, width, device)
    _call('perf_pers_raygen', _pose16(pose), height, width, float(fovy), row0, nrows, _p(o), _p(d), _stream())
    return o, d


def pers_raygen_dev(pose_dev, height, width, fovy, row0=0, nrows=None, out=None):
    """pers_raygen with the pose (float32 [4,4] or [12+]) in device memory; `out` = (o, d) preallocated [nrows*width,3] buffers
    (a captured hipGraph writes the same buffers on every replay)."""
    nrows = height - row0 if nrows is None else nrows
    if _f32(pose_dev, 'pose').numel() < 12:
        raise _lib.PerfError('pose_dev must hold at least 12 floats (row major 3x4)')
    o, d = _ray_bufs(out, nrows, width, pose_dev.device)
    _call('perf_pers_raygen_dev', _p(pose_dev), height, width, float(fovy), row0, nrows, _p(o), _p(d), _stream())
    return o, d


# ---- occupancy marching ----------------------------------------------------------------------------
def occ_pack_bits(binaries: torch.Tensor) -> torch.Tensor:
    b = binaries.reshape(-1)
    if b.dtype == torch.bool:
        b = b.view(torch.uint8)
    n = b.numel()
    bits = torch.empty((n + 31) // 32, dtype=torch.int32, device=b.device)
    _call('perf_occ_pack_bits', _p(b), _p(bits), n, _stream())
    return bits


def occ_jitter_points(seed, call, cell_lo, n, res, aabb, device, out=None):
    """Jittered evaluation points of cells [cell_lo, cell_lo + n) of a res^3 grid -> x [n, 3] (perf_occ_jitter_points)."""
    x = out if out is not None else torch.empty(n, 3, dtype=torch.float32, device=device)
    _call('perf_occ_jitter_points', int(seed) & 0xFFFFFFFFFFFFFFFF, int(call), int(cell_lo), int(n), int(res), _aabb6(aabb), _p(x), _stream())
    return x


def occ_ema_update(occs, occ, ema_decay, sum_out):
    """In place occs = max(occs * ema_decay, occ); sum_out (device float64 [1]) += the new values."""
    if sum_out.dtype != torch.float64:
        raise _lib.PerfError('sum_out must be float64')
    _call('perf_occ_ema_update', _p(_f32(occs, 'occs')), _p(_f32(occ, 'occ')), occs.numel(), float(ema_decay), _p(sum_out), _stream())


def occ_threshold(occs, sum_dev, occ_thre, out=None):
    """-> bool [n]: occs > min(sum / n, occ_thre)."""
    b = out if out is not None else torch.empty(occs.numel(), dtype=torch.bool, device=occs.device)
    _call('perf_occ_threshold', _p(_f32(occs, 'occs')), occs.numel(), _p(sum_dev), float(occ_thre), _p(b.view(torch.uint8)), _stream())
    return b


def exclusive_scan_i32(counts: torch.Tensor, bias=None):
    """-> (offsets, total int64 [1]); with `bias` (host int) also total + bias as a third result (same launch)."""
    n = counts.numel()
    lib = _lib.load()
    out = torch.empty_like(counts)
    totals = torch.empty(2, dtype=torch.int64, device=counts.device)
    ws = torch.empty(lib.perf_scan_workspace_bytes(n) // 8 + 1, dtype=torch.int64, device=counts.device)
    _call('perf_exclusive_scan_i32', _p(counts), _p(out), _p(totals), n, int(bias or 0), _p(totals[1:]) if bias is not None else None,
          _p(ws), ws.numel() * 8, _stream())
    return (out, totals[:1]) if bias is None else (out, totals[:1], totals[1:])


def occ_build_coarse(occ_bits, res):
    """Dilated 4^3-block occupancy for the marching kernel's empty-space skip (None when res % 8 != 0)."""
    words = _lib.load().perf_occ_coarse_words(int(res))
    if words == 0:
        return None
    coarse = torch.empty(words, dtype=torch.int32, device=occ_bits.device)
    _call('perf_occ_build_coarse', _p(occ_bits), int(res), _p(coarse), _stream())
    return coarse


def _origin(t0):
    """Lattice-origin argument of the marching entry points -> (pointer, t0_scale, t0_base).  t0: a float32 tensor [R] (origins
    as given), or a tuple (u, scale, base[, table]): u = stratified draws [R] or None; origin = u * scale (+ base), resp. base."""
    if isinstance(t0, tuple):
        u, scale, base = t0[:3]
        return (_p(_f32(u, 't0')) if u is not None else None), float(scale if u is not None else 0.0), float(base)
    return _p(_f32(t0, 't0')), 0.0, 0.0


def _lat_table(t0):
    """The `lattice_table` argument of the marching entry points: t0 = (None, scale, base, table): the precomputed lattice of a
    launch whose rays all start at the same origin (lattice_table()); t0 = (u, scale, base, runs): the per-ray tables of runs of
    a stratified batch (lattice_runs(), int32); None otherwise."""
    if isinstance(t0, tuple) and len(t0) > 3 and t0[3] is not None:
        if t0[0] is None:
            return _p(_f32(t0[3], 'lattice_table'))
        if t0[3].dtype != torch.int32:
            raise _lib.PerfError('per-ray lattice runs must be int32 (ops.lattice_runs)')
        return _p(t0[3])
    return None


def lattice_runs(t0, step, max_steps, n_rays=None):
    """Per-ray tables of runs of the repeated-addition lattice for a batch with per-ray origins (perf_occ_lattice_runs: one lane per
    ray).  t0: a float32 tensor of origins or a tuple (u, scale, base) -- see _origin.  -> int32 tensor to append to the tuple as its
    fourth element: (u, scale, base, runs)."""
    u = t0[0] if isinstance(t0, tuple) else t0
    n = int(u.shape[0]) if n_rays is None else int(n_rays)
    out = torch.empty(_lib.load().perf_occ_lattice_runs_len(n), dtype=torch.int32, device=u.device)
    _call('perf_occ_lattice_runs', *_origin(t0), n, float(step), int(max_steps), _p(out), _stream())
    return out


def lattice_table(t0_base, step, max_steps, lattice=None, device='cuda'):
    """t_k of the lattice that starts at t0_base, for every k a marching launch of `max_steps` intervals can ask for
    (perf_occ_lattice_table) -- pass it as the fourth element of a (None, 0.0, t0_base, table) origin."""
    n = _lib.load().perf_occ_lattice_table_len(int(max_steps))
    out = torch.empty(n, dtype=torch.float32, device=device)
    _call('perf_occ_lattice_table', float(t0_base), float(step), int(max_steps), _lib.LATTICE[lattice], _p(out), _stream())
    return out


def occ_march_count(rays_o, rays_d, t0, occ_bits, res, aabb, far_plane, step, max_steps, occ_coarse=None, lattice=None):
    """Pass 1 of the marching: -> (keep masks, per-ray counts int32 [R]).  t0: see _origin."""
    R = rays_o.shape[0]
    dev = rays_o.device
    mw = _lib.load().perf_occ_mask_words(max_steps)
    masks = torch.empty(max(R * mw, 1), dtype=torch.int64, device=dev)
    counts = torch.empty(R, dtype=torch.int32, device=dev)
    _call('perf_occ_march_count', _p(_f32(rays_o, 'rays_o')), _p(_f32(rays_d, 'rays_d')), *_origin(t0), R,
          _p(occ_bits), _p(occ_coarse), int(res), _aabb6(aabb), float(far_plane), float(step), int(max_steps), _lib.LATTICE[lattice],
          _lat_table(t0), _p(masks), _p(counts), _stream())
    return masks, counts


def occ_march_count_head(rays_o, rays_d, t0, occ_bits, res, aabb, far_plane, step, max_steps, occ_coarse, head_k, points_aabb,
                         lattice=None):
    """occ_march_count that also writes the first head_k samples of every ray to rows r*head_k.. of R*head_k-row arrays
    (padding rows have sel = 0) -> (masks, counts, (ray_indices, t_starts, t_ends, packed_info, x01, sel))."""
    R = rays_o.shape[0]
    dev = rays_o.device
    mw = _lib.load().perf_occ_mask_words(max_steps)
    masks = torch.empty(max(R * mw, 1), dtype=torch.int64, device=dev)
    counts = torch.empty(R, dtype=torch.int32, device=dev)
    S = R * int(head_k)
    ri = torch.empty(S, dtype=torch.int64, device=dev)
    ts = torch.empty(S, dtype=torch.float32, device=dev)
    te = torch.empty(S, dtype=torch.float32, device=dev)
    packed = torch.empty(R, 2, dtype=torch.int32, device=dev)
    x01 = torch.empty(S, 3, dtype=torch.float32, device=dev)
    sel = torch.empty(S, dtype=torch.uint8, device=dev)
    _call('perf_occ_march_count_head', _p(_f32(rays_o, 'rays_o')), _p(_f32(rays_d, 'rays_d')), *_origin(t0), R,
          _p(occ_bits), _p(occ_coarse), int(res), _aabb6(aabb), float(far_plane), float(step), int(max_steps), _lib.LATTICE[lattice],
          _lat_table(t0), _p(masks), _p(counts), int(head_k), _p(ri), _p(ts), _p(te), _p(packed), _aabb6(points_aabb), _p(x01), _p(sel), _stream())
    return masks, counts, (ri, ts, te, packed, x01, sel)


def occ_march_write(t0, masks, counts, offsets, S, step, max_steps, rays_o=None, rays_d=None, points_aabb=None, rank_lo=0,
                    lattice=None):
    """Pass 2: expand the masks into S-row sample arrays -> (ray_indices, t_starts, t_ends, packed_info[, x01, sel]).
    counts / offsets: how many samples of every ray to write, starting at rank rank_lo, and where."""
    R = counts.shape[0]
    dev = counts.device
    ri = torch.empty(S, dtype=torch.int64, device=dev)
    ts = torch.empty(S, dtype=torch.float32, device=dev)
    te = torch.empty(S, dtype=torch.float32, device=dev)
    packed = torch.empty(R, 2, dtype=torch.int32, device=dev)
    if points_aabb is not None:
        x01 = torch.empty(S, 3, dtype=torch.float32, device=dev)
        sel = torch.empty(S, dtype=torch.uint8, device=dev)
        _call('perf_occ_march_write_points', *_origin(t0), R, float(step), int(max_steps), _lib.LATTICE[lattice], _lat_table(t0), _p(masks), _p(counts), _p(offsets), S,
              _p(ri), _p(ts), _p(te), _p(packed), _p(rays_o), _p(rays_d), _aabb6(points_aabb), _p(x01), _p(sel), int(rank_lo), _stream())
        return ri, ts, te, packed, x01, sel
    if rank_lo != 0:
        raise _lib.PerfError('rank_lo needs points_aabb (perf_occ_march_write_points)')
    _call('perf_occ_march_write', *_origin(t0), R, float(step), int(max_steps), _lib.LATTICE[lattice], _lat_table(t0), _p(masks), _p(counts), _p(offsets), S,
          _p(ri), _p(ts), _p(te), _p(packed), _stream())
    return ri, ts, te, packed


def occ_march(rays_o, rays_d, t0, occ_bits, res, aabb, far_plane, step, max_steps, capacity=None, occ_coarse=None,
              points_aabb=None, lattice=None):
    """Returns (ray_indices i64 [S], t_starts, t_ends f32 [S], packed_info i32 [R,2]).
    capacity=None reads the total back (one host sync, like the reference's boolean indexing);
    an int capacity keeps the call sync-free and returns arrays of that length plus `total` on device.
    points_aabb (6 floats): also return the sample positions (x01 [S,3], sel [S]) normalised to that box, written by
    the same kernel that writes the samples (appended to the result)."""
    masks, counts = occ_march_count(rays_o, rays_d, t0, occ_bits, res, aabb, far_plane, step, max_steps, occ_coarse, lattice=lattice)
    offsets, total = exclusive_scan_i32(counts)
    S = int(total.item()) if capacity is None else int(capacity)
    out = occ_march_write(t0, masks, counts, offsets, S, step, max_steps, rays_o, rays_d, points_aabb, lattice=lattice)
    if capacity is None:
        return out
    return out[:4] + (total,) + out[4:]


def head_tail_counts(counts, head_samples, kept_head=None):
    """kept_head None: min(counts, K); else the tail counts of the rays whose whole head survived (0 for decided rays)."""
    out = torch.empty_like(counts)
    _call('perf_head_tail_counts', _p(counts), counts.shape[0], int(head_samples), _p(kept_head), _p(out), _stream())
    return out


def visibility_count2(head, tail, early_stop_eps=1e-4):
    """head / tail = (sigmas, t_starts, t_ends, packed_info) of the two sample sets -> kept counts int32 [R]."""
    R = head[3].shape[0]
    thr = float(-math.log(early_stop_eps)) if early_stop_eps > 0 else float('inf')
    new_counts = torch.empty(R, dtype=torch.int32, device=head[3].device)
    _call('perf_visibility_count2', _p(head[0]), _p(head[1]), _p(head[2]), _p(head[3]), _p(tail[0]), _p(tail[1]), _p(tail[2]), _p(tail[3]),
          R, thr, _p(new_counts), _stream())
    return new_counts


def compact_prefix2(head, tail, new_counts, capacity, feat_h=None, feat_t=None):
    """head / tail = (sigmas, t_starts, t_ends, packed_info, x01, sel) -> (ray_indices, t_starts, t_ends, sigmas, packed_info,
    total, x01, sel[, feat]) with `capacity` rows; feat_h / feat_t: level-major features of the two sample sets."""
    R = new_counts.shape[0]
    dev = new_counts.device
    new_offsets, total = exclusive_scan_i32(new_counts)
    S = int(capacity)
    ri = torch.empty(S, dtype=torch.int64, device=dev)
    ts = torch.empty(S, dtype=torch.float32, device=dev)
    te = torch.empty(S, dtype=torch.float32, device=dev)
    sg = torch.empty(S, dtype=torch.float32, device=dev)
    xo = torch.empty(S, 3, dtype=torch.float32, device=dev)
    so = torch.empty(S, dtype=torch.uint8, device=dev)
    packed_out = torch.empty(R, 2, dtype=torch.int32, device=dev)
    fo = torch.empty(feat_h.shape[0], S, 2, dtype=feat_h.dtype, device=dev) if feat_h is not None else None
    _call('perf_compact_prefix2', _p(head[0]), _p(head[1]), _p(head[2]), _p(head[3]), _p(head[4]), _p(head[5]),
          _p(tail[0]), _p(tail[1]), _p(tail[2]), _p(tail[3]), _p(tail[4]), _p(tail[5]), _p(new_counts), _p(new_offsets), R, S,
          _p(ri), _p(ts), _p(te), _p(sg), _p(xo), _p(so), _p(packed_out),
          _p(feat_h), feat_h.shape[1] if feat_h is not None else 0, _p(feat_t), feat_t.shape[1] if feat_t is not None else 0,
          _p(fo), S, feat_h.shape[0] if feat_h is not None else 0, _stream())
    res = (ri, ts, te, sg, packed_out, total, xo, so)
    return res + (fo,) if fo is not None else res


# ---- compositing -----------------------------------------------------------------------------------
def visibility_count(sigmas, t_starts, t_ends, packed, early_stop_eps=1e-4, want_exsum=False, march_counts=None, head_samples=0):
    """-> kept counts int32 [R] (+ exsum); with march_counts / head_samples also the two-phase sampler's tail counts (same
    launch): (kept, tail_counts)."""
    R = packed.shape[0]
    thr = float(-math.log(early_stop_eps)) if early_stop_eps > 0 else float('inf')
    new_counts = torch.empty(R, dtype=torch.int32, device=packed.device)
    ex = torch.empty_like(sigmas) if want_exsum else None
    tail = torch.empty(R, dtype=torch.int32, device=packed.device) if march_counts is not None else None
    _call('perf_visibility_count', _p(_f32(sigmas, 'sigmas')), _p(t_starts), _p(t_ends), _p(packed), R, thr,
              _p(new_counts), _p(ex), _p(march_counts), int(head_samples), _p(tail), _stream())
    if march_counts is not None:
        return new_counts, tail
    return (new_counts, ex) if want_exsum else new_counts


INDEX_FEATURES = True      # compact_prefix: rows instead of a feature copy (index_features=False: the copy, tests)


def compact_prefix(packed, new_counts, t_starts, t_ends, sigmas=None, capacity=None, x01=None, sel=None, feat=None,
                   index_features=None):
    """-> (ray_indices, t_starts, t_ends, sigmas, packed_info) of the kept prefixes; with capacity (sync-free mode: the
    arrays keep that length, the kept count stays on the device) also `total` (int64 [1]); with x01/sel also the compacted
    positions, appended to the result; with feat (level-major features of all input samples) their compacted copy or --
    index_features (the default) -- an IndexedFeat that points into `feat` (which must then outlive it)."""
    R = packed.shape[0]
    dev = packed.device
    new_offsets, total = exclusive_scan_i32(new_counts)
    S = int(total.item()) if capacity is None else int(capacity)
    ri = torch.empty(S, dtype=torch.int64, device=dev)
    ts = torch.empty(S, dtype=torch.float32, device=dev)
    te = torch.empty(S, dtype=torch.float32, device=dev)
    sg = torch.empty(S, dtype=torch.float32, device=dev) if sigmas is not None else None
    xo = torch.empty(S, 3, dtype=torch.float32, device=dev) if x01 is not None else None
    so = torch.empty(S, dtype=torch.uint8, device=dev) if sel is not None else None
    packed_out = torch.empty(R, 2, dtype=torch.int32, device=dev)
    by_index = feat is not None and (INDEX_FEATURES if index_features is None else index_features)
    fo = torch.empty(feat.shape[0], S, 2, dtype=feat.dtype, device=dev) if (feat is not None and not by_index) else None     # level major like feat
    fi = torch.empty(S, dtype=torch.int32, device=dev) if by_index else None
    _call('perf_compact_prefix', _p(packed), _p(new_counts), _p(new_offsets), R, _p(t_starts), _p(t_ends), _p(sigmas),
          _p(ri), _p(ts), _p(te), _p(sg), _p(packed_out), _p(x01), _p(sel), _p(xo), _p(so),
          _p(feat if fo is not None else None), feat.shape[1] if fo is not None else 0, _p(fo), S, feat.shape[0] if fo is not None else 0,
          _p(fi), _stream())
    if by_index:
        fo = IndexedFeat(feat, fi)
    res = (ri, ts, te, sg, packed_out)
    if capacity is not None:
        res = res + (total,)
    if x01 is not None:
        res = res + (xo, so)
    if feat is not None:
        res = res + (fo,)
    return res


def composite_fwd(sigmas, rgbs, t_starts, t_ends, packed, want_samples=True):
    R = packed.shape[0]
    S = sigmas.numel()
    dev = sigmas.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    w = f(S) if want_samples else None
    T = f(S) if want_samples else None
    al = f(S) if want_samples else None
    op, dist = f(R, 1), f(R, 1)
    col = f(R, 3) if rgbs is not None else None
    _call('perf_composite_fwd', _p(_f32(sigmas, 'sigmas')), _p(rgbs), _p(t_starts), _p(t_ends), _p(packed), R, _p(w),
              _p(T), _p(al), _p(op), _p(dist), _p(col), _stream())
    return w, T, al, op, dist, col


def composite_distloss_fwd(sigmas, rgbs, t_starts, t_ends, packed):
    """composite_fwd + the per-ray distortion-loss sums in one launch -> (weights, trans, opacity, distance, colour, dl)."""
    R = packed.shape[0]
    S = sigmas.numel()
    dev = sigmas.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    w, T, op, dist, dl = f(S), f(S), f(R, 1), f(R, 1), f(R)
    col = f(R, 3) if rgbs is not None else None
    _call('perf_composite_distloss_fwd', _p(_f32(sigmas, 'sigmas')), _p(rgbs), _p(t_starts), _p(t_ends), _p(packed), R, _p(w),
          _p(T), _p(op), _p(dist), _p(col), _p(dl), _stream())
    return w, T, op, dist, col, dl


def composite_distloss_bwd(sigmas, t_starts, t_ends, packed, weights, trans, opacity, distance, g_opacity, g_distance,
                           scale=1.0, scale_dev=None):
    """d sigma of compositing with the distortion-loss gradient (scale * scale_dev[0] * d dl / d w) formed in the kernel."""
    ds = torch.empty(sigmas.numel(), dtype=torch.float32, device=sigmas.device)      # packed_info tiles [0, S): every sample is written
    _call('perf_composite_distloss_bwd', _p(sigmas), _p(t_starts), _p(t_ends), _p(packed), packed.shape[0], _p(weights), _p(trans),
          _p(opacity), _p(distance), _p(g_opacity), _p(g_distance), float(scale), _p(scale_dev), _p(ds), _stream())
    return ds


def composite_bwd(sigmas, t_starts, t_ends, packed, weights, trans, g_weights=None, g_opacity=None, g_distance=None,
                  g_color=None, g_trans=None, g_alphas=None, want_dsigma=True, want_drgb=False):
    R = packed.shape[0]
    S = sigmas.numel()
    dev = sigmas.device
    # (every sample of every ray is written by the kernel: no zero fill; rows beyond the live count of a capacity-sized batch
    #  stay uninitialised like everywhere else)
    ds = torch.empty(S, dtype=torch.float32, device=dev) if want_dsigma else None
    dr = torch.empty(S, 3, dtype=torch.float32, device=dev) if want_drgb else None
    _call('perf_composite_bwd', _p(sigmas), _p(t_starts), _p(t_ends), _p(packed), R, _p(weights), _p(trans),
              _p(g_weights), _p(g_trans), _p(g_alphas), _p(g_opacity), _p(g_distance), _p(g_color), _p(ds), _p(dr), _stream())
    return ds, dr


def render_finish_eval(opacity, distance=None, color=None, n_dev=None):
    """In place: distance += 5 (1 - opacity), color += 0.5 (1 - opacity) unless the batch (n_dev) holds no sample."""
    _call('perf_render_finish_eval', _p(_f32(opacity, 'opacity')), _p(distance), _p(color), opacity.shape[0], _nd(n_dev), _stream())


def accumulate_fwd(weights, values, packed):
    R = packed.shape[0]
    C = 1 if values is None else values.shape[-1]
    out = torch.empty(R, C, dtype=torch.float32, device=weights.device)
    _call('perf_accumulate_fwd', _p(_f32(weights, 'weights')), _p(values), _p(packed), R, C, _p(out), _stream())
    return out


def pack_info(ray_indices, n_rays):
    packed = torch.empty(n_rays, 2, dtype=torch.int32, device=ray_indices.device)
    _call('perf_pack_info', _p(ray_indices), ray_indices.numel(), n_rays, _p(packed), _stream())
    return packed


def distloss_fwd(w, t_starts, t_ends, packed):
    R = packed.shape[0]
    loss = torch.empty(R, dtype=torch.float32, device=w.device)
    _call('perf_distloss_fwd', _p(_f32(w, 'w')), _p(t_starts), _p(t_ends), _p(packed), R, _p(loss), _stream())
    return loss


def distloss_bwd(w, t_starts, t_ends, packed, scale, scale_dev=None):
    R = packed.shape[0]
    g = torch.zeros_like(w)
    _call('perf_distloss_bwd', _p(_f32(w, 'w')), _p(t_starts), _p(t_ends), _p(packed), R, float(scale), _p(scale_dev), _p(g), _stream())
    return g


_TICKETS = {}


def _ticket(device):
    """A zeroed device int32 per device for kernels that elect their last workgroup (left at zero by every call; the callers
    are serial on their stream)."""
    key = str(device)
    t = _TICKETS.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=device)
        if torch.cuda.is_current_stream_capturing():
            return t               # (created inside a capture: zero-filled by the graph itself on every replay)
        _TICKETS[key] = t
    return t


def geo_loss(opacity, distance, gt_distance, noise, distloss_per_ray, packed, global_batch, depth_weight, distortion_weight,
             ratio_dev, loss_scale):
    """-> (g_opacity [R,1], g_distance [R,1], scalars [3] = depth loss, distortion loss, distloss-backward scale)."""
    R = packed.shape[0]
    dev = opacity.device
    g_op = torch.empty(R, 1, dtype=torch.float32, device=dev); g_d = torch.empty(R, 1, dtype=torch.float32, device=dev)
    sc = torch.empty(_lib.LOSS_SCALARS, dtype=torch.float32, device=dev)
    _call('perf_geo_loss', _p(opacity), _p(distance), _p(_f32(gt_distance.contiguous(), 'gt')), _p(noise), _p(distloss_per_ray), _p(packed), R,
          int(global_batch), float(depth_weight), float(distortion_weight), _p(ratio_dev), float(loss_scale), _p(g_op), _p(g_d), _p(sc),
          _p(_ticket(dev)), _stream())
    return g_op, g_d, sc


def app_loss(opacity, color, bg_color, gt_color, global_batch, color_weight, loss_scale):
    """-> (g_color [R,3], scalars [1] = colour loss)."""
    R = opacity.shape[0]
    g_c = torch.empty(R, 3, dtype=torch.float32, device=opacity.device)
    sc = torch.empty(_lib.LOSS_SCALARS, dtype=torch.float32, device=opacity.device)
    _call('perf_app_loss', _p(opacity), _p(color), _p(bg_color), _p(_f32(gt_color.contiguous(), 'gt')), R, int(global_batch), float(color_weight),
          float(loss_scale), _p(g_c), _p(sc), _stream())
    return g_c, sc


def train_head_geo(sigmas, rgbs, t_starts, t_ends, packed, gt_distance, noise, global_batch, depth_weight, distortion_weight,
                   ratio_dev, loss_scale):
    """The ray head of the geometry step in ONE launch (perf_train_head_geo = composite_distloss_fwd -> geo_loss ->
    composite_distloss_bwd) -> dict(weights, trans, opacity, distance, color, depth_terms, distloss_per_ray, inv_n, d_sigma)."""
    R = packed.shape[0]
    S = sigmas.numel()
    dev = sigmas.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    o = dict(weights=f(S), trans=f(S), opacity=f(R, 1), distance=f(R, 1), color=f(R, 3) if rgbs is not None else None, depth_terms=f(R),
             distloss_per_ray=f(R), inv_n=f(1), d_sigma=f(S))
    _call('perf_train_head_geo', _p(_f32(sigmas, 'sigmas')), _p(rgbs), _p(t_starts), _p(t_ends), _p(packed), R, S,
          _p(_f32(gt_distance.contiguous(), 'gt')), _p(noise), int(global_batch), float(depth_weight), float(distortion_weight), _p(ratio_dev),
          float(loss_scale), _p(o['weights']), _p(o['trans']), _p(o['opacity']), _p(o['distance']), _p(o['color']), _p(o['depth_terms']),
          _p(o['distloss_per_ray']), _p(o['inv_n']), _p(o['d_sigma']), _stream())
    return o


def train_head_app(sigmas, rgbs, t_starts, t_ends, packed, bg_color, gt_color, global_batch, color_weight, loss_scale):
    """The ray head of the colour step in ONE launch (perf_train_head_app = composite_fwd -> app_loss -> composite_bwd) ->
    dict(weights, trans, opacity, distance, color, color_terms, d_rgb)."""
    R = packed.shape[0]
    S = sigmas.numel()
    dev = sigmas.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    o = dict(weights=f(S), trans=f(S), opacity=f(R, 1), distance=f(R, 1), color=f(R, 3), color_terms=f(R), d_rgb=f(S, 3))
    _call('perf_train_head_app', _p(_f32(sigmas, 'sigmas')), _p(_f32(rgbs, 'rgbs')), _p(t_starts), _p(t_ends), _p(packed), R, S, _p(bg_color),
          _p(_f32(gt_color.contiguous(), 'gt')), int(global_batch), float(color_weight), float(loss_scale), _p(o['weights']), _p(o['trans']),
          _p(o['opacity']), _p(o['distance']), _p(o['color']), _p(o['color_terms']), _p(o['d_rgb']), _stream())
    return o


def occ_splat(rays_o, rays_d, dist, res):
    n = rays_o.shape[0]
    occ = torch.zeros(res ** 3, dtype=torch.uint8, device=rays_o.device)
    _call('perf_occ_splat', _p(_f32(rays_o, 'rays_o')), _p(_f32(rays_d, 'rays_d')), _p(_f32(dist.reshape(-1), 'dist')), n,
              int(res), _p(occ), _stream())
    return occ


def gather_supervision(indices, o_all=None, d_all=None, color_all=None, dist_all=None, normal_all=None):
    """One-launch supervision batch: -> dict with 'o','d','color','normal' [n,3] and 'dist' [n,1] for the given sources."""
    n = indices.shape[0]
    dev = indices.device
    idx = indices.contiguous()
    assert idx.dtype == torch.int64
    out, src = {}, {}
    for key, all_, width in (('o', o_all, 3), ('d', d_all, 3), ('color', color_all, 3), ('dist', dist_all, 1), ('normal', normal_all, 3)):
        src[key] = None if all_ is None else _f32(all_, key)
        out[key] = None if all_ is None else torch.empty(n, width, dtype=torch.float32, device=dev)
    _call('perf_gather_supervision', _p(idx), n, _p(src['o']), _p(src['d']), _p(src['color']), _p(src['dist']), _p(src['normal']),
          _p(out['o']), _p(out['d']), _p(out['color']), _p(out['dist']), _p(out['normal']), _stream())
    return out


def draw_train_batch(seed, counter, pool_lo, pool_hi, n_local, first_global, o_all, d_all, color_all, dist_all, normal_all=None,
                     want_bg=False, want_indices=False):
    """One launch: the step's batch indices (uniform over [pool_lo, pool_hi)), the gathered supervision rows and the per-ray
    uniforms (jitter, noise[, bg]) from the counter-based generator (perf_draw_train_batch).  counter: device int64 [1],
    advanced by the launch.  -> dict(o, d, color, dist, normal, jitter [n], noise [n,1], bg [n,3] | None, indices | None)."""
    dev = o_all.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = {'o': f(n_local, 3), 'd': f(n_local, 3), 'color': f(n_local, 3), 'dist': f(n_local, 1),
           'normal': f(n_local, 3) if normal_all is not None else None, 'jitter': f(n_local), 'noise': f(n_local, 1),
           'bg': f(n_local, 3) if want_bg else None,
           'indices': torch.empty(n_local, dtype=torch.int64, device=dev) if want_indices else None}
    _call('perf_draw_train_batch', int(seed) & 0xFFFFFFFFFFFFFFFF, _nd(counter), _p(_ticket(dev)), int(pool_lo), int(pool_hi), int(n_local),
          int(first_global), _p(_f32(o_all, 'o')), _p(_f32(d_all, 'd')), _p(_f32(color_all, 'color')), _p(_f32(dist_all, 'dist')),
          _p(normal_all), _p(out['o']), _p(out['d']), _p(out['color']), _p(out['dist']), _p(out['normal']), _p(out['indices']),
          _p(out['jitter']), _p(out['noise']), _p(out['bg']), _stream())
    return out


# ---- step riders (include/perf_hip_riders.h): the argument blocks of the three stages.  The tensors are the caller's to keep alive. ----
def _q(t):
    return None if t is None else _p(t).value


def rider_draw(seed, counter, pool_lo, pool_hi, n_local, first_global, o_all, d_all, color_all, dist_all, normal_all, out, t0_scale, t0_base,
               step, max_steps, runs, marched_live=None, marched_keep=None):
    """Stage A: draw_train_batch(...) into the tensors of `out` (a dict as draw_train_batch returns) + lattice_runs((out['jitter'], t0_scale,
    t0_base), step, max_steps) into `runs`; [marched_keep = marched_live first]."""
    _nd(counter)
    return _lib.RiderDraw(int(seed) & 0xFFFFFFFFFFFFFFFF, _q(counter), _q(_ticket(o_all.device)), int(pool_lo), int(pool_hi), int(n_local), int(first_global),
                          _q(_f32(o_all, 'o')), _q(_f32(d_all, 'd')), _q(_f32(color_all, 'color')), _q(_f32(dist_all, 'dist')), _q(normal_all),
                          _q(out['o']), _q(out['d']), _q(out['color']), _q(out['dist']), _q(out['normal']), _q(out.get('indices')),
                          _q(out['jitter']), _q(out['noise']), _q(out['bg']), float(t0_scale), float(t0_base), float(step), int(max_steps), _q(runs),
                          _q(marched_live), _q(marched_keep))


def rider_count(rays_o, rays_d, t0, occ_bits, res, aabb, far_plane, step, max_steps, occ_coarse, masks, counts):
    """Stage B: occ_march_count(rays_o, rays_d, t0 = (u, scale, base, runs), ...) into `masks` / `counts`."""
    u, scale, base, runs = t0
    a = _aabb6(aabb)
    return _lib.RiderCount(_q(_f32(rays_o, 'rays_o')), _q(_f32(rays_d, 'rays_d')), _q(_f32(u, 't0')), float(scale), float(base), int(rays_o.shape[0]),
                           _q(occ_bits), _q(occ_coarse), int(res), a, float(far_plane), float(step),
                           int(max_steps), _q(runs), _q(masks), _q(counts))


def rider_write(t0, masks, counts, offsets, total, capacity, step, max_steps, rays_o, rays_d, points_aabb, ri, ts, te, packed, x01, sel):
    """Stage C: exclusive_scan_i32(counts) into `offsets` / `total` + occ_march_write(t0 = (u, scale, base, runs), ..., points_aabb) into the
    sample arrays."""
    u, scale, base, runs = t0
    a = _aabb6(points_aabb)
    _nd(total)
    return _lib.RiderWrite(_q(_f32(u, 't0')), float(scale), float(base), int(counts.shape[0]), float(step), int(max_steps), _q(runs), _q(masks), _q(counts),
                           _q(offsets), _q(total), int(capacity), _q(ri), _q(ts), _q(te), _q(packed), _q(rays_o), _q(rays_d),
                           a, _q(x01), _q(sel))


def pdf_resample(s_in, cdf, n_out, tau=None):
    """s_in, cdf [R, n_in+1] -> s_out [R, n_out+1] (inverse-CDF resampling, see perf_pdf_resample)."""
    R, n1 = s_in.shape
    out = torch.empty(R, n_out + 1, dtype=torch.float32, device=s_in.device)
    _call('perf_pdf_resample', _p(_f32(s_in.contiguous(), 's_in')), _p(_f32(cdf.contiguous(), 'cdf')), _p(tau), R, n1 - 1,
          int(n_out), _p(out), _stream())
    return out


# ---- reprojection visibility tests ---------------------------------------------------------------------------------
def pano_reproject(pts, pose, distance_map, mask, mode, eps=1.0 / 256.0):
    """In place on mask [n] (float 0/1): fold one registered panorama's depth test into it (perf_pano_reproject)."""
    n = pts.shape[0]
    h, w = distance_map.shape
    pose_h = (ctypes.c_float * 16)(*[float(v) for v in torch.as_tensor(pose).detach().cpu().reshape(-1).tolist()])
    _call('perf_pano_reproject', _p(_f32(pts, 'pts')), n, pose_h, _p(_f32(distance_map, 'distance_map')), int(h), int(w), int(mode),
          float(eps), _p(_f32(mask, 'mask')), _stream())
    return mask


def morph_binary(img, element, op):
    """img [H,W] float 0/1, element: 2-D 0/1 array (rows <= 16, cols <= 32), op 'dilate' | 'erode' -> new [H,W] float."""
    h, w = img.shape
    rows, cols = int(element.shape[0]), int(element.shape[1])
    bits = (ctypes.c_uint32 * rows)(*[sum(1 << c for c in range(cols) if float(element[r][c]) > 0.5) for r in range(rows)])
    out = torch.empty_like(img)
    _call('perf_morph_binary', _p(_f32(img, 'img')), _p(out), int(h), int(w), bits, rows, cols, 0 if op == 'dilate' else 1, _stream())
    return out
