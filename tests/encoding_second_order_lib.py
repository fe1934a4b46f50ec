"""The yardstick, the inputs and the rule of the per-level second-order tests of tcnn.Encoding (tests/test_cpu_encoding_second_order.py,
tests/test_gpu_encoding_second_order.py).  Plain helpers: numpy, torch on the CPU and the oracle, nothing of the product.

The operation.  f = encode(x; table) [n, 2L];  gx = d (f . dy) / dx  (perf_hashgrid_bwd_input);  S = (gx . gg);  the second-order pieces
are  d_x = dS/dx, d_dy = dS/d dy  (perf_hashgrid_bwd_bwd_input)  and  d_table = dS/d table  (perf_hashgrid_bwd_bwd_param).

Yardstick T: all of it in float64 under autograd through oracle.hashgrid_encode.  The oracle takes the fractional position from the
same single-rounding fma as the kernels and differentiates it as x * scale, so T is the exact value of the expression the kernels
evaluate in fp32 -- not a neighbouring one.  Emulation o: the same function in float32.

Per level.  A level's share of dx and d_x is the same function with dy zeroed outside that level (the gradient is linear in dy and the
levels only meet in one sum).  Zeroed levels contribute exact zeros in either precision, so the one-level function is evaluated on the
one-level view of the grid (level_view) instead of sixteen times on all of it; tests/test_cpu_encoding_second_order.py holds the two
equal.

The rule, for every block (d_dy[l], the level-l slice of d_table, dx_l and d_x_l of the masked launches, the all-level dx and d_x), with
k the candidate and max|.| taken over the block:
    rms:          rms(k - T) <= 2 * rms(o - T) + 2^-24 * max|T|
    per element:  |k - T|    <= 8 * max|o - T| + 2^-23 * max|T|
Factor 2 is the rule of test_gpu_ops.py and test_gpu_sphere_field.py (two fp32 evaluations of one expression in different summation
orders); one element among a few hundred fluctuates more than a block's rms does, hence 8 and not 2 per element.  Both factors were
set before anything ran on a GPU, from a numpy fp32 restatement of the kernels' own order (test_cpu_encoding_second_order.py), which
gives at most 1.15 and 2.6 for the bare errors rms(k - T) / rms(o - T) and max|k - T| / max|o - T| over both grids, both interpolations
and n in {257, 1300}.  The slack is half / one fp32 ulp of
the block's largest magnitude: blocks in which the emulation happens to be exact (edge rows, where weights are 0 or 1) still allow the
candidate its own final rounding.
The ratios printed and returned are  rms(k - T) / (rms(o - T) + 2^-25 max|T|)  and  max|k - T| / (max|o - T| + 2^-26 max|T|):  the rule
holds iff the first is <= 2 and the second <= 8.  Measured with these: the restatement at n = 257, both grids and interpolations, at most
0.47 and 2.30; the kernels on an MI355X (profiles/encoding_second_order.json, n = 257 and 1300) 0.47 and 2.30 as well, the worst blocks'
figures equal to the last digit: the library is built without fma contraction, which leaves the per-sample kernels no arithmetic
that the restatement does not have.

The old rule (test_encoding_double_backward): whole-tensor relative L2 norm below 1e-4.
"""
import dataclasses

import numpy as np
import torch

from oracle import perf_oracle as O

RMS_FACTOR, ELEM_FACTOR = 2.0, 8.0
OLD_RULE_REL = 1e-4

# 16 -> 2048 is SphereDistanceField's span.  MIXED: levels 0..2 are dense (17^3, 23^3, 31^3 < 2^15), the rest hashed; the finest
# level's scale is 128 times the coarsest's, its share of d_x 128^2 times.  SMALL: every level is hashed and collides (17^3 > 2^10).
GRIDS = {
    'MIXED': dict(n_levels=16, log2_hashmap_size=15, base_resolution=16, per_level_scale=float(np.exp(np.log(2048 / 16) / 15))),
    'SMALL': dict(n_levels=4, log2_hashmap_size=10, base_resolution=16, per_level_scale=float(np.exp(np.log(2048 / 16) / 3))),
}
INTERPS = ('Linear', 'Smoothstep')
N_MAX = 1300
# rows 0..6: the edge rows of test_hashgrid_fwd (cube faces and corners, the centre, one fp32 step inside a face)
EDGE_ROWS = [[0., 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1e-7, 1 - 1e-7, 0.25], [0.999999, 0, 1], [1.0, 0.0, 0.3], [0.3, 1.0, 0.0]]
SPECIAL_LEVELS = {'MIXED': (1, 5), 'SMALL': (0, 2)}      # (a dense and a hashed level | two hashed levels) that get rows of their own


def levels(grid: str) -> O.GridLevels:
    c = GRIDS[grid]
    return O.grid_levels(c['n_levels'], 2, c['log2_hashmap_size'], c['base_resolution'], c['per_level_scale'])


def level_view(lv: O.GridLevels, l: int) -> O.GridLevels:
    """Level l alone, addressing the SAME table (its offset stays absolute)."""
    cut = lambda a: None if a is None else a[l:l + 1]
    return dataclasses.replace(lv, n_levels=1, scale=cut(lv.scale), res=cut(lv.res), size=cut(lv.size), offset=cut(lv.offset),
                               hashed=cut(lv.hashed), local=cut(lv.local), nsx=cut(lv.nsx), nsxy=cut(lv.nsxy))


def special_rows(grid: str) -> torch.Tensor:
    """The edge rows, then for two levels rows at k / scale_l (mid-cell: f = 1/2 up to the fma's rounding, where Smoothstep's second
    derivative 6 - 12 f vanishes) and at (k - 1/2) / scale_l (on a vertex: f = 0 or one step below 1, where Smoothstep's first
    derivative vanishes and the cell changes)."""
    lv = levels(grid)
    rows = [torch.tensor(EDGE_ROWS, dtype=torch.float32)]
    for l in SPECIAL_LEVELS[grid]:
        s = np.float32(lv.scale[l])
        top = int(s)
        ks = np.array([[1, 2, 3], [top // 2, top - 1, 5], [top, 1, top // 3], [7, top // 2 + 1, top - 2]], np.float32)
        rows.append(torch.from_numpy((ks[:2] / s).astype(np.float32)))
        rows.append(torch.from_numpy(((ks[2:] - np.float32(0.5)) / s).astype(np.float32)))
    return torch.cat(rows)


N_SPECIAL = len(EDGE_ROWS) + 2 * 4

_INPUTS = {}


def inputs(grid: str, n: int = N_MAX):
    """(x [n,3], table [total,2], dy [L,n,2], gg [n,3]) fp32, seeded: the first n rows of ONE N_MAX-row set per grid, so that every
    smaller launch is a prefix of the largest.  Table uniform in +-1; dy and gg normal; x uniform in [0, 1) behind the special rows;
    about 10 % of dy's (level, sample) pairs are exactly (0, 0) (the parameter kernel returns early on them)."""
    if grid not in _INPUTS:
        lv = levels(grid)
        g = torch.Generator().manual_seed(20 + sorted(GRIDS).index(grid))
        table = torch.rand(lv.total, 2, generator=g) * 2 - 1
        x = torch.rand(N_MAX, 3, generator=g)
        sp = special_rows(grid)
        assert sp.shape[0] == N_SPECIAL
        x[:N_SPECIAL] = sp
        dy = torch.randn(lv.n_levels, N_MAX, 2, generator=g)
        gg = torch.randn(N_MAX, 3, generator=g)
        dy[torch.rand(lv.n_levels, N_MAX, generator=g) < 0.1] = 0.0
        _INPUTS[grid] = (x, table, dy, gg)
    x, table, dy, gg = _INPUTS[grid]
    assert 0 <= n <= N_MAX
    return x[:n].clone(), table.clone(), dy[:, :n].clone(), gg[:n].clone()


def second_order(x, table, dy, gg, lv, interp, dtype):
    """-> (dx, d_x [n,3], d_table [total,2], d_dy [L,n,2]) as float64 numpy, evaluated in `dtype` under autograd."""
    n = x.shape[0]
    # (clones: t.to(its own dtype) is t itself, and requires_grad_ would mark the caller's tensor)
    xs = x.to(dtype).clone().requires_grad_(True)
    tb = table.to(dtype).clone().requires_grad_(True)
    dl = dy.to(dtype).clone().requires_grad_(True)
    f = O.hashgrid_encode(xs, tb, lv, interpolation=interp)
    (gx,) = torch.autograd.grad((f * dl.permute(1, 0, 2).reshape(n, -1)).sum(), xs, create_graph=True)
    s = (gx * gg.to(dtype).clone()).sum()
    d_x, d_table, d_dy = torch.autograd.grad(s, [xs, tb, dl])
    return tuple(t.detach().double().numpy() for t in (gx, d_x, d_table, d_dy))


def evaluate(x, table, dy, gg, lv, interp, dtype, per_level=False):
    """All blocks of one evaluation: {'dx', 'd_x', 'd_table', 'd_dy'} and, per_level, {'dx_l', 'd_x_l'} [L,n,3]."""
    out = dict(zip(('dx', 'd_x', 'd_table', 'd_dy'), second_order(x, table, dy, gg, lv, interp, dtype)))
    if per_level:
        per = [second_order(x, table, dy[l:l + 1], gg, level_view(lv, l), interp, dtype)[:2] for l in range(lv.n_levels)]
        out['dx_l'] = np.stack([p[0] for p in per])
        out['d_x_l'] = np.stack([p[1] for p in per])
    return out


_YARD = {}


def yardstick(grid: str, interp: str, n: int, per_level=False):
    """(T, o): the float64 yardstick and the float32 emulation on inputs(grid, n); cached, read-only."""
    key = (grid, interp, n)
    if key not in _YARD or (per_level and 'dx_l' not in _YARD[key][0]):
        args = inputs(grid, n) + (levels(grid), interp)
        pair = tuple(evaluate(*args, dtype=dt, per_level=per_level) for dt in (torch.float64, torch.float32))
        for d in pair:
            for a in d.values():
                a.setflags(write=False)
        _YARD[key] = pair
    return _YARD[key]


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def _rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def _amax(a):
    a = np.asarray(a, np.float64)
    return float(np.abs(a).max()) if a.size else 0.0


def ratios(k, o, T):
    """(rms ratio, per-element ratio) of one block; the rule holds iff they are <= RMS_FACTOR and <= ELEM_FACTOR."""
    k, o, T = (np.asarray(a, np.float64) for a in (k, o, T))
    assert k.shape == o.shape == T.shape, (k.shape, o.shape, T.shape)
    top = _amax(T)
    num_r, num_e = _rms(k - T), _amax(k - T)
    den_r, den_e = _rms(o - T) + 2.0 ** -25 * top, _amax(o - T) + 2.0 ** -26 * top
    r = 0.0 if num_r == 0.0 else (num_r / den_r if den_r > 0 else float('inf'))
    e = 0.0 if num_e == 0.0 else (num_e / den_e if den_e > 0 else float('inf'))
    return r, e


def old_rule(k, T) -> bool:
    k, T = np.asarray(k, np.float64), np.asarray(T, np.float64)
    return float(np.linalg.norm(k - T) / (np.linalg.norm(T) + 1e-12)) < OLD_RULE_REL


class Checker:
    """Applies the rule block by block, prints every block's two ratios and keeps the worst per kind and the blocks that missed."""

    def __init__(self, label=''):
        self.label = label
        self.worst = {'rms': (0.0, None), 'elem': (0.0, None)}
        self.failed = []
        self.blocks = {}

    def block(self, name, k, o, T, rms_too=True):
        assert np.isfinite(np.asarray(k, np.float64)).all(), f'{self.label} {name}: not finite'
        r, e = ratios(k, o, T)
        ok = e <= ELEM_FACTOR and (r <= RMS_FACTOR or not rms_too)
        print(f'{self.label} {name}: rms ratio {r:.3f}{"" if rms_too else " (not held)"}  per-element ratio {e:.3f}  max|T| {_amax(T):.3e}'
              f'{"" if ok else "   <-- MISSES"}')
        if rms_too and r > self.worst['rms'][0]:
            self.worst['rms'] = (r, name)
        if e > self.worst['elem'][0]:
            self.worst['elem'] = (e, name)
        if not ok:
            self.failed.append(name)
        self.blocks[name] = ok
        return ok

    def candidate(self, cand, o, T, lv, special=0):
        """Every block `cand` holds.  special > 0: the first `special` rows form one more block per level and output, held by the
        per-element condition only (a dozen rows are no sample for an rms)."""
        for key in ('dx', 'd_x'):
            if key in cand:
                self.block(key, cand[key], o[key], T[key])
        for l in range(lv.n_levels):
            if 'd_dy' in cand:
                self.block(f'd_dy[{l}]', cand['d_dy'][l], o['d_dy'][l], T['d_dy'][l])
            if 'd_table' in cand:
                lo, hi = int(lv.offset[l]), int(lv.offset[l]) + int(lv.size[l])
                self.block(f'd_table[{l}]', cand['d_table'][lo:hi], o['d_table'][lo:hi], T['d_table'][lo:hi])
            for key in ('dx_l', 'd_x_l'):
                if key in cand:
                    self.block(f'{key}[{l}]', cand[key][l], o[key][l], T[key][l])
            if special:
                for key in ('d_dy', 'dx_l', 'd_x_l'):
                    if key in cand:
                        self.block(f'special rows {key}[{l}]', cand[key][l][:special], o[key][l][:special], T[key][l][:special], rms_too=False)
        return not self.failed

    def summary(self):
        return {'rms': {'worst': self.worst['rms'][0], 'block': self.worst['rms'][1], 'bound': RMS_FACTOR},
                'elem': {'worst': self.worst['elem'][0], 'block': self.worst['elem'][1], 'bound': ELEM_FACTOR},
                'blocks': len(self.blocks), 'missed': list(self.failed)}
