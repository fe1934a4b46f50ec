"""The step riders' header (include/perf_hip_riders.h) checked without a GPU: the header's constants and parameter types are the binding's
(that header, binding, record and library agree is tests/test_abi_units.py's); every argument block has the fields of its ctypes mirror, in
order, with matching sizes; the block-index split of every host launch (rider workgroups first, rays per rider workgroup) is the header's
constants in the host code, the kernels and the binding; refusals happen before a launch."""
import ctypes
import os
import re

from tests import abi_units
from tests.abi_units import PERF_E_INVALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'perf_amd', 'csrc')
FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
CTYPE_OF = {'uint64_t': ctypes.c_uint64, 'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'float': ctypes.c_float}


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [riders] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, _ = abi_units.header('riders')
    assert abi_units.const(header, 'PERF_RIDERS_ABI_VERSION') == _lib.RIDERS_ABI_VERSION == 1


def _fields_of(plain, struct):
    """[(name, ctype)] of a struct of the header: pointers -> c_void_p, `float a[6]` -> c_float * 6, several declarators per line."""
    body = re.search(r'typedef struct ' + struct + r' \{(.*?)\} ' + struct + ';', plain, re.S).group(1)
    out = []
    for decl in (d.strip() for d in body.split(';') if d.strip()):
        m = re.match(r'(const\s+)?(\w+)\s*(.*)', decl, re.S)
        base = m.group(2)
        for item in (i.strip() for i in m.group(3).split(',')):
            arr = re.match(r'(\w+)\[(\d+)\]$', item)
            if item.startswith('*') or base.endswith('*'):
                out.append((item.lstrip('* '), ctypes.c_void_p))
            elif arr:
                out.append((arr.group(1), CTYPE_OF[base] * int(arr.group(2))))
            else:
                out.append((item, CTYPE_OF[base]))
    return out


def test_argument_blocks_are_their_ctypes_mirrors_field_for_field():
    from perf_amd import _lib
    _, plain = abi_units.header('riders')
    lib = _lib.load()
    for struct, mirror, size in (('perf_rider_draw', _lib.RiderDraw, lib.perf_sizeof_rider_draw()), ('perf_rider_count', _lib.RiderCount, lib.perf_sizeof_rider_count()),
                                 ('perf_rider_write', _lib.RiderWrite, lib.perf_sizeof_rider_write())):
        # `float *a, *b` declares pointers: normalise the declarator's star onto every item first
        body = re.sub(r'(\w)\s*\*\s*(\w)', r'\1 *\2', plain)
        want = _fields_of(body, struct)
        got = [(n, t) for n, t in mirror._fields_]
        assert [n for n, _ in want] == [n for n, _ in got], struct
        for (n, a), (_, b) in zip(want, got):
            assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is ctypes.c_void_p) == (b is ctypes.c_void_p), (struct, n)
        assert ctypes.sizeof(mirror) == size, struct


def test_block_index_split_is_the_headers_constants_everywhere():
    from perf_amd import _lib
    header, _ = abi_units.header('riders')
    const = {k: int(v) for k, v in re.findall(r'#define\s+(PERF_RIDER_[A-Z_]+)\s+(\d+)', header)}
    assert const == {'PERF_RIDER_THREADS': 256, 'PERF_RIDER_DRAW_RAYS': 256, 'PERF_RIDER_MARCH_RAYS': 4, 'PERF_RIDER_MAX_RAYS': 65536}
    assert (_lib.RIDER_THREADS, _lib.RIDER_DRAW_RAYS, _lib.RIDER_MARCH_RAYS, _lib.RIDER_MAX_RAYS) == (256, 256, 4, 65536)
    # a lane per ray in stage A, a wave per ray in stages B and C -- the bodies index rays by block * 4 + wave resp. block * 256 + thread
    assert const['PERF_RIDER_DRAW_RAYS'] == const['PERF_RIDER_THREADS'] and const['PERF_RIDER_MARCH_RAYS'] * 64 == const['PERF_RIDER_THREADS']
    # (sources compared without white space: a reformatting is no mismatch of the split)
    class Src(str):
        def __contains__(self, s):
            return str.__contains__(self, re.sub(r'\s+', '', s))

        def count(self, s):
            return str.count(self, re.sub(r'\s+', '', s))
    src = lambda name: Src(re.sub(r'\s+', '', open(os.path.join(CSRC, name)).read()))
    march_dev = src('march_device.hpp')
    riders_dev = src('step_riders_device.hpp')
    assert march_dev.count('(int64_t)block * 4') >= 2 and '(int64_t)block * 256 + threadIdx.x' in riders_dev
    # the jobs' block counts (host code, march.hip) come from the header's constants
    march = src('march.hip')
    assert 'job->n_blocks = (int32_t)div_up(a->n_local, PERF_RIDER_DRAW_RAYS);' in march
    assert march.count('job->n_blocks = (int32_t)div_up(a->n_rays, PERF_RIDER_MARCH_RAYS);') == 2
    assert march.count('<= PERF_RIDER_MAX_RAYS') == 3
    # every host: 256-thread workgroups, the riders in the LOWEST block indices, the host's own blocks shifted behind them -- in the
    # kernel and in the launch
    bwd = src('hashgrid_bwd.hip')
    misc = src('misc.hip')
    assert 'constexpr int kCodeWaves = 4;' in bwd and '__launch_bounds__(64 * kCodeWaves) void tile_codes4_kernel' in bwd
    assert 'if (blockIdx.x < (unsigned)draw.n_blocks) { rider_draw_block(draw, (int)blockIdx.x); return; }' in bwd
    assert 'const unsigned bx = blockIdx.x - (unsigned)draw.n_blocks;' in bwd
    assert 'all = (unsigned)draw.n_blocks + own + (unsigned)job.n_blocks;' in bwd
    assert '__launch_bounds__(256) void hashgrid_bwd_reduce_kernel' in bwd
    assert 'const unsigned b = blockIdx.y * rider_cols + blockIdx.x;' in bwd and 'if (b < (unsigned)count.n_blocks) rider_count_block(count, (int)b);' in bwd
    assert 'const unsigned rider_cols = (unsigned)div_up(count.n_blocks, gp.n_levels);' in bwd and 'dim3(rider_cols + kReduceBlocks, gp.n_levels)' in bwd
    assert 'if (bx < (unsigned)rj.n_blocks) { rider_write_block(rj, (int)bx); return; }' in misc and 'bx -= (unsigned)rj.n_blocks;' in misc
    assert 'dim3 g4((unsigned)(div_up(div_up(n, 4), 256) + rj.n_blocks)), b(256);' in misc
    # the stand-alone kernels and the riders call ONE body each
    for body, files in (('draw_train_batch_body(', (misc, riders_dev)), ('march_count_body<', (march, riders_dev)), ('march_write_body(', (march, riders_dev)),
                        ('lattice_runs_row(', (march, riders_dev))):
        assert all(body in f for f in files), body


def test_refusals_happen_before_a_launch():
    from perf_amd import _lib
    from perf_amd.grid import GridConfig, MlpConfig
    lib = _lib.load()
    msg = lambda: (lib.perf_last_error() or b'').decode()
    w = _lib.RiderWrite()
    w.n_rays = _lib.RIDER_MAX_RAYS + 1; w.max_steps = 128; w.step = 0.01
    assert lib.perf_adam_step_dev_riders(FAKE, FAKE, FAKE, FAKE, FAKE, 4096, 0, FAKE, FAKE, None, 0.9, 0.999, 1e-8, 0, None, None, 0, 0, ctypes.byref(w), None) == PERF_E_INVALID
    assert 'perf_rider_write: bad arguments' in msg()
    w.n_rays = 8
    assert lib.perf_adam_step_dev_riders(FAKE, FAKE, FAKE, FAKE, FAKE, 4096, 0, FAKE, FAKE, None, 0.9, 0.999, 1e-8, 0, None, None, 0, 0, ctypes.byref(w), None) == PERF_E_INVALID
    assert 'NULL pointer' in msg()
    gd, md = GridConfig().desc(), MlpConfig(n_levels=16, n_hidden_layers=1, n_output_dims=1, output_activation='Exponential', exp_shift=1.0).desc()
    d = _lib.RiderDraw()
    assert lib.perf_field_bwd_riders(ctypes.byref(gd), ctypes.byref(md), FAKE, FAKE, FAKE, None, 0, None, FAKE, FAKE, 0, 0, None, None, FAKE, 1 << 40, 64, None, 0,
                                     None, ctypes.byref(d), None, None) == PERF_E_INVALID
    assert 'perf_rider_draw' in msg()
    c = _lib.RiderCount()
    c.n_rays = 8; c.res = 128; c.max_steps = 128; c.step = 0.01
    assert lib.perf_field_bwd_riders(ctypes.byref(gd), ctypes.byref(md), FAKE, FAKE, FAKE, None, 0, None, FAKE, FAKE, 0, 0, None, None, FAKE, 1 << 40, 64, None, 0,
                                     None, None, ctypes.byref(c), None) == PERF_E_INVALID
    assert 'perf_rider_count: NULL pointer' in msg()
