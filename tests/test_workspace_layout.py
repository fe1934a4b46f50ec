"""The backward's scratch memory without a device: the sizes the library reports for a workspace (host functions; one layout function
per grid-backward unit computes both the reported size and the offsets a call uses) against the sizes the build BEFORE that
unification reported (tests/golden/workspace_sizes.json), and the grow-only holder a network keeps its workspace in."""
import ctypes
import json
import os

import pytest
import torch

from perf_amd import _lib, ops
from perf_amd.grid import GridConfig, MlpConfig

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_sizes.json')) as _f:
    RECORDED = json.load(_f)

GRIDS = {
    'L16_T18_tcnn': dict(n_levels=16, log2_hashmap_size=18),
    'L16_T18_line_local': dict(n_levels=16, log2_hashmap_size=18, layout='line_local', sb_shift=(3, 3, 2)),
    'L16_T18_line_overlap': dict(n_levels=16, log2_hashmap_size=18, layout='line_overlap', sb_shift=(3, 3, 2)),
    'L16_T16_tcnn': dict(n_levels=16, log2_hashmap_size=16),
    'L20_T24_tcnn': dict(n_levels=20, log2_hashmap_size=24),           # levels on per-tile bitmaps
    'L20_T26_tcnn': dict(n_levels=20, log2_hashmap_size=26),           # levels beyond 2,048 tiles: global atomics
}
NS = (0, 1, 4096, 1 << 20, (1 << 28) - 1, 1 << 28)                      # (2^28: tile codes and bitmaps drop out)
# Where the size query and the call's own layout arithmetic disagreed before they were one function, the call's layout won and the
# reported size GREW to hold it: the L20 grids just below 2^28 samples (the query dropped bitmaps above 2 GiB but kept the code slots
# it had planned WITH bitmap levels: one slot of 1 GiB short) ...
SHORT_BEFORE = {('L20_T24_tcnn', (1 << 28) - 1), ('L20_T26_tcnn', (1 << 28) - 1)}
# ... and these 23 grids of the sweep (L, log2 T, base, scale), whose slab maximum left out the fixed-point plan without bitmap levels
GREW = {f'4,{t},32,1.3819' for t in (20, 21, 22, 23, 24, 25, 26, 28)} | {
    '12,19,4,1.3819', '16,25,16,1.5', '16,25,32,1.3819', '16,25,32,1.5', '20,25,4,1.5', '20,25,16,1.3819', '20,25,16,1.5',
    '20,25,32,1.3819', '20,25,32,1.5', '24,25,4,1.3819', '24,25,4,1.5', '24,25,16,1.3819', '24,25,16,1.5', '24,25,32,1.3819',
    '24,25,32,1.5'}


def _sizes(g, n):
    lib = _lib.load()
    d, md = g.desc(), MlpConfig(g.n_levels).desc()
    query = lib.perf_hashgrid_bwd_workspace_bytes if g.layout == 'tcnn' else lib.perf_hashgrid_bwd_lines_workspace_bytes
    return [int(query(ctypes.byref(d), n)), int(lib.perf_field_bwd_workspace_bytes(ctypes.byref(d), ctypes.byref(md), n, None, None, None))]


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_workspace_sizes_are_the_recorded_ones(name):
    g = GridConfig(**GRIDS[name])
    for n in NS:
        was, now = RECORDED['table'][name][str(n)], _sizes(g, n)
        if (name, n) in SHORT_BEFORE:
            assert now[0] >= was[0] and now[1] >= was[1], (name, n, was, now)
        else:
            assert now == was, (name, n, was, now)


def test_orientation_values():
    assert RECORDED['table']['L16_T18_tcnn'][str(1 << 20)] == [64170896, 204696576]
    assert RECORDED['table']['L16_T18_line_local']['4096'] == [6281504, 7200144]
    assert RECORDED['table']['L20_T24_tcnn'][str(1 << 20)] == [1680465312, 1852440080]


def test_no_grid_of_the_sweep_reports_less_than_before():
    lib = _lib.load()
    assert len(RECORDED['sweep']) == 648 and GREW <= set(RECORDED['sweep'])
    assert RECORDED['sweep']['4,20,32,1.3819'][0] == 8908784
    for key, was in RECORDED['sweep'].items():
        L, T, base, scale = key.split(',')
        d = GridConfig(n_levels=int(L), log2_hashmap_size=int(T), base_resolution=int(base), per_level_scale=float(scale)).desc()
        now = [int(lib.perf_hashgrid_bwd_workspace_bytes(ctypes.byref(d), n)) for n in (4096, 1 << 20)]
        if key in GREW:
            assert now[0] >= was[0] and now[1] >= was[1], (key, was, now)
        else:                           # (query and call agreed: the same to the byte)
            assert now == was, (key, was, now)
    # L4 / T20 / base 32 / 1.3819 at n = 4096: the call's layout ends at 11,411,280 bytes (slabs of 1,425,623 entries, shifts, codes)
    d = GridConfig(n_levels=4, log2_hashmap_size=20, base_resolution=32, per_level_scale=1.3819).desc()
    assert lib.perf_hashgrid_bwd_workspace_bytes(ctypes.byref(d), 4096) >= 11411280


def test_workspace_holder_grows_and_never_shrinks():
    cpu = torch.device('cpu')
    ws = ops.Workspace()
    a = ws.get(1000, cpu)
    assert a.dtype == torch.float32 and a.numel() * 4 >= 1000 and ws.block is a
    assert ws.get(400, cpu) is a and ws.get(1000, cpu) is a            # a smaller request: the same block
    b = ws.get(1100, cpu)
    assert b is not a and ws.block is b and b.numel() * 4 >= 1500       # grown geometrically, not to the exact size
    assert ws.get(1000, cpu) is b and ws.get(8, cpu) is b               # never shrinks
    c = ws.get(100000, cpu)
    assert c.numel() * 4 >= 100000 and ws.get(100000, cpu) is c
    other = ops.Workspace()                                             # two networks: two blocks
    assert other.get(1000, cpu) is not ws.get(1000, cpu) and other.block.data_ptr() != ws.block.data_ptr()
