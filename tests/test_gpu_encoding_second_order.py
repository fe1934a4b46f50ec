"""tcnn.Encoding's input gradient and its double backward (perf_hashgrid_bwd_input, perf_hashgrid_bwd_bwd_input,
perf_hashgrid_bwd_bwd_param), block by block and level by level against a float64 autograd yardstick.

These kernels are the composed path of SphereDistanceField, and tests/test_gpu_sphere_field.py measures the fused sphere kernels by that
path; a level's term of d_x grows with scale_l^2, so a whole-tensor bound sees the finest levels only (level 0 of the 16 -> 2048 grid
carries 5e-5 of d_x).  The yardstick, the inputs and the rule are tests/encoding_second_order_lib.py's; the rule is held here for every
block: d_dy[l], the level-l slice of d_table, dx_l and d_x_l of launches with dy zeroed outside level l, the all-level dx and d_x, and
the rows on the cube's faces and the cells' vertices as blocks of their own.  Every block's ratios are printed before they are
asserted; with PERF_ENCODING_SECOND_ORDER_REPORT=<path> the worst per test are written there as JSON
(profiles/encoding_second_order.json is such a run).

Beside parity: the scatter touches the oracle's corner entries only; a launch's rows do not depend on the launch's size (n = 1, 256,
257 against 1300); asking for one output alone gives the joint call's bits; n = 0 is legal; the line-local layouts are refused; and
tcnn.Encoding's autograd wiring hands exactly these kernels' results on."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import perf_oracle as O  # noqa: E402
from tests import encoding_second_order_lib as E  # noqa: E402

_REPORT = {}


def _report(key, chk):
    _REPORT[key] = chk.summary()
    path = os.environ.get('PERF_ENCODING_SECOND_ORDER_REPORT')
    if path:
        worst = {kind: max(v[kind]['worst'] for v in _REPORT.values()) for kind in ('rms', 'elem')}
        json.dump({'rule': 'rms(k-T) / (rms(o-T) + 2^-25 max|T|) <= 2;  max|k-T| / (max|o-T| + 2^-26 max|T|) <= 8  '
                           '(k kernel, o float32 emulation, T float64 yardstick, per block)',
                   'worst': worst, 'tests': _REPORT}, open(path, 'w'), indent=1)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from perf_amd import ops as _ops
    return _ops


def _cfg(grid, interp):
    from perf_amd.grid import GridConfig
    cfg = GridConfig(**E.GRIDS[grid], interpolation=interp)
    lv = E.levels(grid)
    assert cfg.total == lv.total and np.array_equal(cfg.scale, lv.scale) and np.array_equal(cfg.offset, lv.offset)
    assert np.array_equal(cfg.hashed.astype(bool), lv.hashed)
    return cfg, lv


def _dev(grid, n=E.N_MAX):
    x, table, dy, gg = E.inputs(grid, n)
    return x.cuda(), table.reshape(-1).cuda(), dy.contiguous().cuda(), gg.cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _launch(ops, cfg, x, table, dy, gg):
    dd, d_x = ops.hashgrid_bwd_bwd_input(cfg, x, dy, table, gg)
    return {'dx': ops.hashgrid_bwd_input(cfg, x, dy, table), 'd_x': d_x, 'd_dy': dd, 'd_table': ops.hashgrid_bwd_bwd_param(cfg, x, dy, gg).view(-1, 2)}


@pytest.mark.parametrize('n', [257, 1300])
@pytest.mark.parametrize('interp', E.INTERPS)
@pytest.mark.parametrize('grid', sorted(E.GRIDS))
def test_every_block_within_the_rule(ops, grid, interp, n):
    """n = 257: one full workgroup and a one-thread tail; the launches with dy zeroed outside one level run there.  n = 1300: six
    workgroups, more samples per colliding entry in the scatter."""
    cfg, lv = _cfg(grid, interp)
    per_level = n == 257
    T, o = E.yardstick(grid, interp, n, per_level=per_level)
    x, table, dy, gg = _dev(grid, n)
    cand = {k: _np(v) for k, v in _launch(ops, cfg, x, table, dy, gg).items()}
    if per_level:
        cand['dx_l'], cand['d_x_l'] = np.zeros((lv.n_levels, n, 3), np.float32), np.zeros((lv.n_levels, n, 3), np.float32)
        for l in range(lv.n_levels):
            masked = torch.zeros_like(dy)
            masked[l] = dy[l]
            cand['dx_l'][l] = _np(ops.hashgrid_bwd_input(cfg, x, masked, table))
            cand['d_x_l'][l] = _np(ops.hashgrid_bwd_bwd_input(cfg, x, masked, table, gg, want_ddfeat=False)[1])
    chk = E.Checker(f'{grid} {interp} n={n}')
    chk.candidate(cand, o, T, lv, special=E.N_SPECIAL)
    _report(f'parity {grid} {interp} n={n}', chk)
    print(chk.summary())
    assert not chk.failed, chk.failed


@pytest.mark.parametrize('interp', E.INTERPS)
@pytest.mark.parametrize('grid', sorted(E.GRIDS))
def test_scatter_touches_the_oracles_corner_entries_only(ops, grid, interp):
    """Every nonzero entry of the table gradient is a corner of a (level, sample) pair whose dy is not (0, 0) -- a subset, not equality: a
    corner's weight may be exactly zero (Smoothstep on a vertex).  One sample alone: its 8 L entries form one block under the rule."""
    cfg, lv = _cfg(grid, interp)
    for n, row0 in ((257, 0), (1, 40), (1, 1)):                   # (row 40: a random point; row 1: x = (1, 1, 1), the dense levels' last cell)
        x, table, dy, gg = E.inputs(grid, row0 + n)
        x, dy, gg = x[row0:].contiguous(), dy[:, row0:].contiguous(), gg[row0:].contiguous()
        got = _np(ops.hashgrid_bwd_bwd_param(cfg, x.cuda(), dy.cuda(), gg.cuda())).reshape(-1, 2)
        allowed = np.zeros(lv.total, bool)
        for l in range(lv.n_levels):
            idx, _ = O.grid_corner_indices(x.numpy(), lv, l)
            live = _np((dy[l] != 0).any(-1))
            allowed[idx[live].astype(np.int64).reshape(-1) + int(lv.offset[l])] = True
        touched = (got != 0).any(-1)
        assert not (touched & ~allowed).any(), np.flatnonzero(touched & ~allowed)[:8]
        assert touched.sum() > allowed.sum() // 2                  # (... and the scatter did happen)
        if n == 1:
            T, o = (E.evaluate(x, table, dy, gg, lv, interp, dt)['d_table'] for dt in (torch.float64, torch.float32))
            chk = E.Checker(f'{grid} {interp} one sample (row {row0})')
            ok = chk.block('d_table', got, o, T)
            _report(f'scatter {grid} {interp} row {row0}', chk)
            assert ok


@pytest.mark.parametrize('interp', E.INTERPS)
@pytest.mark.parametrize('grid', sorted(E.GRIDS))
def test_rows_do_not_depend_on_the_launch_shape(ops, grid, interp):
    """No sample reads another: the rows of launches of 1, 256 (one full workgroup) and 257 samples are the first rows of the 1300-sample
    launch, bit for bit, for the two per-sample kernels."""
    cfg, _ = _cfg(grid, interp)
    x, table, dy, gg = _dev(grid)
    dx = ops.hashgrid_bwd_input(cfg, x, dy, table)
    dd, d_x = ops.hashgrid_bwd_bwd_input(cfg, x, dy, table, gg)
    assert bool(dx.any()) and bool(dd.any()) and bool(d_x.any())
    for n in (1, 256, 257):
        xs, dys, ggs = x[:n].contiguous(), dy[:, :n].contiguous(), gg[:n].contiguous()
        assert torch.equal(ops.hashgrid_bwd_input(cfg, xs, dys, table), dx[:n]), n
        dd_n, d_x_n = ops.hashgrid_bwd_bwd_input(cfg, xs, dys, table, ggs)
        assert torch.equal(dd_n, dd[:, :n]) and torch.equal(d_x_n, d_x[:n]), n


@pytest.mark.parametrize('interp', E.INTERPS)
def test_one_output_alone_equals_the_joint_call(ops, interp):
    cfg, _ = _cfg('MIXED', interp)
    x, table, dy, gg = _dev('MIXED', 257)
    dd, d_x = ops.hashgrid_bwd_bwd_input(cfg, x, dy, table, gg)
    dd_only, none_x = ops.hashgrid_bwd_bwd_input(cfg, x, dy, table, gg, want_dx=False)
    none_d, d_x_only = ops.hashgrid_bwd_bwd_input(cfg, x, dy, table, gg, want_ddfeat=False)
    assert none_x is None and none_d is None
    assert torch.equal(dd_only, dd) and torch.equal(d_x_only, d_x)
    # d_dy is the gradient of an expression LINEAR in dy: it does not depend on dy
    other = torch.randn(dy.shape, generator=torch.Generator().manual_seed(5)).cuda()
    assert torch.equal(ops.hashgrid_bwd_bwd_input(cfg, x, other, table, gg)[0], dd)
    assert torch.equal(ops.hashgrid_bwd_bwd_input(cfg, x, other, table, gg, want_dx=False)[0], dd)
    assert not torch.equal(ops.hashgrid_bwd_bwd_input(cfg, x, other, table, gg)[1], d_x)


def test_no_samples_and_refused_layouts(ops):
    from perf_amd import _lib
    from perf_amd.grid import GridConfig
    cfg, lv = _cfg('SMALL', 'Smoothstep')
    x, table, dy, gg = _dev('SMALL', 0)
    assert x.shape == (0, 3) and dy.shape == (lv.n_levels, 0, 2)
    assert ops.hashgrid_bwd_input(cfg, x, dy, table).shape == (0, 3)
    dd, d_x = ops.hashgrid_bwd_bwd_input(cfg, x, dy, table, gg)
    assert dd.shape == (lv.n_levels, 0, 2) and d_x.shape == (0, 3)
    # (the caching allocator hands the next call the block it is given back here, full of ones)
    torch.ones(cfg.n_params, device='cuda').mul_(3.0)
    grad = ops.hashgrid_bwd_bwd_param(cfg, x, dy, gg)
    assert grad.shape == (cfg.n_params,) and not bool(grad.any())
    # the line-local layouts: no input gradient, no second order -- an error, not another layout's entries
    bad = GridConfig(n_levels=4, log2_hashmap_size=12, base_resolution=16, per_level_scale=2.0, layout='line_local', sb_shift=(3, 3, 2),
                     local_min_res=32)
    assert bad.local.any()
    g = torch.Generator().manual_seed(6)
    x = torch.rand(64, 3, generator=g).cuda()
    dy, gg = torch.randn(4, 64, 2, generator=g).cuda(), torch.randn(64, 3, generator=g).cuda()
    table = torch.rand(bad.n_params, generator=g).cuda()
    with pytest.raises(_lib.PerfError, match='tcnn-layout'):
        ops.hashgrid_bwd_input(bad, x, dy, table)
    with pytest.raises(_lib.PerfError, match='tcnn-layout'):
        ops.hashgrid_bwd_bwd_input(bad, x, dy, table, gg)
    with pytest.raises(_lib.PerfError, match='tcnn-layout'):
        ops.hashgrid_bwd_bwd_param(bad, x, dy, gg)
    torch.cuda.synchronize()


@pytest.mark.parametrize('interp', E.INTERPS)
def test_encoding_module_hands_the_kernels_results_on(ops, interp):
    """tcnn.Encoding (dtype='fp32'): autograd.grad(S, [x, params, dout]) of S = (d (y . dout) / dx . gg) IS the three direct calls -- bit
    for bit for x and dout (per-sample kernels) and, for params, within the rule of the yardstick (the scatter's atomics land in another
    order in every launch)."""
    from perf_amd import tcnn
    grid, n = 'MIXED', 257
    cfg, lv = _cfg(grid, interp)
    enc = tcnn.Encoding(3, dict(otype='HashGrid', n_features_per_level=2, interpolation=interp, **E.GRIDS[grid]), dtype='fp32')
    x, table, dy, gg = _dev(grid, n)
    with torch.no_grad():
        assert enc.params.shape == table.shape
        enc.params.copy_(table)
    xg = x.clone().requires_grad_(True)
    dout = dy.permute(1, 0, 2).reshape(n, -1).contiguous().requires_grad_(True)
    assert torch.equal(tcnn._level_major(dout.detach(), enc), dy)
    y = enc(xg)
    assert y.dtype == torch.float32
    (gx,) = torch.autograd.grad((y * dout).sum(), xg, create_graph=True)
    d_x, d_p, d_dout = torch.autograd.grad((gx * gg).sum(), [xg, enc.params, dout])
    direct = _launch(ops, cfg, x, table, dy, gg)
    assert torch.equal(gx.detach(), direct['dx'])
    assert torch.equal(d_x, direct['d_x'])
    assert torch.equal(d_dout, direct['d_dy'].permute(1, 0, 2).reshape(n, -1))
    T, o = E.yardstick(grid, interp, n)
    chk = E.Checker(f'Encoding {interp} params.grad')
    chk.candidate({'d_table': _np(d_p).reshape(-1, 2)}, o, T, lv)
    _report(f'module {grid} {interp}', chk)
    assert not chk.failed, chk.failed
