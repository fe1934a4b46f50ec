"""CPU: the comparator of tests/encoding_second_order_lib.py is satisfiable and discriminating.

Satisfiable: a numpy fp32 restatement of the three kernels of perf_amd/csrc/hashgrid_aux.hip (hashgrid_bwd_input_kernel,
hashgrid_bwd_bwd_input_kernel, hashgrid_bwd_bwd_param_kernel), operation by operation in the source's order, passes the rule on every
block.  (perf_amd/build.py compiles with -ffp-contract=off, so the per-sample kernels have no rounding that numpy lacks; the scatter's
atomics land in an order of their own, here in thread order.)

Discriminating: candidates that are wrong at level 0 ONLY -- its table slice scaled by 1.03, Smoothstep's second derivative 6 - 12 f
replaced by 6 - 6 f, the two mixed terms of the Hessian dropped -- pass the old whole-tensor rule on d_x (level 0 carries 5e-5 of it)
and miss the per-level rule at level 0."""
import numpy as np
import pytest
import torch

from oracle import perf_oracle as O
from tests import encoding_second_order_lib as E

F32 = np.float32


# ---- the kernels, restated -------------------------------------------------------------------------------------------------------
def _corners(x, lv, l):
    idx, f = O.grid_corner_indices(x, lv, l)            # corners_of: the same fma, floor and fp32 subtraction
    return idx.astype(np.int64), [f[:, 0].copy(), f[:, 1].copy(), f[:, 2].copy()]


def _pick(k, d, s):
    """u_d of corner k: s_d or 1 - s_d"""
    return s[d] if (k >> d) & 1 else F32(1) - s[d]


def _sign(k, d):
    return F32(1) if (k >> d) & 1 else F32(-1)


def restate_bwd_input(x, table, dy, lv, interp):
    """hashgrid_bwd_input_kernel -> dx [n,3] fp32"""
    n = x.shape[0]
    out = np.zeros((n, 3), F32)
    for l in range(lv.n_levels):
        idx, f = _corners(x, lv, l)
        scale = F32(lv.scale[l])
        t = table[int(lv.offset[l]):]
        g = dy[l]
        if interp == 'Smoothstep':
            s = [fd * fd * (F32(3) - F32(2) * fd) for fd in f]
            ds = [F32(6) * fd * (F32(1) - fd) for fd in f]
        else:
            s = f
            ds = [np.ones(n, F32)] * 3
        acc = [np.zeros(n, F32) for _ in range(3)]
        for k in range(8):
            v = t[idx[:, k]]
            dot = v[:, 0] * g[:, 0] + v[:, 1] * g[:, 1]
            wx, wy, wz = _pick(k, 0, s), _pick(k, 1, s), _pick(k, 2, s)
            sx, sy, sz = _sign(k, 0), _sign(k, 1), _sign(k, 2)
            acc[0] = acc[0] + sx * wy * wz * dot
            acc[1] = acc[1] + wx * sy * wz * dot
            acc[2] = acc[2] + wx * wy * sz * dot
        for d in range(3):
            out[:, d] = out[:, d] + acc[d] * ds[d] * scale
    return out


def _interp_of(f, interp, scale, defect=None):
    """interp_of: (s, ds, dds) per dimension, scale folded in.  defect == 'dds': the second derivative 6 - 6 f instead of 6 - 12 f."""
    if interp == 'Smoothstep':
        s = [fd * fd * (F32(3) - F32(2) * fd) for fd in f]
        ds = [F32(6) * fd * (F32(1) - fd) * scale for fd in f]
        c = F32(6) if defect == 'dds' else F32(12)
        dds = [(F32(6) - c * fd) * scale * scale for fd in f]
    else:
        s = f
        ds = [np.full(f[0].shape, scale, F32)] * 3
        dds = [np.zeros(f[0].shape, F32)] * 3
    return s, ds, dds


def _corner_dw_dot(s, ds, k, gg):
    u = [_pick(k, d, s) for d in range(3)]
    sg = [_sign(k, d) for d in range(3)]
    return gg[0] * sg[0] * ds[0] * u[1] * u[2] + gg[1] * sg[1] * ds[1] * u[0] * u[2] + gg[2] * sg[2] * ds[2] * u[0] * u[1]


def restate_bwd_bwd_input(x, table, dy, gg, lv, interp, defect=None, defect_level=0):
    """hashgrid_bwd_bwd_input_kernel -> (d_dy [L,n,2], d_x [n,3]) fp32.  defect in (None, 'dds', 'mixed') acts at defect_level only."""
    n = x.shape[0]
    ggc = [gg[:, 0].copy(), gg[:, 1].copy(), gg[:, 2].copy()]
    hx = [np.zeros(n, F32) for _ in range(3)]
    d_dy = np.zeros((lv.n_levels, n, 2), F32)
    for l in range(lv.n_levels):
        bad = defect if l == defect_level else None
        idx, f = _corners(x, lv, l)
        s, ds, dds = _interp_of(f, interp, F32(lv.scale[l]), bad)
        t = table[int(lv.offset[l]):]
        g = dy[l]
        a0, a1 = np.zeros(n, F32), np.zeros(n, F32)
        for k in range(8):
            v = t[idx[:, k]]
            w = _corner_dw_dot(s, ds, k, ggc)
            a0 = a0 + w * v[:, 0]
            a1 = a1 + w * v[:, 1]
            dot = v[:, 0] * g[:, 0] + v[:, 1] * g[:, 1]
            u = [_pick(k, d, s) for d in range(3)]
            sg = [_sign(k, d) for d in range(3)]
            for j in range(3):
                p, q = (j + 1) % 3, (j + 2) % 3
                h = ggc[j] * sg[j] * dds[j] * u[p] * u[q]
                if bad != 'mixed':
                    h = h + ggc[p] * sg[p] * ds[p] * sg[j] * ds[j] * u[q] + ggc[q] * sg[q] * ds[q] * sg[j] * ds[j] * u[p]
                hx[j] = hx[j] + h * dot
        d_dy[l, :, 0], d_dy[l, :, 1] = a0, a1
    return d_dy, np.stack(hx, -1)


def restate_bwd_bwd_param(x, dy, gg, lv, interp):
    """hashgrid_bwd_bwd_param_kernel -> d_table [total,2] fp32 (the atomics in thread order)"""
    out = np.zeros((lv.total, 2), F32)
    ggc = [gg[:, 0].copy(), gg[:, 1].copy(), gg[:, 2].copy()]
    for l in range(lv.n_levels):
        g = dy[l]
        live = ~((g[:, 0] == 0) & (g[:, 1] == 0))
        idx, f = _corners(x, lv, l)
        s, ds, _ = _interp_of(f, interp, F32(lv.scale[l]))
        tb = out[int(lv.offset[l]):]
        for k in range(8):
            w = _corner_dw_dot(s, ds, k, ggc)
            np.add.at(tb[:, 0], idx[live, k], (w * g[:, 0])[live])
            np.add.at(tb[:, 1], idx[live, k], (w * g[:, 1])[live])
    return out


def restate(grid, interp, n, per_level=False, defect=None):
    x, table, dy, gg = (t.numpy() for t in E.inputs(grid, n))
    lv = E.levels(grid)
    d_dy, d_x = restate_bwd_bwd_input(x, table, dy, gg, lv, interp, defect)
    out = {'dx': restate_bwd_input(x, table, dy, lv, interp), 'd_x': d_x, 'd_dy': d_dy, 'd_table': restate_bwd_bwd_param(x, dy, gg, lv, interp)}
    if per_level:
        out['dx_l'], out['d_x_l'] = np.zeros((lv.n_levels, n, 3), F32), np.zeros((lv.n_levels, n, 3), F32)
        for l in range(lv.n_levels):
            masked = np.zeros_like(dy)
            masked[l] = dy[l]
            out['dx_l'][l] = restate_bwd_input(x, table, masked, lv, interp)
            out['d_x_l'][l] = restate_bwd_bwd_input(x, table, masked, gg, lv, interp, defect)[1]
    for a in out.values():
        assert a.dtype == F32
    return out


# ---- the grids and inputs are what the issue of this suite states -------------------------------------------------------------------
def test_grids_and_inputs():
    mixed, small = E.levels('MIXED'), E.levels('SMALL')
    assert mixed.n_levels == 16 and list(mixed.hashed) == [False] * 3 + [True] * 13
    assert small.n_levels == 4 and bool(small.hashed.all()) and int(small.size.max()) == 1024
    for lv in (mixed, small):
        assert abs(float(lv.scale[0]) - 15.0) < 1e-3 and abs(float(lv.scale[-1]) - 2047.0) < 0.5
    assert mixed.scale[-1] / mixed.scale[0] > 128 and int(mixed.size.max()) == 1 << 15
    for grid in E.GRIDS:
        x, table, dy, gg = E.inputs(grid)
        lv = E.levels(grid)
        assert x.shape == (E.N_MAX, 3) and table.shape == (lv.total, 2) and dy.shape == (lv.n_levels, E.N_MAX, 2)
        assert float(x.min()) == 0.0 and float(x.max()) == 1.0 and float(table.abs().max()) <= 1.0
        assert torch.equal(x[:7], torch.tensor(E.EDGE_ROWS))
        zero = (dy == 0).all(-1)
        assert 0.07 < float(zero.float().mean()) < 0.13 and bool(((dy == 0).any(-1) == zero).all())
        # a prefix is a prefix, and nobody can spoil the cached set
        x2, _, dy2, _ = E.inputs(grid, 257)
        assert torch.equal(x2, x[:257]) and torch.equal(dy2, dy[:, :257])
        x2.zero_()
        assert torch.equal(E.inputs(grid, 257)[0], x[:257])
        # the rows on and between the vertices of the two chosen levels: f = 1/2, or f within a step of 0 / 1
        for j, l in enumerate(E.SPECIAL_LEVELS[grid]):
            _, f = O.grid_corner_indices(x[7 + 4 * j:11 + 4 * j].numpy(), lv, l)
            assert np.abs(f[:2] - 0.5).max() < 1e-3, f
            assert np.minimum(f[2:], 1 - f[2:]).max() < 1e-3, f
    # the dense levels' modulo branch (corners_of: last >= size) is reached by x = 1: level 2 of MIXED wraps there
    idx, _ = O.grid_corner_indices(np.ones((1, 3), F32), mixed, 2)
    r = int(mixed.res[2])
    assert 30 + 1 + 31 * r + 31 * r * r >= int(mixed.size[2]) and int(idx.max()) < int(mixed.size[2])


def test_rule_arithmetic():
    g = np.random.default_rng(0)
    T = g.standard_normal(500)
    e = 1e-4 * g.standard_normal(500)
    o = T + e
    assert E.ratios(T, o, T) == (0.0, 0.0)
    r, m = E.ratios(T + 1.5 * e, o, T)
    assert 1.49 < r < 1.5 and 1.49 < m < 1.5
    chk = E.Checker('arith')
    assert chk.block('1.5 e', T + 1.5 * e, o, T) and not chk.block('2.1 e', T + 2.1 * e, o, T) and chk.failed == ['2.1 e']
    # per element: one outlier of 7 x the emulation's worst passes when it does not move the rms; 9 x misses
    big = np.zeros(500)
    big[3] = np.abs(e).max()
    assert E.Checker().block('7 x', T + 7 * big, o, T) and not E.Checker().block('9 x', T + 9 * big, o, T)
    # an exact emulation leaves half an ulp (rms) / one ulp (element) of the largest magnitude
    top = np.abs(T).max()
    assert E.Checker().block('ulp', T + 0.99 * 2.0 ** -24 * top, T, T) and not E.Checker().block('ulp', T + 1.01 * 2.0 ** -24 * top, T, T)
    # all-zero blocks: only zeros pass
    z = np.zeros(4)
    assert E.ratios(z, z, z) == (0.0, 0.0) and E.ratios(z + 1e-30, z, z) == (float('inf'), float('inf'))
    assert E.old_rule(T * (1 + 0.9e-4), T) and not E.old_rule(T * (1 + 1.1e-4), T)


@pytest.mark.parametrize('interp', E.INTERPS)
def test_one_level_view_equals_zeroed_dy(interp):
    """dx_l / d_x_l: the function on level l's view of the grid IS the function with dy zeroed outside level l, in both precisions."""
    lv = E.levels('SMALL')
    x, table, dy, gg = E.inputs('SMALL', 64)
    for l in (0, 3):
        masked = torch.zeros_like(dy)
        masked[l] = dy[l]
        for dt in (torch.float64, torch.float32):
            full = E.second_order(x, table, masked, gg, lv, interp, dt)
            one = E.second_order(x, table, dy[l:l + 1], gg, E.level_view(lv, l), interp, dt)
            assert np.array_equal(full[0], one[0]) and np.array_equal(full[1], one[1]) and np.array_equal(full[2], one[2])
            assert np.array_equal(full[3][l], one[3][0])


@pytest.mark.parametrize('interp', E.INTERPS)
@pytest.mark.parametrize('grid', sorted(E.GRIDS))
def test_restatement_passes_the_rule(grid, interp):
    n = 257
    T, o = E.yardstick(grid, interp, n, per_level=True)
    chk = E.Checker(f'restatement {grid} {interp} n={n}')
    chk.candidate(restate(grid, interp, n, per_level=True), o, T, E.levels(grid), special=E.N_SPECIAL)
    print(chk.summary())
    assert not chk.failed, chk.failed


def _level0_verdicts(cand, interp, blocks):
    """-> {block: passes the rule} for level 0's blocks of the candidate"""
    T, o = E.yardstick('MIXED', interp, 257, per_level=True)
    chk = E.Checker(f'wrong at level 0, {interp}')
    return {b: chk.block(f'{b}[0]', cand[b][0], o[b][0], T[b][0]) for b in blocks}


@pytest.mark.parametrize('interp', E.INTERPS)
def test_scaled_level0_table_passes_the_old_rule_and_misses_the_new(interp):
    n = 257
    lv = E.levels('MIXED')
    x, table, dy, gg = E.inputs('MIXED', n)
    T, _ = E.yardstick('MIXED', interp, n, per_level=True)
    table[:int(lv.size[0])] *= 1.03
    wrong = E.evaluate(x, table, dy, gg, lv, interp, torch.float64, per_level=True)
    assert E.old_rule(wrong['d_x'], T['d_x'])
    assert not E.old_rule(wrong['d_x_l'][0], T['d_x_l'][0])          # (3 % wrong where it is looked at alone)
    verdicts = _level0_verdicts(wrong, interp, ('d_x_l', 'd_dy', 'dx_l'))
    assert verdicts == {'d_x_l': False, 'd_dy': False, 'dx_l': False}, verdicts
    # ... and nowhere else: the other levels' blocks are the yardstick's own
    assert all(np.array_equal(wrong['d_x_l'][l], T['d_x_l'][l]) for l in range(1, lv.n_levels))


@pytest.mark.parametrize('interp,defect', [('Smoothstep', 'dds'), ('Smoothstep', 'mixed'), ('Linear', 'mixed')])
def test_level0_defects_pass_the_old_rule_and_miss_the_new(interp, defect):
    n = 257
    T, o = E.yardstick('MIXED', interp, n, per_level=True)
    wrong = restate('MIXED', interp, n, per_level=True, defect=defect)
    assert E.old_rule(wrong['d_x'], T['d_x'])
    verdicts = _level0_verdicts(wrong, interp, ('d_x_l', 'd_dy', 'dx_l'))
    assert verdicts == {'d_x_l': False, 'd_dy': True, 'dx_l': True}, verdicts      # (the defects sit in the Hessian only)
    chk = E.Checker(f'{defect} at level 0, {interp}: level 1')
    assert chk.block('d_x_l[1]', wrong['d_x_l'][1], o['d_x_l'][1], T['d_x_l'][1])
