"""Parameter gradient of the line-local table layouts ('line_local' / 'line_overlap': perf_hashgrid_bwd_lines) against the oracle's
corner bookkeeping (oracle/perf_oracle.py:grid_corner_indices, the forward's addressing restated in numpy): LDS owners and the
global-atomics scatter, fp32 and fixed-point modes, the overlap fold, accumulate, the repair launch and the one-call field backward."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import perf_oracle as O  # noqa: E402

# (log2_hashmap_size, sb_shift, local_min_res, n_levels): every level line-local / a tcnn-rule prefix / 64 tiles per hashed level /
# super-blocks larger than a tile and levels of 256 tiles (the atomics scatter)
CASES = [(15, (2, 2, 1), 16, 8), (18, (3, 3, 2), 64, 8), (20, (3, 3, 2), 64, 8), (22, (5, 6, 8), 64, 6)]
CASE_IDS = ['T15', 'T18', 'T20', 'T22']


@pytest.fixture(scope='module')
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from perf_amd import ops as _ops
    return _ops


def _cfg(layout, log2_t, sb, min_res, L, interp='Linear'):
    from perf_amd.grid import GridConfig
    pls = 2.0 if L <= 8 else 1.4472692012786865         # (16 levels: PeRF's growth factor)
    cfg = GridConfig(n_levels=L, log2_hashmap_size=log2_t, base_resolution=16, per_level_scale=pls, interpolation=interp,
                     layout=layout, sb_shift=sb, local_min_res=min_res)
    lv = O.grid_levels(L, 2, log2_t, 16, pls, layout=layout, sb_shift=sb, local_min_res=min_res)
    assert int(lv.total) == cfg.total and np.array_equal(np.asarray(lv.local, np.uint32), cfg.local)
    return cfg, lv


def _points(cfg, n, g):
    """Uniform points, then points ON cell, block (4 / 2 cells) and super-block faces of every line-local level and in its last cell,
    then a few far outside the unit cube (their dfeat rows are zero)."""
    x = torch.rand(n, 3, generator=g)
    k = 0
    for l in range(cfg.n_levels):
        if not cfg.local[l]:
            continue
        s, r = float(cfg.scale[l]), int(cfg.res[l])
        faces = [1, 2, 4, 8, 1 << cfg.sb_shift[0], 1 << cfg.sb_shift[1], 1 << cfg.sb_shift[2], 3 * (1 << (cfg.sb_shift[0] - 2)), r - 1]
        for a in range(3):
            for m in faces:
                if k >= n // 4:
                    break
                v = (m - 0.5) / s           # grid_pos = x * s + 0.5 lands on the integer m (up to one rounding)
                if 0.0 <= v <= 1.0:
                    x[k, a] = v
                    k += 1
    x[-1] = 1.0                             # the last cell of every level
    x[-2] = 0.0
    far = torch.tensor([[-0.31, 0.5, 1.7], [5.0, -2.0, 0.2], [1.5, 1.5, 1.5], [-0.7, -0.2, 0.4]])
    x[-7:-3] = far
    return x


def _dfeat(cfg, x, g, scale=1.0):
    d = torch.randn(cfg.n_levels, x.shape[0], 2, generator=g) * scale
    outside = ((x < 0) | (x > 1)).any(1)
    d[:, outside] = 0.0
    return d


def _reference(cfg, lv, x, dfeat, n_live, interp='Linear'):
    """float64 sum of w * dfeat over the corners of the live samples (the association (wx * wy) * wz of the kernels), with the two
    storage copies of every shared vertex of a 'line_overlap' level folded."""
    ref = np.zeros((cfg.total, 2), np.float64)
    xn = x[:n_live].numpy()
    for l in range(cfg.n_levels):
        if n_live == 0:
            break
        idx, f = O.grid_corner_indices(xn, lv, l)
        if interp == 'Smoothstep':
            f = (f * f * (np.float32(3) - np.float32(2) * f)).astype(np.float32)
        d = dfeat[l, :n_live].numpy().astype(np.float64)
        live = np.abs(d).sum(1) > 0
        for c in range(8):
            w = np.ones(n_live, np.float32)
            for a in range(3):
                w = w * (f[:, a] if (c >> a) & 1 else (np.float32(1) - f[:, a]))
            np.add.at(ref, idx[live, c].astype(np.int64) + int(lv.offset[l]), w[live, None].astype(np.float64) * d[live])
    if cfg.layout == 'line_overlap':
        _fold(cfg, ref)
    return ref


def _runs(cfg, table2, l):
    """[row of blocks, block along x, (y, z) in block, x in run, feature] view of line-local level l of a [total, 2] array"""
    runs = 1 << (cfg.sb_shift[0] - 2)
    lo, n = int(cfg.offset[l]), int(cfg.size[l])
    return table2[lo:lo + n].reshape(n // (32 * runs), runs, 8, 4, 2)


def _fold(cfg, ref):
    for l in range(cfg.n_levels):
        if cfg.local[l]:
            v = _runs(cfg, ref, l)
            s = v[:, :-1, :, 3] + v[:, 1:, :, 0]
            v[:, :-1, :, 3] = s
            v[:, 1:, :, 0] = s


def _amax(cfg, dfeat):
    a = torch.zeros(24)
    a[:cfg.n_levels] = dfeat.abs().amax(dim=(1, 2))
    return a.cuda()


def _check_fixed(cfg, got, ref, amax, n_live):
    """per level within the unit bound of the fixed-point mode (tests/test_gpu_ops.py::test_hashgrid_bwd_fixed_point_mode); a folded
    'line_overlap' entry sums two entries' rounding"""
    fold = 2 if cfg.layout == 'line_overlap' else 1
    for l in range(cfg.n_levels):
        lo, hi = int(cfg.offset[l]), int(cfg.offset[l]) + int(cfg.size[l])
        if float(amax[l]) == 0.0:
            continue
        h = min(24, max(12, math.ceil(math.log2(max(8.0 * n_live / int(cfg.size[l]), 1.0))) + 6))
        unit = float(2.0 ** torch.ceil(torch.log2(amax[l].cpu())) * 2.0 ** (h - 31))
        fan = 8.0 * max(n_live, 1) / int(cfg.size[l]) + 8
        err = float(np.abs(got[lo:hi] - ref[lo:hi]).max())
        assert err <= fold * unit * (4 * fan ** 0.5 + 4), (l, err, unit)


def _check_copies(cfg, got):
    if cfg.layout != 'line_overlap':
        return
    for l in range(cfg.n_levels):
        if cfg.local[l]:
            v = _runs(cfg, got, l)
            assert np.array_equal(v[:, :-1, :, 3], v[:, 1:, :, 0]), l        # the two copies of a shared vertex: bit-equal
            assert not v[:, -1, :, 3].any(), l                                 # the never-read last entry of a row's last run


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('interp', ['Linear', 'Smoothstep'])
def test_line_layout_grad_matches_the_oracle(ops, layout, case, interp):
    log2_t, sb, min_res, L = case
    cfg, lv = _cfg(layout, log2_t, sb, min_res, L, interp)
    g = torch.Generator().manual_seed(7 + log2_t)
    n = 3001                                        # ragged: n % 4 != 0
    x = _points(cfg, n, g)
    dfeat = _dfeat(cfg, x, g)
    n_live = n - 6                                  # a device live count below the capacity
    n_dev = torch.tensor([n_live], dtype=torch.int64, device='cuda')
    ref = _reference(cfg, lv, x, dfeat, n_live, interp)
    xc, dc = x.cuda(), dfeat.cuda()
    scale = np.abs(ref).max()
    # fp32 mode: LDS owners (and the atomics scatter for levels beyond 255 tiles)
    got = ops.hashgrid_bwd_lines(cfg, xc, dc, n_dev=n_dev).cpu().numpy().reshape(-1, 2)
    assert np.abs(got - ref).max() < 2e-4 * scale
    _check_copies(cfg, got)
    # fixed point
    amax = _amax(cfg, dfeat)
    flag = ops.overflow_flag(xc.device); flag.zero_()
    fx = ops.hashgrid_bwd_lines(cfg, xc, dc, n_dev=n_dev, level_absmax=amax)
    assert int(flag.item()) == 0
    fxn = fx.cpu().numpy().reshape(-1, 2)
    _check_fixed(cfg, fxn, ref, amax, n_live)
    _check_copies(cfg, fxn)
    # fixed point: the atomics scatter for every line-local level adds the same integers -- and a second run the same again
    at = ops.hashgrid_bwd_lines(cfg, xc, dc, n_dev=n_dev, level_absmax=amax, use_owners=False)
    assert torch.equal(at, fx)
    assert torch.equal(ops.hashgrid_bwd_lines(cfg, xc, dc, n_dev=n_dev, level_absmax=amax, use_codes=False), fx)    # position-streaming owners
    assert torch.equal(ops.hashgrid_bwd_lines(cfg, xc, dc, n_dev=n_dev, level_absmax=amax), fx)
    # fp32 atomics scatter
    got_a = ops.hashgrid_bwd_lines(cfg, xc, dc, n_dev=n_dev, use_owners=False).cpu().numpy().reshape(-1, 2)
    assert np.abs(got_a - ref).max() < 2e-4 * scale
    _check_copies(cfg, got_a)
    # accumulate adds this call's (folded) gradient on top
    acc = torch.from_numpy(got.reshape(-1).copy()).cuda()
    ops.hashgrid_bwd_lines(cfg, xc, dc, out=acc, accumulate=True, n_dev=n_dev)
    accn = acc.cpu().numpy().reshape(-1, 2)
    assert np.abs(accn - 2 * ref).max() < 4e-4 * scale
    acc = fx.clone()
    ops.hashgrid_bwd_lines(cfg, xc, dc, out=acc, accumulate=True, n_dev=n_dev, level_absmax=amax)
    _check_fixed(cfg, acc.cpu().numpy().reshape(-1, 2) / 2, ref, amax, n_live)
    _check_copies(cfg, acc.cpu().numpy().reshape(-1, 2))


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
def test_line_layout_grad_of_no_samples_is_zero(ops, layout):
    cfg, _ = _cfg(layout, 18, (3, 3, 2), 64, 8)
    for amax in (None, torch.ones(24, device='cuda')):
        for owners in (True, False):          # (n = 0: no tile codes either way)
            out = torch.full((cfg.n_params,), float('nan'), device='cuda')
            ops.hashgrid_bwd_lines(cfg, torch.empty(0, 3, device='cuda'), torch.empty(8, 0, 2, device='cuda'), out=out,
                                   level_absmax=amax, use_owners=owners)
            assert not bool(out.any()), (amax is None, owners)          # every entry written: no NaN left, all zero


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
def test_line_layout_ray_ordered_samples_owners_equal_scatter(ops, layout):
    """Ray-ordered samples (many per cell, bursts on a few tiles, some outside the unit cube) at L16 / T18: coded owners, position-streaming
    owners and the scatter, fixed point, bit-identical."""
    cfg, _ = _cfg(layout, 18, (3, 3, 2), 64, 16)
    g = torch.Generator().manual_seed(5)
    rays, per = 400, 64
    o = torch.rand(rays, 1, 3, generator=g) * 0.2 + 0.4
    d = torch.nn.functional.normalize(torch.randn(rays, 1, 3, generator=g), dim=-1)
    t = torch.linspace(0.0, 0.45, per)[None, :, None]
    x = (o + d * t).reshape(-1, 3).contiguous().cuda()
    dfeat = torch.randn(16, x.shape[0], 2, generator=g).cuda()
    amax = _amax(cfg, dfeat.cpu())
    a = ops.hashgrid_bwd_lines(cfg, x, dfeat, level_absmax=amax)
    b = ops.hashgrid_bwd_lines(cfg, x, dfeat, level_absmax=amax, use_owners=False)
    assert torch.equal(a, b)
    assert torch.equal(ops.hashgrid_bwd_lines(cfg, x, dfeat, level_absmax=amax, use_codes=False), b)
    _check_copies(cfg, a.cpu().numpy().reshape(-1, 2))


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
def test_an_overflowed_line_layout_gradient_is_repaired(ops, layout):
    """The headroom forced to its floor overflows the fixed-point fields; the predicated repair launch rewrites the whole table
    gradient (tcnn-rule prefix and line-local levels) with fp32 LDS accumulation, and is a no-op while the flag is clear."""
    cfg, _ = _cfg(layout, 18, (3, 3, 2), 64, 16)
    g = torch.Generator().manual_seed(11)
    n = 60000
    x = (torch.rand(n, 3, generator=g) * 0.3 + 0.35).cuda()
    dfeat = (torch.rand(16, n, 2, generator=g) + 0.5).cuda()            # one sign: the contributions of an entry add up
    amax = _amax(cfg, dfeat.cpu())
    flag = ops.overflow_flag(x.device); flag.zero_()
    ref32 = ops.hashgrid_bwd_lines(cfg, x, dfeat)
    hr = ops.headroom_state(x.device)
    fixed = ops.hashgrid_bwd_lines(cfg, x, dfeat, level_absmax=amax, hr_state=hr)
    assert int(flag.item()) == 0
    kept = fixed.clone()
    ops.hashgrid_bwd_redo(cfg, x, dfeat, kept, hr_state=hr)
    assert torch.equal(kept, fixed)
    hr2 = ops.headroom_state(x.device); hr2[:24] = -24
    broken = ops.hashgrid_bwd_lines(cfg, x, dfeat, level_absmax=amax, hr_state=hr2)
    assert int(flag.item()) == 1, 'the forced overflow did not raise the flag'
    ops.hashgrid_bwd_redo(cfg, x, dfeat, broken, hr_state=hr2)
    assert float((broken - ref32).abs().max()) <= 1e-5 * float(ref32.abs().max())
    assert int(hr2[2 * 24 + 1].item()) >= 1                              # the repair ran
    _check_copies(cfg, broken.cpu().numpy().reshape(-1, 2))
    flag.zero_()


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
def test_line_layout_field_bwd_one_call_equals_three(ops, layout):
    from perf_amd.grid import MlpConfig
    cfg, _ = _cfg(layout, 18, (3, 3, 2), 64, 16)
    mlp = MlpConfig(n_levels=16, n_hidden_layers=1, n_output_dims=1, output_activation='Exponential')
    g = torch.Generator().manual_seed(3)
    n = 5003
    x = torch.rand(n, 3, generator=g).cuda()
    params = torch.cat([torch.randn(mlp.n_params, generator=g) * 0.2, (torch.rand(cfg.n_params, generator=g) * 2 - 1) * 1e-2]).cuda()
    cfg.canonicalize_(params[mlp.n_params:])
    w16 = ops.cast_params(params, 'bf16')
    feat = ops.hashgrid_fwd(cfg, x, w16[mlp.n_params:])
    dout = torch.randn(n, 1, generator=g).cuda()
    n_dev = torch.tensor([n - 3], dtype=torch.int64, device='cuda')
    for fixed in (False, True):
        hr_a, hr_b = ops.headroom_state(x.device), ops.headroom_state(x.device)
        ops.overflow_flag(x.device).zero_()
        one = ops.field_bwd(cfg, mlp, x, w16[:mlp.n_params], feat, dout, fixed=fixed, hr_state=hr_a if fixed else None, n_dev=n_dev).clone()
        ops.FIELD_BWD_ONE_CALL = False
        try:
            three = ops.field_bwd(cfg, mlp, x, w16[:mlp.n_params], feat, dout, fixed=fixed, hr_state=hr_b if fixed else None, n_dev=n_dev)
        finally:
            ops.FIELD_BWD_ONE_CALL = True
        if fixed:
            assert torch.equal(one, three) and torch.equal(hr_a, hr_b)
        else:
            assert torch.equal(one[:mlp.n_params], three[:mlp.n_params])
            assert float((one - three).abs().max()) <= 1e-5 * float(three.abs().max())
        _check_copies(cfg, one[mlp.n_params:].cpu().numpy().reshape(-1, 2))


def test_line_layout_entry_points_refuse_what_they_do_not_serve(ops):
    from perf_amd import _lib
    from perf_amd.grid import GridConfig
    tc = GridConfig()
    x = torch.rand(64, 3, device='cuda'); d = torch.zeros(16, 64, 2, device='cuda')
    with pytest.raises(ValueError, match='hashgrid_bwd'):
        ops.hashgrid_bwd_lines(tc, x, d)
    # the C entry point itself names the one a tcnn grid takes
    desc = tc.desc()
    out = torch.empty(tc.n_params, device='cuda')
    rc = _lib.load().perf_hashgrid_bwd_lines(desc, x.data_ptr(), d.data_ptr(), out.data_ptr(), 64, None, 0, None, None, None, None, 0,
                                             None, None, 0, None)
    assert rc != 0 and b'perf_hashgrid_bwd' in _lib.load().perf_last_error()
    cfg, _ = _cfg('line_local', 18, (3, 3, 2), 64, 16)
    with pytest.raises(_lib.PerfError):             # perf_hashgrid_bwd keeps refusing the line layouts
        ops.hashgrid_bwd(cfg, x, d)
    shifts = torch.zeros(24, dtype=torch.int32, device='cuda')
    ws = torch.empty(1 << 20, device='cuda')
    rc = _lib.load().perf_hashgrid_bwd_lines(cfg.desc(), x.data_ptr(), d.data_ptr(), out.data_ptr(), 64, None, 0, None, None, None,
                                             shifts.data_ptr(), 1, None, ws.data_ptr(), 4 << 20, None)
    assert rc != 0 and b'raw fields' in _lib.load().perf_last_error()
