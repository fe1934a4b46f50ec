"""The backward of a field TO THE BIT, on inputs whose correct result is exactly representable.

A. The fixed-point table gradient is a table of INTEGERS: every contribution is rint(fl32(w g) 2^shift), integer sums do not depend
   on order, replica or rank.  oracle/perf_oracle.py:grid_fixed_fields restates that arithmetic in numpy (int64, the association of the
   weight product named per level class); the kernels -- coded, position-streaming and run-merging owners, replicas and their
   reduction, given and derived units, the closed headroom loop, the line layouts, perf_fixed_unfix -- must give the same integers.
   The kernel-against-kernel tests of tests/test_gpu_ops.py share one rounding, one packing and one unit rule; this file does not.
B. The MLP kernels round to 16 bits in a handful of places and add in fp32.  With small-integer features, sparse small-integer weights
   and small-integer output gradients every one of those roundings is exact, so a float64 forward + autograd is not an approximation
   of the right answer but THE answer: out, dfeat, dw and the level maxima are compared with torch.equal.  The conditions that make it
   so are asserted on the reference before the GPU is touched.

Every comparison in this file is an equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import perf_oracle as O  # noqa: E402
from tests import test_fixed_point_constants as FP  # noqa: E402     (the closed loop restated in Python: imported, not copied)
from tests import test_gpu_line_layout_grad as LL  # noqa: E402      (the line-layout cases, points and copy check)

FLAG_LEVEL = 1 << FP.C['flag']


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from perf_amd import ops as _ops
    return _ops


def _grid(interp='Linear', **kw):
    from perf_amd.grid import GridConfig
    cfg = GridConfig(interpolation=interp, **kw)
    lv = O.grid_levels(cfg.n_levels, 2, cfg.log2_hashmap_size, cfg.base_resolution, cfg.per_level_scale)
    assert lv.total == cfg.total and np.array_equal(lv.size, cfg.size)
    # hashed levels switch the association of the weight product at cell x = 16383 (grid_fixed_weights restates the rule per sample);
    # the grids of this file stay below it, so each level is of ONE class (finer grids, levels of more than 16 tiles and gradients
    # outside the unit cube: tests/test_gpu_exact_gradients_large.py)
    assert all(int(r) + 2 < 16384 for r in cfg.res)
    return cfg, lv


# ---- batches ------------------------------------------------------------------------------------------------------------------
def _ray_points(n, g):
    """ray-ordered samples: consecutive samples of a ray share cells on the coarse levels (runs, bursts on a few tiles)"""
    per = 64
    rays = -(-n // per)
    o = torch.rand(rays, 1, 3, generator=g) * 0.2 + 0.4
    d = torch.nn.functional.normalize(torch.randn(rays, 1, 3, generator=g), dim=-1)
    t = torch.linspace(0.0, 0.4, per)[None, :, None]
    return (o + d * t).reshape(-1, 3)[:n].clamp_(0.0, 1.0).contiguous()


def _face_points(cfg, n, g):
    """uniform points, then points ON cell faces of every level, the corners (0,0,0) and (1,1,1), and a few outside the unit cube"""
    x = torch.rand(n, 3, generator=g)
    k = 0
    for l in range(cfg.n_levels):
        s, r = float(cfg.scale[l]), int(cfg.res[l])
        for a in range(3):
            for m in (1, 2, 3, r // 2, r - 2, r - 1):
                v = (m - 0.5) / s                       # grid position = x * s + 0.5 lands on the integer m (up to one rounding)
                if 0.0 <= v <= 1.0 and k < n // 2:
                    x[k:k + 8, a] = v
                    k += 8
    x[-1] = 1.0
    x[-2] = 0.0
    x[-3] = torch.tensor([0.0, 1.0, 0.0])
    x[-8:-4] = torch.tensor([[-0.31, 0.5, 1.7], [5.0, -2.0, 0.2], [1.5, 1.5, 1.5], [-0.7, -0.2, 0.4]])
    return x


SIGNS = ('neg_pos', 'pos_neg', 'mixed', 'zero_level')


def _dfeat(cfg, x, g, signs, outside=False):
    """outside=True keeps the gradient of the samples outside the unit cube (tests/test_gpu_exact_gradients_large.py)"""
    d = torch.randn(cfg.n_levels, x.shape[0], 2, generator=g) * torch.logspace(-3, 1, cfg.n_levels)[:, None, None]
    if signs == 'neg_pos':                              # the packed pair: a negative low field borrows from the high one
        d[..., 0] = -d[..., 0].abs(); d[..., 1] = d[..., 1].abs()
    elif signs == 'pos_neg':
        d[..., 0] = d[..., 0].abs(); d[..., 1] = -d[..., 1].abs()
    elif signs == 'zero_level':
        d[cfg.n_levels // 2] = 0.0
    if not outside:                                     # (wrap-around outside the cube: tests/test_gpu_exact_gradients_large.py)
        d[:, ((x < 0) | (x > 1)).any(1)] = 0.0
    return d


def _shifts_for(x, dfeat, lv, interp, n_live, weights, top_bit=27):
    """units that put the largest FINAL field of every level just below 2^top_bit (the flag level is 2^29): a trial run of the oracle
    at units of 2^-12 of the largest contribution, then as many bits finer as fit"""
    trial = []
    for l in range(lv.n_levels):
        am = float(dfeat[l, :n_live].abs().max())
        trial.append(12 - int(np.ceil(np.log2(am))) if am > 0 else 0)
    m = O.fixed_field_max(O.grid_fixed_fields(x, dfeat, lv, trial, interp, n_live, weights=weights), lv)
    return [trial[l] + (top_bit - int(m[l] + 1).bit_length() if m[l] > 0 else 0) for l in range(lv.n_levels)]


def _dev_shifts(shifts):
    s = torch.zeros(24, dtype=torch.int32)
    s[:len(shifts)] = torch.tensor(shifts, dtype=torch.int32)
    return s.cuda()


def _assert_same_fields(got, want, lv, what):
    got = got.astype(np.int64)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        lvl = int(np.searchsorted(lv.offset.astype(np.int64), bad[0, 0], side='right') - 1)
        raise AssertionError(f'{what}: {len(bad)} of {want.size} fields differ, first at entry {bad[0, 0]} feature {bad[0, 1]} (level {lvl}): '
                             f'kernel {got[bad[0, 0], bad[0, 1]]} oracle {want[bad[0, 0], bad[0, 1]]}; '
                             f'largest difference {np.abs(got - want).max()} units')


def _check_raw(ops, cfg, lv, x, dfeat, interp, n_live, what, coarse=True, codes=(True, False), weights=None):
    """codes: the values of use_codes to run (a grid with levels on the global-atomics scatter without its bitmaps has no raw fields
    there); weights: grid_fixed_weights of x[:n_live] per level, for a caller that shares them between tests"""
    n = x.shape[0]
    if weights is None:
        weights = [O.grid_fixed_weights(x[:n_live].numpy(), lv, l, interp) for l in range(lv.n_levels)]
    fine = _shifts_for(x, dfeat, lv, interp, n_live, weights)
    xc, dc = x.cuda(), dfeat.cuda()
    n_dev = None if n_live == n else torch.tensor([n_live], dtype=torch.int64, device='cuda')
    flag = ops.overflow_flag(xc.device)
    # 10 bits coarser; and units of the size of the largest contribution itself, so that most contributions round to 0 or +-1
    unit = [1 - int(np.ceil(np.log2(float(dfeat[l, :n_live].abs().max())))) if bool(dfeat[l, :n_live].any()) else 0 for l in range(lv.n_levels)]
    for shifts in ([fine, [s - 10 for s in fine], unit] if coarse else [fine]):
        want = O.grid_fixed_fields(x, dfeat, lv, shifts, interp, n_live, weights=weights)
        m = O.fixed_field_max(want, lv)
        assert int(m.max()) < FLAG_LEVEL and (shifts is not fine or int(m.max()) >= 1 << 26)
        for use_codes in codes:                         # coded owners / position-streaming (and run-merging) owners
            flag.zero_()
            raw = ops.hashgrid_bwd(cfg, xc, dc, shifts=_dev_shifts(shifts), raw_fields=True, n_dev=n_dev, use_codes=use_codes)
            got = raw.view(torch.int32).view(-1, 2).cpu().numpy()
            _assert_same_fields(got, want, lv, f'{what}, {interp}, shifts {shifts}, use_codes={use_codes}')
            assert int(flag.item()) == 0


# ---- A1: given units, raw fields ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['Linear', 'Smoothstep'])
@pytest.mark.parametrize('batch', ['uniform', 'rays', 'faces', 'live'])
def test_raw_fields_equal_the_integer_oracle(ops, batch, interp):
    cfg, lv = _grid(interp)
    g = torch.Generator().manual_seed({'uniform': 1, 'rays': 2, 'faces': 3, 'live': 4}[batch])
    if batch == 'uniform':
        x = torch.rand(4099, 3, generator=g)
    elif batch == 'rays':
        x = _ray_points(65539, g)
    elif batch == 'faces':
        x = _face_points(cfg, 30001, g)
    else:
        x = torch.rand(20011, 3, generator=g)
    n_live = 12345 if batch == 'live' else x.shape[0]   # a live count below capacity (n_dev)
    for signs in SIGNS:
        _check_raw(ops, cfg, lv, x, _dfeat(cfg, x, g, signs), interp, n_live, f'{batch} / {signs}')


def test_raw_fields_of_the_benchmark_batch_equal_the_integer_oracle(ops):
    """2^20 ray-ordered samples on L16 / T18 -- the replicated coarse levels and their integer reduction, run merging, coded owners --
    whole and with a live count of 700,001"""
    cfg, lv = _grid('Linear')
    g = torch.Generator().manual_seed(5)
    x = _ray_points(1 << 20, g)
    dfeat = _dfeat(cfg, x, g, 'mixed')
    dfeat[3, :, 0] = -dfeat[3, :, 0].abs()             # one replicated level with a one-signed low field: carries between the replicas' sums
    _check_raw(ops, cfg, lv, x, dfeat, 'Linear', x.shape[0], 'benchmark batch', coarse=False)
    _check_raw(ops, cfg, lv, x, dfeat, 'Linear', 700001, 'benchmark batch, 700,001 live', coarse=False)
    # every level's low field negative beside a positive high field: the borrow of the packed pair through replicas and their reduction
    _check_raw(ops, cfg, lv, x, _dfeat(cfg, x, g, 'neg_pos'), 'Linear', x.shape[0], 'benchmark batch / neg_pos', coarse=False)


# ---- A2: derived units, the closed loop ---------------------------------------------------------------------------------------
def _amax24(dfeat, n_levels):
    a = torch.zeros(24)
    a[:n_levels] = dfeat.abs().amax(dim=(1, 2))
    return a


def _assert_table(got, fields, lv, shifts, what):
    """the float table a fixed-point call writes: fl32(field) * 2^-shift ((float)int32 rounds above 2^24; restated by the oracle)"""
    want = O.fixed_fields_to_float(fields, lv, shifts)
    got = got.detach().cpu().numpy().reshape(-1, 2)
    for l in range(lv.n_levels):
        lo, hi = int(lv.offset[l]), int(lv.offset[l]) + int(lv.size[l])
        if not np.array_equal(got[lo:hi], want[lo:hi]):
            bad = np.argwhere(got[lo:hi] != want[lo:hi])
            unit = 2.0 ** -shifts[l]
            raise AssertionError(f'{what}: level {l}: {len(bad)} of {2 * (hi - lo)} values differ; first: entry {bad[0, 0]} feature {bad[0, 1]} kernel '
                                 f'{got[lo + bad[0, 0], bad[0, 1]] / unit} oracle {want[lo + bad[0, 0], bad[0, 1]] / unit} units')


@pytest.mark.parametrize('interp', ['Linear', 'Smoothstep'])
def test_derived_units_and_the_closed_headroom_loop(ops, interp):
    cfg, lv = _grid(interp)
    L = cfg.n_levels
    g = torch.Generator().manual_seed(11)
    n, n_live = 30011, 29987
    x = torch.cat([_ray_points(20000, g), torch.rand(n - 20000, 3, generator=g)])
    base = _dfeat(cfg, x, g, 'mixed')
    xc = x.cuda()
    n_dev = torch.tensor([n_live], dtype=torch.int64, device='cuda')
    weights = [O.grid_fixed_weights(x[:n_live].numpy(), lv, l, interp) for l in range(L)]
    flag = ops.overflow_flag(xc.device)
    flag.zero_()
    # without state: the static fan-in guess
    amax = _amax24(base, L)
    shifts = [FP.fixed_point_shift(float(amax[l]), n_live, int(cfg.size[l])) for l in range(L)]
    fields = O.grid_fixed_fields(x, base, lv, shifts, interp, n_live, weights=weights)
    _assert_table(ops.hashgrid_bwd(cfg, xc, base.cuda(), level_absmax=amax.cuda(), n_dev=n_dev), fields, lv, shifts, 'no state')
    assert int(flag.item()) == 0
    # with state: five calls, the gradient jumps x8 and then drops /16; the units follow the restated loop, the state after every call
    # is the restated state (adjustment per level; the level maxima and the ticket are consumed by the call's own feedback)
    hr = ops.headroom_state(xc.device)
    adj = [0] * L
    for call, scale in enumerate((1.0, 1.0, 8.0, 0.5, 0.5)):
        d = base * scale                                # (a power of two: the same fp32 mantissas)
        amax = _amax24(d, L)
        shifts = [FP.fixed_point_shift(float(amax[l]), n_live, int(cfg.size[l]), adj[l]) for l in range(L)]
        fields = O.grid_fixed_fields(x, d, lv, shifts, interp, n_live, weights=weights)
        got = ops.hashgrid_bwd(cfg, xc, d.cuda(), level_absmax=amax.cuda(), n_dev=n_dev, hr_state=hr)
        _assert_table(got, fields, lv, shifts, f'call {call}')
        assert int(flag.item()) == 0, call
        fm = O.fixed_field_max(fields, lv)
        adj = [FP.headroom_feedback(adj[l], int(fm[l])) for l in range(L)]
        state = hr.cpu().tolist()
        assert state[:L] == adj, (call, state[:L], adj)
        assert not any(state[24:24 + L]) and state[48] == 0, (call, state[24:])
    assert len(set(adj)) > 1 and min(adj) < 0          # the loop moved, and not every level alike


# ---- A3: line layouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
@pytest.mark.parametrize('case', LL.CASES[:3], ids=LL.CASE_IDS[:3])
@pytest.mark.parametrize('interp', ['Linear', 'Smoothstep'])
def test_line_layout_fixed_point_table_equals_the_folded_integer_oracle(ops, layout, case, interp):
    log2_t, sb, min_res, L = case
    cfg, lv = LL._cfg(layout, log2_t, sb, min_res, L, interp)
    g = torch.Generator().manual_seed(7 + log2_t)
    n = 3001
    x = LL._points(cfg, n, g)
    dfeat = LL._dfeat(cfg, x, g)
    n_live = n - 6
    n_dev = torch.tensor([n_live], dtype=torch.int64, device='cuda')
    amax = _amax24(dfeat, L)
    shifts = [FP.fixed_point_shift(float(amax[l]), n_live, int(cfg.size[l])) for l in range(L)]
    fields = O.grid_fixed_fields(x, dfeat, lv, shifts, interp, n_live)
    assert np.abs(fields).max() > 1 << 12
    xc, dc = x.cuda(), dfeat.cuda()
    flag = ops.overflow_flag(xc.device); flag.zero_()
    for kw in ({}, {'use_codes': False}, {'use_owners': False}):
        got = ops.hashgrid_bwd_lines(cfg, xc, dc, n_dev=n_dev, level_absmax=amax.cuda(), **kw)
        _assert_table(got, fields, lv, shifts, f'{layout} {kw}')
        LL._check_copies(cfg, got.cpu().numpy().reshape(-1, 2))
    assert int(flag.item()) == 0
    # accumulate=True on a zeroed table is the overwriting call
    over = torch.zeros(cfg.n_params, device='cuda')
    ops.hashgrid_bwd_lines(cfg, xc, dc, out=over, n_dev=n_dev, level_absmax=amax.cuda())
    acc = torch.zeros(cfg.n_params, device='cuda')
    ops.hashgrid_bwd_lines(cfg, xc, dc, out=acc, accumulate=True, n_dev=n_dev, level_absmax=amax.cuda())
    _assert_table(acc, fields, lv, shifts, f'{layout} accumulate')
    assert torch.equal(acc, over)


# ---- A4: the data-parallel pieces ---------------------------------------------------------------------------------------------
def test_two_raw_tables_added_and_unfixed_on_a_slice(ops):
    cfg, lv = _grid('Linear')
    g = torch.Generator().manual_seed(13)
    n, cut = 30011, 11003
    x = torch.cat([_ray_points(15000, g), torch.rand(n - 15000, 3, generator=g)])
    dfeat = _dfeat(cfg, x, g, 'neg_pos')
    shifts = _shifts_for(x, dfeat, lv, 'Linear', n, None)
    want = O.grid_fixed_fields(x, dfeat, lv, shifts)
    sh = _dev_shifts(shifts)
    total = torch.zeros(cfg.n_params, dtype=torch.int32, device='cuda')
    for lo, hi in ((0, cut), (cut, n)):
        f = ops.hashgrid_bwd(cfg, x[lo:hi].contiguous().cuda(), dfeat[:, lo:hi].contiguous().cuda(), shifts=sh, raw_fields=True)
        total += f.view(torch.int32)                    # wrapping int32, as the reduce-scatter adds
    _assert_same_fields(total.view(-1, 2).cpu().numpy(), want, lv, 'sum of two raw tables')
    # a rank's slice: from the middle of level 2 to the middle of level 9
    e_lo = int(cfg.offset[2]) + 1001
    e_hi = int(cfg.offset[9]) + 70001
    shard = total.view(-1, 2)[e_lo:e_hi].clone()
    field_max = torch.full((24,), -1, dtype=torch.int32, device='cuda')
    flag = ops.overflow_flag('cuda'); flag.zero_()
    ops.fixed_unfix(cfg, shard, e_lo, e_hi, sh, field_max=field_max, flag=flag)
    got = shard.view(torch.float32).cpu().numpy()
    assert np.array_equal(got, O.fixed_fields_to_float(want, lv, shifts)[e_lo:e_hi])
    # largest |field| of the slice per level; a negative field v counts as -(v + 1) (fixed_unfix_kernel)
    fm = O.fixed_field_max(want, lv, e_lo, e_hi)
    assert field_max.cpu().tolist() == fm.tolist() + [0] * (24 - cfg.n_levels)
    assert fm[:2].sum() == 0 and fm[2:10].min() > 0 and fm[10:].sum() == 0 and int(flag.item()) == 0


# ---- B: exact-arithmetic cases of the MLP kernels -------------------------------------------------------------------------------
# (the cases' builders, the float64 reference and its conditions live in tests/mlp_range_reference.py, with the units as arguments
#  whose defaults are this file's: features are integers times 2^-2, output gradients integers times 2^-3)
from tests.mlp_range_reference import DT, MIN_NORMAL, S_DOUT, S_FEAT, _check_exact_mlp, _exact_mlp, _exact_reference, _half_maxima, _sparse_int  # noqa: E402,F401


ARCHS = [(1, 1), (1, 16), (2, 3), (2, 16)]
LEVELS = [5, 8, 16, 20, 24]                  # padded inputs; one, two, three k-steps
SIZES = [1, 40, 4003, 300017]
SELS = ['zeros', 'ones', None]


def _exact_cases():
    """every (dtype, network, levels); n and the selector's form cycle so that each size and each form meets each network, each dtype
    and each input width"""
    cases = []
    for di, dt in enumerate(DT):
        for ai, (nh, n_out) in enumerate(ARCHS):
            for li, nl in enumerate(LEVELS):
                n = SIZES[(ai + li + di) % 4]
                sel = SELS[(ai + 2 * li + di) % 3]
                cases.append(pytest.param(dt, nh, n_out, nl, n, sel, id=f'{dt}-nh{nh}-o{n_out}-L{nl}-n{n}-sel_{sel}'))
    return cases


@pytest.mark.parametrize('dt,nh,n_out,n_levels,n,sel_mode', _exact_cases())
def test_mlp_kernels_are_exact_on_exactly_representable_data(ops, dt, nh, n_out, n_levels, n, sel_mode):
    cfgm, w, feat, sel, dout = _exact_mlp(dt, nh, n_out, n_levels, max(n, 64), 100 + n_levels + n_out, sel_mode)
    # (the shares of active / tied units are conditions on a population: a batch of fewer than 64 samples is the head of one -- the
    #  rows with the largest gradients first, so that a batch of ONE is not a sample whose hidden units all rest)
    if n < 64:
        _, dfeat_pop, _ = _exact_reference(cfgm, w, feat, sel, dout, 64, dt)
        order = dfeat_pop.abs().sum(dim=(0, 2)).argsort(descending=True)[:n]
        feat, dout = feat[:, order].contiguous(), dout[order].contiguous()
        sel = None if sel is None else sel[order].contiguous()
        z0 = feat[:, 0].reshape(-1).double() @ w[:64 * cfgm.n_in_pad].view(64, -1)[:, :2 * n_levels].double().t()
        assert bool((z0 > 0).any()) and bool((z0 == 0).any()) and bool((z0 < 0).any())      # (the first row alone: a batch of ONE has all three)
    _check_exact_mlp(ops, dt, cfgm, w, feat, sel, dout, activity=n >= 64)


@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('nh,n_out,n_levels,n,n_live', [(1, 16, 16, 4003, 3970), (2, 3, 16, 4003, 3999), (1, 1, 20, 300017, 150001), (2, 16, 8, 40, 33),
                                                        (2, 3, 5, 4003, 1)])
def test_mlp_kernels_are_exact_below_a_live_count(ops, dt, nh, n_out, n_levels, n, n_live):
    """rows past the device count must not contribute to dw (their dout, features and selector are as live as the others')"""
    cfgm, w, feat, sel, dout = _exact_mlp(dt, nh, n_out, n_levels, max(n, 64), 200 + n_levels, 'zeros')
    _exact_reference(cfgm, w, feat, sel, dout, max(n, 64), dt)          # (the population conditions, on the whole batch)
    if n < 64:
        feat, dout, sel = feat[:, :n].contiguous(), dout[:n].contiguous(), sel[:n].contiguous()
    _check_exact_mlp(ops, dt, cfgm, w, feat, sel, dout, n_live=n_live, activity=n_live >= 64)


@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('nh,n_out,n_levels', [(1, 16, 16), (2, 3, 16), (1, 1, 8), (2, 16, 20)])
def test_mlp_backward_through_an_index_is_exact(ops, dt, nh, n_out, n_levels):
    """IndexedFeat: features of MORE rows than the batch means, and an index that repeats rows and skips others"""
    n, n_src = 4003, 6000
    cfgm, w, feat, sel, dout = _exact_mlp(dt, nh, n_out, n_levels, n, 300 + n_levels, 'zeros', n_src=n_src)
    g = torch.Generator().manual_seed(9)
    index = torch.randint(0, n_src // 2, (n,), generator=g) * 2          # even rows only, many of them twice
    index[:8] = index[8]
    index[-1] = n_src - 1
    index = index.to(torch.int32)
    assert len(set(index.tolist())) < n
    _check_exact_mlp(ops, dt, cfgm, w, feat, sel, dout, index=index)
    _check_exact_mlp(ops, dt, cfgm, w, feat, sel, dout, n_live=n - 37, index=index)


# ---- the field backward to the bit, end to end ----------------------------------------------------------------------------------
@pytest.mark.parametrize('one_call', [True, False])
@pytest.mark.parametrize('dt,nh,n_out', [('bf16', 1, 1), ('bf16', 2, 3), ('fp16', 1, 16), ('fp16', 2, 3)])
def test_field_backward_to_the_bit(ops, dt, nh, n_out, one_call):
    """ops.field_bwd on the exact data: the network part is the float64 reference, the grid part is the integer oracle on the reference's
    dfeat with the units the kernels derive from the reference's level maxima (closed loop, fresh state)."""
    _field_backward_to_the_bit(ops, dt, nh, n_out, one_call, S_DOUT)


@pytest.mark.parametrize('one_call', [True, False])
@pytest.mark.parametrize('nh,n_out', [(1, 16), (2, 3)])
def test_field_backward_to_the_bit_on_subnormal_output_gradients(ops, nh, n_out, one_call):
    """the same in fp16 with output gradients of integers times 2^-24 (what a small per-sample gradient is after the loss scale): dY and
    every dH are fp16 subnormals, and the level maxima of a dfeat of that size still drive the fixed-point units to the oracle's table"""
    _field_backward_to_the_bit(ops, 'fp16', nh, n_out, one_call, 2.0 ** -24)


def _field_backward_to_the_bit(ops, dt, nh, n_out, one_call, s_dout):
    tdt, _ = DT[dt]
    cfg, lv = _grid('Linear')
    L = cfg.n_levels
    n, n_live = 4003, 3990
    cfgm, w, feat, sel, dout = _exact_mlp(dt, nh, n_out, L, n, 400 + n_out, 'zeros', s_dout=s_dout)
    info = {}
    out_ref, dfeat_ref, dw_ref = _exact_reference(cfgm, w, feat, sel, dout, n_live, dt, s_dout=s_dout, info=info)
    if s_dout != S_DOUT:                                 # the edge is reached: every dY and every dH is subnormal in the type
        assert all(float(d.abs().max()) < MIN_NORMAL[dt] for d in info['dz'] + [info['dy']]) and float(dfeat_ref.abs().max()) < MIN_NORMAL[dt]
    g = torch.Generator().manual_seed(17)
    x = torch.cat([_ray_points(2000, g), torch.rand(n - 2000, 3, generator=g)])
    amax, _ = _half_maxima(dfeat_ref[:, :n_live], L)
    shifts = [FP.fixed_point_shift(float(amax[l]), n_live, int(cfg.size[l]), 0) for l in range(L)]
    fields = O.grid_fixed_fields(x, dfeat_ref, lv, shifts, 'Linear', n_live)
    hr = ops.headroom_state('cuda')
    flag = ops.overflow_flag('cuda'); flag.zero_()
    n_dev = torch.tensor([n_live], dtype=torch.int64, device='cuda')
    ops.FIELD_BWD_ONE_CALL = one_call
    try:
        grad = ops.field_bwd(cfg, cfgm, x.cuda(), w.to(tdt).cuda(), feat.to(tdt).cuda(), dout.cuda(), sel=sel.cuda(), fixed=True, redo=True,
                             hr_state=hr, n_dev=n_dev).clone()
    finally:
        ops.FIELD_BWD_ONE_CALL = True
    assert int(flag.item()) == 0
    assert torch.equal(grad[:cfgm.n_params].cpu(), dw_ref)
    _assert_table(grad[cfgm.n_params:], fields, lv, shifts, 'field_bwd')
    fm = O.fixed_field_max(fields, lv)
    assert hr.cpu().tolist()[:L] == [FP.headroom_feedback(0, int(fm[l])) for l in range(L)]



# ---- the forward on exact data: encode, fused and two-kernel inference ------------------------------------------------------------
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('nh,n_out,L', [(1, 1, 16), (2, 3, 16), (1, 16, 5), (2, 16, 8)])
def test_field_inference_is_exact_on_exactly_representable_data(ops, dt, nh, n_out, L):
    _field_inference_is_exact(ops, dt, nh, n_out, L, 1.0)


@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('nh,n_out,L', [(1, 1, 16), (2, 16, 8)])
def test_field_inference_is_exact_on_subnormal_features(ops, dt, nh, n_out, L):
    """the same with the table scaled by a power of two that puts every feature below the type's smallest normal: the encoding's one
    rounding is then a rounding to the subnormals' spacing (nearest, ties to even: torch's CPU cast and the kernels' pack alike), the
    first layer's operands and the hidden activations are subnormals"""
    _field_inference_is_exact(ops, dt, nh, n_out, L, MIN_NORMAL[dt])


def _field_inference_is_exact(ops, dt, nh, n_out, L, table_unit):
    """field_infer (one fused kernel up to FUSED_MAX_SAMPLES rows, encode + MLP beyond), hashgrid_fwd and mlp_fwd against a float64
    forward.  The grid doubles its resolution per level (scale = 16 * 2^l - 1, an integer) and the points are multiples of 1/16, so
    every fraction is a multiple of 1/16 and every trilinear weight a multiple of 2^-12; the table holds integers / 4.  Every
    fp32 sum of the encoding is then exact whatever its order: the 16-bit features are the float64 encoding rounded once, bit for
    bit, and the network on those features -- sparse integer weights, hidden activations rounded to 16 bits -- is exact in turn."""
    from perf_amd.grid import GridConfig
    tdt, _ = DT[dt]
    cfg = GridConfig(n_levels=L, log2_hashmap_size=15, base_resolution=16, per_level_scale=2.0)
    lv = O.grid_levels(L, 2, 15, 16, 2.0)
    assert lv.total == cfg.total and all(float(cfg.scale[l]) == 16 * 2 ** l - 1 == float(lv.scale[l]) for l in range(L))
    cfgm, w, _, _, _ = _exact_mlp(dt, nh, n_out, L, 64, 500 + L + n_out, 'ones')
    g = torch.Generator().manual_seed(23)
    table = torch.randint(-2, 3, (cfg.total, 2), generator=g).float() * 0.25 * table_unit
    w16 = torch.cat([w, table.reshape(-1)]).to(tdt).cuda()
    assert torch.equal(w16.cpu().double(), torch.cat([w, table.reshape(-1)]).double())
    Ws, off = [], 0
    for o, i in cfgm.shapes:
        Ws.append(w[off:off + o * i].view(o, i).double())
        off += o * i
    q = 2.0 ** 14 / table_unit                             # everything below is an integer number of 2^-14 table units
    for n in (1, 37, ops.FUSED_MAX_SAMPLES, ops.FUSED_MAX_SAMPLES + 817):
        x = torch.randint(0, 17, (n, 3), generator=g).float() / 16.0
        x[0] = torch.tensor([0.0, 1.0, 0.5])
        sel = (torch.rand(n, generator=g) > 0.1).to(torch.uint8)
        sel[0] = 1
        # ---- the reference, and the conditions that make it THE answer
        enc64 = O.hashgrid_encode(x, table.double(), lv, 'Linear')                 # fp32 weights, float64 products and sums: exact
        assert enc64.dtype == torch.float64 and torch.equal((enc64 * q).round(), enc64 * q) and float(enc64.abs().max()) <= 0.5 * table_unit
        enc = O.hashgrid_encode(x, table, lv, 'Linear', quant=dt)                  # the oracle's emulation: the same numbers in fp32
        assert torch.equal(enc.double(), enc64)
        feat_ref = enc.to(tdt)                                                     # [n, 2L]: ONE rounding to the storage type
        if table_unit != 1.0:                                                      # the edge is reached: features subnormal, most of them non-zero
            assert float(feat_ref.float().abs().max()) < MIN_NORMAL[dt] and float((feat_ref != 0).float().mean()) > 0.5
        h = torch.cat([feat_ref.double(), torch.zeros(n, cfgm.n_in_pad - 2 * L, dtype=torch.float64)], 1)
        for W in Ws[:-1]:
            assert float((h.abs() @ W.abs().t()).max()) * q < 2 ** 24              # every fp32 sum exact
            h = torch.relu(h @ W.t()).to(tdt).double()                             # hidden activations: rounded to 16 bits (the kernels' rounding)
        assert float((h.abs() @ Ws[-1].abs().t()).max()) * q < 2 ** 24
        out_ref = ((h @ Ws[-1].t())[:, :n_out] * sel.double()[:, None])
        assert torch.equal(out_ref.float().double(), out_ref) and float(out_ref.abs().max()) > 0
        out_ref = out_ref.float()
        level_major = feat_ref.view(n, L, 2).permute(1, 0, 2).contiguous()
        # ---- the kernels
        xc, sc = x.cuda(), sel.cuda()
        out, feat = ops.field_infer(cfg, cfgm, xc, sc, w16, want_features=True)    # fused up to FUSED_MAX_SAMPLES rows, two kernels beyond
        out_only = ops.field_infer(cfg, cfgm, xc, sc, w16)
        feat2 = ops.hashgrid_fwd(cfg, xc, w16[cfgm.n_params:])                     # the two kernels one by one
        out2 = ops.mlp_fwd(cfgm, w16[:cfgm.n_params], feat2, sc)
        out_given = ops.mlp_fwd(cfgm, w16[:cfgm.n_params], level_major.cuda(), sc) # the MLP given the reference's features
        for name, f in (('field_infer', feat), ('hashgrid_fwd', feat2)):
            assert torch.equal(f.cpu().view(torch.int16), level_major.view(torch.int16)), (name, n, int((f.cpu() != level_major).sum()))
        for name, o in (('field_infer + features', out), ('field_infer', out_only), ('hashgrid_fwd + mlp_fwd', out2), ('mlp_fwd', out_given)):
            assert torch.equal(o.cpu(), out_ref), (name, n, int((o.cpu() != out_ref).sum()))
