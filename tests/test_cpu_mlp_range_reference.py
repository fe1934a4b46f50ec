"""The cases of tests/test_gpu_mlp_range.py have teeth, shown without a GPU (tests/mlp_range_reference.py:emulate).

1. The HONEST emulation -- torch on the CPU, real casts to the 16-bit type where the kernels round, fp32 sums, the ReLU mask from the
   rounded activation, the clamp on y - shift in the backward only, a masked sample 0 by selection -- equals the float64 reference
   with torch.equal on every case of parts A and B: the conditions the reference asserts are SUFFICIENT for a kernel that rounds where
   the kernels round.
2. Every emulation that is wrong on purpose differs from the reference -- by inequality, no exception -- on the cases named here:
     dY flushed below the smallest normal             every A case with edge 'dy_sub' or 'both_sub'
     dH flushed                                       the same cases
     hidden activations flushed                       every A case with edge 'h_sub' or 'both_sub'
     ReLU mask from the fp32 pre-activation           mask_case (both types); it EQUALS the reference on every A case, which is why
                                                      that case exists: pre-activations there are a quarter of a subnormal unit
     no clamp in the backward                         every Exponential case of B (dfeat or dw)
     clamp on y instead of y - shift                  every Exponential case of B, at shift 1 and at shift 19
     clamp in the forward too                         every Exponential case of B (the forward's bar, or inf expected)
     selector by multiplication                       every Exponential case of B: the masked row above the overflow point is NaN"""
import pytest
import torch

from tests import mlp_range_reference as R

A_CASES = [pytest.param(c, id=R.range_case_id(c)) for c in R.range_cases()]
B_CASES = [pytest.param(c, id=R.saturated_case_id(c)) for c in R.saturated_cases()]


def _same(got, want, live):
    """(out, dfeat, dw) against (out, dfeat, dw) over the live rows, to the bit; want[0] None: the forward is judged elsewhere"""
    ok = torch.equal(got[1][:, :live], want[1][:, :live]) and torch.equal(got[2], want[2])
    return ok and (want[0] is None or torch.equal(got[0][:live], want[0][:live]))


_A = {}


def _a_case(c):
    if c not in _A:
        dt, nh, n_out, L, n, sel_mode, ui = c
        cfgm, w, feat, sel, dout, s_feat, s_dout, edge = R.build_range_case(*c)
        info = {}
        ref = R._exact_reference(cfgm, w, feat, sel, dout, n, dt, activity=n >= 64, s_feat=s_feat, s_dout=s_dout, info=info)
        R.assert_edge_reached(edge, info, feat, dt)
        _A[c] = (cfgm, w, feat, sel, dout, n, dt), ref, edge
    return _A[c]


@pytest.mark.parametrize('c', A_CASES)
def test_the_honest_emulation_is_the_reference_across_the_range(c):
    args, ref, edge = _a_case(c)
    assert _same(R.emulate(*args), ref, args[5])
    # the ReLU mask from the fp32 pre-activation cannot be told from the packed one here (every pre-activation is exact in 16 bits)
    assert _same(R.emulate(*args, mask_from='pre'), ref, args[5])


@pytest.mark.parametrize('c', A_CASES)
def test_flushed_subnormals_fail_the_range_cases(c):
    args, ref, edge = _a_case(c)
    caught_by = {'dy': ('dy_sub', 'both_sub'), 'dh': ('dy_sub', 'both_sub'), 'h': ('h_sub', 'both_sub')}
    for what, edges in caught_by.items():
        same = _same(R.emulate(*args, flush=(what,)), ref, args[5])
        if edge in edges:
            assert not same, (what, edge)
        if edge in ('h_large', 'dy_large', 'top_h', 'top_dy', 'prod_sub'):       # (nothing of 16 bits is subnormal there)
            assert same, (what, edge)


def test_the_honest_emulation_is_the_reference_through_an_index():
    c, n_src = R.INDEXED_CASE, R.INDEXED_SRC
    cfgm, w, feat, sel, dout, s_feat, s_dout, edge = R.build_range_case(*c, n_src=n_src)
    index = R.indexed_rows(c[4], n_src)
    src = feat[:, index.long()]
    info = {}
    ref = R._exact_reference(cfgm, w, src, sel, dout, c[4], c[0], s_feat=s_feat, s_dout=s_dout, info=info)
    R.assert_edge_reached(edge, info, src, c[0])
    assert _same(R.emulate(cfgm, w, src, sel, dout, c[4], c[0]), ref, c[4])


@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_a_mask_from_the_pre_activation_fails_the_mask_case(dt):
    cfgm, w, feat, sel, dout = R.mask_case(dt)
    n = dout.shape[0]
    want = R.emulate(cfgm, w, feat, sel, dout, n, dt, acc=torch.float64)
    assert float(want[1].abs().max()) > 0 and float(want[2].abs().max()) > 0
    assert _same(R.emulate(cfgm, w, feat, sel, dout, n, dt), want, n)                      # fp32 sums: exact
    assert not _same(R.emulate(cfgm, w, feat, sel, dout, n, dt, mask_from='pre'), want, n)


def _forward_passes(out, k, act, shift):
    """the forward's rule of part B on an `out`: masked rows exactly 0, the rest within the bars"""
    live = k['sel'] != 0
    if not bool((out[~live] == 0).all()):
        return False
    y = k['y'][live]
    units, ok, _ = R.forward_units(out[live], y, act, shift)
    bars, masks = R.forward_bars(y, act, shift)
    return ok and all(not bool(m.any()) or float(units[m].max()) <= bar for (bar, _), m in zip(bars, masks))


@pytest.mark.parametrize('c', B_CASES)
def test_saturated_activations_on_the_emulation(c):
    dt, nh, n_out, L, act, shift, seed, wo_scale = c
    k = R.saturated_case(*c)
    args = (k['cfgm'], k['w'], k['feat'], k['sel'], k['g'], R.SAT_N, dt)
    want = (None, k['dfeat_ref'], k['dw_ref'])
    out, dfeat, dw = R.emulate(*args)
    assert _same((out, dfeat, dw), want, R.SAT_N)
    assert _forward_passes(out, k, act, shift)
    i_hi, i_mid = k['masked']
    assert float(dfeat[:, i_hi].abs().max()) == 0.0 and float(dfeat[:, i_mid].abs().max()) == 0.0
    if act != 'Exponential':
        return
    assert not _same(R.emulate(*args, clamp='none'), want, R.SAT_N)
    assert not _same(R.emulate(*args, clamp='y'), want, R.SAT_N)
    clamped = R.emulate(*args, fwd_clamp=True)
    assert _same(clamped, want, R.SAT_N) and not _forward_passes(clamped[0], k, act, shift)
    multiplied = R.emulate(*args, sel_by='multiply')
    assert _same(multiplied, want, R.SAT_N) and not _forward_passes(multiplied[0], k, act, shift)
    assert bool(torch.isnan(multiplied[0][i_hi]).any()) and float(multiplied[0][i_mid].abs().max()) == 0.0
