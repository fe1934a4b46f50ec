"""The MLP kernels at the ends of the 16-bit range and where the output activation saturates (tests/mlp_range_reference.py holds the
cases, their float64 references and the conditions; tests/test_cpu_mlp_range_reference.py shows on the CPU that each case has teeth).

A. Scale invariance, to the bit.  The exact cases of tests/test_gpu_exact_gradients.py part B -- small integers times a unit -- with
   the units moved by powers of two so that ONE named quantity sits at an end of the type while every rounding stays exact: features
   and hidden activations subnormal (the ReLU pack, the "packed activation is not zero" mask, the MFMA B operands), dY and every dH
   subnormal (pack_active, the dY pack, the MFMA A operands), both at once, the largest hidden pre-activation or gradient in the top
   binade of fp16 or at 2^100 in bf16, and in bf16 operands that are fp32 subnormals as well.  out, dfeat, dw and the level maxima
   are compared with torch.equal against the float64 forward + autograd; that the edge is reached is asserted on the reference first.
   One case goes through ops.IndexedFeat; one more (mask_case) makes "packed activation != 0" and "pre-activation > 0" differ.
B. Output activations where they saturate.  At a feature unit of 2 the network output y is an even integer spread over +-100 and
   more, exactly known.
   forward   against the float64 activation rounded once to fp32, in units of 2^-24 |T| (floor: one fp32 subnormal).  The bar is 4 x
             the worst error of torch's CPU fp32 exp / sigmoid on the same y (at least 4 units), computed in the test, separately
             over the entries whose T is a normal number and over those whose T is subnormal; inf where T is inf; at most one
             subnormal unit, not negative, where T rounds to 0; never NaN.  A masked sample is exactly 0 whatever the network says --
             one masked row lies above the exponential's overflow point, where act(y) * 0 was NaN.
   backward  the "compensated" gradient g = fl32(r / act'(y)) for small integers r times 2^-3: dY = g act'(y) rounds to r again for
             any reasonable expf, so dfeat, dw and the level maxima are compared with torch.equal against the float64 LINEAR backward
             of r.  Exponential: rows down to y - shift = -80, above the clamp at 15 and above the forward's overflow point; exp_shift
             1 and 19 (which tells "clamp y - shift" from "clamp y").  Sigmoid: |y| <= 6.  Entries outside get g = 0 and must
             contribute exact zeros.
   Sigmoid with g of order 1 on all rows, |y| up to 200: finite, and within twice the 16-bit emulation's noise per block
   (tests/test_gpu_ops.py:_assert_blocks_within_twice_the_emulation_noise, imported).

Every comparison in A and in B's backward is an equality.  Measured on an MI355X, the forward's worst error in units of 2^-24 |T|,
kernel / torch CPU emulation, over all networks of a type (the bar is 4 x the emulation's, per case, at least 4), bf16 and fp16 alike
(the activation runs in fp32 on the same exact y):
    Exponential, T normal      1.749 / 0.000   (252,212 entries; torch's exp is correctly rounded on these integer arguments: bar 4)
    Exponential, T subnormal   0.000 / 0.000   (3,722 entries)
    Sigmoid, T normal          1.984 / 1.984   (127,877 entries)
    Sigmoid, T subnormal       584,744 / 584,744   (785 entries: y in [-103, -89], where expf(-y) is inf and both give 0 for a T of up
                                                    to 2^-130 -- the tail an fp32 sigmoid of this form does not have)
Part A found nothing to fix: neither the 16-bit packs nor the MFMA operands flush a subnormal on gfx950, in either type; every case
passed as written.  The masked row above the overflow point is the case the forward's epilogue had to change for: it wrote act(y) * sel, inf * 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mlp_range_reference as R  # noqa: E402
from tests.test_gpu_ops import _assert_blocks_within_twice_the_emulation_noise  # noqa: E402     (imported, not copied)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from perf_amd import ops as _ops
    return _ops


# ---- A ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [pytest.param(c, id=R.range_case_id(c)) for c in R.range_cases()])
def test_mlp_kernels_are_exact_at_the_ends_of_the_range(ops, c):
    dt, nh, n_out, L, n, sel_mode, ui = c
    cfgm, w, feat, sel, dout, s_feat, s_dout, edge = R.build_range_case(*c)
    info = {}
    out_ref, dfeat_ref, dw_ref = R._exact_reference(cfgm, w, feat, sel, dout, n, dt, activity=n >= 64, s_feat=s_feat, s_dout=s_dout, info=info)
    R.assert_edge_reached(edge, info, feat, dt)
    out, back = R._run_kernels(ops, dt, cfgm, w, feat, sel, dout)
    assert torch.equal(out, out_ref), int((out != out_ref).sum())
    R._assert_backward_equal(cfgm, back, (dfeat_ref, dw_ref), n)


def test_mlp_backward_through_an_index_is_exact_on_subnormals(ops):
    c, n_src = R.INDEXED_CASE, R.INDEXED_SRC
    dt, n = c[0], c[4]
    cfgm, w, feat, sel, dout, s_feat, s_dout, edge = R.build_range_case(*c, n_src=n_src)
    index = R.indexed_rows(n, n_src)
    info = {}
    _, dfeat_ref, dw_ref = R._exact_reference(cfgm, w, feat[:, index.long()], sel, dout, n, dt, s_feat=s_feat, s_dout=s_dout, info=info)
    R.assert_edge_reached(edge, info, feat[:, index.long()], dt)
    _, back = R._run_kernels(ops, dt, cfgm, w, feat, sel, dout, index=index)
    R._assert_backward_equal(cfgm, back, (dfeat_ref, dw_ref), n)


@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_the_relu_mask_is_the_packed_activation(ops, dt):
    """pre-activations of a quarter, a half and three quarters of the type's smallest subnormal: the first two pack to 0 and their
    units are INACTIVE in the backward although the fp32 pre-activation is positive (what tcnn's backward does with its stored 16-bit
    activations).  The expectation is the CPU emulation with float64 sums (tests/mlp_range_reference.py:mask_case)."""
    cfgm, w, feat, sel, dout = R.mask_case(dt)
    n = dout.shape[0]
    out_ref, dfeat_ref, dw_ref = R.emulate(cfgm, w, feat, sel, dout, n, dt, acc=torch.float64)
    out, back = R._run_kernels(ops, dt, cfgm, w, feat, sel, dout)
    assert torch.equal(out, out_ref), int((out != out_ref).sum())
    R._assert_backward_equal(cfgm, back, (dfeat_ref, dw_ref), n)


# ---- B ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [pytest.param(c, id=R.saturated_case_id(c)) for c in R.saturated_cases()])
def test_saturated_output_activations(ops, c):
    dt, nh, n_out, L, act, shift, seed, wo_scale = c
    k = R.saturated_case(*c)                             # (asserts its conditions on the reference)
    n = R.SAT_N
    out, back = R._run_kernels(ops, dt, k['cfgm'], k['w'], k['feat'], k['sel'], k['g'])
    # ---- forward: masked rows exactly 0 -- the two masked on purpose among them --, the others within the bars
    live = k['sel'] != 0
    i_hi, i_mid = k['masked']
    assert not bool(live[i_hi]) and not bool(live[i_mid])
    assert not bool(torch.isnan(out).any()), int(torch.isnan(out).sum())
    assert bool((out[~live] == 0).all())
    y = k['y'][live]
    units, ok, T = R.forward_units(out[live], y, act, shift)
    bars, masks = R.forward_bars(y, act, shift)
    for name, (bar, emu), m in zip(('normal T', 'subnormal T'), bars, masks):
        worst = float(units[m].max()) if bool(m.any()) else 0.0
        print(f'[mlp range forward] {R.saturated_case_id(c)} {name}: {int(m.sum())} entries, kernel {worst:.3f} units, emulation {emu:.3f}, bar {bar:.3f}; '
              f'{int(torch.isinf(T).sum())} inf, {int((T == 0).sum())} zero')
    assert ok, 'inf where T is inf; in [0, 2^-149] where T rounds to 0; finite and not negative elsewhere'
    for (bar, _), m in zip(bars, masks):
        assert not bool(m.any()) or float(units[m].max()) <= bar
    # ---- backward: the linear backward of r, to the bit; the masked rows' dfeat exactly 0
    dfeat = back[0]
    assert float(dfeat[:, ~live].abs().max()) == 0.0
    R._assert_backward_equal(k['cfgm'], back, (k['dfeat_ref'], k['dw_ref']), n)


@pytest.mark.parametrize('c', [pytest.param(c, id=R.saturated_case_id(c)) for c in R.saturated_cases() if c[4] == 'Sigmoid'])
def test_sigmoid_backward_beyond_the_compensated_range(ops, c):
    """g of order 1 on every row: the derivative s (1 - s) runs from 1/4 down through the fp32 and 16-bit subnormals to exactly 0
    (1 - s is 0 from y = 17 on, s is 0 where expf(-y) overflows).  Every output finite; per block within twice the emulation's noise."""
    dt = c[0]
    k = R.saturated_case(*c)
    tdt, _ = R.DT[dt]
    g = torch.Generator().manual_seed(31)
    dout = torch.randn(R.SAT_N, k['cfgm'].n_output_dims, generator=g)
    assert float(k['y'].abs().max()) >= 89.0
    out, (dfeat, dw, amax) = R._run_kernels(ops, dt, k['cfgm'], k['w'], k['feat'], k['sel'], dout)
    for t in (out, dfeat, dw, amax):
        assert bool(torch.isfinite(t).all())
    _assert_blocks_within_twice_the_emulation_noise(f'sigmoid {R.saturated_case_id(c)}', k['cfgm'], k['w'].to(tdt), k['feat'].to(tdt), k['sel'], dt,
                                                    out, dout, dfeat, dw)
