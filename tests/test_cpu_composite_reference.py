"""The float64 reference of tests/composite_reference.py against the fp32 oracle and against the closed forms in the kernel
comments, the fp32 emulation's worst error in units of the rounding majorant, and the proof that the bar of
tests/test_gpu_composite_float64.py (four times the emulation's worst) notices a subtly wrong kernel: eight deliberately wrong
variants of the emulation each exceed it on the GPU test's own inputs."""
import functools

import numpy as np
import pytest
import torch

from oracle import perf_oracle as O
from tests import composite_reference as CR

MARGIN = 4.0


@functools.lru_cache(maxsize=None)
def _case(gain, tail_empty=False):
    return CR.make_case(gain, tail_empty)


@functools.lru_cache(maxsize=None)
def _clean(gain, tail_empty=False):
    return CR.emulation_worst(_case(gain, tail_empty))


def test_batch_holds_every_shape_the_kernels_branch_on():
    c = _case(1.0)
    n = c.counts
    assert c.R == 203 and c.R % 4 != 0 and int(n.max()) == 200
    assert {0, 1, 63, 64, 65, 128, 129, 199}.issubset(set(n.tolist()))
    assert int(n[0:16].max()) <= 4 and int(n[16:20].max()) <= 16 and int(n[16:20].max()) > 4
    assert sorted(n[20:24].tolist())[-1] > 16 and sorted(n[20:24].tolist())[-2] <= 16           # a group of four broken by one long ray
    assert (n[32:48] > 4).sum() == 1                                                            # a group of sixteen broken by one long ray
    assert c.S < 32 * c.R                                                                       # the ray head runs by teams
    for r in range(c.R):                                                                        # sorted, disjoint samples
        lo, k = int(c.packed[r, 0]), int(n[r])
        if k >= 2:                                                                              # (adjacent cells meet to an fp32 rounding)
            assert np.all(c.ts[lo + 1:lo + k] > c.ts[lo:lo + k - 1]) and np.all(c.ts[lo + 1:lo + k] >= c.te[lo:lo + k - 1] - 1e-6)
        assert np.all(c.te[lo:lo + k] > c.ts[lo:lo + k])
    t = _case(1.0, True)
    assert t.last == c.R - CR.TAIL_EMPTY - 1 and CR.TAIL_EMPTY >= 70 and np.array_equal(t.sig[:t.S], c.sig[:t.S])
    long = CR.sub_case(c)
    assert long.S >= 32 * long.R and long.R % 4 != 0 and {0, 1, 64, 65, 200}.issubset(set(long.counts.tolist()))      # the ray head without teams
    for key, u in CR.emulation_worst(long).items():
        assert np.isfinite(u) and u < 64, key
    f = CR.truth_fwd(_case(20.0))['_']
    assert float(f['ex'].max()) > 1000 and bool((f['T'] == 0).any()) and bool(((f['T'] > 0) & (f['T'] < 2.0 ** -126)).any())


@pytest.mark.parametrize('gain', CR.GAINS)
@pytest.mark.parametrize('noise_on,bg_on', [(True, True), (False, False)])
def test_no_ray_sits_on_a_kink(gain, noise_on, bg_on):
    for tail in (False, True):
        c = _case(gain, tail)
        md, mpre, mc, n_neg, n_empty_pos, mlive = CR.kink_margins(c, CR.make_loss_inputs(c), noise_on, bg_on)
        assert md >= 0.25 and mc >= 0.25, (md, mc)
        if noise_on:
            assert mpre >= 1e-3, mpre
            assert n_neg >= 8 and n_empty_pos == int((c.counts == 0).sum()) > 0
        else:
            # without noise pre IS the distance, a sum of products of positive numbers: exactly 0 on a ray without samples in either
            # arithmetic (relu' = 0 there in both), positive and far above the fp32 underflow on every other ray -- no rounding moves it
            assert mpre == 0.0 and n_neg == 0 and mlive >= 1e-12, (mpre, mlive)
        ref = CR.truth_head_geo(c, CR.make_loss_inputs(c)['gt_noise' if noise_on else 'gt_plain'],
                                CR.make_loss_inputs(c)['noise'] if noise_on else None, c.R, CR.RATIO)
        live = ref['_pre'] > 0
        assert bool(ref['_quad'][live].any()) and bool((~ref['_quad'][live]).any())             # both smooth-L1 branches


def test_truth_agrees_with_the_fp32_oracle_on_thin_rays():
    c = _case(0.05)
    fw = CR.truth_fwd(c)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x[:c.S]))
    w, T, al = O.render_weight_from_density(t(c.ts), t(c.te), t(c.sig), c.packed)
    ri = torch.from_numpy(c.ri)
    op = O.accumulate_along_rays(w, None, ri, c.R)
    dist = O.accumulate_along_rays(w, ((t(c.ts) + t(c.te)) / 2)[:, None], ri, c.R)
    col = O.accumulate_along_rays(w, t(c.rgb), ri, c.R)
    for got, name in ((w, 'w'), (T, 'T'), (al, 'alphas'), (op, 'opacity'), (dist, 'distance'), (col, 'colour')):
        truth = fw[name][0]
        err = float(np.max(np.abs(got.numpy().reshape(truth.shape).astype(np.float64) - truth)))
        assert err <= 2e-6 * max(1.0, float(np.abs(truth).max())), (name, err)
    # the distortion loss through the oracle's own function, in float64: the same number
    td = lambda x: t(x).double()
    mid, sec = (td(c.ts) + td(c.te)) / 2, td(c.te) - td(c.ts)
    want = float(O.flatten_eff_distloss(torch.from_numpy(fw['w'][0]), mid, sec, ri))
    per = CR.distloss_parts(c, fw['w'][0])[0]
    assert abs(per.sum() / (c.last + 1) - want) <= 1e-12 * abs(want)
    # ... and the float64 loss heads against oracle.geo_step_loss / app_step_loss called on float64 tensors
    li = CR.make_loss_inputs(c)
    out = {'distance': torch.from_numpy(fw['distance'][0]), 'weights': torch.from_numpy(fw['w'][0]), 't_starts': td(c.ts), 't_ends': td(c.te),
           'ray_indices': ri}
    loss, dl, distl = O.geo_step_loss(out, torch.from_numpy(li['gt_plain'].astype(np.float64)), CR.RATIO / 2, CR.DEPTH_W, CR.DIST_W, CR.LOSS_SCALE)
    hd = CR.truth_head_geo(c, li['gt_plain'], None, c.R, CR.RATIO)
    for a, b in zip((float(loss), float(dl), float(distl)), hd['_loss']):
        assert abs(a - b) <= 1e-12 * abs(a)
    closs, cl = O.app_step_loss({'rgb': torch.from_numpy(fw['colour'][0])}, torch.from_numpy(li['gtc_plain'].astype(np.float64)), CR.COLOR_W, CR.LOSS_SCALE)
    ap = CR.truth_app_loss(c, fw['opacity'][0], fw['colour'][0], None, li['gtc_plain'], c.R)
    assert abs(ap['loss'][0] - float(cl)) <= 1e-12 * float(cl)


@pytest.mark.parametrize('gain', CR.GAINS)
def test_closed_form_gradients_equal_float64_autograd(gain):
    """d sigma and the distortion-loss gradient of the kernel comments, evaluated in float64, against autograd: to 1e-12 of the
    gradient's majorant element by element (an opaque ray's late samples have no other scale) and of its largest entry overall."""
    c = _case(gain)
    gi = CR.grads_in(c)
    f = CR.truth_fwd(c)['_']
    ref = CR.truth_bwd(c, **gi)
    g64 = {k: v.astype(np.float64) for k, v in gi.items()}
    G = g64['g_w'] + g64['g_op'][c.ri] + g64['g_d'][c.ri] * f['m']
    closed = CR.dsigma_closed(c, f, G, g64['g_T'], g64['g_al'])
    auto, A, _ = ref['d_sigma']
    assert bool(np.all(np.abs(closed - auto) <= 1e-12 * A)) and float(np.abs(closed - auto).max()) <= 1e-12 * float(np.abs(auto).max())
    assert bool(np.all(np.abs(f['w'][:, None] * g64['g_col'][c.ri] - ref['d_rgb'][0]) <= 1e-12 * ref['d_rgb'][1]))
    # distortion loss: autograd of the per-ray sums w.r.t. the weights
    g = CR._Graph(c)
    w = torch.from_numpy(f['w']).requires_grad_(True)
    auto_w, = torch.autograd.grad(g.distloss(w).sum(), w)
    _, _, grad, gmaj = CR.distloss_parts(c, f['w'])
    assert bool(np.all(np.abs(grad - auto_w.numpy()) <= 1e-12 * gmaj)) and float(np.abs(grad - auto_w.numpy()).max()) <= 1e-12 * float(np.abs(grad).max())
    # the fused chain: G with the distortion gradient in it
    fu = CR.truth_fused(c, gi['g_op'], gi['g_d'], CR.FUSED_SCALE)
    Gf = g64['g_op'][c.ri] + g64['g_d'][c.ri] * f['m'] + CR.FUSED_SCALE * grad
    closed = CR.dsigma_closed(c, f, Gf, 0.0, 0.0)
    assert bool(np.all(np.abs(closed - fu['d_sigma'][0]) <= 1e-12 * fu['d_sigma'][1]))


@pytest.mark.parametrize('tail_empty', [False, True])
@pytest.mark.parametrize('gain', CR.GAINS)
def test_emulation_worst_error_in_units(gain, tail_empty):
    """What fp32 reaches on the GPU test's inputs; finite and below 64 (a guard against a broken majorant, not the GPU test's bar)."""
    tab = _clean(gain, tail_empty)
    for (op, name), u in sorted(tab.items()):
        print(f'[composite f64] {op} {name} gain {gain:g}{" tail-empty" if tail_empty else ""}: emulation {u:.2f} units')
        assert np.isfinite(u) and u < 64, (op, name, u)


@pytest.mark.parametrize('bug', CR.BUGS)
def test_wrong_variants_exceed_the_bar(bug):
    """Each deliberately wrong variant, on the same inputs, exceeds MARGIN times the clean emulation's worst in some output."""
    worst = 0.0
    where = None
    tail = bug == 'n_rays'
    for gain in CR.GAINS:
        clean, wrong = _clean(gain, tail), CR.emulation_table(_case(gain, tail), bug=bug)
        for key, u in wrong.items():
            ratio = u / max(MARGIN * clean[key], 1e-300)
            if ratio > worst:
                worst, where = ratio, (key, gain, u, clean[key])
    print(f'[composite f64] wrong variant {bug}: {where[0][0]} {where[0][1]} gain {where[1]:g}: {where[2]:.3g} units against {where[3]:.2f} clean')
    assert worst > 1.0, (bug, where)
    assert where[2] > 100 * MARGIN * max(where[3], 0.5), (bug, where)           # ... and not by a hair
