"""The packed-ray kernels of perf_amd/csrc/composite.hip -- compositing forward / backward, the distortion loss, their fused forms, the
two loss heads, the one-launch ray head -- and perf_normal_composite (field_normal.hip) against float64, on thin, mixed and OPAQUE rays
(densities exp(N(2, 2)) at gains 0.05 / 1 / 20: at 20 the transmittance runs through the fp32 denormals to exactly 0 and the exponent
sums reach the thousands), sorted samples, every ray count the kernels branch on, and a variant whose last 75 rays are empty.

Reference, majorant and emulation: tests/composite_reference.py.  An output's error is counted in units of its own rounding majorant,
|got - truth| / (2^-24 A + floor); the bar, per output and gain, is FOUR TIMES the worst error of the fp32 emulation of the kernel's
arithmetic on the same inputs, computed here at run time on the CPU -- never from the kernel.  tests/test_cpu_composite_reference.py
shows that eight subtly wrong variants of the emulation exceed that bar by four to seven orders of magnitude.

The kernels that consume another kernel's outputs (composite_bwd, distloss_fwd / _bwd, geo_loss, app_loss, accumulate_fwd,
normal_composite) are given the emulated forward's fp32 arrays, so that kernel and emulation start from the same bits; the chains
(composite_distloss_fwd -> _bwd, train_head_geo, train_head_app) run on the device's own forward.  Every output array is handed to
the kernel filled with a sentinel: rows past the live count stay untouched.  Rays without samples give exact zeros; the gradient of
the linear smooth-L1 branch is +- fl(inv_bs * weight * scale) to 2 units; inv_n is bit-equal to fp32 1 / n.

Measured on an MI355X, worst over the two batch variants, kernel / emulation in units (bar = 4 x emulation):
    op                     output           gain 0.05        gain 1       gain 20
    composite_fwd          w              0.21 / 0.54   1.48 / 1.74   2.19 / 2.19
    composite_fwd          T              1.47 / 1.85   2.53 / 2.53   2.44 / 2.53
    composite_fwd          alphas         0.27 / 0.96   0.48 / 1.08   0.54 / 1.07
    composite_fwd          opacity        0.10 / 0.43   0.09 / 0.42   0.50 / 0.52
    composite_fwd          distance       0.13 / 0.43   0.25 / 0.42   0.72 / 0.89
    composite_fwd          colour         0.09 / 0.43   0.54 / 0.69   1.32 / 1.40
    composite_bwd          d_sigma        1.48 / 3.71   1.05 / 2.13   0.80 / 2.09
    composite_bwd          d_rgb          0.31 / 0.55   1.47 / 1.60   2.12 / 2.16
    distloss               dl             1.97 / 1.97   1.69 / 2.25   1.86 / 1.86
    distloss               g_w            5.41 / 5.41   5.50 / 8.19   4.62 / 4.83
    composite_distloss     dl             0.02 / 0.12   0.05 / 0.12   0.08 / 0.12
    composite_distloss     d_sigma        0.46 / 1.28   0.89 / 1.28   0.58 / 1.28
    geo_loss/noise         g_opacity      0.28 / 0.28   0.38 / 0.38   0.52 / 0.52
    geo_loss/noise         g_distance     0.29 / 0.32   0.29 / 0.29   0.29 / 0.29
    geo_loss/noise         depth          0.01 / 0.02   0.00 / 0.01   0.00 / 0.01
    geo_loss/noise         distl          0.69 / 2.05   0.96 / 1.64   0.25 / 0.91
    geo_loss/noise         scale          0.16 / 0.16   0.16 / 0.16   0.16 / 0.16
    geo_loss/plain         g_opacity      0.00 / 0.00   0.00 / 0.00   0.00 / 0.00
    geo_loss/plain         g_distance     0.74 / 0.94   0.62 / 0.62   0.39 / 0.57
    geo_loss/plain         depth          0.08 / 0.08   0.00 / 0.07   0.04 / 0.04
    geo_loss/plain         distl          1.05 / 2.05   0.96 / 1.90   0.28 / 0.88
    geo_loss/plain         scale          0.29 / 0.29   0.29 / 0.29   0.29 / 0.29
    app_loss/bg            g_color        1.04 / 1.04   1.04 / 1.04   1.04 / 1.04
    app_loss/bg            loss           0.09 / 0.13   0.02 / 0.10   0.06 / 0.07
    app_loss/plain         g_color        0.97 / 1.01   0.88 / 0.88   0.88 / 0.88
    app_loss/plain         loss           0.06 / 0.39   0.07 / 0.17   0.05 / 0.09
    train_head_geo/noise   depth_terms    0.23 / 0.23   0.23 / 0.23   0.23 / 0.23
    train_head_geo/noise   inv_n          0.29 / 0.29   0.29 / 0.29   0.29 / 0.29
    train_head_geo/noise   d_sigma        0.12 / 0.82   1.01 / 1.01   0.78 / 0.81
    train_head_geo/plain   depth_terms    0.23 / 0.39   0.23 / 0.41   0.43 / 0.54
    train_head_geo/plain   d_sigma        0.15 / 0.59   0.82 / 0.84   0.76 / 0.80
    train_head_app/bg      color_terms    0.29 / 0.29   0.29 / 0.29   0.29 / 0.29
    train_head_app/bg      d_rgb          0.18 / 0.48   1.26 / 1.45   2.09 / 2.09
    train_head_app/plain   color_terms    0.91 / 0.91   0.91 / 0.91   0.91 / 0.91
    accumulate_fwd         C1             2.05 / 2.06   1.93 / 2.04   1.79 / 2.32
    accumulate_fwd         C3             2.26 / 2.51   2.91 / 3.79   2.47 / 2.47
    normal_composite       normal         0.56 / 0.82   0.52 / 0.62   0.79 / 0.79
    (train_head_geo / _app: w, T, opacity, distance, colour and dl measure what composite_fwd / composite_distloss do, d_rgb of
     train_head_app/plain what /bg does: the same bits.  The ray heads launched with a wavefront per ray, on the batch's long rays
     alone: d sigma 0.50 / 0.90, d rgb 1.20 / 1.21 at the worst.  The largest kernel / emulation ratio of any output is 1.2, the
     margin 4; no kernel was changed.)
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import composite_reference as CR  # noqa: E402

MARGIN = 4.0
SENT = 7.25
F = np.float32
CASES = [(g, t) for g in CR.GAINS for t in (False, True)]
IDS = [f'gain{g:g}{"-tail-empty" if t else ""}' for g, t in CASES]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from perf_amd import ops as _ops
    return _ops


class _Ctx:
    def __init__(self, gain, tail, long_rays=False):
        self.gain, self.tail = gain, tail
        self.c = CR.make_case(gain, tail)
        if long_rays:
            self.c = CR.sub_case(self.c)
        self.li = CR.make_loss_inputs(self.c)
        for noise_on in (True, False):                     # float64: no ray sits on a kink of its loss (tests/test_cpu_composite_reference.py)
            md, mpre, mc, n_neg, n_empty_pos, mlive = CR.kink_margins(self.c, self.li, noise_on, noise_on)
            assert md >= 0.25 and mc >= 0.25 and (mpre >= 1e-3 and (n_neg >= 8 or long_rays) and n_empty_pos > 0 if noise_on else mlive >= 1e-12)
        self.bar = CR.emulation_worst(self.c, self.li)
        self.fw = CR.emu_fwd(self.c)                       # the emulated forward (host expf): input of the kernels that consume one
        self.gi = CR.grads_in(self.c)
        c = self.c
        self.sig, self.rgb, self.ts, self.te = (_dev(x) for x in (c.sig, c.rgb, c.ts, c.te))
        self.packed = _dev(c.packed)
        self.cap = c.sig.shape[0]

    def rows(self, v, fill=0.5):
        """A per-sample fp32 array -> device, padded to the batch's capacity."""
        v = np.asarray(v, F)
        out = np.full((self.cap,) + v.shape[1:], fill, F)
        out[:self.c.S] = v[:self.c.S]
        return _dev(out)

    def live(self, t, untouched=SENT):
        """The live rows of a per-sample output; the rows behind them were not written."""
        a = t.detach().cpu().numpy()
        assert a.shape[0] == self.cap and bool(np.all(a[self.c.S:] == untouched)), 'rows past the live count were written'
        return a[:self.c.S]

    def check(self, op, ref, got, names):
        bad = []
        for name in names:
            k, e = CR.units(got[name], ref[name]), self.bar[(op, name)]
            print(f'[composite f64] {op} {name} gain {self.gain:g}{" tail-empty" if self.tail else ""}: kernel {k:.2f} units, emulation {e:.2f} units')
            if not k <= MARGIN * e:
                bad.append((name, k, e))
        assert not bad, (op, bad)

    def zeros_on_empty_rays(self, *per_ray):
        empty = self.c.counts == 0
        for a in per_ray:
            assert bool(np.all(np.asarray(a).reshape(self.c.R, -1)[empty] == 0.0))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ctx(gain, tail, long_rays=False):
    return _Ctx(gain, tail, long_rays)


@contextlib.contextmanager
def _sentinel_outputs():
    """perf_amd.ops allocates its outputs with torch.empty: inside this block an fp32 one comes filled with SENT."""
    real = torch.empty

    def filled(*size, dtype=None, device=None, **kw):
        if dtype is torch.float32 and not kw:
            if len(size) == 1 and not isinstance(size[0], int):
                size = tuple(size[0])
            return torch.full(tuple(size), SENT, dtype=dtype, device=device)
        return real(*size, dtype=dtype, device=device, **kw)

    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real


def _linear_branch_is_exact(g, ref_g, linear, k32):
    """+- fl(inv_bs * weight * scale) to 2 units where the smooth-L1 is in its linear branch."""
    g, want = np.asarray(g, np.float64).reshape(-1)[linear.reshape(-1)], np.sign(ref_g.reshape(-1)[linear.reshape(-1)]) * float(k32)
    assert g.size > 0 and bool(np.all(np.abs(g - want) <= 2 * CR.U * abs(float(k32))))


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_composite_fwd(ops, gain, tail):
    x = _ctx(gain, tail)
    with _sentinel_outputs():
        w, T, al, op, dist, col = ops.composite_fwd(x.sig, x.rgb, x.ts, x.te, x.packed)
    torch.cuda.synchronize()
    got = {'w': x.live(w), 'T': x.live(T), 'alphas': x.live(al), 'opacity': _np(op), 'distance': _np(dist), 'colour': _np(col)}
    x.zeros_on_empty_rays(got['opacity'], got['distance'], got['colour'])
    x.check('composite_fwd', CR.truth_fwd(x.c), got, ('w', 'T', 'alphas', 'opacity', 'distance', 'colour'))


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_composite_bwd(ops, gain, tail):
    """d sigma with all of g_weights, g_opacity, g_distance, g_trans, g_alphas, and d rgb."""
    x = _ctx(gain, tail)
    gi = x.gi
    with _sentinel_outputs():
        ds, drgb = ops.composite_bwd(x.sig, x.ts, x.te, x.packed, x.rows(x.fw['w']), x.rows(x.fw['T']), g_weights=x.rows(gi['g_w']),
                                     g_opacity=_dev(gi['g_op']), g_distance=_dev(gi['g_d']), g_color=_dev(gi['g_col']), g_trans=x.rows(gi['g_T']),
                                     g_alphas=x.rows(gi['g_al']), want_drgb=True)
    x.check('composite_bwd', CR.truth_bwd(x.c, **gi), {'d_sigma': x.live(ds), 'd_rgb': x.live(drgb)}, ('d_sigma', 'd_rgb'))


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_distloss_fwd_bwd(ops, gain, tail):
    """On weights a forward produced, with scale and scale_dev."""
    x = _ctx(gain, tail)
    w = x.rows(x.fw['w'])
    with _sentinel_outputs():
        dl = ops.distloss_fwd(w, x.ts, x.te, x.packed)
    gw = ops.distloss_bwd(w, x.ts, x.te, x.packed, CR.FUSED_SCALE_HOST, scale_dev=_dev(np.array([CR.FUSED_SCALE_DEV], F)))
    x.zeros_on_empty_rays(_np(dl))
    x.check('distloss', CR.truth_distloss(x.c, x.fw['w'], CR.FUSED_SCALE), {'dl': _np(dl), 'g_w': x.live(gw, untouched=0.0)}, ('dl', 'g_w'))


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_composite_distloss_fused(ops, gain, tail):
    x = _ctx(gain, tail)
    gi = x.gi
    with _sentinel_outputs():
        w, T, op, dist, col, dl = ops.composite_distloss_fwd(x.sig, x.rgb, x.ts, x.te, x.packed)
        ds = ops.composite_distloss_bwd(x.sig, x.ts, x.te, x.packed, w, T, op, dist, _dev(gi['g_op']), _dev(gi['g_d']), CR.FUSED_SCALE_HOST,
                                        scale_dev=_dev(np.array([CR.FUSED_SCALE_DEV], F)))
    x.zeros_on_empty_rays(_np(dl), _np(op), _np(dist), _np(col))
    x.live(w); x.live(T)
    x.check('composite_distloss', CR.truth_fused(x.c, gi['g_op'], gi['g_d'], CR.FUSED_SCALE), {'dl': _np(dl), 'd_sigma': x.live(ds)}, ('dl', 'd_sigma'))


def _geo_variants(x):
    li = x.li
    return (('noise', li['noise'], li['gt_noise'], CR.RATIO, x.c.R), ('plain', None, li['gt_plain'], 1.0, 4 * x.c.R))


def _app_variants(x):
    li = x.li
    return (('bg', li['bg'], li['gtc_bg'], x.c.R), ('plain', None, li['gtc_plain'], 4 * x.c.R))


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_geo_loss(ops, gain, tail):
    """g_opacity, g_distance and the three scalars: with noise, the ramp and the batch's own normaliser; without, data-parallel."""
    x = _ctx(gain, tail)
    fw = x.fw
    op, dist, dl = _dev(fw['opacity'][:, None]), _dev(fw['distance'][:, None]), _dev(fw['dl'])
    for tag, noise, gt, ratio, gb in _geo_variants(x):
        ratio_dev = _dev(np.array([ratio], F)) if noise is not None else None
        g_op, g_d, sc = ops.geo_loss(op, dist, _dev(gt), None if noise is None else _dev(noise), dl, x.packed, gb, CR.DEPTH_W, CR.DIST_W, ratio_dev,
                                     CR.LOSS_SCALE)
        sc = _np(sc)
        ref = CR.truth_geo_loss(x.c, fw['opacity'], fw['distance'], fw['dl'], gt, noise, gb, ratio)
        x.check('geo_loss/' + tag, ref, {'g_opacity': _np(g_op), 'g_distance': _np(g_d), 'depth': sc[0], 'distl': sc[1], 'scale': sc[2]},
                ('g_opacity', 'g_distance', 'depth', 'distl', 'scale'))
        k32 = F(1) / F(gb) * F(CR.DEPTH_W) * F(CR.LOSS_SCALE)
        _linear_branch_is_exact(_np(g_d), ref['g_distance'][0], (ref['_pre'] > 0) & ~ref['_quad'], k32)
        assert bool(np.all(_np(g_d).reshape(-1)[ref['_pre'] <= 0] == 0.0))                      # relu: no gradient where pre <= 0


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_app_loss(ops, gain, tail):
    x = _ctx(gain, tail)
    fw = x.fw
    op, col = _dev(fw['opacity'][:, None]), _dev(fw['colour'])
    for tag, bg, gt, gb in _app_variants(x):
        g_c, sc = ops.app_loss(op, col, None if bg is None else _dev(bg), _dev(gt), gb, CR.COLOR_W, CR.LOSS_SCALE)
        ref = CR.truth_app_loss(x.c, fw['opacity'], fw['colour'], bg, gt, gb)
        x.check('app_loss/' + tag, ref, {'g_color': _np(g_c), 'loss': _np(sc)[0]}, ('g_color', 'loss'))
        _linear_branch_is_exact(_np(g_c), ref['g_color'][0], ~ref['_quad'], F(1) / F(gb * 3) * F(CR.COLOR_W) * F(CR.LOSS_SCALE))


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_train_head_geo(ops, gain, tail):
    """Every per-sample and per-ray output, the per-ray depth terms, inv_n, and d sigma as the derivative of the whole scaled loss."""
    _head_geo(ops, _ctx(gain, tail))


def _head_geo(ops, x):
    for tag, noise, gt, ratio, gb in _geo_variants(x):
        ratio_dev = _dev(np.array([ratio], F)) if noise is not None else None
        with _sentinel_outputs():
            hd = ops.train_head_geo(x.sig, x.rgb, x.ts, x.te, x.packed, _dev(gt), None if noise is None else _dev(noise), gb, CR.DEPTH_W, CR.DIST_W,
                                    ratio_dev, CR.LOSS_SCALE)
        got = {'w': x.live(hd['weights']), 'T': x.live(hd['trans']), 'opacity': _np(hd['opacity']), 'distance': _np(hd['distance']),
               'colour': _np(hd['color']), 'dl': _np(hd['distloss_per_ray']), 'depth_terms': _np(hd['depth_terms']), 'inv_n': _np(hd['inv_n'])[0],
               'd_sigma': x.live(hd['d_sigma'])}
        x.zeros_on_empty_rays(got['opacity'], got['distance'], got['colour'], got['dl'])
        n = gb if gb != x.c.R else x.c.last + 1
        assert got['inv_n'] == F(1) / F(n)
        x.check('train_head_geo/' + tag, CR.truth_head_geo(x.c, gt, noise, gb, ratio), got,
                ('w', 'T', 'opacity', 'distance', 'colour', 'dl', 'depth_terms', 'inv_n', 'd_sigma'))


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_train_head_app(ops, gain, tail):
    _head_app(ops, _ctx(gain, tail))


def _head_app(ops, x):
    for tag, bg, gt, gb in _app_variants(x):
        with _sentinel_outputs():
            ha = ops.train_head_app(x.sig, x.rgb, x.ts, x.te, x.packed, None if bg is None else _dev(bg), _dev(gt), gb, CR.COLOR_W, CR.LOSS_SCALE)
        got = {'w': x.live(ha['weights']), 'T': x.live(ha['trans']), 'opacity': _np(ha['opacity']), 'distance': _np(ha['distance']),
               'colour': _np(ha['color']), 'color_terms': _np(ha['color_terms']), 'd_rgb': x.live(ha['d_rgb'])}
        x.zeros_on_empty_rays(got['opacity'], got['distance'], got['colour'])
        x.check('train_head_app/' + tag, CR.truth_head_app(x.c, bg, gt, gb), got, ('w', 'T', 'opacity', 'distance', 'colour', 'color_terms', 'd_rgb'))


@pytest.mark.parametrize('gain', CR.GAINS)
def test_train_heads_with_a_wavefront_per_ray(ops, gain):
    """The batch's long rays alone (0, 1, 63 .. 200 samples; 32 or more per ray on average): the host launches the ray heads without
    ray teams."""
    x = _ctx(gain, False, True)
    assert x.c.S >= 32 * x.c.R and x.c.R % 4 != 0
    _head_geo(ops, x)
    _head_app(ops, x)


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_accumulate_fwd(ops, gain, tail):
    x = _ctx(gain, tail)
    w = x.rows(x.fw['w'])
    for tag, values in (('C1', None), ('C3', x.c.rgb)):
        out = _np(ops.accumulate_fwd(w, None if values is None else x.rgb, x.packed))
        x.zeros_on_empty_rays(out)
        x.check('accumulate_fwd', {tag: CR.truth_accumulate(x.c, x.fw['w'], values)['out']}, {tag: out}, (tag,))


@pytest.mark.parametrize('gain,tail', CASES, ids=IDS)
def test_normal_composite(ops, gain, tail):
    """unit(sum_i w_i * -g_i / |g_i|): gradient magnitudes 1e-30 .. 1e30, exactly-zero and infinite rows skipped, rays without samples
    and a ray whose sum cancels give exactly zero."""
    x = _ctx(gain, tail)
    w, g, r_cancel = CR.make_normal_inputs(x.c, x.fw['w'])
    assert bool(np.any(np.isinf(g))) and bool(np.any(np.all(g == 0, 1))) and float(np.abs(g[np.isfinite(g)]).max()) > 1e28
    out = _np(ops.normal_composite(x.rows(w), x.rows(g), x.packed))
    x.zeros_on_empty_rays(out)
    assert bool(np.all(out[r_cancel] == 0.0))
    x.check('normal_composite', CR.truth_normal(x.c, w, g), {'normal': out}, ('normal',))
