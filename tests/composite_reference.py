"""Float64 reference of the packed-ray kernels of perf_amd/csrc/composite.hip (compositing forward / backward, distortion loss,
their fused forms, the two loss heads, the one-launch ray head) and of perf_normal_composite (field_normal.hip), the rounding
majorant their fp32 error is measured in, and an fp32 emulation of the kernels' arithmetic.  Plain numpy / torch: no GPU.

    delta = t1 - t0,  m = (t0 + t1) / 2,  sd = sigma delta,  ex_i = sum_{j<i} sd_j
    T = exp(-ex),  alpha = 1 - exp(-sd),  w = T alpha,  opacity = sum w,  distance = sum w m,  colour = sum w rgb (w detached)
    distortion loss of a ray = sum_i ( delta_i w_i^2 / 3 + 2 w_i (m_i W_i - WM_i) ),  W, WM exclusive prefixes of w, w m
    d sigma_i = delta_i ( (G_i T_i + gA_i) exp(-sd_i) - sum_{j>i} (G_j w_j + gT_j T_j) ),  G = g_w + g_op + g_dist m
    d loss / d w_i = scale ( 2/3 delta_i w_i + 2 ( m_i (W_i - Wsuf_i) - (WM_i - WMsuf_i) ) )

TRUTH.  Values in numpy float64; gradients by float64 autograd (torch) of the plain formulas, the per-ray exclusive sum written as
a product with a strictly triangular matrix so that its backward is a direct suffix sum (a cumsum whose backward is total minus
prefix loses, on an opaque ray, every late sample even in float64).

MAJORANT.  An output's error is counted in UNITS: |got - truth| / (2^-24 A + floor).  A is the output's own expression evaluated in
float64 with every term replaced by its absolute value and every subtraction by an addition; whatever passed through exp(-x)
carries a factor (2 + x), an absolute error of the exponent being a relative error of the result:
    T: T (2 + ex);  alpha: 1 + e^-sd (2 + sd);  w: the product of the two;  per-ray sums: the sums of the samples' majorants
    d sigma_i: delta_i ( (|G_i| T_i + |gA_i| e^-sd_i) c_i + (|G_i| w_i + |gT_i| T_i) c_i + sum_{j>i} (|G_j| w_j + |gT_j| T_j) c_j ),
               c = 2 + ex + sd, |G| = |g_w| + |g_op| + |g_dist| m
    distortion gradient: |scale| ( 2/3 delta_i w_i + 2 ( m_i sum w + sum w m ) )
    fused kernels: G's own majorant A_G (the loss head's, the distortion gradient's and the forward's behind them) goes through the
               same recursion: + delta_i ( A_G_i T_i e^-sd_i + A_G_i w_i + sum_{j>i} A_G_j w_j )
The floor is 2^-126 times the magnitudes that multiply a value the device may flush to zero (T, e^-sd, w and their products).

EMULATION.  The kernels' expressions in numpy float32, in their order (-ffp-contract=off: no fused multiply-add): sd = fl(s fl(t1 - t0)),
oracle.packed_exclusive_sum_canonical for the prefix scans, Kogge-Stone suffix sums inside 64-sample chunks with a carry between
them, lane-strided partial sums folded by the xor butterfly, Wsuf = totW - W - w in distloss_bwd, W = totW - Wsuf - w in the fused
backward, expf(-s delta) for 1 - alpha, the loss heads' workgroup sums.  It need not equal the device bit for bit: expf is not correctly
rounded on either side, so the emulation runs under four models of it (EXP_MODELS) and its worst error is the worst of the four.  It
shows what fp32 reaches on these inputs; the GPU test's bar is four times that.  `bug=` selects a deliberately wrong variant (BUGS)."""
import numpy as np
import torch

from oracle import perf_oracle as O

U = 2.0 ** -24
TINY = 2.0 ** -126
F = np.float32
GAINS = (0.05, 1.0, 20.0)
BETA_D, BETA_C = 1e-2, 5e-2
DEPTH_W, DIST_W, COLOR_W, LOSS_SCALE, RATIO = 1.0, 0.5, 1.0, 128.0, float(np.float32(0.6))
STEP = 1.5 / 256
BUGS = ('drop_carry', 'later_inclusive', 'third', 'no_gA', 'gop_sign', 'n_rays', 'sl1_linear', 'total_minus_prefix')

# ---- the batch -------------------------------------------------------------------------------------------------------------------
# rays 0..15   an aligned group of sixteen with <= 4 samples each (4-lane teams); ray 0 and ray 7 are empty
# rays 16..31  four aligned groups of four: <= 16 each (quarter waves); one broken by a ray of 65; <= 4 each; one broken by a ray of 17
# rays 32..47  sixteen rays of <= 4 samples but for one of 199
# rays 48..59  0 1 63 64 65 128 129 199 200 16 17 5 samples
# rays 60..202 drawn: half of them <= 4 samples, a quarter <= 16, a quarter up to 120   (203 rays: not a multiple of four)
_HEAD_COUNTS = [0, 1, 2, 3, 4, 4, 1, 0, 2, 3, 4, 1, 2, 3, 4, 4,
                16, 5, 9, 12, 3, 65, 7, 16, 1, 4, 0, 2, 17, 2, 0, 15,
                2, 3, 1, 4, 0, 4, 199, 1, 3, 3, 2, 4, 1, 0, 4, 2,
                0, 1, 63, 64, 65, 128, 129, 199, 200, 16, 17, 5]
N_RAYS = 203
TAIL_EMPTY = 75            # the tail-empty variant's last rays without a sample (more than one 64-ray ballot)
THIN_RAYS = (1, 2, 3, 4, 5, 6, 8, 9, 10, 11)        # nearly transparent at every gain, close to the origin


def ray_counts(seed=7):
    rng = np.random.default_rng(seed)
    rest = []
    for _ in range(N_RAYS - len(_HEAD_COUNTS)):
        k = rng.integers(4)
        rest.append(int(rng.integers(0, 5)) if k < 2 else int(rng.integers(5, 17)) if k == 2 else int(rng.integers(17, 121)))
    return np.asarray(_HEAD_COUNTS + rest, np.int64)


class Case:
    """A packed batch (fp32 numpy; the live samples are rows [0, S) in ray order, `pad` rows of capacity behind them)."""

    def __init__(self, packed, ts, te, sig, rgb, gain=None, thin=()):
        self.packed, self.ts, self.te, self.sig, self.rgb, self.gain, self.thin = packed, ts, te, sig, rgb, gain, tuple(thin)
        self.counts = packed[:, 1].astype(np.int64)
        self.R, self.S = len(self.counts), int(self.counts.sum())
        self.ri = np.repeat(np.arange(self.R), self.counts)
        self.pos = np.arange(self.S) - packed[:, 0].astype(np.int64)[self.ri]
        self.nch = max(1, (int(self.counts.max()) + 63) // 64)
        self.L = 64 * self.nch
        live = np.nonzero(self.counts > 0)[0]
        self.last = int(live.max()) if live.size else -1

    def dense(self, v, dtype=np.float64):
        out = np.zeros((self.R, self.L), dtype)
        out[self.ri, self.pos] = v[:self.S]
        return out

    def flat(self, d):
        return d[self.ri, self.pos]

    def seg(self, v):
        """per-ray sums in float64"""
        v = np.asarray(v, np.float64)
        if v.ndim == 1:
            return np.bincount(self.ri, v, self.R)
        return np.stack([np.bincount(self.ri, v[:, k], self.R) for k in range(v.shape[1])], -1)

    def excl(self, v):
        d = self.dense(v)
        return self.flat(np.cumsum(d, 1) - d)

    def suffix_excl(self, v):
        d = self.dense(v)
        return self.flat(np.cumsum(d[:, ::-1], 1)[:, ::-1] - d)

    def f64(self):
        S = self.S
        ts, te, sig = (x[:S].astype(np.float64) for x in (self.ts, self.te, self.sig))
        return ts, te, sig, te - ts, (ts + te) * 0.5


def make_case(gain, tail_empty=False, seed=7, pad=37):
    """Sorted lattice positions inside every ray (distinct cells of a 256-cell lattice from a per-ray near point), densities
    gain * exp(N(2, 2)) -- times 1e-3 / gain on THIN_RAYS --, colours U[0, 1).  Every ray has its own generator: the tail-empty
    variant keeps the leading rays' samples."""
    counts = ray_counts(seed)
    if tail_empty:
        counts[N_RAYS - TAIL_EMPTY:] = 0
    ts, te, sig, rgb = [], [], [], []
    for r, n in enumerate(counts):
        rng = np.random.default_rng([seed, r])
        near = rng.uniform(0.0, 0.05)
        cells = np.sort(rng.choice(16 if r in THIN_RAYS else 256, size=int(n), replace=False))
        t0 = (near + cells * STEP).astype(F)
        ts.append(t0); te.append((t0 + F(STEP)).astype(F))
        s = np.exp(2.0 + 2.0 * rng.standard_normal(int(n))) * (1e-3 if r in THIN_RAYS else gain)
        sig.append(s.astype(F)); rgb.append(rng.uniform(0, 1, (int(n), 3)).astype(F))
    rng = np.random.default_rng([seed, 10 ** 6])
    ts.append(rng.uniform(0, 1, pad).astype(F)); te.append((ts[-1] + F(STEP)).astype(F))
    sig.append(rng.uniform(0, 50, pad).astype(F)); rgb.append(rng.uniform(0, 1, (pad, 3)).astype(F))
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    packed = np.stack([starts, counts], -1).astype(np.int32)
    return Case(packed, np.concatenate(ts), np.concatenate(te), np.concatenate(sig), np.concatenate(rgb), gain, THIN_RAYS)


LONG_RAYS = (38, 21, 50, 51, 52, 53, 54, 55, 56, 48, 49)       # 199 65 63 64 65 128 129 199 200 0 1 samples


def sub_case(c, rays=LONG_RAYS):
    """The batch of the given rays of c alone (no capacity rows).  LONG_RAYS: at least 32 samples per ray on average, where the host
    launches the ray head with a wavefront per ray instead of ray teams."""
    rows = np.concatenate([np.arange(c.packed[r, 0], c.packed[r, 0] + c.packed[r, 1]) for r in rays]).astype(np.int64)
    counts = c.counts[list(rays)]
    packed = np.stack([np.concatenate([[0], np.cumsum(counts)[:-1]]), counts], -1).astype(np.int32)
    return Case(packed, c.ts[rows], c.te[rows], c.sig[rows], c.rgb[rows], c.gain)


def units(got, ref):
    """Worst error of `got` against ref = (truth, A, floor), in units."""
    truth, A, floor = ref
    got = np.asarray(got, np.float64).reshape(np.shape(truth))
    if got.size == 0:
        return 0.0
    e = np.abs(got - truth) / (U * np.asarray(A, np.float64) + floor)
    return float(np.max(np.where(np.isfinite(e), e, np.inf)))


# ---- truth: values -----------------------------------------------------------------------------------------------------------------
def truth_fwd(c):
    """-> dict name -> (truth, A, floor) of the compositing forward, float64, plus the pieces the other majorants are made of."""
    ts, te, sig, d, m = c.f64()
    sd = sig * d
    ex = c.excl(sd)
    T, E, al = np.exp(-ex), np.exp(-sd), -np.expm1(-sd)
    w = T * al
    rgb = c.rgb[:c.S].astype(np.float64)
    A_T, A_al = T * (2 + ex), 1 + E * (2 + sd)
    A_w = A_T * A_al
    cnt = c.counts.astype(np.float64)
    one = np.ones_like(w)
    out = {'T': (T, A_T, TINY * one), 'alphas': (al, A_al, TINY * one), 'w': (w, A_w, 2 * TINY * one),
           'opacity': (c.seg(w), c.seg(A_w), 2 * TINY * (cnt + 1)), 'distance': (c.seg(w * m), c.seg(A_w * m), 2 * TINY * (c.seg(m) + 1)),
           'colour': (c.seg(w[:, None] * rgb), c.seg(A_w[:, None] * rgb), 2 * TINY * (c.seg(rgb) + 1))}
    out['_'] = dict(d=d, m=m, sd=sd, ex=ex, T=T, E=E, al=al, w=w, A_w=A_w, A_T=A_T, c=2 + ex + sd)
    return out


def distloss_parts(c, w):
    """Per-ray distortion loss of the weights w (float64), its closed-form gradient and their majorants."""
    ts, te, sig, d, m = c.f64()
    w = np.asarray(w, np.float64)[:c.S]
    W, WM = c.excl(w), c.excl(w * m)
    Wsuf, WMsuf = c.suffix_excl(w), c.suffix_excl(w * m)
    totW, totWM = c.seg(w)[c.ri], c.seg(w * m)[c.ri]
    per = c.seg(d * w * w / 3 + 2 * w * (m * W - WM))
    A_per = c.seg(d * w * w / 3 + 2 * w * (m * W + WM))
    grad = 2.0 / 3.0 * d * w + 2 * (m * (W - Wsuf) - (WM - WMsuf))
    gmaj = 2.0 / 3.0 * d * w + 2 * (m * totW + totWM)
    return per, A_per, grad, gmaj


def truth_distloss(c, w32, scale):
    """distloss_fwd / distloss_bwd on given fp32 weights (exact inputs) -> {'dl', 'g_w'}."""
    ts, te, sig, d, m = c.f64()
    per, A_per, grad, gmaj = distloss_parts(c, w32)
    cnt = c.counts.astype(np.float64)
    mmax = np.zeros(c.R); np.maximum.at(mmax, c.ri, m)
    fl_g = TINY * (1 + abs(scale) * (1 + d + 4 * (cnt * mmax)[c.ri]))
    return {'dl': (per, A_per, TINY * (cnt + 1 + c.seg(gmaj))), 'g_w': (scale * grad, abs(scale) * gmaj, fl_g)}


def dsigma_closed(c, f, G, gT, gA):
    """The kernel comment's closed form in float64 (f = truth_fwd(c)['_'])."""
    later = c.suffix_excl(G * f['w'] + gT * f['T'])
    return f['d'] * ((G * f['T'] + gA) * f['E'] - later)


def dsigma_majorant(c, f, Gabs, gT, gA, A_G=None):
    q = (Gabs * f['w'] + np.abs(gT) * f['T']) * f['c']
    A = f['d'] * ((Gabs * f['T'] + np.abs(gA) * f['E']) * f['c'] + q + c.suffix_excl(q))
    if A_G is not None:
        A = A + f['d'] * (A_G * f['T'] * f['E'] + A_G * f['w'] + c.suffix_excl(A_G * f['w']))
    floor = TINY * (1 + f['d'] * (1 + Gabs + np.abs(gA) + c.suffix_excl(1 + Gabs + np.abs(gT))))
    return A, floor


# ---- truth: gradients by float64 autograd ----------------------------------------------------------------------------------------
class _Graph:
    """The forward in torch float64 from sigma (and rgb) as leaves."""

    def __init__(self, c):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).double()
        S = c.S
        self.c = c
        self.ri, self.pos = torch.from_numpy(c.ri), torch.from_numpy(c.pos)
        self.ts, self.te = t(c.ts[:S]), t(c.te[:S])
        self.sig = t(c.sig[:S]).requires_grad_(True)
        self.rgb = t(c.rgb[:S]).requires_grad_(True)
        self.d, self.m = self.te - self.ts, (self.ts + self.te) * 0.5
        self.tri = torch.triu(torch.ones(c.L, c.L, dtype=torch.float64), diagonal=1)        # [i, j] = 1 for i < j
        sd = self.sig * self.d
        self.T = torch.exp(-self.excl(sd))
        self.al = 1.0 - torch.exp(-sd)                      # (not -expm1: torch differentiates that as result + 1, which drops e^-sd below 1e-16)
        self.w = self.T * self.al
        self.op, self.dist = self.seg(self.w), self.seg(self.w * self.m)
        self.col = self.seg(self.w.detach()[:, None] * self.rgb)

    def excl(self, v):
        dense = torch.zeros(self.c.R, self.c.L, dtype=torch.float64).index_put((self.ri, self.pos), v)
        return (dense @ self.tri)[self.ri, self.pos]

    def seg(self, v):
        return torch.zeros((self.c.R,) + tuple(v.shape[1:]), dtype=torch.float64).index_add(0, self.ri, v)

    def distloss(self, w=None):
        w = self.w if w is None else w
        W, WM = self.excl(w), self.excl(w * self.m)
        return self.seg(self.d * w * w / 3 + 2 * w * (self.m * W - WM))

    def grad(self, loss, leaf):
        g, = torch.autograd.grad(loss, leaf, retain_graph=True, allow_unused=True)
        return np.zeros(tuple(leaf.shape)) if g is None else g.numpy()


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))


def _z(x, n):
    return np.zeros(n) if x is None else np.asarray(x, np.float64).reshape(n)


def truth_bwd(c, g_w=None, g_op=None, g_d=None, g_T=None, g_al=None, g_col=None):
    """composite_bwd -> {'d_sigma', 'd_rgb'}: autograd of sum(g . output) from sigma / rgb."""
    g = _Graph(c)
    S, R = c.S, c.R
    gw, gT, gA, gop, gd = _z(g_w, S), _z(g_T, S), _z(g_al, S), _z(g_op, R), _z(g_d, R)
    gc = _z(g_col, (R, 3))
    loss = (_t(gw) * g.w).sum() + (_t(gT) * g.T).sum() + (_t(gA) * g.al).sum() + (_t(gop) * g.op).sum() + (_t(gd) * g.dist).sum()
    f = truth_fwd(c)['_']
    Gabs = np.abs(gw) + np.abs(gop)[c.ri] + np.abs(gd)[c.ri] * f['m']
    A, floor = dsigma_majorant(c, f, Gabs, gT, gA)
    drgb = g.grad((_t(gc) * g.col).sum(), g.rgb)
    agc = np.abs(gc)[c.ri]
    return {'d_sigma': (g.grad(loss, g.sig), A, floor), 'd_rgb': (drgb, f['A_w'][:, None] * agc + np.abs(drgb), TINY * (1 + agc))}


def _fused_majorant(c, f, gop, gd, A_gop, A_gd, dls):
    """|G| and G's own majorant in the fused backward: G = g_op + g_dist m + dls * (d distortion / d w), w and its sums the forward's."""
    m, d = f['m'], f['d']
    _, _, _, gmaj = distloss_parts(c, f['w'])
    Aw = f['A_w']
    prop = 2.0 / 3.0 * d * Aw + 2 * (m * c.seg(Aw)[c.ri] + c.seg(Aw * m)[c.ri])
    Gabs = np.abs(gop)[c.ri] + np.abs(gd)[c.ri] * m + abs(dls) * gmaj
    A_G = (A_gop + np.abs(gop))[c.ri] + (A_gd + np.abs(gd))[c.ri] * m + abs(dls) * (gmaj + prop)
    return Gabs, A_G


def truth_fused(c, g_op, g_d, scale):
    """composite_distloss_fwd / _bwd -> {'dl', 'd_sigma'} from sigma: loss = sum g_op op + sum g_d dist + scale sum dl."""
    g = _Graph(c)
    R = c.R
    gop, gd = _z(g_op, R), _z(g_d, R)
    dl = g.distloss()
    loss = (_t(gop) * g.op).sum() + (_t(gd) * g.dist).sum() + scale * dl.sum()
    f = truth_fwd(c)['_']
    per, A_per, _, gmaj = distloss_parts(c, f['w'])
    Gabs, A_G = _fused_majorant(c, f, gop, gd, np.zeros(R), np.zeros(R), scale)
    A, floor = dsigma_majorant(c, f, Gabs, np.zeros(c.S), np.zeros(c.S), A_G)
    cnt = c.counts.astype(np.float64)
    return {'dl': (dl.detach().numpy(), A_per + c.seg(gmaj * f['A_w']), TINY * (cnt + 1 + c.seg(gmaj))),
            'd_sigma': (g.grad(loss, g.sig), A, floor)}


# ---- truth: the loss heads ---------------------------------------------------------------------------------------------------------
def inv_n_of(c, global_batch):
    if global_batch != c.R:
        return 1.0 / global_batch
    return 1.0 / (c.last + 1) if c.last >= 0 else 1.0


def _sl1(x, beta):
    return torch.nn.functional.smooth_l1_loss(x, torch.zeros_like(x), beta=beta, reduction='none')


def _geo_loss_t(op, dist, dl, gt, noise, inv_n, global_batch, ratio):
    """scene.py / oracle.geo_step_loss on torch float64 per-ray tensors -> (scaled loss, depth loss, distortion loss, per-ray terms, pre)."""
    nz = 0.0 if noise is None else _t(noise) * 2.0 - 1.0
    pre = dist + nz * (1.0 - op)
    terms = _sl1(torch.relu(pre) - _t(gt), BETA_D)
    depth = terms.sum() / global_batch
    distl = dl.sum() * inv_n
    return (depth * DEPTH_W + distl * DIST_W * ratio) * LOSS_SCALE, depth, distl, terms, pre


def _geo_majorants(op, dist, gt, noise, A_op, A_d, global_batch):
    """numpy float64, per ray -> (g_d, A_gd, g_op, A_gop, A_terms, quad, pre)."""
    k = DEPTH_W * LOSS_SCALE / global_batch
    nz = np.zeros_like(op) if noise is None else 2.0 * noise - 1.0
    nza = np.zeros_like(op) if noise is None else 2.0 * np.abs(noise) + 1.0
    pre = dist + nz * (1 - op)
    live = pre > 0
    diff = np.maximum(pre, 0) - gt
    quad = np.abs(diff) < BETA_D
    A_diff = np.where(live, A_d + nza * A_op + np.abs(dist) + nza * (1 + np.abs(op)), 0.0) + np.abs(gt)
    sg = np.where(quad, diff / BETA_D, np.sign(diff))
    gd = np.where(live, sg * k, 0.0)
    A_gd = np.where(live, np.where(quad, k * A_diff / BETA_D, 0.0) + np.abs(gd), 0.0)
    gop = -nz * gd
    A_gop = nza * A_gd + np.abs(gop)
    sl = np.where(quad, 0.5 * diff * diff / BETA_D, np.abs(diff) - 0.5 * BETA_D)
    A_terms = np.where(quad, np.abs(diff) * A_diff / BETA_D, A_diff + 0.5 * BETA_D) + sl
    return gd, A_gd, gop, A_gop, A_terms, quad, pre


def truth_geo_loss(c, op32, dist32, dl32, gt, noise, global_batch, ratio):
    """perf_geo_loss on given fp32 per-ray inputs (exact) -> {'g_opacity', 'g_distance', 'depth', 'distl', 'scale'}."""
    R = c.R
    op = _t(np.asarray(op32).reshape(R)).requires_grad_(True); dist = _t(np.asarray(dist32).reshape(R)).requires_grad_(True)
    inv_n = inv_n_of(c, global_batch)
    loss, depth, distl, terms, pre = _geo_loss_t(op, dist, _t(np.asarray(dl32).reshape(R)), gt, noise, inv_n, global_batch, ratio)
    g_op, g_d = (np.zeros(R) if x is None else x.numpy() for x in torch.autograd.grad(loss, (op, dist), allow_unused=True))
    z = np.zeros(R)
    gd, A_gd, gop, A_gop, A_terms, quad, _ = _geo_majorants(op.detach().numpy(), dist.detach().numpy(), gt, noise, z, z, global_batch)
    sc = inv_n * DIST_W * ratio * LOSS_SCALE
    fl = TINY * (1 + LOSS_SCALE / BETA_D)
    return {'g_distance': (g_d, A_gd, fl), 'g_opacity': (g_op, A_gop, fl),
            'depth': (float(depth.detach()), A_terms.sum() / global_batch + float(depth.detach()), fl),
            'distl': (float(distl.detach()), np.abs(np.asarray(dl32, np.float64)).sum() * inv_n, fl), 'scale': (sc, abs(sc), fl), '_quad': quad,
            '_pre': pre.detach().numpy(), '_k': DEPTH_W * LOSS_SCALE / global_batch}


def _app_majorants(op, col, bg, gt, A_op, A_col, global_batch):
    k = COLOR_W * LOSS_SCALE / (3 * global_batch)
    b = np.zeros_like(col) if bg is None else bg
    cc = col + b * (1 - op)[:, None]
    diff = cc - gt
    quad = np.abs(diff) < BETA_C
    A_c = A_col + np.abs(b) * (A_op + 1 + np.abs(op))[:, None] + np.abs(col) + np.abs(gt)
    g = np.where(quad, diff / BETA_C, np.sign(diff)) * k
    A_g = np.where(quad, k * A_c / BETA_C, 0.0) + np.abs(g)
    sl = np.where(quad, 0.5 * diff * diff / BETA_C, np.abs(diff) - 0.5 * BETA_C)
    A_terms = np.where(quad, np.abs(diff) * A_c / BETA_C, A_c + 0.5 * BETA_C) + sl
    return g, A_g, sl, A_terms, quad


def truth_app_loss(c, op32, col32, bg, gt, global_batch):
    """perf_app_loss on given fp32 per-ray inputs -> {'g_color', 'loss'}; the background's opacity is detached."""
    R = c.R
    op = _t(np.asarray(op32).reshape(R)); col = _t(np.asarray(col32).reshape(R, 3)).requires_grad_(True)
    cc = col if bg is None else col + _t(bg) * (1.0 - op)[:, None]
    terms = _sl1(cc - _t(gt), BETA_C)
    closs = terms.sum() / (3 * global_batch)
    g_col, = torch.autograd.grad(closs * COLOR_W * LOSS_SCALE, col)
    z = np.zeros(R)
    _, A_g, _, A_terms, quad = _app_majorants(op.numpy(), col.detach().numpy(), bg, gt, z, np.zeros((R, 3)), global_batch)
    fl = TINY * (1 + LOSS_SCALE / BETA_C)
    return {'_k': COLOR_W * LOSS_SCALE / (3 * global_batch), 'g_color': (g_col.numpy(), A_g, fl), 'loss': (float(closs.detach()), A_terms.sum() / (3 * global_batch) + float(closs.detach()), fl), '_quad': quad}


def truth_head_geo(c, gt, noise, global_batch, ratio):
    """perf_train_head_geo from sigma: the forward's outputs, the per-ray loss terms, inv_n and d (whole scaled loss) / d sigma."""
    g = _Graph(c)
    fw = truth_fwd(c)
    f = fw['_']
    inv_n = inv_n_of(c, global_batch)
    dl = g.distloss()
    loss, depth, distl, terms, pre = _geo_loss_t(g.op, g.dist, dl, gt, noise, inv_n, global_batch, ratio)
    gd, A_gd, gop, A_gop, A_terms, quad, _ = _geo_majorants(fw['opacity'][0], fw['distance'][0], gt, noise, fw['opacity'][1], fw['distance'][1],
                                                           global_batch)
    dls = inv_n * DIST_W * ratio * LOSS_SCALE
    Gabs, A_G = _fused_majorant(c, f, gop, gd, A_gop, A_gd, dls)
    A, floor = dsigma_majorant(c, f, Gabs, np.zeros(c.S), np.zeros(c.S), A_G)
    per, A_per, _, gmaj = distloss_parts(c, f['w'])
    cnt = c.counts.astype(np.float64)
    out = {k: fw[k] for k in ('w', 'T', 'opacity', 'distance', 'colour')}
    out.update({'dl': (dl.detach().numpy(), A_per + c.seg(gmaj * f['A_w']), TINY * (cnt + 1 + c.seg(gmaj))),
                'depth_terms': (terms.detach().numpy(), A_terms, TINY), 'inv_n': (inv_n, inv_n, TINY),
                'd_sigma': (g.grad(loss, g.sig), A, floor), '_quad': quad, '_pre': pre.detach().numpy(), '_k': DEPTH_W * LOSS_SCALE / global_batch,
                '_loss': (float(loss.detach()), float(depth.detach()), float(distl.detach()))})
    return out


def truth_head_app(c, bg, gt, global_batch):
    """perf_train_head_app from sigma / rgb: outputs, per-ray colour terms, d (scaled colour loss) / d rgb."""
    g = _Graph(c)
    fw = truth_fwd(c)
    f = fw['_']
    cc = g.col if bg is None else g.col + _t(bg) * (1.0 - g.op.detach())[:, None]
    terms = _sl1(cc - _t(gt), BETA_C)
    loss = terms.sum() / (3 * global_batch) * COLOR_W * LOSS_SCALE
    gc, A_gc, _, A_terms, quad = _app_majorants(fw['opacity'][0], fw['colour'][0], bg, gt, fw['opacity'][1], fw['colour'][1], global_batch)
    drgb = g.grad(loss, g.rgb)
    A = f['A_w'][:, None] * np.abs(gc)[c.ri] + f['w'][:, None] * A_gc[c.ri] + np.abs(drgb)
    out = {k: fw[k] for k in ('w', 'T', 'opacity', 'distance', 'colour')}
    out.update({'color_terms': (terms.sum(1).detach().numpy(), A_terms.sum(1), TINY), 'd_rgb': (drgb, A, TINY * (1 + np.abs(gc)[c.ri])),
                '_quad': quad, '_k': COLOR_W * LOSS_SCALE / (3 * global_batch)})
    return out


def truth_accumulate(c, w32, values):
    w = np.asarray(w32, np.float64)[:c.S]
    v = np.ones((c.S, 1)) if values is None else np.asarray(values, np.float64)[:c.S]
    return {'out': (c.seg(w[:, None] * v), c.seg(np.abs(w[:, None] * v)), TINY * (c.counts[:, None] + 1.0))}


def truth_normal(c, w32, grad32):
    """perf_normal_composite: unit(sum_i w_i * -g_i / |g_i|), rows with a non-finite component or all zero skipped; zero where the sum is."""
    w = np.asarray(w32, np.float64)[:c.S]
    g = np.asarray(grad32, np.float64)[:c.S]
    ok = np.isfinite(g).all(1) & (np.abs(g).max(1) > 0)
    gn = np.linalg.norm(np.where(ok[:, None], g, 1.0), axis=1)
    n = np.where(ok[:, None], -g / gn[:, None], 0.0)
    N = c.seg(w[:, None] * n)
    nn = np.linalg.norm(N, axis=1)
    out = np.where(nn[:, None] > 0, N / np.where(nn > 0, nn, 1.0)[:, None], 0.0)
    A_N = c.seg(np.abs(w) * ok)
    safe = np.where(nn > 0, nn, 1.0)
    A = np.where(nn[:, None] > 0, 2 * (A_N / safe)[:, None] + np.abs(out), 0.0)
    floor = TINY + np.where(nn > 0, 2 * TINY * (c.counts + 1.0) / safe, 0.0)[:, None]
    return {'normal': (out, A, floor * np.ones_like(out))}


# ---- the loss inputs ---------------------------------------------------------------------------------------------------------------
def make_loss_inputs(c, seed=11):
    """Targets from the float64 forward so that every smooth-L1 branch is populated and no ray sits on a kink: noise 0 on THIN_RAYS
    (pre < 0), noise >= 0.6 on rays without samples (pre > 0), elsewhere U[0, 1) moved away from pre = 0; the distance target is
    d64 - diff with diff cycling through +-0.5 beta, +-3 beta; the colour target likewise.  fp32 numpy."""
    rng = np.random.default_rng([seed, int(c.S)])
    fw = truth_fwd(c)
    op, dist, col = fw['opacity'][0], fw['distance'][0], fw['colour'][0]
    noise = rng.uniform(0, 1, c.R)
    noise[c.counts == 0] = rng.uniform(0.6, 1.0, int((c.counts == 0).sum()))
    thin = [r for r in c.thin if c.counts[r] > 0]
    noise[thin] = 0.0
    noise = noise.astype(F)
    for _ in range(8):
        pre = dist + (2.0 * noise - 1.0) * (1 - op)
        near = np.abs(pre) < 4e-3
        noise[near] = np.where(noise[near] < 0.5, noise[near] + F(0.11), noise[near] - F(0.11))
    bg = rng.uniform(0, 1, (c.R, 3)).astype(F)
    cyc = np.array([0.5, -0.5, 3.0, -3.0])
    out = {'noise': noise, 'bg': bg}
    for key, nz in (('gt_noise', 2.0 * noise.astype(np.float64) - 1.0), ('gt_plain', np.zeros(c.R))):
        d64 = np.maximum(dist + nz * (1 - op), 0.0)
        out[key] = (d64 - BETA_D * cyc[(np.arange(c.R) + 1) % 4]).astype(F)
    for key, b in (('gtc_bg', bg.astype(np.float64)), ('gtc_plain', np.zeros((c.R, 3)))):
        c64 = col + b * (1 - op)[:, None]
        out[key] = (c64 - BETA_C * cyc[(np.arange(3 * c.R).reshape(c.R, 3) + 2) % 4]).astype(F)
    return out


def kink_margins(c, li, noise_on, bg_on):
    """Float64 distances from the kinks -> (min | |diff_d| - beta_d | / beta_d, min |pre|, min | |diff_c| - beta_c | / beta_c, #pre<0, #empty pre>0, min |pre| over rays with samples)."""
    fw = truth_fwd(c)
    op, dist, col = fw['opacity'][0], fw['distance'][0], fw['colour'][0]
    nz = 2.0 * li['noise'].astype(np.float64) - 1.0 if noise_on else np.zeros(c.R)
    pre = dist + nz * (1 - op)
    dd = np.maximum(pre, 0) - li['gt_noise' if noise_on else 'gt_plain'].astype(np.float64)
    b = li['bg'].astype(np.float64) if bg_on else np.zeros((c.R, 3))
    dc = col + b * (1 - op)[:, None] - li['gtc_bg' if bg_on else 'gtc_plain'].astype(np.float64)
    md = float(np.min(np.abs(np.abs(dd) - BETA_D))) / BETA_D
    mc = float(np.min(np.abs(np.abs(dc) - BETA_C))) / BETA_C
    empty = c.counts == 0
    return md, float(np.min(np.abs(pre))), mc, int((pre < 0).sum()), int((pre[empty] > 0).sum()), float(np.min(np.abs(pre[~empty])))


# ---- emulation: the kernels' fp32 arithmetic -------------------------------------------------------------------------------------
# expf is the one operation of these kernels that is not correctly rounded, on the host or on the device: its documented accuracy is one
# ulp.  The emulation therefore runs under four models of it -- the host library's value, that value moved one ulp up, one ulp down, and
# moved by -1 / 0 / +1 ulp at random (seeded) --, exp(0) = 1 staying exact, and the emulation's worst error is the worst of the four.
EXP_MODELS = ('libm', 'up', 'down', 'random')
_exp_model = 'libm'


def _expf(x):
    x = np.asarray(x, F)
    y = np.exp(x)
    if _exp_model == 'libm':
        return y
    if _exp_model == 'random':
        k = np.random.default_rng(x.size + 5).integers(-1, 2, x.shape)
    else:
        k = np.full(x.shape, 1 if _exp_model == 'up' else -1)
    moved = np.where(k > 0, np.nextafter(y, F(np.inf)), np.where(k < 0, np.nextafter(y, F(0)), y))
    return np.where((x == 0) | (y == 0), y, moved).astype(F)


def _canon(c, v):
    return O.packed_exclusive_sum_canonical(np.asarray(v, F), c.packed) if c.S else np.zeros(0, F)


def _lane_sum(c, v):
    """Lane-strided partial sums over the chunks, then the xor butterfly 32..1 (team_sum / wave_sum)."""
    D = c.dense(np.asarray(v, F), F).reshape(c.R, c.nch, 64)
    acc = np.zeros((c.R, 64), F)
    for q in range(c.nch):
        acc = acc + D[:, q]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ off]
    return acc[:, 0]


def _block_sum(v):
    """The loss heads' sums: one element per thread, xor butterfly inside each wavefront, the four wavefronts of a workgroup added in
    order, the workgroups' totals folded by one more butterfly."""
    v = np.asarray(v, F).reshape(-1)
    nb = max(1, -(-v.size // 256))
    x = np.zeros(nb * 256, F)
    x[:v.size] = v
    x = x.reshape(nb, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ off]
    x = x[..., 0]
    tot = np.zeros(64, F)
    tot[:nb] = ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]
    for off in (32, 16, 8, 4, 2, 1):
        tot = tot + tot[lane ^ off]
    return tot[0]


def _suffix_excl32(c, v, bug=None):
    """sum over the later samples of the ray as the backward kernels form it: Kogge-Stone inclusive suffix inside the 64-sample chunk,
    minus the sample, plus the carry of the later chunks."""
    v = np.asarray(v, F)
    X = c.dense(v, F)
    if bug == 'total_minus_prefix':
        inc = np.cumsum(X, 1, dtype=F)
        return c.flat((inc[:, -1:] - inc).astype(F))
    X = X.reshape(c.R, c.nch, 64)
    suf = X.copy()
    for off in (1, 2, 4, 8, 16, 32):
        Y = np.zeros_like(suf)
        Y[..., :-off] = suf[..., off:]
        suf = suf + Y
    out = np.zeros_like(X)
    carry = np.zeros(c.R, F)
    for q in range(c.nch - 1, -1, -1):
        own = suf[:, q] if bug == 'later_inclusive' else suf[:, q] - X[:, q]
        out[:, q] = own if bug == 'drop_carry' else carry[:, None] + own
        carry = carry + suf[:, q, 0]
    return c.flat(out.reshape(c.R, c.L))


def _f32(c):
    S = c.S
    ts, te, sig = c.ts[:S], c.te[:S], c.sig[:S]
    return ts, te, sig, te - ts, (ts + te) * F(0.5)


def emu_distloss_fwd(c, w):
    ts, te, sig, d, m = _f32(c)
    w = np.asarray(w, F)[:c.S]
    Wp, WMp = _canon(c, w), _canon(c, w * m)
    return _lane_sum(c, d * w * w * F(1.0 / 3.0) + F(2) * w * (m * Wp - WMp))


def emu_fwd(c):
    """composite_fwd_kernel (with the distortion sums of its fused form) -> dict of fp32 arrays."""
    ts, te, sig, d, m = _f32(c)
    sd = sig * d
    ex = _canon(c, sd)
    T = _expf(-ex)
    al = F(1) - _expf(-sd)
    w = T * al
    rgb = c.rgb[:c.S]
    col = np.stack([_lane_sum(c, w * rgb[:, k]) for k in range(3)], -1)
    return {'w': w, 'T': T, 'alphas': al, 'opacity': _lane_sum(c, w), 'distance': _lane_sum(c, w * m), 'colour': col,
            'dl': emu_distloss_fwd(c, w)}


def _dl_grad32(c, w, W, Wsuf, WM, WMsuf, scale, bug):
    ts, te, sig, d, m = _f32(c)
    k = F(1.0 / 3.0) if bug == 'third' else F(2.0) / F(3.0)
    return scale * (k * d * w + F(2) * (m * (W - Wsuf) - (WM - WMsuf)))


def emu_distloss_bwd(c, w, scale, bug=None):
    ts, te, sig, d, m = _f32(c)
    w = np.asarray(w, F)[:c.S]
    totW, totWM = _lane_sum(c, w)[c.ri], _lane_sum(c, w * m)[c.ri]
    W, WM = _canon(c, w), _canon(c, w * m)
    return _dl_grad32(c, w, W, totW - W - w, WM, totWM - WM - w * m, F(scale), bug)


def emu_bwd(c, w, T, g_w=None, g_op=None, g_d=None, g_T=None, g_al=None, g_col=None, fused=None, bug=None):
    """composite_bwd_kernel -> (d_sigma, d_rgb).  fused = (totW [R], totWM [R], scale): the distortion gradient formed in the kernel."""
    ts, te, sig, d, m = _f32(c)
    S, R = c.S, c.R
    z = lambda x, n: np.zeros(n, F) if x is None else np.asarray(x, F).reshape(n)
    w, T = np.asarray(w, F)[:S], np.asarray(T, F)[:S]
    gop, gd = z(g_op, R), z(g_d, R)
    G = gop[c.ri] + gd[c.ri] * m + z(g_w, S)
    gT, gA = z(g_T, S), z(g_al, S)
    if bug == 'no_gA':
        gA = np.zeros(S, F)
    if fused is not None:
        totW, totWM, scale = fused
        wm = w * m
        Wsuf, WMsuf = _suffix_excl32(c, w), _suffix_excl32(c, wm)
        W = np.asarray(totW, F).reshape(R)[c.ri] - Wsuf - w
        WM = np.asarray(totWM, F).reshape(R)[c.ri] - WMsuf - wm
        G = G + _dl_grad32(c, w, W, Wsuf, WM, WMsuf, F(scale), bug)
    later = _suffix_excl32(c, G * w + gT * T, bug)
    ds = d * ((G * T + gA) * _expf(-sig * d) - later)
    drgb = None if g_col is None else w[:, None] * np.asarray(g_col, F).reshape(R, 3)[c.ri]
    return ds, drgb


def _sl1_32(diff, beta, bug):
    a = np.abs(diff)
    quad = (a < F(beta)) & (bug != 'sl1_linear')
    term = np.where(a < F(beta), F(0.5) * diff * diff / F(beta), a - F(0.5) * F(beta)).astype(F)
    sg = np.where(quad, diff / F(beta), np.sign(diff)).astype(F)
    return term, sg


def emu_geo_loss(c, op, dist, dl, gt, noise, global_batch, ratio, bug=None):
    """geo_loss_kernel -> dict(g_opacity, g_distance, depth, distl, scale, terms, inv_n)."""
    R = c.R
    op, dist, dl, gt = (np.asarray(x, F).reshape(R) for x in (op, dist, dl, gt))
    inv_bs = F(1) / F(global_batch)
    nz = np.zeros(R, F) if noise is None else np.asarray(noise, F) * F(2) - F(1)
    pre = dist + nz * (F(1) - op)
    diff = np.maximum(pre, F(0)) - gt
    term, sg = _sl1_32(diff, BETA_D, bug)
    gd = np.where(pre > 0, sg * inv_bs * F(DEPTH_W) * F(LOSS_SCALE), F(0)).astype(F)
    gop = (nz * gd if bug == 'gop_sign' else -nz * gd).astype(F)
    if global_batch != R:
        inv_n = inv_bs
    else:
        n = F(R) if bug == 'n_rays' else F(c.last + 1 if c.last >= 0 else 1)
        inv_n = F(1) / n
    return {'g_opacity': gop, 'g_distance': gd, 'depth': _block_sum(term) * inv_bs, 'distl': _block_sum(dl) * inv_n,
            'scale': inv_n * F(DIST_W) * F(ratio) * F(LOSS_SCALE), 'terms': term, 'inv_n': inv_n}


def emu_app_loss(c, op, col, bg, gt, global_batch, bug=None):
    """app_loss_kernel -> dict(g_color, loss, terms [R])."""
    R = c.R
    op, col, gt = np.asarray(op, F).reshape(R), np.asarray(col, F).reshape(R, 3), np.asarray(gt, F).reshape(R, 3)
    inv_n = F(1) / F(global_batch * 3)
    b = np.zeros((R, 3), F) if bg is None else np.asarray(bg, F)
    diff = (col + b * (F(1) - op)[:, None]) - gt
    term, sg = _sl1_32(diff, BETA_C, bug)
    return {'g_color': (sg * inv_n * F(COLOR_W) * F(LOSS_SCALE)).astype(F), 'loss': _block_sum(term) * inv_n, 'terms': (term[:, 0] + term[:, 1]) + term[:, 2]}


def emu_head_geo(c, gt, noise, global_batch, ratio, bug=None):
    """train_head_kernel<geometry>: forward -> the ray's loss head -> fused backward."""
    fw = emu_fwd(c)
    lo = emu_geo_loss(c, fw['opacity'], fw['distance'], fw['dl'], gt, noise, global_batch, ratio, bug)
    ds, _ = emu_bwd(c, fw['w'], fw['T'], g_op=lo['g_opacity'], g_d=lo['g_distance'], fused=(fw['opacity'], fw['distance'], lo['scale']), bug=bug)
    out = {k: fw[k] for k in ('w', 'T', 'opacity', 'distance', 'colour', 'dl')}
    out.update(depth_terms=lo['terms'], inv_n=lo['inv_n'], d_sigma=ds)
    return out


def emu_head_app(c, bg, gt, global_batch, bug=None):
    fw = emu_fwd(c)
    lo = emu_app_loss(c, fw['opacity'], fw['colour'], bg, gt, global_batch, bug)
    _, drgb = emu_bwd(c, fw['w'], fw['T'], g_col=lo['g_color'])
    out = {k: fw[k] for k in ('w', 'T', 'opacity', 'distance', 'colour')}
    out.update(color_terms=lo['terms'], d_rgb=drgb)
    return out


def emu_accumulate(c, w, values):
    w = np.asarray(w, F)[:c.S]
    if values is None:
        return _lane_sum(c, w * F(1))[:, None]
    v = np.asarray(values, F)[:c.S]
    return np.stack([_lane_sum(c, w * v[:, k]) for k in range(v.shape[1])], -1)


def emu_normal(c, w, grad):
    """normal_composite_kernel: rows scaled by their largest component before the norm, 16 lanes per ray, xor butterfly 8..1."""
    S, R = c.S, c.R
    w, g = np.asarray(w, F)[:S], np.asarray(grad, F)[:S]
    with np.errstate(all='ignore'):
        mx = np.abs(g).max(1)
        ok = (mx > 0) & (mx <= F(3.0e38))
        u = np.where(ok[:, None], g / np.where(ok, mx, F(1))[:, None], F(0)).astype(F)
        k = (-w / np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2] + (~ok).astype(F))).astype(F)
    term = np.where(ok[:, None], k[:, None].astype(np.float64) * u, 0.0)        # fmaf(k, u, a): the product enters the sum unrounded
    nsl = max(1, (int(c.counts.max()) + 15) // 16)
    acc = np.zeros((R, nsl, 16, 3))
    acc[c.ri, c.pos // 16, c.pos % 16] = term
    a = np.zeros((R, 16, 3), F)
    for q in range(nsl):
        a = (a + acc[:, q]).astype(F)
    lane = np.arange(16)
    for off in (8, 4, 2, 1):
        a = a + a[:, lane ^ off]
    a = a[:, 0]
    mx = np.abs(a).max(1)
    ok = (mx > 0) & (mx <= F(3.0e38))
    u = (a / np.where(ok, mx, F(1))[:, None]).astype(F)
    kk = F(1) / np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2] + (~ok).astype(F))
    return np.where(ok[:, None], u * kk[:, None], F(0)).astype(F)


def make_normal_inputs(c, w32, seed=13):
    """Gradient rows of magnitude 1e-30 .. 1e30 (their squares leave fp32) with exactly-zero and infinite rows, and -- on ray 21 (65
    samples) -- weights and rows rewritten so that the sum cancels exactly.  -> (weights, grad) fp32, and that ray's index."""
    rng = np.random.default_rng([seed, int(c.S)])
    g = rng.standard_normal((c.S, 3)) * 10.0 ** rng.uniform(-30, 30, (c.S, 1))
    g = g.astype(F)
    kind = rng.integers(0, 12, c.S)
    g[kind == 0] = 0.0
    g[kind == 1, 1] = np.inf
    w = np.asarray(w32, F)[:c.S].copy()
    r = 21 if c.R > 21 else 1
    lo = int(c.packed[r, 0])
    n = int(c.counts[r])
    if n >= 2:
        g[lo:lo + n] = 0.0; w[lo:lo + n] = F(0.125)
        g[lo] = (F(3e20), 0, 0); g[lo + n - 1] = (F(-5e-20), 0, 0)
    return w, g, r


# ---- the pieces every comparison is made of ----------------------------------------------------------------------------------------
def grads_in(c, seed=17):
    """Upstream gradients of composite_bwd: fp32 normal draws."""
    rng = np.random.default_rng([seed, int(c.S)])
    n = lambda *s: rng.standard_normal(s).astype(F)
    return dict(g_w=n(c.S), g_op=n(c.R), g_d=n(c.R), g_T=(0.5 * n(c.S)).astype(F), g_al=(0.5 * n(c.S)).astype(F), g_col=n(c.R, 3))


FUSED_SCALE_HOST, FUSED_SCALE_DEV = float(np.float32(0.74)), 0.5        # scale and scale_dev[0] of the distortion kernels
FUSED_SCALE = FUSED_SCALE_HOST * FUSED_SCALE_DEV


def emulation_table(c, li=None, bug=None):
    """Every comparison of the GPU test made on the emulation: {(op, output): units}.  `bug`: the wrong variant."""
    li = make_loss_inputs(c) if li is None else li
    gi = grads_in(c)
    tab = {}

    def put(op, ref, got, names):
        for name in names:
            tab[(op, name)] = units(got[name], ref[name])

    fw = emu_fwd(c)
    put('composite_fwd', truth_fwd(c), fw, ('w', 'T', 'alphas', 'opacity', 'distance', 'colour'))
    ds, drgb = emu_bwd(c, fw['w'], fw['T'], **gi, bug=bug)
    put('composite_bwd', truth_bwd(c, **gi), {'d_sigma': ds, 'd_rgb': drgb}, ('d_sigma', 'd_rgb'))
    put('distloss', truth_distloss(c, fw['w'], FUSED_SCALE),
        {'dl': emu_distloss_fwd(c, fw['w']), 'g_w': emu_distloss_bwd(c, fw['w'], FUSED_SCALE, bug)}, ('dl', 'g_w'))
    dsf, _ = emu_bwd(c, fw['w'], fw['T'], g_op=gi['g_op'], g_d=gi['g_d'], fused=(fw['opacity'], fw['distance'], FUSED_SCALE), bug=bug)
    put('composite_distloss', truth_fused(c, gi['g_op'], gi['g_d'], FUSED_SCALE), {'dl': fw['dl'], 'd_sigma': dsf}, ('dl', 'd_sigma'))
    for tag, noise, gt, ratio, gb in (('noise', li['noise'], li['gt_noise'], RATIO, c.R), ('plain', None, li['gt_plain'], 1.0, 4 * c.R)):
        lo = emu_geo_loss(c, fw['opacity'], fw['distance'], fw['dl'], gt, noise, gb, ratio, bug)
        put('geo_loss/' + tag, truth_geo_loss(c, fw['opacity'], fw['distance'], fw['dl'], gt, noise, gb, ratio), lo,
            ('g_opacity', 'g_distance', 'depth', 'distl', 'scale'))
        hd = emu_head_geo(c, gt, noise, gb, ratio, bug)
        put('train_head_geo/' + tag, truth_head_geo(c, gt, noise, gb, ratio), hd,
            ('w', 'T', 'opacity', 'distance', 'colour', 'dl', 'depth_terms', 'inv_n', 'd_sigma'))
    for tag, bg, gt, gb in (('bg', li['bg'], li['gtc_bg'], c.R), ('plain', None, li['gtc_plain'], 4 * c.R)):
        lo = emu_app_loss(c, fw['opacity'], fw['colour'], bg, gt, gb, bug)
        put('app_loss/' + tag, truth_app_loss(c, fw['opacity'], fw['colour'], bg, gt, gb), lo, ('g_color', 'loss'))
        put('train_head_app/' + tag, truth_head_app(c, bg, gt, gb), emu_head_app(c, bg, gt, gb, bug),
            ('w', 'T', 'opacity', 'distance', 'colour', 'color_terms', 'd_rgb'))
    rgb = c.rgb[:c.S]
    tab[('accumulate_fwd', 'C1')] = units(emu_accumulate(c, fw['w'], None), truth_accumulate(c, fw['w'], None)['out'])
    tab[('accumulate_fwd', 'C3')] = units(emu_accumulate(c, fw['w'], rgb), truth_accumulate(c, fw['w'], rgb)['out'])
    wn, gn, _ = make_normal_inputs(c, fw['w'])
    tab[('normal_composite', 'normal')] = units(emu_normal(c, wn, gn), truth_normal(c, wn, gn)['normal'])
    return tab


def emulation_worst(c, li=None):
    """{(op, output): the emulation's worst error in units over the four models of expf}: what the GPU test's bar is four times of."""
    global _exp_model
    li = make_loss_inputs(c) if li is None else li
    worst = {}
    try:
        for _exp_model in EXP_MODELS:
            for key, u in emulation_table(c, li).items():
                worst[key] = max(worst.get(key, 0.0), u)
    finally:
        _exp_model = 'libm'
    return worst
