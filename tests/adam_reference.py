"""Float64 reference of the fused Adam step (perf_amd/csrc/misc.hip: adam_kernel / adam4_kernel), the per-element error
bars of the fp32 kernel against it, and an fp32 emulation of the kernel's expression order.  Plain torch / numpy: no GPU.

    m' = m + (1-b1)(g-m)
    v' = v b2 + (1-b2) g g
    p' = p - (lr/(1-b1^t)) * m' / (sqrt(v')/sqrt(1-b2^t) + eps)

The hyper-parameters are taken at their fp32-rounded values, which is what the kernel receives; 1-b is the fp32
subtraction (exact for 0.5 <= b < 1).

The bars count the fp32 roundings of the kernel's expression (u = 2^-24; -ffp-contract=off, correctly rounded / and sqrt):
    m' : a subtraction, a product, an addition, each of magnitude <= |m|+|g|          -> 4u(|m|+|g|)
    v' : three products and an addition of magnitude <= |v|+g^2                       -> 4u(|v|+g^2)
    p' : the final subtraction rounds at |p'| (and p' itself to fp32) -> 2u|p'|; the step S m'/D carries the roundings of m',
         of v' (halved by the sqrt), of sqrt, the product with 1/sqrt(bc2), the addition of eps, the division and the product
         with S, and the roundings of the two scalars S and 1/sqrt(bc2): about a dozen u of S(|m|+|g|)/D  -> 16u K_t S(|m|+|g|)/D
K_t = 1 when the scalars are formed in double on the host (perf_adam_step).  The device entry (perf_adam_step_dev) forms
1 - powf(b, t) in fp32: the cancellation amplifies the last-place error of powf by b^t/(1-b^t), for either beta:
K_t = 1 + b1^t/(1-b1^t) + b2^t/(1-b2^t)."""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149

# (beta1, beta2, eps, lr)
HYPERS = [(0.9, 0.999, 1e-8, 1e-2), (0.9, 0.99, 1e-15, 1e-3), (0.5, 0.75, 1e-8, 0.25)]
FAMILIES = ('wide', 'sparse', 'matched')


def _f32(x):
    return float(np.float32(x))


def rounded(lr, beta1, beta2, eps):
    """-> (lr, b1, b2, eps, 1-b1, 1-b2) as Python floats holding the fp32 values the kernel receives."""
    lr, b1, b2, eps = _f32(lr), _f32(beta1), _f32(beta2), _f32(eps)
    omb1 = float(np.float32(1.0) - np.float32(b1)); omb2 = float(np.float32(1.0) - np.float32(b2))
    return lr, b1, b2, eps, omb1, omb2


def _scalars_f64(t, lr, b1, b2):
    """-> (S = lr/(1-b1^t), 1/sqrt(1-b2^t), K_t of the device entry), in double."""
    t = float(int(t))
    p1, p2 = b1 ** t, b2 ** t
    bc1, bc2 = 1.0 - p1, 1.0 - p2
    return lr / bc1, 1.0 / np.sqrt(bc2), 1.0 + p1 / bc1 + p2 / bc2


def _step_f64(p, m, v, g, t, lr, beta1, beta2, eps):
    lr, b1, b2, eps, omb1, omb2 = rounded(lr, beta1, beta2, eps)
    p, m, v, g = (x.detach().cpu().double() for x in (p, m, v, g))
    S, inv, K = _scalars_f64(t, lr, b1, b2)
    m1 = m + omb1 * (g - m)
    v1 = v * b2 + omb2 * g * g
    D = v1.sqrt() * inv + eps
    p1 = p - S * (m1 / D)
    return p1, m1, v1, S, D, K


def adam_step_f64(p, m, v, g, t, lr, beta1, beta2, eps):
    """One Adam step in float64 -> (p', m', v') as float64 CPU tensors."""
    return _step_f64(p, m, v, g, t, lr, beta1, beta2, eps)[:3]


def adam_bounds(p, m, v, g, t, lr, beta1, beta2, eps, dev=False):
    """Per-element bars of the fp32 kernel against adam_step_f64 from the same state -> (tol_p, tol_m, tol_v), float64.
    dev: the device-scalar entry (bias corrections formed in fp32 by the kernel's prologue)."""
    p1, m1, v1, S, D, K = _step_f64(p, m, v, g, t, lr, beta1, beta2, eps)
    m, v, g = (x.detach().cpu().double() for x in (m, v, g))
    mg = m.abs() + g.abs()
    tol_m = 4 * U * mg + TINY
    tol_v = 4 * U * (v.abs() + g * g) + TINY
    tol_p = 2 * U * p1.abs() + 16 * U * (K if dev else 1.0) * S * mg / D + TINY
    return tol_p, tol_m, tol_v


def entry_gap_bound(p, m, v, g, t, lr, beta1, beta2, eps):
    """How far the device-scalar entry's p' may lie from the host-scalar entry's, from the same state: the two differ in the
    scalars S and 1/sqrt(bc2) only -> 16u K_t S(|m|+|g|)/D + 2u|p'|, K_t the device entry's (m' and v' do not differ at all)."""
    p1, m1, v1, S, D, K = _step_f64(p, m, v, g, t, lr, beta1, beta2, eps)
    mg = m.detach().cpu().double().abs() + g.detach().cpu().double().abs()
    return 16 * U * K * S * mg / D + 2 * U * p1.abs()


def adam_emulated_f32(p, m, v, g, t, lr, beta1, beta2, eps, dev=False):
    """The kernel's expression in fp32, operation by operation in its order -> (p', m', v') float32.  dev: the bias corrections
    as the device prologue forms them (1.0f - powf(b, t), lr / bc1, 1.0f / sqrtf(bc2)); otherwise in double on the host, then
    rounded.  For the CPU test of the bars and for printed ratios only."""
    lr, b1, b2, eps, omb1, omb2 = rounded(lr, beta1, beta2, eps)
    f = np.float32
    if dev:
        tf = f(int(t))
        bc1 = f(1.0) - np.power(f(b1), tf, dtype=f); bc2 = f(1.0) - np.power(f(b2), tf, dtype=f)
        step_size = float(f(lr) / bc1); inv = float(f(1.0) / np.sqrt(bc2, dtype=f))
    else:
        S, i64, _ = _scalars_f64(t, lr, b1, b2)
        step_size = _f32(S); inv = _f32(i64)
    p, m, v, g = (x.detach().cpu().float() for x in (p, m, v, g))
    m1 = m + omb1 * (g - m)
    v1 = v * b2 + (omb2 * g) * g
    denom = v1.sqrt() * inv + eps
    p1 = p - step_size * (m1 / denom)
    return p1, m1, v1


def make_state(family, n, seed):
    """Seeded fp32 CPU state (p, m, v, g) of one family:
    wide     exponents of g and m uniform in [-40, 10] with random signs, exponents of v uniform in [-80, 20], p ~ 0.3 randn;
    sparse   wide, with half of g exactly 0 and 30 % of (m, v) exactly 0 together (table entries no sample touched);
    matched  g as wide, m = g U(-1, 1), v = g^2 U(0.01, 2) (moments that have seen gradients of this size).
    No non-zero |g| is below 2^-40: g^2 and v' stay normal numbers."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    sign = lambda: torch.where(rnd() < 0.5, -1.0, 1.0).double()
    mag = lambda lo, hi: torch.exp2(lo + (hi - lo) * rnd())
    p = 0.3 * torch.randn(n, generator=gen, dtype=torch.float64)
    g = sign() * mag(-40, 10)
    if family == 'matched':
        m = g * (2 * rnd() - 1)
        v = g * g * (0.01 + 1.99 * rnd())
    else:
        m = sign() * mag(-40, 10)
        v = mag(-80, 20)
    if family == 'sparse':
        g = torch.where(rnd() < 0.5, torch.zeros_like(g), g)
        untouched = rnd() < 0.3
        m = torch.where(untouched, torch.zeros_like(m), m)
        v = torch.where(untouched, torch.zeros_like(v), v)
    elif family not in FAMILIES:
        raise ValueError(family)
    p, m, v, g = (x.float() for x in (p, m, v, g))
    assert not bool(((g != 0) & (g.abs() < 2.0 ** -40)).any())
    return p, m, v, g
