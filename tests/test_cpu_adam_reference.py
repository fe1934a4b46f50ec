"""The float64 Adam reference of tests/adam_reference.py against torch.optim.Adam, and its error bars against an fp32
emulation of the kernel's expression: the bars the GPU tests (tests/test_gpu_step_tail.py) assert stay honest."""
import pytest
import torch

from tests import adam_reference as AR

STEPS = (1, 2, 3, 10, 100, 1000, 10000, 100000)


@pytest.mark.parametrize('hyper', [None] + AR.HYPERS[1:])
def test_adam_step_f64_chained_from_zero_moments_equals_torch_adam(hyper):
    """5 steps from zero moments; torch.optim.Adam on float64 tensors with the same fp32-rounded hyper-parameters."""
    b1, b2, eps, lr = hyper if hyper is not None else (0.9, 0.999, 1e-8, 1e-2)
    lr_r, b1_r, b2_r, eps_r, _, _ = AR.rounded(lr, b1, b2, eps)
    gen = torch.Generator().manual_seed(5)
    n = 1031
    p = torch.randn(n, generator=gen)
    ref = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([ref], lr=lr_r, betas=(b1_r, b2_r), eps=eps_r)
    P, M, V = p.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 6):
        g = torch.randn(n, generator=gen) * 128
        g[torch.rand(n, generator=gen) < 0.3] = 0.0
        ref.grad = g.double().clone()
        opt.step()
        P, M, V = AR.adam_step_f64(P, M, V, g, t, lr, b1, b2, eps)
        assert P.dtype == torch.float64
        st = opt.state[ref]
        for got, want in ((P, ref.detach()), (M, st['exp_avg']), (V, st['exp_avg_sq'])):
            assert bool(((got - want).abs() <= 1e-12 * want.abs()).all()), t


@pytest.mark.parametrize('dev', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('family', AR.FAMILIES)
def test_fp32_emulation_stays_within_six_tenths_of_the_bars(family, dev):
    """The kernel's expression order evaluated in fp32 on the CPU, against float64, on the state families of the GPU tests."""
    st = AR.make_state(family, 20011, seed=3)
    worst = [0.0, 0.0, 0.0]
    for b1, b2, eps, lr in AR.HYPERS:
        for t in STEPS:
            ref = AR.adam_step_f64(*st, t, lr, b1, b2, eps)
            tol = AR.adam_bounds(*st, t, lr, b1, b2, eps, dev=dev)
            emu = AR.adam_emulated_f32(*st, t, lr, b1, b2, eps, dev=dev)
            for k, (r, e, bar) in enumerate(zip(ref, emu, tol)):
                assert bool(torch.isfinite(r).all()) and bool((bar > 0).all())
                ratio = float(((e.double() - r).abs() / bar).max())
                worst[k] = max(worst[k], ratio)
                assert ratio <= 0.6, ('pmv'[k], family, dev, t, (b1, b2, eps, lr), ratio)
    print(f'emulation / bar, {family}, dev={dev}: p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}')

