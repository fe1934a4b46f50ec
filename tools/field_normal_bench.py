"""The fused density-gradient kernel (ops.field_grad_x) against the composed path it replaces -- ops.hashgrid_fwd ->
ops.mlp_bwd(need_dfeat=True) -> ops.hashgrid_bwd_input -- at 1 M samples, uniform and ray-ordered, alternated in one process.

  python tools/field_normal_bench.py [--n 1048576] [--dtype fp16] [--rounds 5] [--iters 20]

Prints one JSON object: per ordering the median milliseconds per call of both paths (device events around `iters` back-to-back
calls, `rounds` alternations after a warm-up), the speed-up, the largest difference between the two gradients, and the fused kernel's
algorithmic-bytes roofline fraction (12 B position + 1 B selector + L x 8 corners x 4 B gathered + 16 B written per sample, over the
time, against 8 TB/s)."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from perf_amd import ops
from perf_amd.grid import GridConfig, MlpConfig
from perf_amd.scene import gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=1 << 20)
ap.add_argument('--dtype', default='fp16')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=20)
args = ap.parse_args()
HBM_PEAK = 8.0e12

dev = 'cuda'
torch.manual_seed(0)
grid = GridConfig()
mlp = MlpConfig(n_levels=grid.n_levels, n_hidden_layers=1, n_output_dims=1, output_activation='Exponential')
n_net = mlp.n_params
g = torch.Generator(device='cpu').manual_seed(1337)
params = torch.cat([(torch.rand(o * i, generator=g) * 2 - 1) * (6.0 / (i + o)) ** 0.5 for (o, i) in mlp.shapes]
                   + [(torch.rand(grid.n_params, generator=g) * 2 - 1) * 0.5]).to(dev)
w16 = ops.cast_params(params, args.dtype)
table32 = params[n_net:].contiguous()
n = args.n


def uniform():
    return torch.rand(n, 3, device=dev)


def ray_ordered(per_ray=64, step=5e-4):
    """Consecutive samples of a panorama's rays, as a frame's sample arrays hold them: per_ray steps of the render step along each ray."""
    n_rays = n // per_ray
    h = int((n_rays // 2) ** 0.5)
    rays = gen_pano_rays(torch.eye(4), h, 2 * h)
    d = rays.d.reshape(-1, 3)
    reps = -(-n_rays // d.shape[0])
    d = d.repeat(reps, 1)[:n_rays]
    t0 = 0.2 + 0.5 * torch.rand(n_rays, 1, device=dev)
    t = t0 + step * torch.arange(per_ray, device=dev)[None, :]
    x = (d[:, None, :] * t[:, :, None]).reshape(-1, 3)
    x = torch.cat([x, x[:n - x.shape[0]]]) if x.shape[0] < n else x[:n]
    return ((x + 1.0) * 0.5).contiguous()


def fused(x01, sel):
    return ops.field_grad_x(grid, mlp, x01, sel, w16, None)[1]


def composed(x01, sel, dout):
    feat = ops.hashgrid_fwd(grid, x01, w16[n_net:])
    dfeat, _ = ops.mlp_bwd(mlp, w16[:n_net], feat, dout, sel, need_dfeat=True)
    return ops.hashgrid_bwd_input(grid, x01, dfeat, table32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


out = {'n': n, 'dtype': args.dtype, 'levels': grid.n_levels, 'rounds': args.rounds, 'iters_per_round': args.iters, 'orderings': {}}
bytes_per_sample = 12 + 1 + grid.n_levels * 8 * 4 + 16
with torch.no_grad():
    for name, make in (('uniform', uniform), ('ray_ordered', ray_ordered)):
        x01 = make()
        sel = ((x01 > 0) & (x01 < 1)).all(-1).to(torch.uint8)
        dout = torch.ones(n, 1, device=dev)
        gf, gc = fused(x01, sel), composed(x01, sel, dout)
        scale = gc.abs().amax(dim=1).clamp_min(1e-30)
        diff = float(((gf - gc).abs().amax(dim=1) / scale).quantile(0.99)) if n <= (1 << 24) else None
        for _ in range(3):
            fused(x01, sel); composed(x01, sel, dout)
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(args.rounds):
            tf.append(timed(lambda: fused(x01, sel)))
            tc.append(timed(lambda: composed(x01, sel, dout)))
        mf, mc = statistics.median(tf), statistics.median(tc)
        out['orderings'][name] = {'fused_ms': mf, 'fused_ms_all': tf, 'composed_ms': mc, 'composed_ms_all': tc, 'speedup': mc / mf,
                                  'p99_relative_difference_of_the_two_gradients': diff,
                                  'fused_algorithmic_bytes_per_sample': bytes_per_sample,
                                  'fused_algorithmic_TB_per_s': bytes_per_sample * n / (mf * 1e-3) / 1e12,
                                  'fused_roofline_fraction_of_8_TB_per_s': bytes_per_sample * n / (mf * 1e-3) / HBM_PEAK}
print(json.dumps(out, indent=1))
