"""What training on surface normals costs: the fused backward of the density gradient (ops.field_grad_x_bwd) against the first-order
field backward (ops.field_bwd on kept features: it does a subset of the work, so the ratio is the cost of the second column and
of the global atomics) at 32,768 and 1 M ray-ordered samples, alternated in one process; and an eager geometry step with and without
the normal loss.

  python tools/field_normal_train_bench.py [--dtype fp16] [--rounds 5] [--iters 20] [--steps 30] [--out profiles/field_normal_train.json]

Prints one JSON object and, with --out, merges it into that file under the key 'bench' (the file's other keys -- the figures the GPU
tests report -- are kept).  Figures are reported, nothing is asserted."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import ops, synthetic
from perf_amd.grid import GridConfig, MlpConfig
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='fp16')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--steps', type=int, default=30)
ap.add_argument('--out', default=None)
args = ap.parse_args()

dev = 'cuda'
torch.manual_seed(0)
grid = GridConfig()
mlp = MlpConfig(n_levels=grid.n_levels, n_hidden_layers=1, n_output_dims=1, output_activation='Exponential')
n_net = mlp.n_params
g = torch.Generator(device='cpu').manual_seed(1337)
params = torch.cat([(torch.rand(o * i, generator=g) * 2 - 1) * (6.0 / (i + o)) ** 0.5 for (o, i) in mlp.shapes]
                   + [(torch.rand(grid.n_params, generator=g) * 2 - 1) * 0.5]).to(dev)
w16 = ops.cast_params(params, args.dtype)


def ray_ordered(n, per_ray=64, step=5e-4):
    """Consecutive samples of a panorama's rays, as a step's sample arrays hold them (tools/field_normal_bench.py)."""
    n_rays = max(n // per_ray, 1)
    h = max(int((n_rays // 2) ** 0.5), 1)
    d = gen_pano_rays(torch.eye(4), h, 2 * h).d.reshape(-1, 3)
    d = d.repeat(-(-n_rays // d.shape[0]), 1)[:n_rays]
    t = 0.2 + 0.5 * torch.rand(n_rays, 1, device=dev) + step * torch.arange(per_ray, device=dev)[None, :]
    x = (d[:, None, :] * t[:, :, None]).reshape(-1, 3)
    x = torch.cat([x, x[:n - x.shape[0]]]) if x.shape[0] < n else x[:n]
    return ((x + 1.0) * 0.5).contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


out = {'dtype': args.dtype, 'levels': grid.n_levels, 'rounds': args.rounds, 'iters_per_round': args.iters, 'calls': {}}
with torch.no_grad():
    for n in (32768, 1 << 20):
        x01 = ray_ordered(n)
        sel = ((x01 > 0) & (x01 < 1)).all(-1).to(torch.uint8)
        ds, dg = torch.randn(n, device=dev), torch.randn(n, 3, device=dev)
        feat = ops.hashgrid_fwd(grid, x01, w16[n_net:])
        dout = ds[:, None].contiguous()
        ws_a, ws_b = ops.Workspace(), ops.Workspace()
        grad_a = torch.empty(n_net + grid.n_params, device=dev)
        grad_b = torch.empty_like(grad_a)
        hr = ops.headroom_state(dev)

        def second():
            ops.field_grad_x_bwd(grid, mlp, x01, sel, w16, None, ds, dg, grad=grad_a, ws=ws_a)

        def first():
            ops.field_bwd(grid, mlp, x01, w16[:n_net], feat, dout, sel, fixed=True, redo=True, hr_state=hr, grad=grad_b, ws=ws_b)

        for _ in range(3):
            second(); first()
        torch.cuda.synchronize()
        t2, t1 = [], []
        for _ in range(args.rounds):
            t2.append(timed(second))
            t1.append(timed(first))
        m2, m1 = statistics.median(t2), statistics.median(t1)
        out['calls'][str(n)] = {'field_grad_x_bwd_ms': m2, 'field_grad_x_bwd_ms_all': t2, 'field_bwd_ms': m1, 'field_bwd_ms_all': t1,
                                'ratio': m2 / m1, 'atomics_per_call': int(sel.sum()) * grid.n_levels * 16,
                                'atomics_per_second': int(sel.sum()) * grid.n_levels * 16 / (m2 * 1e-3)}


def wall_normals(d, half=(0.9, 0.7, 0.5)):
    h = torch.tensor(half, device=d.device)
    axis = (h / d.abs().clamp_min(1e-12)).argmin(-1)
    nrm = torch.zeros_like(d)
    nrm.scatter_(1, axis[:, None], -torch.sign(torch.gather(d, 1, axis[:, None])))
    return nrm


def step_ms(weight):
    """Median milliseconds of an EAGER geometry step (fused steps off for both runs: the two differ by the loss alone)."""
    torch.manual_seed(0); np.random.seed(0)
    scene = NeRFScene(dtype=args.dtype)
    scene.fused_steps = False
    rays = gen_pano_rays(torch.eye(4), 256, 512)
    dist, rgb = synthetic.room(rays.d)
    pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist, wall_normals(rays.d.reshape(-1, 3)))
    scene.train_conf.pixel_loss_batch_size = 4096
    scene.train_conf.normal_loss_weight = weight
    scene.set_train(); scene.prepare_occupancy(pool); scene.nerf.reset_geo()
    opt = scene.make_optimizer(scene.nerf.geo_mlp, 1e-3)
    times = []
    for i in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        scene.train_one_step_geo(opt, pool, progress=0.5)
        b.record()
        torch.cuda.synchronize()
        if i >= 5:
            times.append(a.elapsed_time(b))
    kept = int(scene.last_normal_batch['keep'].sum()) if weight > 0 else None
    return statistics.median(times), kept


without, _ = step_ms(0.0)
with_loss, kept = step_ms(0.05)
out['eager_geometry_step'] = {'batch_rays': 4096, 'steps_timed': args.steps - 5, 'without_normal_loss_ms': without, 'with_normal_loss_ms': with_loss,
                              'ratio': with_loss / without, 'kept_samples_in_the_last_step': kept}
print(json.dumps(out, indent=1))
if args.out:
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rec['bench'] = out
    json.dump(rec, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
