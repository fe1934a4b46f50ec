"""What the fused alignment step buys (include/perf_hip_joint.h, perf_amd/joint_align.py), measured on the GPU at the reference's size:
60 views x 256 samples, R = 384, Rn = 128, a 512 x 1024 panorama, the field at L = 16, T = 2^19.

  (a) one full iteration of each phase ('global', 'hybrid') -- draws, gradient reset, the step, the three plain torch Adam steps as
      JointAligner runs them -- with the composed head around the fused field (what the package could do before these kernels) and
      with the fused head, the two alternated in one process;
  (b) each new entry point alone, and the TV kernel's achieved bytes per second (one read of the map, one write of its gradient) next
      to the rate the package's Adam kernel reaches on this chip;
  (c) with --tests-report, the figures the GPU tests reported (PERF_JOINT_ALIGN_REPORT of tests/test_gpu_joint_align.py).

  python tools/joint_align_bench.py [--rounds 5] [--iters 20] [--tests-report report.json] [--out profiles/joint_align.json]

HIP events around a window of --iters calls after a warm-up, medians over --rounds windows, the variants alternated.  `spread_ms` is
max - min over the windows.  Prints one JSON object and, with --out, writes it there.  Figures are reported, nothing is asserted;
without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from perf_amd import ops
from perf_amd.joint_align import StepScratch, align_step, align_step_composed
from perf_amd.sphere_field import SphereDistanceField

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--views', type=int, default=60)
ap.add_argument('--batch', type=int, default=256)
ap.add_argument('--res', type=int, default=384)
ap.add_argument('--normal-res', type=int, default=128)
ap.add_argument('--tests-report', default=None)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('tools/joint_align_bench.py measures on the GPU: no HIP device')
dev = 'cuda'
P, B, R, Rn, H, W = args.views, args.batch, args.res, args.normal_res, 512, 1024
ADAM_BYTES_PER_S = 6.0e12          # what perf_adam_step reaches on this chip


def timed(fn, iters=None):
    iters = iters or args.iters
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, warm=3):
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            ts[k].append(timed(f))
    return {k: {'median_ms': statistics.median(v), 'spread_ms': max(v) - min(v), 'all_ms': v} for k, v in ts.items()}


def inputs(seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    base = F.normalize(r(P, 3, 1, 1), dim=1)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, R, device=dev), torch.linspace(-1, 1, R, device=dev), indexing='ij')
    dirs = F.normalize(base + 0.4 * torch.stack([xx, yy, xx * yy], 0)[None] * r(P, 3, 1, 1), dim=1)          # smooth direction maps, as a view's are
    sup = torch.cat([dirs, 0.8 + 0.4 * torch.rand(P, 1, R, R, device=dev, generator=g), F.normalize(-dirs + 0.2 * r(P, 3, R, R), dim=1)], 1).contiguous()
    ref = torch.stack([1.0 + 0.2 * torch.rand(H, W, device=dev, generator=g), (torch.rand(H, W, device=dev, generator=g) < 0.3).float()]).contiguous()
    return sup, ref


def make_field(seed=0):
    torch.manual_seed(seed)
    f = SphereDistanceField.joint(fused=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        w = f.geo_mlp.layers[0].weight
        w[:, 3:] = (torch.randn(64, w.shape[1] - 3, generator=g) * 0.05).to(w.device)
        f.hash_grid.params.uniform_(-0.1, 0.1, generator=torch.Generator(device=dev).manual_seed(seed + 2))
    f.train()
    return f


def iteration(fused, hybrid, sup, ref):
    """One iteration as JointAligner.align runs it, on its own field, parameters and optimisers."""
    field = make_field()
    scale = torch.zeros([P], device=dev, requires_grad=True)
    bias_global = torch.zeros([P], device=dev, requires_grad=True)
    bias_d = (0.01 * torch.randn(P, 1, R, R, device=dev)).requires_grad_(True)
    bias_n = (0.01 * torch.randn(P, 3, Rn, Rn, device=dev)).requires_grad_(True)
    opt_sp = torch.optim.Adam(field.parameters(), lr=1e-2)
    opt_global = torch.optim.Adam([scale, bias_global], lr=1e-1)
    opt_local = torch.optim.Adam([bias_d, bias_n], lr=1e-1)
    scratch = StepScratch()
    progress = 0.75 if hybrid else 0.25

    def step():
        np.random.randint(low=0, high=P)
        coords = torch.rand(P, B, 1, 2, device=dev) * 2. - 1
        ortho = torch.randn([P, B, 3], device=dev)
        opt_global.zero_grad()
        opt_sp.zero_grad()
        if fused:
            align_step(field, sup, ref, scale, bias_d, bias_n, coords, ortho, progress, hybrid, reg_loss_weight=0.0, scratch=scratch)
        else:
            if hybrid:
                opt_local.zero_grad()
            align_step_composed(field, sup, ref, scale, bias_d, bias_n, coords, ortho, progress, hybrid, reg_loss_weight=0.0)
        opt_global.step()
        opt_sp.step()
        if hybrid:
            opt_local.step()
    return step


p = torch.cuda.get_device_properties(0)
out = {'box': {'device': p.name, 'arch': p.gcnArchName, 'compute_units': p.multi_processor_count, 'torch': torch.__version__, 'hip': torch.version.hip},
       'size': {'views': P, 'batch': B, 'res': R, 'normal_res': Rn, 'panorama': [H, W], 'levels': 16, 'log2_hashmap_size': 19},
       'rounds': args.rounds, 'iters_per_round': args.iters}
sup, ref = inputs()

# ---- (a) one iteration of each phase -----------------------------------------------------------------------------------------------------
out['iteration'] = {}
for phase in ('global', 'hybrid'):
    res = alternate({'composed_head': iteration(False, phase == 'hybrid', sup, ref), 'fused_head': iteration(True, phase == 'hybrid', sup, ref)})
    c, f = res['composed_head'], res['fused_head']
    res['composed_over_fused'] = c['median_ms'] / f['median_ms']
    res['fused_below_composed_by_more_than_the_spread'] = c['median_ms'] - f['median_ms'] > max(c['spread_ms'], f['spread_ms'])
    out['iteration'][phase] = res
    torch.cuda.empty_cache()

# ---- (b) the entry points alone ------------------------------------------------------------------------------------------------------------
bias_d, bias_n = 0.01 * torch.randn(P, 1, R, R, device=dev), 0.01 * torch.randn(P, 3, Rn, Rn, device=dev)
coords = (torch.rand(P, B, 2, device=dev) * 2 - 1).contiguous()
u, rec = ops.joint_sample(sup, bias_d, bias_n, ref, coords)
N = P * B
d, g, o = 1.0 + 0.1 * torch.randn(N, device=dev), torch.randn(N, 3, device=dev), torch.randn(N, 3, device=dev)
scale = torch.zeros(P, device=dev)
gd, gn, tv = torch.empty_like(bias_d), torch.empty_like(bias_n), torch.zeros(2, device=dev)
ws_l, ws_t = ops.Workspace(), ops.Workspace()
res = alternate({
    'joint_sample': lambda: ops.joint_sample(sup, bias_d, bias_n, ref, coords),
    'joint_loss_global': lambda: ops.joint_loss(rec, coords, scale, u, d, g, o, R, Rn, 5.0, 0.0, 1e-2, ws=ws_l),
    'joint_loss_hybrid': lambda: ops.joint_loss(rec, coords, scale, u, d, g, o, R, Rn, 15.0, 0.0, 1e-2, 1e-2, tv=tv, gbias_d=gd, gbias_n=gn, ws=ws_l),
    'joint_tv_distance_map': lambda: ops.joint_tv(bias_d, 1.0, grad=gd, value=tv[0:1], ws=ws_t),
    'joint_tv_normal_map': lambda: ops.joint_tv(bias_n, 1e-2, grad=gn, value=tv[1:2], ws=ws_t),
})
for name, m in (('joint_tv_distance_map', bias_d), ('joint_tv_normal_map', bias_n)):
    nbytes = 2 * 4 * m.numel()                      # one read of the map, one write of its gradient
    res[name]['bytes'] = nbytes
    res[name]['bytes_per_s'] = nbytes / (res[name]['median_ms'] * 1e-3)
    res[name]['share_of_adam_rate'] = res[name]['bytes_per_s'] / ADAM_BYTES_PER_S
out['entry_points'] = res

# ---- (c) the figures of the GPU tests ------------------------------------------------------------------------------------------------------
if args.tests_report and os.path.exists(args.tests_report):
    rep = json.load(open(args.tests_report))
    blocks = {k: v for k, v in rep.items() if isinstance(v, dict) and 'kernels_rms' in v}
    ratios = [v['kernels_rms'] / v['composed_rms'] for v in blocks.values() if v['composed_rms'] > 0]
    out['tests'] = {'blocks': len(blocks), 'misses': sorted(k for k, v in blocks.items() if not v['holds']),
                    'largest_kernels_rms_over_rms_T': max((v['kernels_rms'] / v['rms_T'] for v in blocks.values() if v['rms_T']), default=None),
                    'kernels_over_composed': {'min': min(ratios, default=None), 'median': statistics.median(ratios) if ratios else None, 'max': max(ratios, default=None)},
                    'fit': rep.get('fit')}

print(json.dumps(out, indent=1))
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
