"""What the fused sphere distance field buys (include/perf_hip_sphere.h, perf_amd/sphere_field.py), measured on the GPU:

  (a) the two kernels alone at 15,360 and 32,768 directions;
  (b) one full optimiser iteration, fused and composed from the same seeds, alternated in one process: the refiner's loop (32,768
      directions, the loss and Adam of pano_geo_refiner.py:99-142 restated here) and the joint predictor's field part (15,360
      directions, the same loss on SphereDistanceField.joint());
  (c) time and peak allocator memory of the full-panorama (distance, grad) query at 512 x 1024 and 1024 x 2048, fused (under no_grad)
      and composed (with its graph, as the reference runs it); an out-of-memory of the composed path is recorded as such;
  (d) with --tests-report, the parity errors the GPU tests reported (PERF_SPHERE_FIELD_REPORT of tests/test_gpu_sphere_field.py).

  python tools/sphere_field_bench.py [--rounds 5] [--iters 10] [--tests-report report.json] [--out profiles/sphere_field.json]

HIP events around a window of --iters calls after a warm-up, medians over --rounds windows, the two variants alternated.  Prints one JSON
object and, with --out, writes it there.  Figures are reported, nothing is asserted; without a GPU the tool fails."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from perf_amd import ops
from perf_amd.sphere_field import SphereDistanceField

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--tests-report', default=None)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('tools/sphere_field_bench.py measures on the GPU: no HIP device')
dev = 'cuda'


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
    """{name: median ms} of the callables, warmed up, then timed in alternating windows."""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            ts[k].append(timed(f))
    return {k: {'median_ms': statistics.median(v), 'all_ms': v} for k, v in ts.items()}


def unit_dirs(n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return F.normalize(torch.randn(n, 3, generator=g, device=dev), dim=-1)


def make(variant, fused, seed=0, **kw):
    """A field of the given variant, moved off its initial state (the first layer's feature columns start at zero: the table would get no
    gradient and the kernels' sparse-zero arithmetic would flatter them)."""
    torch.manual_seed(seed)
    f = getattr(SphereDistanceField, variant)(fused=fused, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        first = f.geo_mlp.layers[0]
        w = first.weight_v if f.geo_mlp.weight_norm else first.weight
        w[:, 3:] = (torch.randn(64, w.shape[1] - 3, generator=g) * 0.05).to(w.device)
        f.hash_grid.params.uniform_(-0.1, 0.1, generator=torch.Generator(device=dev).manual_seed(seed + 2))
    return f


def box():
    p = torch.cuda.get_device_properties(0)
    info = {'device': p.name, 'arch': p.gcnArchName, 'compute_units': p.multi_processor_count, 'total_memory_gib': p.total_memory / 2 ** 30,
            'torch': torch.__version__, 'hip': torch.version.hip}
    try:            # (a read-only query of the engine clock at the moment of the call, MHz; under load the driver raises it)
        info['engine_clock_mhz_idle'] = torch.cuda.clock_rate()
    except Exception as e:      # noqa: BLE001
        info['engine_clock_mhz_idle'] = f'not read: {type(e).__name__}'
    return info


def clock_now():
    try:
        return torch.cuda.clock_rate()
    except Exception:           # noqa: BLE001
        return None


out = {'box': box(), 'rounds': args.rounds, 'iters_per_round': args.iters}

# ---- (a) the two kernels alone ---------------------------------------------------------------------------------------------------------
out['kernels'] = {}
field = make('refiner', True)
grid = field.hash_grid.grid
table = field.hash_grid.params.detach()
net = torch.cat([p.detach().reshape(-1) for p in field.geo_mlp.effective_parameters()]).float().contiguous()
for n in (15360, 32768):
    u = unit_dirs(n, 3)
    a, c = torch.randn(n, device=dev), torch.randn(n, 3, device=dev)
    grad = torch.empty(net.numel() + table.numel(), device=dev)
    ws = ops.Workspace()
    res = alternate({'fwd_raw_only': lambda: ops.sphere_field_fwd(grid, table, net, u, want_grad=False),
                     'fwd_raw_and_grad': lambda: ops.sphere_field_fwd(grid, table, net, u, want_grad=True),
                     'bwd': lambda: ops.sphere_field_bwd(grid, table, net, u, a, c, grad=grad, ws=ws)})
    # the operations the algorithm needs (multiply-adds of the matrix products, x 2), per sample
    mac_fwd = 64 * 35 + 64 * 64 + 64
    mac_grad = 64 * 64 + 64 * 35
    mac_bwd = 2 * (64 * 35 + 64 * 64) + 2 * (64 * 64 + 64 * 32) + 2 * (64 * 64 + 64 * 35)
    res['flop_per_sample'] = {'fwd_raw_only': 2 * mac_fwd, 'fwd_raw_and_grad': 2 * (mac_fwd + mac_grad), 'bwd': 2 * mac_bwd}
    for k in ('fwd_raw_only', 'fwd_raw_and_grad', 'bwd'):
        res[k]['tflops'] = res['flop_per_sample'][k] * n / (res[k]['median_ms'] * 1e-3) / 1e12
    res['engine_clock_mhz_after'] = clock_now()
    out['kernels'][str(n)] = res
del field, table, net


# ---- (b) one optimiser iteration -------------------------------------------------------------------------------------------------------
def refiner_loss(distance, grads, dirs, ref_distance, ref_normal, ortho_a, ortho_b):
    val_a = (grads * ortho_a).sum(-1, True) * dirs + ortho_a
    val_a = val_a / torch.linalg.norm(val_a, 2, -1, True)
    val_b = (grads * ortho_b).sum(-1, True) * dirs + ortho_b
    val_b = val_b / torch.linalg.norm(val_b, 2, -1, True)
    errors = torch.cat([(val_a * ref_normal).sum(-1, True), (val_b * ref_normal).sum(-1, True)], -1)
    return F.smooth_l1_loss(ref_distance, distance, beta=1e-2) + 5e-2 * F.smooth_l1_loss(errors, torch.zeros_like(errors), beta=5e-1)


def iteration(variant, fused, batch):
    field = make(variant, fused)
    field.train()
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    gen = torch.Generator(device=dev).manual_seed(7)
    ref_distance = 0.5 + 0.2 * torch.rand(batch, device=dev, generator=gen)
    ref_normal = -unit_dirs(batch, 8)

    def step():
        dirs = F.normalize(torch.randn(batch, 3, device=dev, generator=gen), dim=-1)
        oa = torch.randn(batch, 3, device=dev, generator=gen)
        ob = F.normalize(torch.linalg.cross(dirs, oa), dim=-1)
        oa = F.normalize(torch.linalg.cross(ob, dirs), dim=-1)
        distance, grads = field(dirs, requires_grad=True)
        loss = refiner_loss(distance, grads, dirs, ref_distance, ref_normal, oa, ob)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


out['iteration'] = {}
for name, variant, batch in (('refiner_32768', 'refiner', 32768), ('joint_15360', 'joint', 15360)):
    res = alternate({'fused': iteration(variant, True, batch), 'composed': iteration(variant, False, batch)})
    res['composed_over_fused'] = res['composed']['median_ms'] / res['fused']['median_ms']
    out['iteration'][name] = res
    torch.cuda.empty_cache()

# ---- (c) the full-panorama query -------------------------------------------------------------------------------------------------------
out['panorama_query'] = {}
for (h, w) in ((512, 1024), (1024, 2048)):
    dirs = unit_dirs(h * w, 9)
    rec = {}
    for name in ('fused', 'composed'):
        field = make('refiner', name == 'fused')
        field.eval()

        def query():
            if name == 'fused':
                with torch.no_grad():
                    d, g = field(dirs, requires_grad=True)
            else:
                d, g = field(dirs, requires_grad=True)
            return d.detach(), g.detach()
        try:
            query()
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ms = statistics.median([timed(query, 1) for _ in range(args.rounds)])
            rec[name] = {'median_ms': ms, 'peak_bytes': torch.cuda.max_memory_allocated() - base}
        except torch.cuda.OutOfMemoryError as e:
            rec[name] = {'out_of_memory': str(e).splitlines()[0]}
        del field
        torch.cuda.empty_cache()
    out['panorama_query'][f'{h}x{w}'] = rec

# ---- (d) the parity errors of the GPU tests --------------------------------------------------------------------------------------------
if args.tests_report and os.path.exists(args.tests_report):
    out['tests'] = json.load(open(args.tests_report))

print(json.dumps({k: v for k, v in out.items() if k != 'tests'}, indent=1))
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
