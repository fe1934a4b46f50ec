"""The closest point of a mesh (include/staged/perf_hip_meshnear.h) and what is built on it -- mesh_deviation, simplify_to_tolerance -- on
the trained analytic room of tools/meshsimp_bench.py.

  python tools/meshnear_bench.py [--rounds 5] [--dense-resolutions 256] [--sparse-resolutions 1024] [--out profiles/meshnear.json]

The meshes are the room's after cull_unseen (the training panorama, tol 1/256) and clean_mesh(min_faces=64), the cases of
profiles/meshsimp.json.  Per resolution, with the simplification at a cell of 4 lattice spacings under 'quadric':
(a) closest_point of the simplified mesh's vertices and of its order-2 samples against the ORIGINAL mesh on the default grid: device
    milliseconds (HIP events, medians of `rounds` after a warm-up) and points per second, beside the SAME kernel on a grid of one cell --
    brute force on the device -- for the first --brute-points of them; the two must agree to the bit.
(b) the same against a chunked torch brute force that restates the rule in float64, for the first --torch-points; equal to the bit.
(c) mesh_deviation end to end (host clock ending in a synchronise, both grids and all host reads included) and simplify_to_tolerance per
    ladder step at a tolerance of one lattice spacing.
(d) the symmetric sampled deviation of 'mean' against 'quadric' placement at cells of 2 and 4 lattice spacings, measured against the
    original mesh, not against the analytic walls."""
import argparse, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import mesh as M
from perf_amd import synthetic
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--dense-resolutions', type=int, nargs='*', default=[256])
ap.add_argument('--sparse-resolutions', type=int, nargs='*', default=[1024])
ap.add_argument('--geo', type=int, default=150)
ap.add_argument('--app', type=int, default=100)
ap.add_argument('--min-faces', type=int, default=64)
ap.add_argument('--brute-points', type=int, default=2048, help='points of the one-cell grid: every one of them tests every face')
ap.add_argument('--torch-points', type=int, default=64)
ap.add_argument('--out', default=None)
args = ap.parse_args()


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def clock_s(fn):
    t0 = sync_clock()
    out = fn()
    return sync_clock() - t0, out


def event_ms(fn, rounds):
    times = []
    for _ in range(rounds + 1):                      # (the first round is the warm-up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times[1:])


def same_bits(x, y):
    return all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32), b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))
               for a, b in zip((x.dist2, x.face, x.u, x.v), (y.dist2, y.face, y.u, y.v)))


def torch_rule(p, a, b, c):
    """The header's rule in torch float64, operation for operation (eager torch does not contract); p [n, 1, 3], a, b, c [1, F, 3] ->
    (dist2, u, v) [n, F]."""
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va, e, g = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4, d4 - d3, d5 - d6
    ra, rb, rc = dot(ap, ap), dot(bp, bp), dot(cp, cp)
    region = torch.where(rc < torch.minimum(ra, rb), 2, torch.where(rb < ra, 1, 0))          # 8, then backwards: the first test that holds wins
    tests = [((ap == 0).all(-1), 0), ((bp == 0).all(-1), 1), ((cp == 0).all(-1), 2), ((d1 <= 0) & (d2 <= 0), 0), ((d3 >= 0) & (d4 <= d3), 1), ((d6 >= 0) & (d5 <= d6), 2),
             ((vc <= 0) & (d1 >= 0) & (d3 <= 0) & ((d1 - d3) > 0), 4), ((vb <= 0) & (d2 >= 0) & (d6 <= 0) & ((d2 - d6) > 0), 5),
             ((va <= 0) & (e >= 0) & (g >= 0) & ((e + g) > 0), 6), ((va > 0) & (vb > 0) & (vc > 0), 7)]
    for test, code in reversed(tests):
        region = torch.where(test, code, region)
    zero, one, v6, den = torch.zeros_like(d1), torch.ones_like(d1), e / (e + g), (va + vb) + vc
    u = torch.where(region == 1, one, torch.where(region == 4, d1 / (d1 - d3), torch.where(region == 6, 1.0 - v6, torch.where(region == 7, vb / den, zero))))
    v = torch.where(region == 2, one, torch.where(region == 5, d2 / (d2 - d6), torch.where(region == 6, v6, torch.where(region == 7, vc / den, zero))))
    q = (a + u[..., None] * ab) + v[..., None] * ac
    r = torch.where((region == 0)[..., None], ap, torch.where((region == 1)[..., None], bp, torch.where((region == 2)[..., None], cp, p - q)))
    return dot(r, r), u, v


def torch_closest(mesh, points, budget=1 << 22):
    """Brute force over all faces in chunks of points -> (dist2 float64, face int32, u, v fp32).  The room's faces are all valid."""
    vt, f = mesh.vertices.double(), mesh.faces.long()
    a, b, c = vt[f[:, 0]][None], vt[f[:, 1]][None], vt[f[:, 2]][None]
    step = max(1, budget // max(int(f.shape[0]), 1))
    outs = []
    for first in range(0, int(points.shape[0]), step):
        dist2, u, v = torch_rule(points[first:first + step].double()[:, None, :], a, b, c)
        best = dist2.argmin(dim=1, keepdim=True)          # (the first of equal minima)
        outs.append((dist2.gather(1, best)[:, 0], best[:, 0].int(), u.gather(1, best)[:, 0].float(), v.gather(1, best)[:, 0].float()))
    return M.NearestHits(torch.cat([o[0] for o in outs]), None, torch.cat([o[1] for o in outs]), torch.cat([o[2] for o in outs]), torch.cat([o[3] for o in outs]))


def deviation_dict(d):
    keep = ('max', 'mean', 'rms', 'p90', 'argmax_point', 'argmax_face_of_b', 'n_samples', 'n_beyond')
    out = {k: getattr(d, k) for k in keep}
    for side in ('a_to_b', 'b_to_a'):
        if getattr(d, side) is not None:
            out[side] = {k: getattr(getattr(d, side), k) for k in keep}
    return out


def prepared(res, sparse):
    mesh = M.extract_mesh_sparse(scene, res) if sparse else M.extract_mesh(scene, res)
    mesh = M.clean_mesh(M.cull_unseen(mesh, views), min_faces=args.min_faces)
    return M.Mesh(mesh.vertices.contiguous(), mesh.faces.contiguous(), mesh.colors, mesh.normals)


def measure(res, mesh):
    spacing = EXTENT / res
    entry = {'vertices': int(mesh.vertices.shape[0]), 'faces': int(mesh.faces.shape[0]), 'lattice_spacing': spacing}
    build_s, grid = clock_s(lambda: M.build_ray_grid(mesh))
    one_s, one = clock_s(lambda: M.build_ray_grid(mesh, 4 * EXTENT))
    assert one.dims == (1, 1, 1)
    entry['grid'] = {'cell': grid.cell, 'dims': grid.dims, 'references': int(grid.refs.numel()), 'build_s': build_s, 'one_cell_build_s': one_s}
    small = M.simplify_mesh(mesh, 4 * spacing, BOX, placement='quadric')[0]
    entry['simplified'] = {'cell': 4 * spacing, 'vertices': int(small.vertices.shape[0]), 'faces': int(small.faces.shape[0])}
    # (a) and (b)
    entry['closest_point'] = {}
    for name, points in (('vertices', small.vertices.contiguous()), ('order_2_samples', M.surface_samples(small, 2)[0])):
        n = int(points.shape[0])
        ms = event_ms(lambda: M.closest_point(mesh, grid, points), args.rounds)
        e = {'points': n, 'ms': ms, 'points_per_s': n / (ms * 1e-3)}
        hits = M.closest_point(mesh, grid, points)
        e['largest_distance'], e['mean_distance'] = float(hits.distance.max()), float(hits.distance.double().mean())
        few = points[:args.brute_points].contiguous()
        e['one_cell'] = {'points': int(few.shape[0]), 'ms': event_ms(lambda: M.closest_point(mesh, one, few), 1),
                         'same_points_on_the_grid_ms': event_ms(lambda: M.closest_point(mesh, grid, few), args.rounds)}
        e['one_cell']['points_per_s'] = int(few.shape[0]) / (e['one_cell']['ms'] * 1e-3)
        e['one_cell']['grid_over_one_cell'] = e['one_cell']['ms'] / e['one_cell']['same_points_on_the_grid_ms']
        e['one_cell']['equal_to_the_bit'] = same_bits(M.closest_point(mesh, one, few), M.closest_point(mesh, grid, few))
        fewer = points[:args.torch_points].contiguous()
        torch_s, theirs = clock_s(lambda: torch_closest(mesh, fewer))
        e['torch_brute_force'] = {'points': int(fewer.shape[0]), 's': torch_s, 'equal_to_the_bit': same_bits(theirs, M.closest_point(mesh, grid, fewer))}
        entry['closest_point'][name] = e
    # (c)
    seconds, deviation = clock_s(lambda: M.mesh_deviation(small, mesh))
    entry['mesh_deviation'] = {'s': seconds, **deviation_dict(deviation)}
    ladder = M.tolerance_ladder(mesh)
    entry['simplify_to_tolerance'] = {'tolerance': spacing, 'median_edge_length': M.median_edge_length(mesh), 'steps': []}
    import warnings
    for cell in ladder:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            seconds, (candidate, _, d) = clock_s(lambda: M.simplify_to_tolerance(mesh, spacing, cells=[cell], box=BOX))
        entry['simplify_to_tolerance']['steps'].append({'cell': cell, 's': seconds, 'faces': int(candidate.faces.shape[0]), 'max': d.max, 'mean': d.mean, 'passes': d.max <= spacing})
    seconds, (chosen, cell, d) = clock_s(lambda: M.simplify_to_tolerance(mesh, spacing, box=BOX))
    entry['simplify_to_tolerance'].update({'s': seconds, 'cell': cell, 'faces': int(chosen.faces.shape[0]), 'max': d.max})
    # (d)
    entry['placement'] = {}
    for factor in (2, 4):
        for placement in ('mean', 'quadric'):
            candidate = M.simplify_mesh(mesh, factor * spacing, BOX, placement=placement)[0]
            entry['placement'][f'{placement}_{factor}'] = {'cell': factor * spacing, 'vertices': int(candidate.vertices.shape[0]), **deviation_dict(M.mesh_deviation(candidate, mesh))}
    return entry


torch.manual_seed(0); np.random.seed(0)
scene = NeRFScene(dtype='fp16')
rays = gen_pano_rays(torch.eye(4), 256, 512)
dist, rgb = synthetic.room(rays.d)
pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
scene.train_conf.pixel_loss_batch_size = 4096
scene.train_one_episode(pool, args.geo, args.app)
scene.set_eval()
views = [{'pose': torch.eye(4), 'distance_map': dist.reshape(256, 512).float().cuda().contiguous()}]
aabb = [float(v) for v in scene.nerf._aabb_host]
BOX = (aabb[:3], aabb[3:])
EXTENT = aabb[3] - aabb[0]
out = {'rounds': args.rounds, 'min_faces': args.min_faces, 'box': BOX,
       'training': {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': math.log(2.0) / scene.renderer.render_step_size}, 'room': {}}
for res, sparse in [(r, False) for r in args.dense_resolutions] + [(r, True) for r in args.sparse_resolutions]:
    out['room'][str(res)] = measure(res, prepared(res, sparse))
    print(json.dumps({str(res): out['room'][str(res)]}), flush=True)
    if args.out:          # (after every resolution: what is measured is kept)
        json.dump(out, open(args.out, 'w'), indent=1)
        open(args.out, 'a').write('\n')
