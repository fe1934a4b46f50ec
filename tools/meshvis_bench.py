"""Culling the faces no registered panorama saw (include/perf_hip_meshvis.h), stage by stage, beside the composed route it replaces, and
what it leaves of the trained analytic room of tools/meshcc_bench.py.

  python tools/meshvis_bench.py [--rounds 5] [--dense-resolutions 256] [--sparse-resolutions 1024] [--out profiles/meshvis.json]

Views: K = 1, the panorama the room is trained on (256 x 512 from the origin), and K = 25, that one and the analytic room's distance
panoramas (128 x 256) from 24 further positions inside it.  (a) Per resolution and K, host-clock seconds that end in a device synchronise
(medians of `rounds` after a warm-up) of cull_unseen and of the composed route on the same mesh -- 2 K ops.pano_reproject launches on the
vertices, torch for the face rule and torch.unique for the re-indexing --, and the device milliseconds of each entry point of one more
cull (HIP events around each call), stage 1's (vertex, view) pairs per second among them.  (b) The outcome at tol = 1/256, 2/256, 4/256
with and without the facing test: faces kept, components before and after, what clean_mesh(min_faces=64) leaves of the culled mesh, and the
50th / 90th percentile of the kept vertices' distance to the nearest analytic wall beside the raw mesh's."""
import argparse, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import mesh as M
from perf_amd import ops, synthetic
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--dense-resolutions', type=int, nargs='*', default=[256])
ap.add_argument('--sparse-resolutions', type=int, nargs='*', default=[1024])
ap.add_argument('--geo', type=int, default=150)
ap.add_argument('--app', type=int, default=100)
ap.add_argument('--min-faces', type=int, default=64)
ap.add_argument('--out', default=None)
args = ap.parse_args()
HALF = (0.9, 0.7, 0.5)
TOLS = (1 / 256, 2 / 256, 4 / 256)


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def median_s(fn, rounds):
    times = []
    for _ in range(rounds + 1):                      # (the first round is the warm-up)
        t0 = sync_clock(); fn(); times.append(sync_clock() - t0)
    return statistics.median(times[1:])


def composed(mesh, views, tol, free_tol, facing):
    """The same cull without the new unit: 2 K launches of the reprojection kernel, a dozen torch passes, torch.unique."""
    v = mesh.vertices
    n = v.shape[0]
    visible = torch.zeros(n, dtype=torch.int64, device=v.device)
    free = torch.zeros_like(visible)
    for k, view in enumerate(views):
        for word, eps in ((visible, tol), (free, -free_tol)):
            mask = torch.zeros(n, device=v.device)
            ops.pano_reproject(v, view['pose'], view['distance_map'], mask, 0, eps)
            word |= (mask > 0.5).long() << k
    f = mesh.faces.long()
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    bits = visible[a] & visible[b] & visible[c]
    if facing:
        va = v[a].double()
        normal = torch.cross(v[b].double() - va, v[c].double() - va, dim=1)
        for k, view in enumerate(views):
            s = (normal * (view['pose'][:3, 3].double().to(v.device) - va)).sum(dim=1)
            bits &= ~((~(s > 0)).long() << k)
    kept = f[bits != 0]
    index, inverse = torch.unique(kept, return_inverse=True)
    return v[index], inverse.int(), visible, free


def wall_distance(vertices):
    h = torch.tensor(HALF, device=vertices.device) / synthetic.ROOM_SCALE
    return (vertices.abs() - h).abs().min(dim=1).values


def percentiles(vertices):
    if not len(vertices):
        return None
    d = wall_distance(vertices)
    return [float(torch.quantile(d, q)) for q in (0.5, 0.9)]


def measure(res, sparse):
    mesh = M.extract_mesh_sparse(scene, res) if sparse else M.extract_mesh(scene, res)
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    entry = {'path': 'extract_mesh_sparse' if sparse else 'extract_mesh', 'vertices': V, 'faces': F, 'components': int(M.connected_components(mesh).faces.numel()),
             'raw_wall_distance_p50_p90': percentiles(mesh.vertices), 'views': {}}
    for name, views in (('1', views_1), ('25', views_25)):
        k = len(views)
        e = {'cull_unseen_s': median_s(lambda: M.cull_unseen(mesh, views), args.rounds),
             'composed_s': median_s(lambda: composed(mesh, views, 1 / 256, 1 / 256, True), args.rounds)}
        ops.start_kernel_timing()                    # device milliseconds per entry point of one more cull
        culled = M.cull_unseen(mesh, views)
        e['device_ms'] = {key: v[1] for key, v in ops.stop_kernel_timing().items()}
        e['stage1_pairs_per_s'] = V * k / (e['device_ms']['perf_meshvis_vertex_bits'] * 1e-3)
        e['composed_over_cull'] = e['composed_s'] / e['cull_unseen_s']
        cv, cf, visible, free = composed(mesh, views, 1 / 256, 1 / 256, True)
        vis = M.vertex_visibility(mesh.vertices, views)
        e['composed_agrees'] = bool(torch.equal(cv, culled.vertices) and torch.equal(cf, culled.faces) and torch.equal(visible, vis.visible) and torch.equal(free, vis.free))
        e['outcome'] = []
        for tol in TOLS:
            for facing in (True, False):
                out = M.cull_unseen(mesh, views, tol=tol, facing=facing)
                comps = M.connected_components(out)
                cleaned = M.clean_mesh(out, min_faces=args.min_faces)
                e['outcome'].append({'tol': tol, 'facing': facing, 'faces_kept': int(out.faces.shape[0]), 'vertices_kept': int(out.vertices.shape[0]),
                                     'components_after': int(comps.faces.numel()), 'largest_component_faces': int(comps.faces.max()) if comps.faces.numel() else 0,
                                     'faces_after_clean_min_faces': int(cleaned.faces.shape[0]), 'wall_distance_p50_p90': percentiles(out.vertices),
                                     'cleaned_wall_distance_p50_p90': percentiles(cleaned.vertices)})
        entry['views'][name] = e
    return entry


torch.manual_seed(0); np.random.seed(0)
scene = NeRFScene(dtype='fp16')
rays = gen_pano_rays(torch.eye(4), 256, 512)
dist, rgb = synthetic.room(rays.d)
pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
scene.train_conf.pixel_loss_batch_size = 4096
scene.train_one_episode(pool, args.geo, args.app)
scene.set_eval()
views_1 = [{'pose': torch.eye(4), 'distance_map': dist.reshape(256, 512).float().cuda().contiguous()}]
views_25 = list(views_1)
rng = np.random.default_rng(0)
for _ in range(24):                                  # 24 further positions inside the room; room_with_box without its box is the room from anywhere
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor(rng.uniform(-0.6, 0.6, 3) * np.array(HALF) / synthetic.ROOM_SCALE, dtype=torch.float32)
    r = gen_pano_rays(pose, 128, 256)
    d, _ = synthetic.room_with_box(r.o, r.d, box_h=(0.0, 0.0, 0.0))
    views_25.append({'pose': pose, 'distance_map': d.reshape(128, 256).float().cuda().contiguous()})
out = {'rounds': args.rounds, 'min_faces': args.min_faces, 'wall_distance_bound': 0.0688,
       'training': {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': math.log(2.0) / scene.renderer.render_step_size}, 'room': {}}
for res, sparse in [(r, False) for r in args.dense_resolutions] + [(r, True) for r in args.sparse_resolutions]:
    out['room'][str(res)] = measure(res, sparse)
    print(json.dumps({str(res): out['room'][str(res)]}), flush=True)
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
