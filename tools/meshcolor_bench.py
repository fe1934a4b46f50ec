"""Colouring a mesh from the registered panoramas (include/perf_hip_meshcolor.h) beside the composed route it replaces, and what it leaves
of the trained analytic room of tools/meshvis_bench.py.

  python tools/meshcolor_bench.py [--rounds 5] [--dense-resolutions 256] [--sparse-resolutions 1024] [--out profiles/meshcolor.json]

Views: K = 1, the panorama the room is trained on (256 x 512 from the origin), and K = 25, that one and the analytic room's panoramas
(128 x 256) from 24 further positions inside it, each with its colours.  The mesh is the extracted one after cull_unseen with the same
views and clean_mesh(min_faces=64).  (a) Per resolution and K, host-clock seconds that end in a device synchronise (medians of `rounds`
after a warm-up) of color_from_panoramas (normals from faces, box given: one host read) and of the composed route on the same mesh --
per view the existing reprojection kernel for the depth test, torch for the direction, a grid_sample of the colour map and the weights,
then the sum over the views; index_add_ of the faces' cross products for the normals -- TWICE, like for like: both with their per-view
state built once outside the timed region (`*_prebuilt_s`: the kernel's descriptors; the composed route's device copies of the poses),
and both building it in every call (`color_from_panoramas_s`, `composed_s`: what the public call given the views themselves does).  Also
face_normals alone beside the index_add_ normals, and the device milliseconds of each entry point of one more colouring (HIP events
around each call) with the blend's (vertex, view) pairs per second.  (b) The outcome: the share of vertices coloured, the mean absolute
difference between the panoramas' colours and the field's query_rgb at the same vertices, the largest difference between the composed
route's colours and the kernel's (with the kernel's normals and with its own), and the vertex at which face_normals is furthest from
the index_add_ normals, with its fixed-point sum."""
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
TOL = 1 / 256


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def median_s(fn, rounds):
    times = []
    for _ in range(rounds + 1):                      # (the first round is the warm-up)
        t0 = sync_clock(); fn(); times.append(sync_clock() - t0)
    return statistics.median(times[1:])


def composed_normals(mesh):
    """Area-weighted vertex normals with torch: the faces' cross products in double, index_add_ (floating-point atomics), normalise."""
    v, f = mesh.vertices.double(), mesh.faces.long()
    a = v[f[:, 0]]
    n = torch.cross(v[f[:, 1]] - a, v[f[:, 2]] - a, dim=1)
    acc = torch.zeros_like(v)
    for corner in range(3):
        acc.index_add_(0, f[:, corner], n)
    return torch.nn.functional.normalize(acc, dim=1).float()


def prepare(views, device):
    """The composed route's per-view state: the CPU pose the reprojection kernel takes (it reads it on the host: a device pose would cost
    a synchronising read-back per view), device copies of the rotation and the centre, the colour map as grid_sample's [1, 3, H, W]."""
    return [{'pose': v['pose'], 'rot': v['pose'][:3, :3].to(device), 't': v['pose'][:3, 3].to(device), 'distance_map': v['distance_map'],
             'image': v['color_map'].permute(2, 0, 1)[None]} for v in views]


def composed(mesh, views, tol, power, prepared=None, normals=None):
    """The same colouring without the new unit: per view one launch of the reprojection kernel for the depth test, torch for the
    direction and the weights, grid_sample for the colour; then the sum over the views.  prepared None: the per-view state is built in
    the call, as color_from_panoramas builds its descriptors when it is given the views themselves.  normals None: its own."""
    v = mesh.vertices
    n = v.shape[0]
    prepared = prepare(views, v.device) if prepared is None else prepared
    normals = (composed_normals(mesh) if normals is None else normals).double()
    num = torch.zeros(n, 3, dtype=torch.float64, device=v.device)
    den = torch.zeros(n, dtype=torch.float64, device=v.device)
    for view in prepared:
        mask = torch.zeros(n, device=v.device)
        ops.pano_reproject(v, view['pose'], view['distance_map'], mask, 0, tol)
        local = (v - view['t']) @ view['rot']
        dist = local.norm(dim=1)
        d = local / dist[:, None]
        gx = (-torch.atan2(d[:, 1], d[:, 0]) / (2 * math.pi) + 0.5) * 2 - 1
        gy = (-torch.asin(d[:, 2].clamp(-1, 1)) / math.pi + 0.5) * 2 - 1
        grid = torch.stack([gx, gy], dim=1)[None, None]
        c = torch.nn.functional.grid_sample(view['image'], grid, mode='bilinear', padding_mode='border', align_corners=False)[0, :, 0].t()
        g = view['t'].double() - v.double()
        s = (normals * g).sum(dim=1)
        cos = s / (normals.norm(dim=1) * g.norm(dim=1))
        w = cos ** power / dist.double() ** 2
        w = torch.where((mask > 0.5) & (s > 0) & (dist > 0), w, torch.zeros_like(w))
        num += w[:, None] * c.double()
        den += w
    return torch.where(den[:, None] > 0, num / den[:, None], torch.full_like(num, 0.5)).float(), den > 0


def worst_normal(mesh, normals, scale_log2):
    """Where face_normals is furthest from the index_add_ normals: the vertex, its int64 sum and that sum's length in units of the fixed
    point beside the sum of its terms' lengths (how far its faces cancel), and its valence."""
    other = composed_normals(mesh)
    i = int((normals - other).abs().max(dim=1).values.argmax())
    acc, _ = ops.meshcolor_normal_sums(mesh.vertices, mesh.faces, scale_log2)
    v, f = mesh.vertices.double(), mesh.faces.long()
    named = (f == i).any(dim=1)
    a = v[f[named, 0]]
    terms = torch.cross(v[f[named, 1]] - a, v[f[named, 2]] - a, dim=1) * 2.0 ** scale_log2
    return {'vertex': i, 'max_abs_difference': float((normals[i] - other[i]).abs().max()), 'acc': [int(x) for x in acc[i].tolist()],
            'acc_length': float(acc[i].double().norm()), 'sum_of_term_lengths': float(terms.norm(dim=1).sum()), 'valence': int(named.sum()),
            'face_normals': normals[i].tolist(), 'index_add_normals': other[i].tolist()}


def measure(res, sparse):
    raw = M.extract_mesh_sparse(scene, res, colors=True) if sparse else M.extract_mesh(scene, res, colors=True)
    entry = {'path': 'extract_mesh_sparse' if sparse else 'extract_mesh', 'extracted_vertices': int(raw.vertices.shape[0]), 'extracted_faces': int(raw.faces.shape[0]),
             'views': {}}
    for name, views in (('1', views_1), ('25', views_25)):
        k = len(views)
        mesh = M.clean_mesh(M.cull_unseen(raw, views, tol=TOL), min_faces=args.min_faces)
        V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        cv = M._color_views('meshcolor_bench', views)                     # both routes' per-view state built once, outside the timed region ...
        prepared = prepare(views, mesh.vertices.device)
        e = {'vertices': V, 'faces': F,
             'color_from_panoramas_prebuilt_s': median_s(lambda: M.color_from_panoramas(mesh, cv, box=BOX, tol=TOL), args.rounds),
             'composed_prebuilt_s': median_s(lambda: composed(mesh, views, TOL, 2, prepared), args.rounds),
             'color_from_panoramas_s': median_s(lambda: M.color_from_panoramas(mesh, views, box=BOX, tol=TOL), args.rounds),          # ... and built in every call
             'composed_s': median_s(lambda: composed(mesh, views, TOL, 2), args.rounds),
             'face_normals_s': median_s(lambda: M.face_normals(mesh, BOX), args.rounds),
             'composed_normals_s': median_s(lambda: composed_normals(mesh), args.rounds)}
        ops.start_kernel_timing()                    # device milliseconds per entry point of one more colouring
        normals = M.face_normals(mesh, BOX)
        out = M.panorama_colors(mesh.vertices, cv, normals, tol=TOL, fallback=mesh.colors)
        e['device_ms'] = {key: v[1] for key, v in ops.stop_kernel_timing().items()}
        e['blend_pairs_per_s'] = V * k / (e['device_ms']['perf_meshcolor_blend'] * 1e-3)
        e['composed_over_color_from_panoramas_prebuilt'] = e['composed_prebuilt_s'] / e['color_from_panoramas_prebuilt_s']
        e['composed_over_color_from_panoramas'] = e['composed_s'] / e['color_from_panoramas_s']
        e['composed_normals_over_face_normals'] = e['composed_normals_s'] / e['face_normals_s']
        on = out.used != 0
        for key, given in (('same_normals', normals), ('own_normals', None)):          # the composed route with the kernel's normals, and with its index_add_ ones
            want, want_on = composed(mesh, views, TOL, 2, prepared, given)
            both = on & want_on
            diff = (out.colors - want).abs().max(dim=1).values * both
            i = int(diff.argmax())
            e['composed_' + key] = {'agrees_on_which_vertices': int((on == want_on).sum()) / max(V, 1), 'coloured_by_one_route_only': int((on != want_on).sum()),
                                    'max_abs_difference': float(diff[i]), 'at_vertex': i}
        e['normals_worst_vertex'] = worst_normal(mesh, normals, M._normal_scale(BOX))
        e['share_coloured'] = int(on.sum()) / max(V, 1)
        e['mean_views_per_coloured_vertex'] = sum(int(((out.used >> b) & 1).sum()) for b in range(k)) / max(int(on.sum()), 1)
        e['mean_abs_difference_to_query_rgb'] = float((out.colors[on] - mesh.colors[on]).abs().mean())
        best = M.panorama_colors(mesh.vertices, cv, normals, tol=TOL, select='best', fallback=mesh.colors)
        e['best_over_blend_mean_abs_difference'] = float((best.colors[on] - out.colors[on]).abs().mean())
        e['unfacing_share_coloured'] = int((M.panorama_colors(mesh.vertices, cv, tol=TOL, facing=False).used != 0).sum()) / max(V, 1)
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
aabb = [float(v) for v in scene.nerf._aabb_host]
BOX = (aabb[:3], aabb[3:])
views_1 = [{'pose': torch.eye(4), 'distance_map': dist.reshape(256, 512).float().cuda().contiguous(), 'color_map': rgb.reshape(256, 512, 3).float().cuda().contiguous()}]
views_25 = list(views_1)
rng = np.random.default_rng(0)
for _ in range(24):                                  # 24 further positions inside the room; room_with_box without its box is the room from anywhere
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor(rng.uniform(-0.6, 0.6, 3) * np.array(HALF) / synthetic.ROOM_SCALE, dtype=torch.float32)
    r = gen_pano_rays(pose, 128, 256)
    d, c = synthetic.room_with_box(r.o, r.d, box_h=(0.0, 0.0, 0.0))
    views_25.append({'pose': pose, 'distance_map': d.reshape(128, 256).float().cuda().contiguous(), 'color_map': c.reshape(128, 256, 3).float().cuda().contiguous()})
out = {'rounds': args.rounds, 'min_faces': args.min_faces, 'tol': TOL, 'power': 2,
       'training': {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': math.log(2.0) / scene.renderer.render_step_size}, 'room': {}}
for res, sparse in [(r, False) for r in args.dense_resolutions] + [(r, True) for r in args.sparse_resolutions]:
    out['room'][str(res)] = measure(res, sparse)
    print(json.dumps({str(res): out['room'][str(res)]}), flush=True)
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
