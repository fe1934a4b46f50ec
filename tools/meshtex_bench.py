"""Baking a texture atlas from the registered panoramas (include/perf_hip_meshtex.h) on the trained analytic room of tools/meshvis_bench.py:
the fused bake beside the composed route of the same inputs, and what the atlas adds to the appearance of a simplified mesh.

  python tools/meshtex_bench.py [--rounds 5] [--resolution 1024] [--sizes 1024 2048 4096] [--points 100000] [--out profiles/meshtex.json]

The mesh is the sparse extraction after cull_unseen (the training panorama, tol 1/256), clean_mesh(min_faces=64) and simplify_mesh to a cell
of 1/128 of the box.  Views: K = 1, the panorama the room is trained on (256 x 512 from the origin), and K = 25, that one and the analytic
room's panoramas (128 x 256) from 24 further positions inside it.  (a) Per atlas size and K, host-clock seconds that end in a device
synchronise (medians of `rounds` after a warm-up) and the peak of the allocator above what was held before the call, of
bake_panorama_texture (the fused kernel: one launch) and of the composed route: atlas_points, then panorama_colors -- the blend kernel -- on
the S^2 points.  Both with the per-view descriptors built once outside the timed region.  Also the device milliseconds per entry point of
one more run of each (HIP events around each call), and whether the two routes' images are equal to the bit on the covered texels.
(b) The appearance, at `points` random points of the mesh's faces (faces drawn by area, barycentrics uniform): the panorama blend evaluated
at the point itself with its face's normal -- the truth of this colour model -- beside the barycentric interpolation of
color_from_panoramas' vertex colours and beside sample_atlas of each bake; the mean and the 90 % absolute difference of each route to the
truth over the points some view passed for; the share of gutter texels and of interior texels no view passed for.  Nothing is asserted."""
import argparse, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import mesh as M
from perf_amd import ops, synthetic
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--resolution', type=int, default=1024)
ap.add_argument('--sizes', type=int, nargs='*', default=[1024, 2048, 4096])
ap.add_argument('--points', type=int, default=100000)
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


def median_s_and_peak(fn, rounds):
    """(the median of the rounds' seconds after a warm-up, the allocator's peak above what was held before the call, in bytes)"""
    times, peak = [], 0
    for _ in range(rounds + 1):
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = sync_clock(); out = fn(); times.append(sync_clock() - t0)
        peak = max(peak, torch.cuda.max_memory_allocated() - held)
        del out
    return statistics.median(times[1:]), peak


def device_ms(fn):
    ops.start_kernel_timing()
    fn()
    return {key: v[1] for key, v in ops.stop_kernel_timing().items()}


def composed(mesh, cv, size, tile):
    """The bake without the fused kernel: the materialised texel -> point map, then the blend kernel on the S^2 points."""
    points, point_normals, _, coverage = M.atlas_points(mesh, size, tile)
    return M.panorama_colors(points, cv, point_normals, tol=TOL), coverage


def spread(diff):
    d = diff.abs().flatten().double()
    return {'mean_abs': float(d.mean()), 'p90_abs': float(torch.quantile(d[torch.randperm(d.numel(), device=d.device)[:1 << 22]], 0.9))}


def measure(mesh, name, views, sample):
    face_ids, bary, at, normal = sample
    cv = M._color_views('meshtex_bench', views)          # both routes' per-view state built once, outside the timed region
    F = int(mesh.faces.shape[0])
    truth = M.panorama_colors(at, cv, normal, tol=TOL)
    seen = truth.used != 0
    vertex = M.color_from_panoramas(mesh, cv, box=BOX, tol=TOL).colors[mesh.faces[face_ids].long()]          # [N, 3 corners, 3]
    e = {'views': len(views), 'points_some_view_passed_for': int(seen.sum()) / max(len(at), 1),
         'per_vertex_to_truth': spread(((bary[:, :, None] * vertex).sum(dim=1) - truth.colors)[seen]), 'sizes': {}}
    for size in args.sizes:
        size, tile = M.atlas_layout(F, size=size)
        fused_s, fused_peak = median_s_and_peak(lambda: M.bake_panorama_texture(mesh, cv, size=size, tile=tile, tol=TOL), args.rounds)
        composed_s, composed_peak = median_s_and_peak(lambda: composed(mesh, cv, size, tile), args.rounds)
        s = {'size': size, 'tile': tile, 'texels_inside_per_face': (tile - 2) * (tile - 1) // 2, 'fused_s': fused_s, 'composed_s': composed_s,
             'composed_over_fused': composed_s / fused_s, 'fused_peak_bytes': fused_peak, 'composed_peak_bytes': composed_peak,
             'fused_device_ms': device_ms(lambda: M.bake_panorama_texture(mesh, cv, size=size, tile=tile, tol=TOL)),
             'composed_device_ms': device_ms(lambda: composed(mesh, cv, size, tile))}
        s['bake_pairs_per_s'] = size * size * len(views) / (s['fused_device_ms']['perf_meshtex_bake'] * 1e-3)
        atlas = M.bake_panorama_texture(mesh, cv, size=size, tile=tile, tol=TOL)
        want, coverage = composed(mesh, cv, size, tile)
        covered = (coverage != 0).view(size, size)
        s['equal_to_the_bit_on_covered_texels'] = bool(torch.equal(atlas.image[covered].view(torch.int32), want.colors.view(size, size, 3)[covered].view(torch.int32))
                                                       and torch.equal(atlas.used[covered], want.used.view(size, size)[covered]))
        del want
        inside, gutter = atlas.coverage == 1, atlas.coverage == 2
        s['share_of_texels'] = {'inside': float(inside.float().mean()), 'gutter': float(gutter.float().mean()), 'no_face': float((atlas.coverage == 0).float().mean())}
        s['no_view_passed'] = {'inside': float((atlas.used[inside] == 0).float().mean()), 'gutter': float((atlas.used[gutter] == 0).float().mean())}
        s['atlas_to_truth'] = spread((M.sample_atlas(atlas, face_ids, bary) - truth.colors.double())[seen])
        e['sizes'][str(size)] = s
        del atlas
        print(json.dumps({name: {str(size): s}}), flush=True)
    return e


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

raw = M.extract_mesh_sparse(scene, args.resolution, colors=True)
fine = M.clean_mesh(M.cull_unseen(raw, views_1, tol=TOL), min_faces=args.min_faces)
cell = (aabb[3] - aabb[0]) / 128
mesh = M.simplify_mesh(fine, cell, BOX)[0]
mesh = M.Mesh(mesh.vertices, mesh.faces)          # (no fallback: a texel no view passed for shows as fill)
del raw
# the random points: faces by area, barycentrics uniform; each with its face's unit normal
tri = mesh.vertices[mesh.faces.long()].double()
cross = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
area = cross.norm(dim=1)
face_ids = torch.multinomial(area / area.sum(), args.points, replacement=True)
r = torch.rand(args.points, 2, dtype=torch.float64, device='cuda')
r = torch.where((r.sum(dim=1) > 1)[:, None], 1 - r, r)
bary = torch.cat([1 - r.sum(dim=1, keepdim=True), r], dim=1)
at = (bary[:, :, None] * tri[face_ids]).sum(dim=1).float().contiguous()
normal = torch.nn.functional.normalize(cross[face_ids], dim=1).float().contiguous()
out = {'rounds': args.rounds, 'min_faces': args.min_faces, 'tol': TOL, 'power': 2, 'points': args.points, 'resolution': args.resolution, 'simplify_cell': cell,
       'training': {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': math.log(2.0) / scene.renderer.render_step_size},
       'fine': {'vertices': int(fine.vertices.shape[0]), 'faces': int(fine.faces.shape[0])},
       'mesh': {'vertices': int(mesh.vertices.shape[0]), 'faces': int(mesh.faces.shape[0])}, 'views': {}}
del fine
for name, views in (('1', views_1), ('25', views_25)):
    out['views'][name] = measure(mesh, name, views, (face_ids, bary.float(), at, normal))
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
print(json.dumps({'mesh': out['mesh'], 'fine': out['fine']}))
