"""Simplifying an extracted mesh by vertex clustering (include/perf_hip_meshsimp.h), stage by stage, beside the composed torch route it
replaces, and what it makes of the trained analytic room of tools/meshvis_bench.py.

  python tools/meshsimp_bench.py [--rounds 5] [--dense-resolutions 256] [--sparse-resolutions 1024] [--out profiles/meshsimp.json]

The meshes are the room's after cull_unseen (the training panorama, tol 1/256) and clean_mesh(min_faces=64).  (a) Per resolution and cell
(2 and 4 lattice spacings), host-clock seconds that end in a device synchronise (medians of `rounds` after a warm-up) of simplify_mesh and
of the composed route on the same mesh -- the cell rule in torch doubles, torch.unique on the keys, index_add_ of int64, torch.unique(dim=0)
on the canonical triples, torch.unique for the re-indexing; it places by the mean and finds no representative --, and the device
milliseconds of each entry point of one more simplification (HIP events around each call), the two vertex passes as fractions of the bytes
they must move at the rate perf_adam_step reaches.  (b) The same number of vertices all in ONE cell beside the mesh's own.  (c) The outcome:
the finest mesh simplified to a cell of 1/128 of the box under 'mean' and 'member' beside the direct extraction at 256: faces, vertices,
components, and the 50th / 90th percentile of the vertices' distance to the nearest analytic wall."""
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
ADAM_BYTES_PER_S = 6.0e12          # what perf_adam_step reaches on this chip


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def median_s(fn, rounds):
    times = []
    for _ in range(rounds + 1):                      # (the first round is the warm-up)
        t0 = sync_clock(); fn(); times.append(sync_clock() - t0)
    return statistics.median(times[1:])


def composed(mesh, cell, box):
    """The same simplification ('mean', 'oriented') without the new unit."""
    lo, h, n = M._cluster_grid('composed', mesh.vertices, cell, box)
    dev = mesh.vertices.device
    lo64, n64 = torch.tensor(lo, dtype=torch.float64, device=dev), torch.tensor(n, dtype=torch.float64, device=dev)
    t = torch.minimum(((mesh.vertices.double() - lo64) / h).clamp_min(0.0), n64)
    i = torch.minimum(t.floor().long(), n64.long() - 1)
    q = torch.round((t - i.double()) * 4294967296.0).long()
    key = i[:, 0] << 42 | i[:, 1] << 21 | i[:, 2]
    uniq, inverse = torch.unique(key, return_inverse=True)
    C, V = uniq.numel(), key.numel()
    index = torch.arange(V, device=dev)
    first = torch.full((C,), V, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, index, 'amin')
    rank = torch.empty_like(first)
    rank[torch.argsort(first)] = torch.arange(C, device=dev)          # ids: the ranks of the smallest members
    vc = rank[inverse]
    S = torch.zeros(C, 3, dtype=torch.int64, device=dev).index_add_(0, vc, q)
    count = torch.zeros(C, dtype=torch.int64, device=dev).index_add_(0, vc, torch.ones_like(vc))
    cells = torch.zeros(C, 3, dtype=torch.int64, device=dev)
    cells[vc] = i
    p = (lo64 + (cells.double() + S.double() / (count.double() * 4294967296.0)[:, None]) * h).float()
    r = vc[mesh.faces.long()]
    ok = (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])
    rows = torch.nonzero(ok)[:, 0]
    r = r[rows]
    shift = r.argmin(dim=1)
    canon = torch.stack([r.gather(1, ((shift + k) % 3)[:, None])[:, 0] for k in range(3)], dim=1)
    _, which = torch.unique(canon, dim=0, return_inverse=True)
    winner = torch.full((int(which.max()) + 1 if len(which) else 0,), len(rows), dtype=torch.int64, device=dev).scatter_reduce_(0, which, torch.arange(len(rows), device=dev), 'amin')
    kept = r[torch.sort(winner).values]
    used, new = torch.unique(kept, return_inverse=True)
    return p[used], new.int()


def wall_distance(vertices):
    h = torch.tensor(HALF, device=vertices.device) / synthetic.ROOM_SCALE
    return (vertices.abs() - h).abs().min(dim=1).values


def shape_of(mesh):
    d = wall_distance(mesh.vertices) if len(mesh.vertices) else None
    return {'vertices': int(mesh.vertices.shape[0]), 'faces': int(mesh.faces.shape[0]), 'components': int(M.connected_components(mesh).faces.numel()),
            'wall_distance_p50_p90': [float(torch.quantile(d, q)) for q in (0.5, 0.9)] if d is not None else None}


def device_ms(fn):
    ops.start_kernel_timing()
    fn()
    return {key: v[1] for key, v in ops.stop_kernel_timing().items()}


def prepared(res, sparse):
    mesh = M.extract_mesh_sparse(scene, res) if sparse else M.extract_mesh(scene, res)
    return M.clean_mesh(M.cull_unseen(mesh, views), min_faces=args.min_faces)


def measure(res, mesh):
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    entry = {'vertices': V, 'faces': F, 'cells': {}}
    for factor in (2, 4):
        cell = factor * EXTENT / res
        e = {'cell': cell, 'simplify_mesh_s': median_s(lambda: M.simplify_mesh(mesh, cell, BOX), args.rounds),
             'simplify_mesh_member_s': median_s(lambda: M.simplify_mesh(mesh, cell, BOX, placement='member'), args.rounds),
             'simplify_mesh_own_box_s': median_s(lambda: M.simplify_mesh(mesh, cell), args.rounds),
             'composed_s': median_s(lambda: composed(mesh, cell, BOX), args.rounds)}
        e['composed_over_simplify'] = e['composed_s'] / e['simplify_mesh_s']
        out, _ = M.simplify_mesh(mesh, cell, BOX)
        cv, cf = composed(mesh, cell, BOX)
        e['composed_agrees'] = bool(torch.equal(cv.view(torch.int32), out.vertices.view(torch.int32)) and torch.equal(cf, out.faces))
        e['vertices_after'], e['faces_after'] = int(out.vertices.shape[0]), int(out.faces.shape[0])
        e['device_ms'] = device_ms(lambda: M.simplify_mesh(mesh, cell, BOX))
        clusters = M.cluster_vertices(mesh.vertices, cell, BOX)
        e['clusters'] = clusters.n_clusters
        # a clustering must read 12 bytes and write 4 per vertex; a placement reads 16 per vertex and writes 16 per cluster
        e['cluster_fraction_of_adam_rate'] = 16 * V / (e['device_ms']['perf_meshsimp_cluster'] * 1e-3) / ADAM_BYTES_PER_S
        e['place_fraction_of_adam_rate'] = (16 * V + 16 * clusters.n_clusters) / (e['device_ms']['perf_meshsimp_place'] * 1e-3) / ADAM_BYTES_PER_S
        entry['cells'][str(factor)] = e
    # the same number of vertices in ONE cell: one slot, three sums and one minimum that every wave goes to
    g = torch.Generator(device='cuda').manual_seed(0)
    hot = torch.rand(V, 3, device='cuda', generator=g) * 0.8 + 0.1
    one = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    M.cluster_vertices(hot, 1.0, one); M.cluster_vertices(hot, 1.0 / 256, one)          # (the warm-up)
    entry['one_cell'] = {'device_ms': device_ms(lambda: M.cluster_vertices(hot, 1.0, one)),
                         'spread_device_ms': device_ms(lambda: M.cluster_vertices(hot, 1.0 / 256, one)),
                         'clusters': M.cluster_vertices(hot, 1.0, one).n_clusters, 'spread_clusters': M.cluster_vertices(hot, 1.0 / 256, one).n_clusters}
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
out = {'rounds': args.rounds, 'min_faces': args.min_faces, 'adam_bytes_per_s': ADAM_BYTES_PER_S, 'box': BOX,
       'training': {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': math.log(2.0) / scene.renderer.render_step_size}, 'room': {}}
meshes = {}
for res, sparse in [(r, False) for r in args.dense_resolutions] + [(r, True) for r in args.sparse_resolutions]:
    meshes[res] = prepared(res, sparse)
    out['room'][str(res)] = measure(res, meshes[res])
    print(json.dumps({str(res): out['room'][str(res)]}), flush=True)
fine, coarse = max(meshes), min(meshes)
cell = EXTENT / 128
out['outcome'] = {'cell': cell, 'fine_resolution': fine, 'direct_resolution': coarse, 'fine': shape_of(meshes[fine]), 'direct': shape_of(meshes[coarse]),
                  'mean': shape_of(M.simplify_mesh(meshes[fine], cell, BOX)[0]), 'member': shape_of(M.simplify_mesh(meshes[fine], cell, BOX, placement='member')[0]),
                  'mean_unoriented': shape_of(M.simplify_mesh(meshes[fine], cell, BOX, dedupe='unoriented')[0]),
                  'direct_mean': shape_of(M.simplify_mesh(meshes[coarse], cell, BOX)[0])}
print(json.dumps({'outcome': out['outcome']}), flush=True)
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
