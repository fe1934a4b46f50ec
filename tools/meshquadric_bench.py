"""Quadric error placement of a simplified mesh's vertices (include/perf_hip_meshquadric.h) beside the 'mean' placement and beside the
composed torch route, on the trained analytic room of tools/meshsimp_bench.py, and what it makes of the room's walls.

  python tools/meshquadric_bench.py [--rounds 5] [--dense-resolutions 256] [--sparse-resolutions 1024] [--out profiles/meshquadric.json]
                                    [--other-library libperf_hip_plain.so --other-label plain]

The meshes are the room's after cull_unseen (the training panorama, tol 1/256) and clean_mesh(min_faces=64), the cases of
profiles/meshsimp.json.  (a) Per resolution and cell (2 and 4 lattice spacings): host-clock seconds that end in a device synchronise
(medians of `rounds` after a warm-up) of simplify_mesh under 'mean' and under 'quadric' in the same session; the two new calls alone on
a clustering made before the clock starts, beside the composed route with the same output shape -- the terms in torch doubles, index_add_
of the float64 terms, torch.linalg.solve --; the device milliseconds of each entry point (HIP events around each call), the sums as a
fraction of the bytes of their atomics at 1.3 TB/s; the same faces all in ONE cell.  --other-library names a second build of the library
(the sums kernel in its plain form, -DPERF_MESHQUADRIC_PLAIN_SUMS on meshquadric.hip): its perf_meshquadric_sums is timed on the same
inputs in the same session and its sums are compared to the bit.  (b) The outcome at a cell of 1/128 of the box on the finest mesh: the 50th / 90th percentile of the vertices' distance to the
nearest analytic wall under both placements, the same restricted to the clusters within one cell of a wall edge or corner, the faces the
2^60 rule skipped and the components the clamp touched (both counted by the composed route)."""
import argparse, ctypes, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import _lib
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
ap.add_argument('--other-library', default=None, help='a second build of libperf_hip.so whose perf_meshquadric_sums is timed beside this one')
ap.add_argument('--other-label', default='other')
ap.add_argument('--out', default=None)
args = ap.parse_args()
HALF = (0.9, 0.7, 0.5)
ATOMIC_BYTES_PER_S = 1.3e12          # what global float atomics reach chip-wide; no figure exists for 64-bit integer atomics


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def median_s(fn, rounds):
    times = []
    for _ in range(rounds + 1):                      # (the first round is the warm-up)
        t0 = sync_clock(); fn(); times.append(sync_clock() - t0)
    return statistics.median(times[1:])


def event_ms(fn, rounds):
    times = []
    for _ in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times[1:])


def device_ms(fn):
    ops.start_kernel_timing()
    fn()
    return {key: v[1] for key, v in ops.stop_kernel_timing().items()}


def composed(mesh, grid, clusters):
    """The same placement without the new unit: float64 terms, never quantised -> (vertices fp32 [C, 3], x before the clamp, solved,
    the number of faces the 2^60 rule would skip)."""
    lo, h, n = grid
    dev = mesh.vertices.device
    lo64, n64 = torch.tensor(lo, dtype=torch.float64, device=dev), torch.tensor(n, dtype=torch.float64, device=dev)
    C = clusters.n_clusters
    v = mesh.vertices.double()
    f = mesh.faces.long()
    cl = clusters.vertex_cluster.long()[f]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    nrm = torch.linalg.cross((b - a) / h, (c - a) / h)
    pairs = torch.stack([nrm[:, i] * nrm[:, j] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], dim=1)
    fits = ((pairs * 2.0 ** 40).abs() < 2.0 ** 60).all(dim=1) & (cl >= 0).all(dim=1)
    acc = torch.zeros(C, 9, dtype=torch.float64, device=dev)

    def centred(x):
        t = torch.minimum(((x - lo64) / h).clamp_min(0.0), n64)
        i = torch.minimum(t.floor(), n64 - 1)
        return i, t - i - 0.5

    for k in range(3):
        _, r = centred(v[f[:, k]])
        d = (nrm * r).sum(dim=1)
        acc.index_add_(0, cl[fits, k], torch.cat([pairs, nrm * d[:, None]], dim=1)[fits])
    tr = acc[:, 0] + acc[:, 3] + acc[:, 5]
    i, _ = centred(v[clusters.representative.long()])
    anchor = clusters.vertices.double()
    m = (anchor - lo64) / h - (i + 0.5)
    lam = tr / 1024
    Mx = torch.stack([torch.stack([acc[:, 0] + lam, acc[:, 1], acc[:, 2]], 1), torch.stack([acc[:, 1], acc[:, 3] + lam, acc[:, 4]], 1),
                      torch.stack([acc[:, 2], acc[:, 4], acc[:, 5] + lam], 1)], 1)
    solved = tr > 0
    Mx[~solved] = torch.eye(3, dtype=torch.float64, device=dev)
    x = torch.linalg.solve(Mx, (acc[:, 6:] + lam[:, None] * m)[:, :, None])[:, :, 0]
    p = lo64 + (i + 0.5 + x.clamp(-0.5, 0.5)) * h
    return torch.where(solved[:, None], p, anchor).float(), x, solved, int(((cl >= 0).all(dim=1) & ~fits).sum())


def other_sums(lib, mesh, grid, clusters, acc, flags):
    lo, h, n = grid
    lo3 = (ctypes.c_float * 3)(*lo)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.perf_meshquadric_sums(p(mesh.vertices), mesh.vertices.shape[0], p(mesh.faces), mesh.faces.shape[0], lo3, h, *n, p(clusters.vertex_cluster), clusters.n_clusters,
                                   p(acc), p(flags), ctypes.c_void_p(flags.data_ptr() + 8), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.perf_last_error()


def wall_distance(vertices):
    h = torch.tensor(HALF, device=vertices.device) / synthetic.ROOM_SCALE
    return (vertices.abs() - h).abs()


def quantiles(d):
    return [float(torch.quantile(d, q)) for q in (0.5, 0.9)] if d.numel() else None


def prepared(res, sparse):
    mesh = M.extract_mesh_sparse(scene, res) if sparse else M.extract_mesh(scene, res)
    mesh = M.clean_mesh(M.cull_unseen(mesh, views), min_faces=args.min_faces)
    return M.Mesh(mesh.vertices.contiguous(), mesh.faces.contiguous(), mesh.colors, mesh.normals)


def measure(res, mesh):
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    entry = {'vertices': V, 'faces': F, 'cells': {}}
    for factor in (2, 4):
        cell = factor * EXTENT / res
        grid = M._cluster_grid('bench', mesh.vertices, cell, BOX)
        lo, h, n = grid
        e = {'cell': cell, 'simplify_mesh_mean_s': median_s(lambda: M.simplify_mesh(mesh, cell, BOX), args.rounds),
             'simplify_mesh_quadric_s': median_s(lambda: M.simplify_mesh(mesh, cell, BOX, placement='quadric'), args.rounds)}
        e['quadric_over_mean'] = e['simplify_mesh_quadric_s'] / e['simplify_mesh_mean_s']
        e['device_ms'] = device_ms(lambda: M.simplify_mesh(mesh, cell, BOX, placement='quadric'))
        clusters = M.cluster_vertices(mesh.vertices, cell, BOX)
        e['clusters'] = clusters.n_clusters

        def placement():
            acc, _ = ops.meshquadric_sums(mesh.vertices, mesh.faces, lo, h, n, clusters.vertex_cluster, clusters.n_clusters)
            return ops.meshquadric_place(mesh.vertices, lo, h, n, clusters.vertices, clusters.representative, acc)

        e['placement_s'] = median_s(placement, args.rounds)
        e['composed_placement_s'] = median_s(lambda: composed(mesh, grid, clusters), args.rounds)
        e['composed_over_placement'] = e['composed_placement_s'] / e['placement_s']
        ours, (theirs, x, solved, skipped) = placement(), composed(mesh, grid, clusters)
        off = (ours.double() - theirs.double()).abs().max(dim=1).values / h
        e['largest_difference_to_composed_cells'], e['clusters_off_composed_by_a_hundredth_of_a_cell'] = float(off.max()), int((off > 0.01).sum())
        quanta = ops.meshquadric_sums(mesh.vertices, mesh.faces, lo, h, n, clusters.vertex_cluster, clusters.n_clusters)[0][:, (0, 3, 5)].sum(dim=1)
        e['largest_trace_of_those_in_quanta'] = int(quanta[off > 0.01].max()) if bool((off > 0.01).any()) else None          # (tr in units of 2^-40)
        e['median_trace_in_quanta'] = int(quanta.median())
        e['skipped_faces'], e['clamped_components'], e['clusters_solved'] = skipped, int((x.abs() > 0.5)[solved].sum()), int(solved.sum())
        # the sums alone (the call: three clears and the kernel), and the bytes of their atomics: 72 per face wholly in one cluster, 216 otherwise
        cl = clusters.vertex_cluster.long()[mesh.faces.long()]
        whole = int(((cl[:, 0] == cl[:, 1]) & (cl[:, 1] == cl[:, 2])).sum())
        e['faces_in_one_cluster'], e['atomic_bytes'] = whole, 72 * whole + 216 * (F - whole)
        e['sums_ms'] = event_ms(lambda: ops.meshquadric_sums(mesh.vertices, mesh.faces, lo, h, n, clusters.vertex_cluster, clusters.n_clusters), args.rounds)
        e['sums_fraction_of_atomic_rate'] = e['atomic_bytes'] / (e['sums_ms'] * 1e-3) / ATOMIC_BYTES_PER_S
        if OTHER is not None:
            acc, flags = ops.meshquadric_sums(mesh.vertices, mesh.faces, lo, h, n, clusters.vertex_cluster, clusters.n_clusters)
            acc2, flags2 = torch.empty_like(acc), torch.empty_like(flags)
            e[f'sums_{args.other_label}_ms'] = event_ms(lambda: other_sums(OTHER, mesh, grid, clusters, acc2, flags2), args.rounds)
            e[f'sums_{args.other_label}_agrees'] = bool(torch.equal(acc, acc2) and torch.equal(flags, flags2))
        entry['cells'][str(factor)] = e
    # the same faces in ONE cell: every lane on one 72-byte row
    one = M._cluster_grid('bench', mesh.vertices, 4 * EXTENT, BOX)
    hot = M.cluster_vertices(mesh.vertices, 4 * EXTENT, BOX)
    entry['one_cell'] = {'clusters': hot.n_clusters, 'sums_ms': event_ms(lambda: ops.meshquadric_sums(mesh.vertices, mesh.faces, *one, hot.vertex_cluster, hot.n_clusters), args.rounds)}
    if OTHER is not None:
        acc2, flags2 = torch.empty(hot.n_clusters, 9, dtype=torch.int64, device='cuda'), torch.empty(2, dtype=torch.int64, device='cuda')
        entry['one_cell'][f'sums_{args.other_label}_ms'] = event_ms(lambda: other_sums(OTHER, mesh, one, hot, acc2, flags2), args.rounds)
    return entry


def outcome(mesh, cell):
    mean, _ = M.simplify_mesh(mesh, cell, BOX)
    quadric, _ = M.simplify_mesh(mesh, cell, BOX, placement='quadric')
    assert torch.equal(mean.faces, quadric.faces)
    dm, dq = wall_distance(mean.vertices), wall_distance(quadric.vertices)
    near = (dm < cell).sum(dim=1) >= 2          # within one cell of two walls or three: an edge or a corner of the room (by the mean's vertex)
    return {'cell': cell, 'vertices': int(mean.vertices.shape[0]), 'faces': int(mean.faces.shape[0]), 'vertices_near_an_edge_or_corner': int(near.sum()),
            'moved_vertices': int((mean.vertices != quadric.vertices).any(dim=1).sum()),
            'mean': {'wall_distance_p50_p90': quantiles(dm.min(dim=1).values), 'near_edges_p50_p90': quantiles(dm.min(dim=1).values[near]),
                     'near_edges_second_wall_p50_p90': quantiles(dm.sort(dim=1).values[:, 1][near])},
            'quadric': {'wall_distance_p50_p90': quantiles(dq.min(dim=1).values), 'near_edges_p50_p90': quantiles(dq.min(dim=1).values[near]),
                        'near_edges_second_wall_p50_p90': quantiles(dq.sort(dim=1).values[:, 1][near])}}


OTHER = None
if args.other_library:
    _lib.load()
    OTHER = ctypes.CDLL(os.path.abspath(args.other_library))
    OTHER.perf_meshquadric_sums.restype, OTHER.perf_meshquadric_sums.argtypes = _lib._SIGS_MESHQUADRIC['perf_meshquadric_sums']
    OTHER.perf_last_error.restype = ctypes.c_char_p
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
out = {'rounds': args.rounds, 'min_faces': args.min_faces, 'atomic_bytes_per_s': ATOMIC_BYTES_PER_S, 'box': BOX, 'other_library': args.other_label if OTHER is not None else None,
       'training': {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': math.log(2.0) / scene.renderer.render_step_size}, 'room': {}, 'outcome': {}}
meshes = {}
for res, sparse in [(r, False) for r in args.dense_resolutions] + [(r, True) for r in args.sparse_resolutions]:
    meshes[res] = prepared(res, sparse)
    out['room'][str(res)] = measure(res, meshes[res])
    print(json.dumps({str(res): out['room'][str(res)]}), flush=True)
    out['outcome'][str(res)] = outcome(meshes[res], EXTENT / 128)
    print(json.dumps({'outcome': {str(res): out['outcome'][str(res)]}}), flush=True)
    if args.out:          # (after every resolution: what is measured is kept)
        json.dump(out, open(args.out, 'w'), indent=1)
        open(args.out, 'a').write('\n')
