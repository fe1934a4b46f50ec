"""Cleaning an extracted mesh by its connected components (include/perf_hip_meshcc.h), stage by stage, beside the extraction it follows
and beside the host route it replaces, on the trained analytic room of tools/mesh_bench.py.

  python tools/meshcc_bench.py [--rounds 5] [--dense-resolutions 256] [--sparse-resolutions 1024 2048] [--out profiles/meshcc.json]

Per resolution, host-clock seconds that end in a device synchronise (medians of `rounds` after a warm-up): the extraction (extract_mesh at
the dense resolutions, extract_mesh_sparse at the sparse ones, without colours and normals); label (ops.meshcc_label and the read of the
component count), stats (ops.meshcc_stats), filter (ops.meshcc_filter_count, the read of the two counts, ops.meshcc_filter_write) and
clean_mesh as a whole with min_faces=64, orientation='inward' (and the device milliseconds of each of its entry points; filter also with
every component kept, the most it can write); and the host route on the same faces: the copy off the device and
scipy.sparse.csgraph.connected_components (`host-rounds` of it: it takes seconds).  Also C and the face counts before and after."""
import argparse, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import mesh as M
from perf_amd import ops, synthetic
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--host-rounds', type=int, default=1)
ap.add_argument('--dense-resolutions', type=int, nargs='*', default=[256])
ap.add_argument('--sparse-resolutions', type=int, nargs='*', default=[1024, 2048])
ap.add_argument('--geo', type=int, default=150)
ap.add_argument('--app', type=int, default=100)
ap.add_argument('--min-faces', type=int, default=64)
ap.add_argument('--out', default=None)
args = ap.parse_args()


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def median_s(fn, rounds):
    times = []
    for _ in range(rounds + 1):                      # (the first round is the warm-up)
        t0 = sync_clock(); fn(); times.append(sync_clock() - t0)
    return statistics.median(times[1:])


def host_route(faces, n_vertices):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = faces.cpu().numpy().astype(np.int64)
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n_vertices, n_vertices))
    return connected_components(graph, directed=False)


def measure(res, sparse):
    extract = (lambda: M.extract_mesh_sparse(scene, res)) if sparse else (lambda: M.extract_mesh(scene, res))
    entry = {'path': 'extract_mesh_sparse' if sparse else 'extract_mesh', 'extract_s': median_s(extract, args.rounds)}
    mesh = extract()
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    state = {}

    def label():
        state['vc'], counts, state['ws'] = ops.meshcc_label(mesh.faces, V, state.get('ws'))
        state['C'], state['bad'] = counts.tolist()

    def stats():
        state['stats'] = ops.meshcc_stats(mesh.faces, state['vc'], state['C'], mesh.vertices)

    def filt():
        counts, ws = ops.meshcc_filter_count(mesh.faces, state['vc'], state['keep'], state['ws'])
        nv, nf = counts.tolist()
        state['out'] = ops.meshcc_filter_write(mesh.faces, state['vc'], state['keep'], ws, nv, nf, mesh.vertices)

    entry['label_s'] = median_s(label, args.rounds)
    entry['stats_s'] = median_s(stats, args.rounds)
    comps = M.Components(state['vc'], *state['stats'])
    state['keep'] = M.select_components(comps, min_faces=args.min_faces, orientation='inward')
    entry['select_s'] = median_s(lambda: M.select_components(comps, min_faces=args.min_faces, orientation='inward'), args.rounds)
    entry['filter_s'] = median_s(filt, args.rounds)
    kept = (int(state['out'][0].shape[0]), int(state['out'][1].shape[0]))
    selected, state['keep'] = state['keep'], torch.ones_like(state['keep'])          # and with every component kept: all vertices and faces are rewritten
    entry['filter_keep_all_s'] = median_s(filt, args.rounds)
    state['keep'] = selected
    entry['clean_mesh_s'] = median_s(lambda: M.clean_mesh(mesh, min_faces=args.min_faces, orientation='inward'), args.rounds)
    ops.start_kernel_timing()                        # device milliseconds per entry point of one more cleaning (HIP events around each call)
    M.clean_mesh(mesh, min_faces=args.min_faces, orientation='inward')
    entry['clean_mesh_device_ms'] = {k: v[1] for k, v in ops.stop_kernel_timing().items()}
    entry['host_route_s'] = median_s(lambda: state.__setitem__('host', host_route(mesh.faces, V)), args.host_rounds)
    per_faces = comps.faces
    entry.update({'vertices': V, 'faces': F, 'components': state['C'], 'host_components': int(state['host'][0]), 'kept_components': int(state['keep'].sum()),
                  'faces_after': kept[1], 'vertices_after': kept[0], 'largest_component_faces': int(per_faces.max()) if state['C'] else 0,
                  'components_below_min_faces': int((per_faces < args.min_faces).sum()), 'workspace_bytes': int(state['ws'].numel() * 8),
                  'clean_over_extract': entry['clean_mesh_s'] / entry['extract_s'], 'host_over_clean': entry['host_route_s'] / entry['clean_mesh_s']})
    assert entry['components'] == entry['host_components'] and state['bad'] == -1
    return entry


torch.manual_seed(0); np.random.seed(0)
scene = NeRFScene(dtype='fp16')
rays = gen_pano_rays(torch.eye(4), 256, 512)
dist, rgb = synthetic.room(rays.d)
pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
scene.train_conf.pixel_loss_batch_size = 4096
scene.train_one_episode(pool, args.geo, args.app)
out = {'rounds': args.rounds, 'host_rounds': args.host_rounds, 'min_faces': args.min_faces, 'orientation': 'inward',
       'training': {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': math.log(2.0) / scene.renderer.render_step_size}, 'room': {}}
for res in args.dense_resolutions:
    out['room'][str(res)] = measure(res, False)
    print(json.dumps({str(res): out['room'][str(res)]}), flush=True)
for res in args.sparse_resolutions:
    out['room'][str(res)] = measure(res, True)
    print(json.dumps({str(res): out['room'][str(res)]}), flush=True)
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
