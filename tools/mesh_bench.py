"""The two surface-nets passes (ops.mesh_count, ops.mesh_write) at 256^3 and 512^3 cells, on an analytic ball and on the trained
synthetic room, and the whole extract_mesh split into its stages.

  python tools/mesh_bench.py [--rounds 5] [--iters 10] [--out profiles/mesh.json]
                             [--sparse-resolutions 256 512 1024 2048] [--sparse-out profiles/brickmesh.json]

Per lattice: the median milliseconds of each pass (device events around `iters` back-to-back calls, `rounds` of them after a warm-up),
the bytes the pass must move -- count: the field once and 16 B per 64-cell chunk written; write: those 16 B read and the vertices and
faces written once (the corners of active cells, read again, are not counted) -- and that over the time, beside the 6 TB/s
perf_adam_step reaches.  The count pass is timed with its scan (every launch of perf_mesh_count); the write pass
with the 16-byte read-back that perf_mesh_write refuses short capacities by.  The stages of extract_mesh are host-clock times that end
in a device synchronise.  With --sparse-resolutions the stages of extract_mesh_sparse (select, corners, density, count, write; the same
host clock) on the same trained room, beside extract_mesh where the dense lattice fits (up to 512), are written to --sparse-out."""
import argparse, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import mesh as M
from perf_amd import ops, synthetic
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--resolutions', type=int, nargs='+', default=[256, 512])
ap.add_argument('--geo', type=int, default=150)
ap.add_argument('--app', type=int, default=100)
ap.add_argument('--out', default=None)
ap.add_argument('--sparse-resolutions', type=int, nargs='*', default=[])
ap.add_argument('--sparse-out', default=None)
args = ap.parse_args()
ADAM_TB_PER_S = 6.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


def passes(field, thr, lo, hi):
    res = field.shape[0] - 1
    counts, ws = ops.mesh_count(field, thr)
    nv, nf = counts.tolist()
    for _ in range(2):
        ops.mesh_count(field, thr, ws); ops.mesh_write(field, thr, lo, hi, ws, nv, nf)
    torch.cuda.synchronize()
    tc = [timed(lambda: ops.mesh_count(field, thr, ws)) for _ in range(args.rounds)]
    tw = [timed(lambda: ops.mesh_write(field, thr, lo, hi, ws, nv, nf)) for _ in range(args.rounds)]
    chunks = res * res * -(-res // 64)
    count_bytes = field.numel() * 4 + 16 * chunks
    write_bytes = 16 * chunks + 12 * nv + 12 * nf
    mc, mw = statistics.median(tc), statistics.median(tw)
    return {'cells': res ** 3, 'vertices': nv, 'faces': nf, 'count_ms': mc, 'count_ms_all': tc, 'write_ms': mw, 'write_ms_all': tw,
            'count_bytes': count_bytes, 'write_bytes': write_bytes, 'count_TB_per_s': count_bytes / (mc * 1e-3) / 1e12,
            'write_TB_per_s': write_bytes / (mw * 1e-3) / 1e12, 'count_fraction_of_adam_rate': count_bytes / (mc * 1e-3) / 1e12 / ADAM_TB_PER_S}


def ball(res):
    g = torch.arange(res + 1, device='cuda', dtype=torch.float32)
    c = [0.51 * res, 0.47 * res, 0.53 * res]
    return 0.37 * res - torch.sqrt((g[:, None, None] - c[0]) ** 2 + (g[None, :, None] - c[1]) ** 2 + (g[None, None, :] - c[2]) ** 2)


out = {'rounds': args.rounds, 'iters_per_round': args.iters, 'adam_TB_per_s_of_DESIGN_section_6': ADAM_TB_PER_S, 'ball': {}, 'room': {}}
for res in args.resolutions:
    out['ball'][str(res)] = passes(ball(res), 0.0, [-1, -1, -1], [1, 1, 1])

torch.manual_seed(0); np.random.seed(0)
scene = NeRFScene(dtype='fp16')
rays = gen_pano_rays(torch.eye(4), 256, 512)
dist, rgb = synthetic.room(rays.d)
pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
scene.train_conf.pixel_loss_batch_size = 4096
scene.train_one_episode(pool, args.geo, args.app)
thr = math.log(2.0) / scene.renderer.render_step_size
aabb = scene.nerf._aabb_host
out['room']['training'] = {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': thr}
for res in args.resolutions:
    field = M.density_lattice(scene, res)
    entry = passes(field, thr, aabb[:3], aabb[3:])
    del field
    stages = {'lattice_s': [], 'count_s': [], 'write_s': [], 'attributes_s': []}
    for _ in range(args.rounds + 1):                 # (the first round is the warm-up)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        field = M.density_lattice(scene, res)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        counts, ws = ops.mesh_count(field, thr)
        nv, nf = counts.tolist()
        t2 = time.perf_counter()
        vertices, faces = ops.mesh_write(field, thr, aabb[:3], aabb[3:], ws, nv, nf)
        torch.cuda.synchronize(); t3 = time.perf_counter()
        M.vertex_colors(scene, vertices); M.vertex_normals(scene, vertices)
        torch.cuda.synchronize(); t4 = time.perf_counter()
        for k, v in zip(stages, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            stages[k].append(v)
        del field
    entry['extract_mesh_stages_s'] = {k: statistics.median(v[1:]) for k, v in stages.items()}
    entry['extract_mesh_total_s'] = sum(entry['extract_mesh_stages_s'].values())
    entry['lattice_corners_per_s'] = (res + 1) ** 3 / entry['extract_mesh_stages_s']['lattice_s']
    out['room'][str(res)] = entry
print(json.dumps(out, indent=1))
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def sparse_stages(res):
    """One extract_mesh_sparse, stage by stage as perf_amd/mesh.py runs it -> (seconds per stage, figures)."""
    est, nerf, shape = scene.estimator, scene.nerf, (res,) * 3
    t = {k: 0.0 for k in ('select_s', 'corners_s', 'density_s', 'count_s', 'write_s')}
    t0 = sync_clock()
    ids, table = M.select_bricks(est.binaries, shape)
    t1 = sync_clock(); t['select_s'] = t1 - t0
    m = int(ids.numel())
    values = torch.empty(m, 512, dtype=torch.float32, device='cuda')
    for first in range(0, m, 8192):
        count = min(8192, m - first)
        a = sync_clock()
        x01, sel, interior = ops.brickmesh_corners(ids, first, count, shape, est.binaries)
        b = sync_clock(); t['corners_s'] += b - a
        sigma = nerf.density_at(x01, interior).float()
        values[first:first + count] = torch.where(sel.bool(), sigma, torch.zeros_like(sigma)).view(count, 512)
        t['density_s'] += sync_clock() - b
    t2 = sync_clock()
    counts, ws = ops.brickmesh_count(values, ids, table, shape, thr, 0.0)
    nv, nf, bad = counts.tolist()
    t3 = time.perf_counter(); t['count_s'] = t3 - t2
    vertices, faces, cells = ops.brickmesh_write(values, ids, table, shape, thr, 0.0, aabb[:3], aabb[3:], ws, nv, nf)
    t['write_s'] = sync_clock() - t3
    held = values.numel() * 4 + ids.numel() * 4 + table.numel() * 4 + ws.numel() * 8 + vertices.numel() * 4 + faces.numel() * 4 + cells.numel() * 8
    return t, {'live_bricks': m, 'bricks': table.numel(), 'corners_evaluated': m * 512, 'share_of_lattice_corners': m * 512 / (res + 1) ** 3, 'vertices': nv, 'faces': nf,
               'violations': bad, 'bytes_held': held}


if args.sparse_resolutions:
    sparse = {'rounds': args.rounds, 'training': out['room']['training'], 'room': {}}
    for res in args.sparse_resolutions:
        rounds = [sparse_stages(res) for _ in range(args.rounds + 1)]          # (the first round is the warm-up)
        entry = dict(rounds[-1][1])
        entry['sparse_stages_s'] = {k: statistics.median(r[0][k] for r in rounds[1:]) for k in rounds[0][0]}
        entry['sparse_total_s'] = sum(entry['sparse_stages_s'].values())
        whole = []
        for _ in range(args.rounds + 1):
            t0 = sync_clock(); M.extract_mesh_sparse(scene, res); whole.append(sync_clock() - t0)
        entry['extract_mesh_sparse_s'] = statistics.median(whole[1:])
        if res <= 512:
            dense = []
            for _ in range(args.rounds + 1):
                t0 = sync_clock(); M.extract_mesh(scene, res); dense.append(sync_clock() - t0)
            entry['extract_mesh_dense_s'] = statistics.median(dense[1:])
        sparse['room'][str(res)] = entry
    print(json.dumps(sparse, indent=1))
    if args.sparse_out:
        json.dump(sparse, open(args.sparse_out, 'w'), indent=1)
