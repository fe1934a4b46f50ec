"""Rays against the extracted mesh (include/perf_hip_meshray.h) on the trained analytic room of tools/meshvis_bench.py: what the grid
costs, what the occlusion test adds to the cull, how fast a distance panorama of the mesh is, and how far it lies from the field's own.

  python tools/meshray_bench.py [--rounds 5] [--dense-resolutions 256] [--sparse-resolutions 1024] [--out profiles/meshray.json]

Views as in tools/meshvis_bench.py: K = 1, the panorama the room is trained on, and K = 25.  Per resolution: the grid (host-clock seconds of
build_ray_grid that end in a device synchronise, its cells, bytes and references per face); per K: cull_occluded beside cull_unseen on the
same mesh (medians of `rounds` after a warm-up), the device milliseconds of each entry point of one more cull, and the occlusion segments
per second (a segment per set bit of the visibility).  Then render_mesh_distance of a 512 x 1024 panorama from the origin: seconds, the
closest-hit kernel's rays per second, and the median / 90th percentile of |mesh distance - the field's rendered 'distance'| over the rays
both hit.  At the first dense resolution the same kernel on a 1 x 1 x 1 grid (brute force) on a ray subset shows what the grid buys.  The
compiler's resource report of the unit's kernels (VGPRs, occupancy, scratch) is recorded beside the timings."""
import argparse, json, math, os, re, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import build as B
from perf_amd import mesh as M
from perf_amd import ops, synthetic
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--dense-resolutions', type=int, nargs='*', default=[256])
ap.add_argument('--sparse-resolutions', type=int, nargs='*', default=[1024])
ap.add_argument('--geo', type=int, default=150)
ap.add_argument('--app', type=int, default=100)
ap.add_argument('--brute-rays', type=int, default=8192)
ap.add_argument('--out', default=None)
args = ap.parse_args()
HALF = (0.9, 0.7, 0.5)


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def median_s(fn, rounds):
    times = []
    for _ in range(rounds + 1):                      # (the first round is the warm-up)
        t0 = sync_clock(); fn(); times.append(sync_clock() - t0)
    return statistics.median(times[1:])


def resource_report():
    """{kernel: {vgprs, sgprs, occupancy_waves_per_simd, scratch_bytes_per_lane, lds_bytes}} from the compiler's remarks, None without hipcc."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc] + B.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(B.CSRC, 'meshray.hip'), '-o', os.devnull]
    try:
        text = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.TimeoutExpired):
        return None
    out, name = {}, None
    keys = {'VGPRs': 'vgprs', 'TotalSGPRs': 'sgprs', 'Occupancy [waves/SIMD]': 'occupancy_waves_per_simd', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane',
            'LDS Size [bytes/block]': 'lds_bytes'}
    for line in text.splitlines():
        m = re.search(r'remark:\s+Function Name: (\S+)', line)
        if m:
            name = re.sub(r'^_ZN4perf\d+', '', m.group(1))
            name = re.match(r'[a-z_]+', name).group(0) + ('<any>' if 'ILb1E' in m.group(1) else '<closest>' if 'ILb0E' in m.group(1) else '')
            out[name] = {}
        for key, short in keys.items():
            m = re.search(r'remark:\s+' + re.escape(key) + r': (\d+)', line)
            if m and name:
                out[name][short] = int(m.group(1))
    return out or None


def grid_entry(mesh, grid, seconds):
    cells = grid.dims[0] * grid.dims[1] * grid.dims[2]
    refs = int(grid.refs.numel())
    return {'build_s': seconds, 'cell': grid.cell, 'dims': list(grid.dims), 'cells': cells, 'references': refs, 'references_per_face': refs / max(grid.n_faces, 1),
            'bytes': {'counts_transient': 4 * cells, 'offsets': 4 * cells, 'refs': 4 * refs, 'kept': 4 * cells + 4 * refs}, 'bad_face': grid.bad_face}


def measure(res, sparse, brute):
    mesh = M.extract_mesh_sparse(scene, res) if sparse else M.extract_mesh(scene, res)
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    entry = {'path': 'extract_mesh_sparse' if sparse else 'extract_mesh', 'vertices': V, 'faces': F, 'views': {}}
    grid = M.build_ray_grid(mesh)
    entry['grid'] = grid_entry(mesh, grid, median_s(lambda: M.build_ray_grid(mesh), args.rounds))
    for name, views in (('1', views_1), ('25', views_25)):
        k = len(views)
        e = {'cull_occluded_s': median_s(lambda: M.cull_occluded(mesh, views), args.rounds), 'cull_unseen_s': median_s(lambda: M.cull_unseen(mesh, views), args.rounds)}
        e['occluded_over_unseen'] = e['cull_occluded_s'] / e['cull_unseen_s']
        ops.start_kernel_timing()                    # device milliseconds per entry point of one more cull
        culled = M.cull_occluded(mesh, views)
        e['device_ms'] = {key: v[1] for key, v in ops.stop_kernel_timing().items()}
        visibility = M.vertex_visibility(mesh.vertices, views)
        occluded = M.vertex_occlusion(mesh, grid, views, visibility)
        popcount = lambda bits: int(sum(((bits >> b) & 1).sum() for b in range(k)))
        e['segments'], e['segments_occluded'] = popcount(visibility.visible), popcount(occluded)
        e['segments_per_s'] = e['segments'] / (e['device_ms']['perf_meshray_occluded'] * 1e-3)
        unseen = M.cull_unseen(mesh, views)
        e['faces_kept'] = {'cull_unseen': int(unseen.faces.shape[0]), 'cull_occluded': int(culled.faces.shape[0]),
                           'cull_unseen_no_facing': int(M.cull_unseen(mesh, views, facing=False).faces.shape[0]),
                           'cull_occluded_no_facing': int(M.cull_occluded(mesh, views, facing=False).faces.shape[0])}
        entry['views'][name] = e
        if name == '1':
            kept = culled
    # the distance panorama of the mesh beside the field's
    pano = gen_pano_rays(torch.eye(4), 512, 1024)
    n_rays = 512 * 1024
    p = {'rays': n_rays, 'render_mesh_distance_s': median_s(lambda: scene.render_mesh_distance(mesh, pano, grid), args.rounds)}
    ops.start_kernel_timing()
    mesh_d = scene.render_mesh_distance(mesh, pano, grid)
    p['cast_ms'] = ops.stop_kernel_timing()['perf_meshray_cast'][1]
    p['closest_hit_rays_per_s'] = n_rays / (p['cast_ms'] * 1e-3)
    field_d = scene.render(pano, query_keys=['distance'])['distance']
    assert mesh_d.shape == field_d.shape
    for label, m in (('raw_mesh', mesh), ('cull_occluded_1_view', kept)):
        d = scene.render_mesh_distance(m, pano) if m is not mesh else mesh_d
        hit = d != 5.0
        diff = (d - field_d).abs()[hit].double().cpu().numpy()          # (float64 on the host: the quantiles of exactly the rays that hit)
        values, counts = np.unique(diff, return_counts=True)          # (ties: how many rays share one difference, and how many the median's)
        top = int(counts.argmax()) if diff.size else 0
        p[label] = {'rays_hit': int(hit.sum()), 'rays_differing_from_raw_mesh': int((d != mesh_d).sum()), 'distinct_differences': int(values.size),
                    'most_common_difference': [float(values[top]), int(counts[top])] if diff.size else None,
                    'rays_at_the_median_difference': int((diff == np.quantile(diff, 0.5)).sum()) if diff.size else 0,
                    'rays_at_the_p90_difference': int((diff == np.quantile(diff, 0.9)).sum()) if diff.size else 0,
                    'rays_with_distinct_field_distance': int(torch.unique(field_d[hit]).numel()), 'rays_with_distinct_mesh_distance': int(torch.unique(d[hit]).numel()),
                    'abs_difference_mean': float(diff.mean()) if diff.size else None, 'abs_difference_max': float(diff.max()) if diff.size else None,
                    'abs_difference_p50_p90': [float(np.quantile(diff, q)) for q in (0.5, 0.9)] if diff.size else None}
    entry['panorama_512x1024'] = p
    # the worst case of the one-thread-per-face passes: one more face as large as the box, which one lane lists in every cell
    lo, hi = mesh.vertices.min(dim=0).values, mesh.vertices.max(dim=0).values
    corners = torch.stack([lo, torch.stack([hi[0], lo[1], hi[2]]), torch.stack([lo[0], hi[1], hi[2]])])
    big = M.Mesh(torch.cat([mesh.vertices, corners]).contiguous(), torch.cat([mesh.faces, torch.tensor([[V, V + 1, V + 2]], dtype=torch.int32, device=mesh.faces.device)]).contiguous())
    big_grid = M.build_ray_grid(big, grid.cell)
    entry['grid_with_one_box_sized_face'] = {'build_s': median_s(lambda: M.build_ray_grid(big, grid.cell), args.rounds), 'dims': list(big_grid.dims),
                                             'references': int(big_grid.refs.numel()), 'same_cell_build_s': entry['grid']['build_s']}
    del big, big_grid
    if brute:                                        # the same kernel on a grid of one cell: every ray tests every face
        o, d = pano.o.reshape(-1, 3), pano.d.reshape(-1, 3)
        pick = torch.randperm(n_rays, device=o.device)[:args.brute_rays]
        o, d = o[pick].contiguous(), d[pick].contiguous()
        longest = float((mesh.vertices.max(dim=0).values - mesh.vertices.min(dim=0).values).max())
        one = M.build_ray_grid(mesh, 4 * longest)
        assert one.dims == (1, 1, 1)
        b = {'rays': int(o.shape[0]), 'grid_s': median_s(lambda: M.cast_rays(mesh, grid, o, d), args.rounds), 'one_cell_s': median_s(lambda: M.cast_rays(mesh, one, o, d), 2)}
        b['one_cell_over_grid'] = b['one_cell_s'] / b['grid_s']
        a, c = M.cast_rays(mesh, grid, o, d), M.cast_rays(mesh, one, o, d)
        b['results_bit_equal'] = bool(all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, c)))
        entry['brute_force'] = b
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
for _ in range(24):                                  # 24 further positions inside the room, as tools/meshvis_bench.py places them
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor(rng.uniform(-0.6, 0.6, 3) * np.array(HALF) / synthetic.ROOM_SCALE, dtype=torch.float32)
    r = gen_pano_rays(pose, 128, 256)
    d, _ = synthetic.room_with_box(r.o, r.d, box_h=(0.0, 0.0, 0.0))
    views_25.append({'pose': pose, 'distance_map': d.reshape(128, 256).float().cuda().contiguous()})
out = {'rounds': args.rounds, 'training': {'geo_iterations': args.geo, 'app_iterations': args.app, 'threshold': math.log(2.0) / scene.renderer.render_step_size},
       'kernel_resources': resource_report(), 'room': {}}
first = True
for res, sparse in [(r, False) for r in args.dense_resolutions] + [(r, True) for r in args.sparse_resolutions]:
    out['room'][str(res)] = measure(res, sparse, first and not sparse)
    first = False
    print(json.dumps({str(res): out['room'][str(res)]}), flush=True)
if args.out:
    json.dump(out, open(args.out, 'w'), indent=1)
    open(args.out, 'a').write('\n')
