"""BASELINE config 4 (render_dense, core_exp_runner.py:223-247): a dense camera trajectory through a trained scene,
512x1024 panoramic frames (--cam-type pano, the reference's default: rotation reset to identity) or res x res perspective
frames of a 75-degree field of view that keep the trajectory's look-at rotation (--cam-type pers, the reference's
gen_pers_rays branch), fp16 inference, reference-faithful variable-count sampling.

  python tools/render_dense.py [--poses 600] [--geo-steps 300] [--app-steps 150] [--cam-type pers [--fov-deg 75] [--res 512]] [--normals]

Frames are rendered back to back on the device (the reference writes PNGs and a video in between: host IO, out of
scope); prints the camera, frames/s (--normals: also with the 'normal' query key, the two graphs alternated), rays/s, ray-samples/s actually evaluated, and a checksum of the frames."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import ops, synthetic
from perf_amd.pose_sampler import CirclePoseSampler, DenseTravelPoseSampler
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays, gen_pers_rays

ap = argparse.ArgumentParser()
ap.add_argument('--poses', type=int, default=600)
ap.add_argument('--geo-steps', type=int, default=300)
ap.add_argument('--app-steps', type=int, default=150)
ap.add_argument('--dtype', default='fp16')
ap.add_argument('--head', type=int, default=2, help='two-phase sampler: density first on that many samples per ray (0 = one phase)')
ap.add_argument('--batch', type=int, default=32768, help='rays per graph-captured eval batch (the reference hard-codes 32768, nerf.py:86)')
ap.add_argument('--cam-type', choices=('pano', 'pers'), default='pano', help="the reference's render_dense(cam_type=...): 'pano' or a perspective frame")
ap.add_argument('--fov-deg', type=float, default=75., help='field of view of the perspective frames (core_exp_runner.py:235)')
ap.add_argument('--res', type=int, default=512, help='side of the square perspective frames (core_exp_runner.py:235)')
ap.add_argument('--normals', action='store_true', help="also render ('rgb', 'distance', 'normal') frames and report frames/s with and without the key")
args = ap.parse_args()

torch.manual_seed(0); np.random.seed(0)
scene = NeRFScene(dtype=args.dtype)
H, W = 1024, 2048
rays = gen_pano_rays(torch.eye(4), H, W)
dist, rgb = synthetic.room(rays.d)
pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
# The anchors only need the panorama's distance map: the dense trajectory (10,000-step tour annealing on the host, 0.2 s) is
# started in a worker process NOW and runs beside the training below (off config 4's critical path)
sparse = CirclePoseSampler(dist.reshape(H, W).cpu(), traverse_ratios=[.2, .4, .6], n_anchors_per_ratio=[8, 8, 8])
rng0 = np.random.get_state()
t0 = time.perf_counter()
dense_future = DenseTravelPoseSampler.start(sparse, n_dense_poses=args.poses)
t_start_call = time.perf_counter() - t0
scene.set_train(); scene.prepare_occupancy(pool)
tc = scene.train_conf
scene.nerf.reset_geo()
opt = scene.make_optimizer(scene.nerf.geo_mlp, 0.0)
for i in range(args.geo_steps):
    scene.update_lr(opt, tc.geo_optimizer, i / args.geo_steps)
    scene.train_one_step_geo(opt, pool, progress=i / args.geo_steps)
opt = scene.make_optimizer(scene.nerf.app_mlp, 0.0)
for i in range(args.app_steps):
    scene.update_lr(opt, tc.app_optimizer, i / args.app_steps)
    scene.train_one_step_app(opt, pool, progress=i / args.app_steps)
torch.cuda.synchronize()

# pose samplers run on the host (utils of the reference, restated in perf_amd/pose_sampler.py)
t0 = time.perf_counter()
dense = dense_future.result()                                       # (finished long ago: it ran beside the training)
t_wait = time.perf_counter() - t0
from perf_amd import pose_sampler as _ps
_ps._DENSE_CACHE.clear(); rng1 = np.random.get_state(); np.random.set_state(rng0)
t0 = time.perf_counter()
dense_seq = DenseTravelPoseSampler(sparse, n_dense_poses=args.poses)   # the same trajectory computed in line, for the record
t_sampler = time.perf_counter() - t0
assert torch.equal(dense_seq.sample_poses, dense.sample_poses) and np.array_equal(np.random.get_state()[1], rng1[1])
pano = args.cam_type == 'pano'
fov = float(np.deg2rad(args.fov_deg))
poses = []
for i in range(dense.n_poses):
    p = dense.sample_pose(i).clone().float()
    if pano:
        p[:3, :3] = torch.eye(3)                                    # core_exp_runner.py:232 (a perspective frame keeps it, :235)
    poses.append(p)

fh, fw = (512, 1024) if pano else (args.res, args.res)
def frame_rays(p):
    return gen_pano_rays(p, fh, fw) if pano else gen_pers_rays(p, fov, args.res)
def frame_eager(p):
    return scene.render(frame_rays(p), ['rgb', 'distance'], batch_size=args.batch)

# ONE hipGraph per frame: ray generation from a device-resident pose + the eval batches of 32,768 rays (nerf.py:86)
scene.renderer.head_samples = args.head or None
frame = scene.make_graphed_render(fh, fw, ('rgb', 'distance'), batch_size=args.batch, fovy=None if pano else fov)
for p in poses[:3]:
    frame(p)
torch.cuda.synchronize()
ref = frame_eager(poses[1]); got = frame(poses[1])
same = bool(torch.equal(ref['rgb'], got['rgb']) and torch.equal(ref['distance'], got['distance']))
ops.start_kernel_timing()
frame_eager(poses[0]); torch.cuda.synchronize()
kern = ops.stop_kernel_timing()
t0 = time.perf_counter()
for p in poses:
    last = frame(p)
torch.cuda.synchronize()
t = time.perf_counter() - t0
checksum = float(last['rgb'].double().sum())
t0 = time.perf_counter()
for p in poses[:60]:
    frame_eager(p)
torch.cuda.synchronize()
t_eager = (time.perf_counter() - t0) / 60
normals = None
if args.normals:
    # the same trajectory with the 'normal' key, a graph of its own; the two graphs alternated twice so that both see the same box state
    frame_n = scene.make_graphed_render(fh, fw, ('rgb', 'distance', 'normal'), batch_size=args.batch, fovy=None if pano else fov)
    for p in poses[:3]:
        frame_n(p)
    torch.cuda.synchronize()
    def timed(fn):
        t0 = time.perf_counter()
        for p in poses:
            out = fn(p)
        torch.cuda.synchronize()
        return len(poses) / (time.perf_counter() - t0), out
    fps = {'without': [], 'with': []}
    for _ in range(2):
        fps['without'].append(timed(frame)[0])
        f, last_n = timed(frame_n)
        fps['with'].append(f)
    plain = frame(poses[-1])
    nn = last_n['normal']
    len_n = torch.linalg.vector_norm(nn, dim=-1)
    normals = {'frames_per_s_without_normal': fps['without'], 'frames_per_s_with_normal': fps['with'],
               'rgb_and_distance_equal_without_the_key': bool(torch.equal(plain['rgb'], last_n['rgb']) and torch.equal(plain['distance'], last_n['distance'])),
               'last_frame_unit_or_zero': bool((((len_n - 1).abs() < 1e-5) | (len_n == 0)).all()),
               'last_frame_rays_with_a_normal': float((len_n > 0).float().mean()),
               'last_frame_mean_minus_dir_dot_normal': float((-(frame_rays(poses[-1]).d.reshape(-1, 3)) * nn.reshape(-1, 3)).sum(-1)[len_n.reshape(-1) > 0].mean())}
from perf_amd.scene import Rays as _Rays
# sample counts of every frame of the trajectory, rendered once more outside the timed loop: the samples whose density was
# evaluated (the two-phase sampler's head samples + the tails of the rays still alive) and the samples kept by the visibility
# compaction (what the colour field and the compositing evaluate)
scene.set_eval(); scene.renderer.sample_capacity = fh * fw * 64
_counts = []
with torch.no_grad():
    for p in poses:
        _r = frame_rays(p)
        _c = scene.render_once(_Rays(_r.o.reshape(-1, 3), _r.d.reshape(-1, 3)), ['n_marched_dev', 'n_samples_dev'])
        _counts.append(torch.stack([_c['n_marched_dev'].reshape(()), _c['n_samples_dev'].reshape(())]))
_counts = torch.stack(_counts).cpu()
scene.renderer.sample_capacity = None
marched_total, kept_total = (int(v) for v in _counts.sum(0))
print(json.dumps({'config': 'render_dense: %d poses, %dx%d %s frames in %d hipGraph-captured %d-ray batches, %s, variable-count sampling' % (len(poses), fw, fh, 'panoramic' if pano else 'perspective', (fh * fw + args.batch - 1) // args.batch, args.batch, args.dtype),
                  'camera': args.cam_type, 'fov_deg': None if pano else args.fov_deg, 'frame_hw': [fh, fw],
                  'frame0_marched_samples': int(_counts[0, 0]), 'frame0_kept_samples': int(_counts[0, 1]),
                  'frames_per_s': len(poses) / t, 'rays_per_s': len(poses) * fh * fw / t, 'seconds': t,
                  'ray_samples_per_s': {'density_evaluated': marched_total / t, 'kept': kept_total / t},
                  'samples_per_ray': {'density_evaluated': marched_total / (len(poses) * fh * fw), 'kept': kept_total / (len(poses) * fh * fw)},
                  'count_capacity_exceeded': bool((_counts[:, 0] > fh * fw * 64).any()),
                  'eager_sync_free_frames_per_s': 1.0 / t_eager, 'graphed_frame_equals_eager_frame': same,
                  'per_ray_sample_capacity': frame.state['per_ray'], 'head_samples': args.head,
                  'pose_sampler_host_s': t_sampler, 'pose_sampler_start_call_s': t_start_call, 'pose_sampler_wait_s': t_wait,
                  'wall_s_including_sampler': {'overlapped (started before training, as this tool does)': t + t_start_call + t_wait,
                                               'in line (round 2)': t + t_sampler},
                  'last_frame_rgb_sum': checksum, 'normals': normals,
                  'kernel_ms_one_frame': {k: round(n * ms, 3) for k, (n, ms) in sorted(kern.items(), key=lambda kv: -kv[1][0] * kv[1][1])}}, indent=1))
