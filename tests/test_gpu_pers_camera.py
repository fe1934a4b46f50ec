"""The perspective camera on the device: gen_pers_rays (utils/camera_utils.py:60-80, 237-241) as perf_pers_raygen(_dev), the
graph-captured perspective frame of NeRFScene.make_graphed_render(fovy=...), and render_dense for cam_type != 'pano'
(core_exp_runner.py:235), which keeps the trajectory's look-at rotation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FOV = float(np.deg2rad(75.))


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from perf_amd import ops as _ops
    return _ops


def _pers_torch(pose, fovy, height, width):
    """cam_rays_cam_space(height, width, fovy) + gen_pers_rays (camera_utils.py:60-80, 237-241) restated on the CPU, for any
    height x width (the oracle only takes square frames)."""
    span_y = np.tan(fovy * .5)
    span_x = span_y * (width / height)
    y = torch.linspace(-span_y, span_y, height)
    x = torch.linspace(-span_x, span_x, width)
    y, x = torch.meshgrid(y, x, indexing='ij')
    xyz = torch.stack([x, y, torch.ones_like(x)], -1)
    d = xyz / torch.linalg.norm(xyz, 2, -1, True)
    pose = torch.as_tensor(pose, dtype=torch.float32)
    o = torch.zeros_like(d) + pose[:3, 3][None, None, :]
    d = torch.matmul(pose[:3, :3], d[..., None])[..., 0]
    return o, d


def _look(to, t=(0., 0., 0.)):
    """A camera at t looking along `to` (camera_utils.look_at with the default up vector, as the dense trajectory builds it)."""
    from perf_amd.pose_sampler import look_at
    p = torch.eye(4)
    p[:3, :3] = look_at(torch.tensor([to], dtype=torch.float32))[0]
    p[:3, 3] = torch.tensor(t, dtype=torch.float32)
    return p


POSES = (_look((1., 0.3, 0.1), (0.02, -0.03, 0.01)), _look((-0.4, 1., -0.3), (0.1, -0.05, 0.02)),
         _look((0.2, -0.7, 0.6), (-0.15, 0.1, -0.04)))


def test_pers_raygen_matches_the_reference_golden(ops, golden_dir):
    g = np.load(f'{golden_dir}/rays.npz')
    for name in ('eye', 'rt'):
        pose = torch.from_numpy(g[f'pose_{name}'])
        o, d = ops.pers_raygen(pose, 64, 64, np.deg2rad(75.))
        assert o.shape == d.shape == (64, 64, 3)
        # the tolerance of test_pano_raygen: unit vectors, fp32 -> 2e-6 absolute
        assert np.abs(d.cpu().numpy() - g[f'pers_{name}_d']).max() < 2e-6
        assert np.array_equal(o.cpu().numpy(), g[f'pers_{name}_o'])


def test_pers_raygen_larger_and_non_square_frames(ops):
    from oracle import perf_oracle as O
    for pose in POSES:
        o, d = ops.pers_raygen(pose, 512, 512, FOV)
        o_ref, d_ref = O.pers_rays(pose, FOV, 512)
        assert (d.cpu() - d_ref).abs().max() < 2e-6
        assert torch.equal(o.cpu(), o_ref)
        for (h, w, fov) in ((384, 640, FOV), (640, 384, np.deg2rad(50.)), (257, 129, np.deg2rad(120.)), (2, 3, FOV)):
            o, d = ops.pers_raygen(pose, h, w, fov)
            o_ref, d_ref = _pers_torch(pose, fov, h, w)
            assert o.shape == d.shape == (h, w, 3)
            assert (d.cpu() - d_ref).abs().max() < 2e-6, (h, w)
            assert torch.equal(o.cpu(), o_ref)
            assert (d.norm(dim=-1) - 1).abs().max() < 1e-6
        # odd sizes: the centre pixel looks along the camera's forward axis, R (0, 0, 1)
        for (h, w) in ((63, 63), (257, 129), (5, 7)):
            _, d = ops.pers_raygen(pose, h, w, FOV)
            assert (d[h // 2, w // 2].cpu() - pose[:3, 2]).abs().max() < 1e-6


def test_pers_raygen_row_shards_and_device_pose(ops):
    pose = POSES[2]
    o1, d1 = ops.pers_raygen(pose, 300, 200, FOV)
    for row0, nrows in ((0, 1), (64, 32), (150, 150), (299, 1), (0, 300)):
        o2, d2 = ops.pers_raygen(pose, 300, 200, FOV, row0=row0, nrows=nrows)
        assert torch.equal(d1[row0:row0 + nrows], d2) and torch.equal(o1[row0:row0 + nrows], o2)
    pose_dev = pose.cuda()
    o3, d3 = ops.pers_raygen_dev(pose_dev, 300, 200, FOV)
    assert torch.equal(d3, d1) and torch.equal(o3, o1)
    # a [3, 4] device pose, one row shard, written into preallocated [nrows * W, 3] buffers (what a captured frame does)
    bufs = (torch.empty(32 * 200, 3, device='cuda'), torch.empty(32 * 200, 3, device='cuda'))
    ops.pers_raygen_dev(pose_dev[:3].contiguous(), 300, 200, FOV, row0=64, nrows=32, out=bufs)
    assert torch.equal(bufs[1].view(32, 200, 3), d1[64:96]) and torch.equal(bufs[0].view(32, 200, 3), o1[64:96])


def test_pers_raygen_refuses_bad_shapes(ops):
    from perf_amd._lib import PerfError
    pose = POSES[0]
    for (h, w) in ((1, 64), (64, 1), (0, 8)):
        with pytest.raises(PerfError, match='shape'):
            ops.pers_raygen(pose, h, w, FOV, nrows=1)
    for (row0, nrows) in ((-1, 4), (60, 5), (64, 1)):
        with pytest.raises(PerfError, match='shape'):
            ops.pers_raygen(pose, 64, 64, FOV, row0=row0, nrows=nrows)
    with pytest.raises(PerfError, match='fovy'):
        ops.pers_raygen_dev(pose.cuda(), 64, 64, np.pi)
    with pytest.raises(PerfError):
        ops.pers_raygen_dev(pose.cuda(), 64, 64, FOV, out=(torch.empty(64 * 63, 3, device='cuda'), torch.empty(64 * 64, 3, device='cuda')))
    # the panorama's shape check is unchanged
    with pytest.raises(PerfError, match='panorama'):
        ops.pano_raygen(pose, 64, 64, row0=60, nrows=5)


# ---- the graph-captured perspective frame and render_dense('pers') on a trained scene -----------------------------------
@pytest.fixture(scope='module')
def trained_scene():
    """Built as tests/test_gpu_config4.py builds its scene: the synthetic room, trained from one 256x512 panorama at the origin."""
    from perf_amd import synthetic
    from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays
    torch.manual_seed(0); np.random.seed(0)
    scene = NeRFScene(dtype='fp16')
    rays = gen_pano_rays(torch.eye(4), 256, 512)
    dist, rgb = synthetic.room(rays.d)
    pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
    scene.train_conf.pixel_loss_batch_size = 4096
    scene.train_one_episode(pool, 150, 100)
    return scene, pool, dist, rays


def _assert_frame_equals(got, ref, h, w):
    for k in ref:
        assert got[k].shape == ref[k].shape == (h, w, ref[k].shape[-1]), k
        assert torch.equal(got[k], ref[k]), k


def test_graphed_pers_frame_equals_eager_render(trained_scene, ops):
    from perf_amd.scene import Rays, gen_pers_rays
    scene = trained_scene[0]
    keys = ('rgb', 'distance', 'opacities')
    for (h, w, batch) in ((128, 128, 32768), (256, 256, 16384), (96, 160, 4096)):     # one batch; four; a non-square frame in four
        frame = scene.make_graphed_render(h, w, keys, batch_size=batch, fovy=FOV)
        for pose in POSES:
            got = {k: v.clone() for k, v in frame(pose).items()}
            if h == w:
                rays = gen_pers_rays(pose, FOV, h)
            else:
                rays = Rays(*ops.pers_raygen(pose, h, w, FOV))
            ref = scene.render(rays, list(keys), batch_size=batch, sync_free=False)        # the synced reference path
            _assert_frame_equals(got, ref, h, w)
            assert torch.isfinite(got['rgb']).all() and torch.isfinite(got['distance']).all()
            assert float(got['opacities'].min()) >= 0.0 and float(got['opacities'].max()) <= 1.0 + 1e-4
            again = frame(pose)                                                           # a replay is deterministic
            assert torch.equal(again['rgb'], got['rgb']) and torch.equal(again['distance'], got['distance'])
        # the rotation turns the camera: same position, another look-at direction, another frame
        turned = POSES[0].clone(); turned[:3, :3] = POSES[1][:3, :3]
        seen = frame(turned)['rgb'].clone()
        assert not torch.equal(seen, frame(POSES[0])['rgb'])


def test_graphed_pers_frame_recaptures_when_the_capacity_is_too_small(trained_scene):
    from perf_amd.scene import gen_pers_rays
    scene = trained_scene[0]
    pose = POSES[1]
    ref = scene.render(gen_pers_rays(pose, FOV, 96), ['rgb', 'distance'], batch_size=4096, sync_free=False)
    frame = scene.make_graphed_render(96, 96, ('rgb', 'distance'), batch_size=4096, samples_per_ray=1, fovy=FOV)
    got = frame(pose)
    assert frame.state['per_ray'] > 1
    _assert_frame_equals(got, ref, 96, 96)


def test_render_dense_pers_keeps_the_look_at_rotation(trained_scene):
    from perf_amd.pose_sampler import CirclePoseSampler, DenseTravelPoseSampler
    from perf_amd.scene import gen_pano_rays, gen_pers_rays
    from perf_amd.traverse import render_dense
    scene, pool, dist, _ = trained_scene
    sparse = CirclePoseSampler(dist.reshape(256, 512).cpu(), traverse_ratios=[.2, .4, .6], n_anchors_per_ratio=[8, 8, 8])
    dense = DenseTravelPoseSampler(sparse, n_dense_poses=24)
    res = 64
    frames = render_dense(scene, sparse, n_poses=24, max_frames=4, dense=dense, cam_type='pers', fov=FOV, res=res,
                          query_keys=('rgb', 'distance'))
    eager = render_dense(scene, sparse, n_poses=24, max_frames=4, dense=dense, cam_type='pers', fov=FOV, res=res,
                         query_keys=('rgb', 'distance'), graphed=False)
    assert len(frames) == len(eager) == 4
    for i, (f, e) in enumerate(zip(frames, eager)):
        pose = dense.sample_pose(i).clone().float()
        assert (pose[:3, :3] - torch.eye(3)).abs().max() > 0.1                  # a real look-at rotation
        ref = scene.render(gen_pers_rays(pose, FOV, res), ['rgb', 'distance'], batch_size=32768, sync_free=False)
        _assert_frame_equals(f, ref, res, res)
        _assert_frame_equals(e, ref, res, res)
        reset = pose.clone(); reset[:3, :3] = torch.eye(3)                       # the panorama's reset must not leak in
        assert not torch.equal(f['rgb'], scene.render(gen_pers_rays(reset, FOV, res), ['rgb'], batch_size=32768, sync_free=False)['rgb'])
    # the default camera is the panorama, exactly as before
    pano = render_dense(scene, sparse, n_poses=24, height=64, width=128, max_frames=2, dense=dense)
    pano_kw = render_dense(scene, sparse, n_poses=24, height=64, width=128, max_frames=2, dense=dense, cam_type='pano')
    for i, (a, b) in enumerate(zip(pano, pano_kw)):
        pose = dense.sample_pose(i).clone().float(); pose[:3, :3] = torch.eye(3)
        ref = scene.render(gen_pano_rays(pose, 64, 128), ['rgb', 'distance'], batch_size=32768, sync_free=False)
        _assert_frame_equals(a, ref, 64, 128)
        _assert_frame_equals(b, ref, 64, 128)


def test_pers_frame_sees_the_room(trained_scene):
    """From the origin, the frame's distances are the room's analytic distances along its own rays (the bound config 4 uses
    for panoramas)."""
    from perf_amd import synthetic
    from perf_amd.scene import gen_pers_rays
    scene, _, dist, pano = trained_scene
    res = 128
    frame = scene.make_graphed_render(res, res, ('distance',), fovy=FOV)
    pano_d = pano.d.reshape(-1, 3)
    for to in ((1., 0., 0.), (0., 1., 0.), (-1., 0.5, 0.2), (0.3, -0.2, -0.9)):
        pose = _look(to)
        rays = gen_pers_rays(pose, FOV, res)
        # synthetic.room divides by 1.05x the farthest distance among the rays it is given, the supervision by that of the training
        # panorama: evaluated with the panorama's rays in front, the frame's distances are scaled back to the supervision's units
        both, _ = synthetic.room(torch.cat([pano_d, rays.d.reshape(-1, 3)]))
        ref = (both[len(pano_d):] * (dist.max() / both[:len(pano_d)].max())).reshape(res, res, 1)
        got = frame(pose)['distance']
        assert float((got - ref).abs().mean()) < 0.05, to
