"""Dense fly-through rendering (core_exp_runner.py:223-246 `CoreRunner.render_dense`, BASELINE config 4) without the
image/video IO: a DenseTravelPoseSampler trajectory through the anchor poses, one frame per pose.  cam_type='pano' (the
reference's default): a 512x1024 panorama with the rotation reset to identity (:231-233); any other cam_type: a res x res
perspective frame of field of view fov that keeps the trajectory's look-at rotation (:235).  Every frame is ONE replay of a
hipGraph that holds ray generation from a device-resident pose plus the 32,768-ray eval batches of NeRFScene.render
(NeRFScene.make_graphed_render): no per-batch host work, sample counts stay on the device."""
import numpy as np
import torch

from .pose_sampler import DensePoseFuture, DenseTravelPoseSampler


@torch.no_grad()
def render_dense(scene, pose_sampler, n_poses=180, height=512, width=1024, query_keys=('rgb', 'distance'),
                 on_frame=None, max_frames=None, batch_size=32768, graphed=True, dense=None, cam_type='pano',
                 fov=np.deg2rad(75.), res=512):
    """Returns the list of per-frame result dicts (or calls on_frame(i, pose, result) and keeps nothing; the tensors
    handed to on_frame belong to the graph and are overwritten by the next frame).
    dense: a DenseTravelPoseSampler, or the DensePoseFuture of DenseTravelPoseSampler.start(pose_sampler, n_poses) issued
    earlier (e.g. before the scene was trained): the 10,000-step tour annealing has then run beside the GPU work and the
    frame loop starts at once.  Without it the trajectory is started here and the frame graph is captured meanwhile.
    height, width: the panorama's size (cam_type='pano'); fov (radians), res: the perspective frame's (any other cam_type).
    query_keys: any of 'rgb', 'distance', 'opacities', 'normal' (world-frame unit normals from the density gradient, [H, W, 3]; two more
    launches per batch, only when asked for)."""
    pano = cam_type == 'pano'
    if dense is None:
        dense = DenseTravelPoseSampler.start(pose_sampler, n_dense_poses=n_poses)
    fh, fw = (height, width) if pano else (res, res)
    frame_fn = scene.make_graphed_render(fh, fw, tuple(query_keys), batch_size=batch_size,
                                         fovy=None if pano else float(fov)) if graphed else None
    if isinstance(dense, DensePoseFuture):
        dense = dense.result()
    frames = []
    n = dense.n_poses if max_frames is None else min(dense.n_poses, max_frames)
    for i in range(n):
        pose = dense.sample_pose(i).clone().float()
        if pano:
            pose[:3, :3] = torch.eye(3, device=pose.device)                            # core_exp_runner.py:232
        if frame_fn is not None:
            out = frame_fn(pose)
        else:
            from .scene import Rays, gen_pano_rays, gen_pers_rays
            rays = gen_pano_rays(pose, height, width) if pano else gen_pers_rays(pose, fov, res)      # :233 / :235
            out = scene.render(Rays(rays.o, rays.d), query_keys=list(query_keys), batch_size=batch_size)
        if on_frame is not None:
            on_frame(i, pose, out)
        else:
            frames.append({k: v.clone() for k, v in out.items()} if frame_fn is not None else out)
    return frames
