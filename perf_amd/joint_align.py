"""The alignment loop of PeRF's PanoJointPredictor (modules/geo_predictors/pano_joint_predictor.py:101-305) around the fused
SphereDistanceField: 2 x 1500 Adam iterations that align 60 perspective depth / normal predictions on one distance field over the
sphere.  The field's part of an iteration was two kernels already (include/perf_hip_sphere.h); this module takes the rest of the
iteration -- three grid_samples with their backward scatters, the panorama look-up, two losses with the tangent construction, four
total-variation terms over 11.8 M map entries -- from about seventy torch launches to the kernels of include/perf_hip_joint.h.

One iteration (P views, B samples per view, N = P B; grid_sample is bilinear, align_corners=False, padding_mode='border'):

    s  = grid_sample(sup [P,7,R,R], coords)            direction (3), predicted distance (1), predicted normal (3)
    db = grid_sample(bias_d [P,1,R,R], coords),  nb = grid_sample(bias_n [P,3,Rn,Rn], coords)
    u  = unit(s[0:3]);  rd = s[3] softplus(scale_p) + db;  rn = unit(s[4:7] + nb)
    (pr, pm) = ref [2,H,W] (distance, mask) looked up at u (border padding, no wrap at the seam)
    (d, g) = field(u, requires_grad=True)
    L_d   = smooth-L1_0.5(rd, d)
    L_n   = smooth-L1_0.5((v_a . rn, v_b . rn), 0),   v_t = unit((g . t) u + t),  b = unit(u x o),  a = unit(b x u),  o = randn
    L_reg = (mean softplus(scale) - 1)^2
    L_ref = mean(smooth-L1_0.01(pr, d) [pm < 1/2])
    TV(m) = smooth-L1_0.01(m[:,:,1:,:], m[:,:,:-1,:]) + smooth-L1_0.01(m[:,:,:,1:], m[:,:,:,:-1])        ('hybrid' phase only)
    loss  = 20 progress L_ref + L_d + w_reg L_reg + w_n L_n + TV(bias_d) + w_ntv TV(bias_n)

align_step_composed is that iteration in plain torch (any dtype: in float64 it is the tests' yardstick; in float32 the fallback);
align_step is the same iteration on the kernels.  Neither draws, zeroes gradients or steps an optimiser: JointAligner does."""
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .visibility import direction_to_img_coord, img_coord_to_sample_coord

LOSS_NAMES = ('distance', 'normal', 'reg', 'ref', 'tv_distance', 'tv_normal', 'total')      # the loss block of perf_joint_loss, in its order
RECORD_FIELDS = {'sd': slice(0, 1), 'db': slice(1, 2), 'sn': slice(2, 5), 'nb': slice(5, 8), 'pr': slice(8, 9), 'pm': slice(9, 10)}


class AlignStep(NamedTuple):
    """What one iteration leaves behind: losses (dict over LOSS_NAMES of 0-d tensors), the directions u [N,3], the per-sample record
    (dict over RECORD_FIELDS: [N,1] or [N,3]) and the upstreams dd = d loss/d d [N], dg = d loss/d g [N,3] handed to the field."""
    losses: dict
    u: torch.Tensor
    record: dict
    dd: torch.Tensor
    dg: torch.Tensor


def _unit(x):
    return x / torch.linalg.norm(x, 2, -1, True)


def _tv(m):
    return F.smooth_l1_loss(m[:, :, 1:, :], m[:, :, :-1, :], beta=1e-2) + F.smooth_l1_loss(m[:, :, :, 1:], m[:, :, :, :-1], beta=1e-2)


def _sample_views(sup, coords):
    """(s [P,B,7], u [P,B,3]): the supervision sampled at the draws and its direction channels normalised -- ONE statement of these
    torch ops for both paths, so that both hand the field the same bits (see align_step)."""
    P, B = coords.shape[0], coords.shape[1]
    s = F.grid_sample(sup, coords.reshape(P, B, 1, 2), padding_mode='border', align_corners=False)[:, :, :, 0].permute(0, 2, 1)
    return s, _unit(s[..., :3])


def align_step_composed(field, sup, ref, scale, bias_d, bias_n, coords, ortho, progress, hybrid, reg_loss_weight=1e-1,
                        normal_loss_weight=1e-2, normal_tv_loss_weight=1e-2):
    """One iteration in plain torch, in the dtype of its inputs, loss.backward() included: the gradients ACCUMULATE in .grad of the
    field's parameters, of scale and -- in both phases, as autograd has it -- of the two maps (the caller zeroes what it steps).
    field: a callable (u [N,3], requires_grad=True) -> (d [N], g [N,3]) that keeps its graph; coords: [P,B,1,2]; ortho: [P,B,3]."""
    P, B = coords.shape[0], coords.shape[1]
    grid = coords.reshape(P, B, 1, 2)
    s, u = _sample_views(sup, coords)                                                                                  # [P, B, 7], [P, B, 3]
    db = F.grid_sample(bias_d, grid, padding_mode='border', align_corners=False)[:, :, :, 0].permute(0, 2, 1)        # [P, B, 1]
    nb = F.grid_sample(bias_n, grid, padding_mode='border', align_corners=False)[:, :, :, 0].permute(0, 2, 1)        # [P, B, 3]
    rd = s[..., 3:4] * F.softplus(scale[:, None, None]) + db
    rn = _unit(s[..., 4:] + nb)
    d, g = field(u.reshape(-1, 3), requires_grad=True)
    d, g = d.reshape(P, B, 1), g.reshape(P, B, 3)
    if d.requires_grad:
        d.retain_grad()
        g.retain_grad()
    l_d = F.smooth_l1_loss(rd, d, beta=5e-1, reduction='mean')
    b = _unit(torch.linalg.cross(u, ortho))
    a = _unit(torch.linalg.cross(b, u))
    v_a = _unit((g * a).sum(-1, True) * u + a)
    v_b = _unit((g * b).sum(-1, True) * u + b)
    errors = torch.cat([(v_a * rn).sum(-1, True), (v_b * rn).sum(-1, True)], -1)
    l_n = F.smooth_l1_loss(errors, torch.zeros_like(errors), beta=5e-1, reduction='mean')
    l_reg = (F.softplus(scale).mean() - 1.) ** 2
    zero = torch.zeros((), dtype=sup.dtype, device=sup.device)
    tv_d, tv_n = (_tv(bias_d), _tv(bias_n)) if hybrid else (zero, zero)
    sc = img_coord_to_sample_coord(direction_to_img_coord(u.reshape(-1, 3)))
    looked = F.grid_sample(ref[None], sc[None, :, None, :], padding_mode='border', align_corners=False)              # [1, 2, N, 1]
    pr, pm = looked[0, 0].reshape(-1), looked[0, 1].reshape(-1)
    l_ref = (F.smooth_l1_loss(pr, d.reshape(-1), beta=1e-2, reduction='none') * (pm < .5)).mean()
    loss = l_ref * 20. * progress + l_d + l_reg * reg_loss_weight + l_n * normal_loss_weight + tv_d * 1. + tv_n * normal_tv_loss_weight
    if loss.requires_grad:
        loss.backward()
    losses = dict(zip(LOSS_NAMES, (l_d, l_n, l_reg, l_ref, tv_d, tv_n, loss)))
    record = {'sd': s[..., 3:4], 'db': db, 'sn': s[..., 4:], 'nb': nb, 'pr': pr[:, None], 'pm': pm[:, None]}
    none = lambda t: None if t.grad is None else t.grad.reshape(P * B, -1)
    return AlignStep({k: v.detach() for k, v in losses.items()}, u.detach().reshape(-1, 3), {k: v.detach().reshape(P * B, -1) for k, v in record.items()},
                     None if none(d) is None else none(d)[:, 0], none(g))


class StepScratch:
    """The scratch memory of align_step, kept between iterations by its owner (JointAligner)."""

    def __init__(self):
        self.loss, self.tv = ops.Workspace(), ops.Workspace()
        self.tv_values = None


def align_step(field, sup, ref, scale, bias_d, bias_n, coords, ortho, progress, hybrid, reg_loss_weight=1e-1, normal_loss_weight=1e-2,
               normal_tv_loss_weight=1e-2, scratch=None):
    """The same iteration on the kernels of include/perf_hip_joint.h, all fp32: perf_joint_sample -> field(u, requires_grad=True) ->
    perf_joint_loss -> torch.autograd.backward([d, g], [dd, dg]) into the field's parameters (accumulated, as autograd does).
    The directions u are formed by the torch ops of align_step_composed (_sample_views: three small launches) and handed to the
    kernel, not formed in it: the field is steep in u -- on its finest levels (resolution 2048) an fp32 ulp of u moves g by 1e-4 of
    itself -- and the loop amplifies such a difference, so a kernel that rounds u its own way (even correctly) trains to a visibly
    different field than the torch path from the same seed.  With the same bits in u the two paths differ by the head's arithmetic only.
    scale.grad is SET to the kernel's d loss/d scale.  hybrid: bias_d.grad and bias_n.grad are WRITTEN in full by perf_joint_tv (into the
    tensors they hold, or new ones) and the samples' scatter is added on top.  Not hybrid: the maps and their .grad are not touched --
    the reference neither reads nor steps them in the 'global' phase and zeroes what piled up at the first 'hybrid' iteration.
    There is no fallback: a CPU tensor or a missing kernel raises."""
    scratch = scratch or StepScratch()
    P, B = coords.shape[0], coords.shape[1]
    R, Rn = bias_d.shape[-1], bias_n.shape[-1]
    coords = coords.detach().reshape(P, B, 2)
    sup, ref, scale_v, map_d, map_n = sup.detach(), ref.detach(), scale.detach(), bias_d.detach(), bias_n.detach()
    tv = None
    if hybrid:
        if scratch.tv_values is None or scratch.tv_values.device != sup.device:
            scratch.tv_values = torch.zeros(2, dtype=torch.float32, device=sup.device)
        tv = scratch.tv_values
        for k, (m, leaf, weight) in enumerate(((map_d, bias_d, 1.0), (map_n, bias_n, normal_tv_loss_weight))):
            if leaf.grad is None or not leaf.grad.is_contiguous():
                leaf.grad = torch.empty_like(m, memory_format=torch.contiguous_format)
            ops.joint_tv(m, weight, grad=leaf.grad, value=tv[k:k + 1], ws=scratch.tv)
    with torch.no_grad():
        u = _sample_views(sup, coords)[1].reshape(-1, 3).contiguous()
    u, rec = ops.joint_sample(sup, map_d, map_n, ref, coords, u=u)
    d, g = field(u, requires_grad=True)
    losses, dd, dg, dscale = ops.joint_loss(rec, coords, scale_v, u, d.detach().contiguous(), g.detach().contiguous(), ortho.detach().contiguous(),
                                            R, Rn, 20. * progress, reg_loss_weight, normal_loss_weight, normal_tv_loss_weight if hybrid else 0.0,
                                            tv=tv, gbias_d=bias_d.grad if hybrid else None, gbias_n=bias_n.grad if hybrid else None,
                                            ws=scratch.loss)
    if d.requires_grad:
        torch.autograd.backward([d, g], [dd.view_as(d), dg.view_as(g)])
    scale.grad = dscale.view_as(scale)
    return AlignStep({k: losses[i] for i, k in enumerate(LOSS_NAMES)}, u, {k: rec[:, v] for k, v in RECORD_FIELDS.items()}, dd, dg)


class JointAligner:
    """The two phases of the reference's loop (pano_joint_predictor.py:186-297): `iters` iterations that train the field and the
    per-view scales ('global'), then `iters` that also train the two bias maps with their total variation ('hybrid'); three plain
    torch.optim.Adam optimisers with the reference's learning rates (field 1e-2, scales 1e-1, maps 1e-1) and its cosine schedule
    lr = init ((cos(progress pi) + 1) (1 - 0.01) + 0.01) over progress in [0, 1) across both phases.

    fused=True: align_step (the kernels); fused=False: align_step_composed around the same field.  A pair (fused_global,
    fused_hybrid) sets the phases separately.  Draws are torch calls in the reference's order and shapes (coords = rand(P,B,1,2) 2 - 1,
    then o = randn(P,B,3)) on the supervision's device; the reference's unused np.random.randint draw per iteration is kept, so the
    numpy stream is consumed as there.  bias_params_global sits in the scales' optimiser and in no loss, as in the reference."""

    LR_ALPHA, LR_GLOBAL, LR_FIELD, LR_LOCAL = 1e-2, 1e-1, 1e-2, 1e-1

    def __init__(self, field=None, fused=True):
        self.field = field
        self.fused = tuple(fused) if isinstance(fused, (tuple, list)) else (fused, fused)
        self.scratch = StepScratch()
        self.scale_params = self.bias_params_global = self.bias_params_local_distance = self.bias_params_local_normal = None
        self.last = None
        self.history = []               # the total loss of every iteration (0-d device tensors: nothing is read back)

    def align(self, sup, ref_distance_mask, iters=1500, reg_loss_weight=1e-1, normal_loss_weight=1e-2, normal_tv_loss_weight=1e-2,
              batch=256, normal_res=128, progress_bar=False):
        """sup: [P,7,R,R] (direction, predicted distance, predicted normal per view); ref_distance_mask: [2,H,W] -> the trained field."""
        from .sphere_field import SphereDistanceField
        dev = sup.device
        P, R = sup.shape[0], sup.shape[-1]
        if self.field is None:
            self.field = SphereDistanceField.joint().to(dev)
        field = self.field
        field.train()
        self.scale_params = torch.zeros([P], device=dev, requires_grad=True)
        self.bias_params_global = torch.zeros([P], device=dev, requires_grad=True)
        self.bias_params_local_distance = torch.zeros([P, 1, R, R], device=dev, requires_grad=True)
        self.bias_params_local_normal = torch.zeros([P, 3, normal_res, normal_res], device=dev, requires_grad=True)
        scale, bias_d, bias_n = self.scale_params, self.bias_params_local_distance, self.bias_params_local_normal
        optimizer_sp = torch.optim.Adam(field.parameters(), lr=self.LR_FIELD)
        optimizer_global = torch.optim.Adam([scale, self.bias_params_global], lr=self.LR_GLOBAL)
        optimizer_local = torch.optim.Adam([bias_d, bias_n], lr=self.LR_LOCAL)
        self.history = []
        weights = dict(reg_loss_weight=reg_loss_weight, normal_loss_weight=normal_loss_weight, normal_tv_loss_weight=normal_tv_loss_weight)
        for phase, fused in zip(('global', 'hybrid'), self.fused):
            hybrid = phase == 'hybrid'
            steps = range(iters)
            if progress_bar:
                from tqdm import tqdm
                steps = tqdm(steps)
            for iter_step in steps:
                progress = iter_step / iters * .5 + (.5 if hybrid else 0.)
                lr_ratio = (np.cos(progress * np.pi) + 1.) * (1. - self.LR_ALPHA) + self.LR_ALPHA
                for opt, lr in ((optimizer_global, self.LR_GLOBAL), (optimizer_local, self.LR_LOCAL), (optimizer_sp, self.LR_FIELD)):
                    for group in opt.param_groups:
                        group['lr'] = lr * lr_ratio
                np.random.randint(low=0, high=P)
                coords = torch.rand(P, batch, 1, 2, device=dev) * 2. - 1
                ortho = torch.randn([P, batch, 3], device=dev)
                optimizer_global.zero_grad()
                optimizer_sp.zero_grad()
                if fused:
                    self.last = align_step(field, sup, ref_distance_mask, scale, bias_d, bias_n, coords, ortho, progress, hybrid, scratch=self.scratch,
                                           **weights)
                else:
                    if hybrid:
                        optimizer_local.zero_grad()
                    self.last = align_step_composed(field, sup, ref_distance_mask, scale, bias_d, bias_n, coords, ortho, progress, hybrid, **weights)
                self.history.append(self.last.losses['total'])
                optimizer_global.step()
                optimizer_sp.step()
                if hybrid:
                    optimizer_local.step()
        return field


# ---- the view set: the 20 faces of an icosahedron, one vertex at the pole -----------------------------------------------------------
def icosahedron():
    """The unit icosahedron (12 vertices from the three golden rectangles, 20 faces), turned about x by atan(0.5257 / 0.8507) so that one
    vertex is the pole: every face then has two vertices at one height (utils/geo_utils.py:115-121, without trimesh or scipy)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                  [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    faces = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                      [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    ang = np.arctan(.525731112119133606 / .850650808352039932)
    c, s = np.cos(ang), np.sin(ang)
    rot = np.array([[1., 0., 0.], [0., c, -s], [0., s, c]])
    return (v @ rot.T).astype(np.float32), faces


def verts_to_dirs(pt_a, pt_b, pt_c, gen_res, ratio):
    """One face -> one perspective view (utils/geo_utils.py:15-65): the image plane is the face's plane, centred on the face's centre,
    `ratio` times the circumradius wide to either side, 'down' pointing away from the pole.  pt_*: float32 numpy [3], two of them at
    one height -> (dirs [res,res,3] unit, ratios [res,res,1] = |pixel| / |centre|, to_vec, down_vec, right_vec), float32 on the CPU."""
    def same_z(a, b):
        return abs(a[2] - b[2]) < 1e-4

    if same_z(pt_a, pt_b):                   # pt_a becomes the vertex that is alone at its height
        pt_a, pt_c = pt_c, pt_a
    elif same_z(pt_a, pt_c):
        pt_a, pt_b = pt_b, pt_a
    if not same_z(pt_b, pt_c):
        raise ValueError('verts_to_dirs: two of the three vertices must share their height')
    if np.cross(pt_c, pt_b)[2] < 0.:
        pt_b, pt_c = pt_c, pt_b
    pt_a, pt_b, pt_c = (torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)) for p in (pt_a, pt_b, pt_c))
    down_vec = pt_a - (pt_b + pt_c) * .5
    if down_vec[2] > 0.:
        down_vec = -down_vec
    pt_center = (pt_a + pt_b + pt_c) / 3.
    right_vec = pt_c - pt_b
    right_len = torch.linalg.norm(right_vec, 2, -1).item()
    down_len = torch.linalg.norm(down_vec, 2, -1).item()
    half_len = torch.linalg.norm(pt_center - pt_b, 2, -1).item() * ratio
    right_vec = right_vec / right_len * half_len
    down_vec = down_vec / down_len * half_len
    pt_base = pt_center - right_vec - down_vec
    right_vec = right_vec * 2
    down_vec = down_vec * 2
    lin = torch.linspace(.5 / gen_res, 1. - .5 / gen_res, gen_res)
    ii, jj = torch.meshgrid(lin, lin, indexing='ij')
    to_vec = pt_base + right_vec * .5 + down_vec * .5
    dirs = pt_base[None, None, :] + down_vec[None, None, :] * ii[:, :, None] + right_vec[None, None, :] * jj[:, :, None]
    ratios = torch.linalg.norm(dirs, 2, -1, True) / torch.linalg.norm(to_vec, 2, -1, True)[None, None]
    return _unit(dirs), ratios, to_vec, down_vec * .5, right_vec * .5


def panorama_to_pers_directions(gen_res=512, ratio=1., ex_rot=None):
    """The 20 views of one ratio (utils/geo_utils.py:107-161) -> (dirs [20,res,res,3], ratios [20,res,res,1], to_vecs, down_vecs,
    right_vecs [20,3]) on the CPU.  ex_rot: None, 'rand' (one np.random.rand() angle about z, as the reference) or an angle in radians."""
    vertices, faces = icosahedron()
    outs = [verts_to_dirs(vertices[f[0]].copy(), vertices[f[1]].copy(), vertices[f[2]].copy(), gen_res, ratio) for f in faces]
    dirs, ratios, to_vecs, down_vecs, right_vecs = (torch.stack(x, 0) for x in zip(*outs))
    if ex_rot is None:
        return dirs, ratios, to_vecs, down_vecs, right_vecs
    ang = np.random.rand() * 2. * np.pi if isinstance(ex_rot, str) and ex_rot == 'rand' else float(ex_rot)
    c, s = np.cos(ang), np.sin(ang)
    rot = torch.from_numpy(np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]]).astype(np.float32))
    turn = lambda x: torch.matmul(rot, x[..., None])[..., 0]
    return turn(dirs), ratios, turn(to_vecs), turn(down_vecs), turn(right_vecs)


def img_coord_from_hw(h, w, device=None):
    i = torch.linspace(.5 / h, 1. - .5 / h, h, device=device)
    j = torch.linspace(.5 / w, 1. - .5 / w, w, device=device)
    ii, jj = torch.meshgrid(i, j, indexing='ij')
    return torch.stack([ii, jj], -1)


def img_coord_to_pano_direction(coords):
    """utils/camera_utils.py:120-155: (row, col) in [0,1] -> the unit direction of that panorama pixel."""
    beta, alpha = -(coords[..., 0] - .5) * np.pi, -(coords[..., 1] - .5) * 2. * np.pi
    return torch.stack([torch.cos(alpha) * torch.cos(beta), torch.sin(alpha) * torch.cos(beta), torch.sin(beta)], dim=-1)


def grads_to_normal(grads):
    """pano_joint_predictor.py:81-99: the panorama of distance gradients [H,W,3] -> unit normals that face the centre."""
    height, width, _ = grads.shape
    pano_dirs = img_coord_to_pano_direction(img_coord_from_hw(height, width, device=grads.device))
    ortho_a = torch.randn([height, width, 3], device=grads.device)
    ortho_b = _unit(torch.linalg.cross(pano_dirs, ortho_a))
    ortho_a = _unit(torch.linalg.cross(ortho_b, pano_dirs))
    val_a = _unit((grads * ortho_a).sum(-1, True) * pano_dirs + ortho_a)
    val_b = _unit((grads * ortho_b).sum(-1, True) * pano_dirs + ortho_b)
    normals = _unit(torch.linalg.cross(val_a, val_b))
    is_inside = ((normals * pano_dirs).sum(-1, True) < 0.).float()
    return normals * is_inside + -normals * (1. - is_inside)


class PanoJointPredictor:
    """The reference's PanoJointPredictor with its alignment loop on JointAligner.  depth_predictor.predict_depth(img [1,3,res,res],
    intri=) -> [1,1,res,res] and normal_predictor.predict_normal(img) -> [1,3,res,res] in [0,1] are the reference's Omnidata wrappers
    (not part of this package); fused as JointAligner's."""

    def __init__(self, depth_predictor, normal_predictor, fused=True):
        self.depth_predictor, self.normal_predictor, self.fused = depth_predictor, normal_predictor, fused

    def __call__(self, img, ref_distance, mask, gen_res=384, reg_loss_weight=1e-1, normal_loss_weight=1e-2, normal_tv_loss_weight=1e-2):
        """img [H,W,3], ref_distance [H,W] or [H,W,1], mask likewise (1 where the panorama is to be inpainted) -> (distance [H,W,1],
        normals [H,W,3]).  One image at a time."""
        height, width, _ = img.shape
        device = img.device
        img = img.clone().squeeze().permute(2, 0, 1)
        mask = mask.clone().squeeze()[..., None].float().permute(2, 0, 1)
        ref_distance = ref_distance.clone().squeeze()[..., None].float().permute(2, 0, 1)
        ref_distance_mask = torch.cat([ref_distance, mask], 0).contiguous()
        views = [panorama_to_pers_directions(gen_res=gen_res, ratio=ratio, ex_rot='rand') for ratio in (1.1, 1.4, 1.7)]
        pers_dirs, pers_ratios, to_vecs, down_vecs, right_vecs = (torch.cat(x, 0).to(device) for x in zip(*views))
        norm = lambda x: torch.linalg.norm(x, 2, -1, True)
        fx = norm(to_vecs) / norm(right_vecs) * gen_res * .5
        fy = norm(to_vecs) / norm(down_vecs) * gen_res * .5
        rot_c2w = torch.linalg.inv(torch.stack([right_vecs / norm(right_vecs), down_vecs / norm(down_vecs), to_vecs / norm(to_vecs)], dim=1))
        n_pers = len(pers_dirs)
        sample_coords = img_coord_to_sample_coord(direction_to_img_coord(pers_dirs))
        pers_imgs = F.grid_sample(img[None].expand(n_pers, -1, -1, -1), sample_coords, padding_mode='border', align_corners=False)
        pred_distances_raw, pred_normals_raw = [], []
        with torch.no_grad():
            for i in range(n_pers):
                intri = {'fx': fx[i].item(), 'fy': fy[i].item(), 'cx': gen_res * .5, 'cy': gen_res * .5}
                pred_depth = self.depth_predictor.predict_depth(pers_imgs[i: i + 1], intri=intri).to(device).clip(0., None)
                pred_depth = pred_depth / (pred_depth.mean() + 1e-5)
                pred_distances_raw.append(pred_depth * pers_ratios[i].permute(2, 0, 1)[None])
                pred_normals = self.normal_predictor.predict_normal(pers_imgs[i: i + 1]).to(device) * 2. - 1.
                pred_normals = pred_normals / torch.linalg.norm(pred_normals, ord=2, dim=1, keepdim=True)
                pred_normals = torch.matmul(rot_c2w[i], pred_normals.permute(0, 2, 3, 1)[..., None])[..., 0]
                pred_normals_raw.append(pred_normals.permute(0, 3, 1, 2))
        sup = torch.cat([pers_dirs.permute(0, 3, 1, 2), torch.cat(pred_distances_raw, 0), torch.cat(pred_normals_raw, 0)], dim=1).contiguous()
        # (bound to the reference's class by install_joint_predictor_shim this method runs after the REFERENCE's __init__, which sets
        # the two predictors and no `fused`: the fused loop is then the default)
        aligner = JointAligner(fused=getattr(self, 'fused', True))
        field = aligner.align(sup.float(), ref_distance_mask, reg_loss_weight=reg_loss_weight, normal_loss_weight=normal_loss_weight,
                              normal_tv_loss_weight=normal_tv_loss_weight)
        pano_dirs = img_coord_to_pano_direction(img_coord_from_hw(height, width, device=device))
        with torch.set_grad_enabled(not getattr(field, 'fused', False)):
            new_distances, new_grads = field(pano_dirs.reshape(-1, 3), requires_grad=True)
        return new_distances.detach().reshape(height, width, 1), grads_to_normal(new_grads.detach().reshape(height, width, 3))
