"""Host-side mirror of PeRF's modules/fields/ngp_nerf.py on the gfx950 kernels: same class names, method
names, argument meaning and state_dict keys (`aabb`, `geo_mlp.params`, `app_mlp.params`).

The arithmetic of the two tcnn networks is in perf_amd.tcnn; what this file adds is the reference's glue
(ngp_nerf.py:136-176): aabb normalisation, the 0<x<1 selector, trunc_exp on the density logit -- fused here
into the position and MLP-epilogue kernels (PERF_ACT_EXP + selector), so a density query is three launches.
"""
import weakref
from typing import List, Union

import numpy as np
import torch
import torch.nn as nn

from . import ops
from . import tcnn
from .grid import LOCAL_MIN_RES
from .tcnn import _DualFieldFn, field_apply

PER_LEVEL_SCALE = 1.4472692012786865


def _grid_cfg(n_levels=16, log2_hashmap_size=18, base_resolution=16, per_level_scale=PER_LEVEL_SCALE, layout_kw=None):
    cfg = {"otype": "HashGrid", "n_levels": n_levels, "n_features_per_level": 2,
           "log2_hashmap_size": log2_hashmap_size, "base_resolution": base_resolution,
           "per_level_scale": per_level_scale}
    cfg.update(layout_kw or {})         # (GridConfig.from_tcnn's optional keys layout / sb_shift / local_min_res)
    return cfg


class _TruncExp(torch.autograd.Function):
    """exp forward, gradient exp(min(x, 15)) (ngp_nerf.py:24-40)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15))


trunc_exp = _TruncExp.apply


def contract_to_unisphere(x, aabb, eps: float = 1e-6):
    """Scene contraction of mip-NeRF 360 as used by ngp_nerf.py:43-65 for `unbounded=True` (never enabled by PeRF):
    points of the box map to the inner half of the unit ball, everything beyond to the shell between radius 1 and 2;
    the result is rescaled to [0, 1]^3.  (The reference's `derivative=True` branch has no caller and is not mirrored.)"""
    lo, hi = aabb[..., :3], aabb[..., 3:]
    u = (x - lo) / (hi - lo) * 2.0 - 1.0                      # box -> [-1, 1]^3
    r = torch.linalg.vector_norm(u, dim=-1, keepdim=True)
    outside = r > 1.0
    r_safe = torch.where(outside, r, torch.ones_like(r))
    u = torch.where(outside, (2.0 - 1.0 / r_safe) * (u / r_safe), u)
    return u * 0.25 + 0.5


class _DensityGradFn(torch.autograd.Function):
    """(sigma, d sigma / d x) of the density network, differentiable with respect to its PARAMETERS: forward ops.field_grad_x, backward
    ops.field_grad_x_bwd, both on the 16-bit working copy.  Positions get no gradient."""

    @staticmethod
    def forward(ctx, x01, params, sel, net, inv_extent, n_dev):
        w16 = net.working_copy(params)
        out = None
        if n_dev is not None:       # (rows at and beyond the device count are not written by the kernel: zeros, not allocator garbage)
            out = (torch.zeros(x01.shape[0], dtype=torch.float32, device=x01.device), torch.zeros(x01.shape[0], 3, dtype=torch.float32, device=x01.device))
        sigma, grad = ops.field_grad_x(net.grid, net.mlp, x01, sel, w16, inv_extent, n_dev=n_dev, out=out)
        ctx.net, ctx.inv_extent, ctx.n_dev, ctx.has_sel = net, inv_extent, n_dev, sel is not None
        ctx.save_for_backward(x01, w16, sel if sel is not None else torch.empty(0, device=x01.device))
        ctx.set_materialize_grads(False)
        return sigma, grad

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dsigma, dgrad):
        if dsigma is None and dgrad is None:
            return None, None, None, None, None, None
        x01, w16, sel = ctx.saved_tensors
        net = ctx.net
        g = ops.field_grad_x_bwd(net.grid, net.mlp, x01, sel if ctx.has_sel else None, w16, ctx.inv_extent,
                                 None if dsigma is None else dsigma.contiguous().float(), None if dgrad is None else dgrad.contiguous().float(),
                                 n_dev=ctx.n_dev, ws=net.bwd_workspace)
        return None, g, None, None, None, None


def unit_normals(g):
    """n = -g / |g| per row of a density gradient [..., 3], in torch (differentiable): scaled by the largest component first, as
    NGPNeRF.query_normal does (|g|^2 of a trunc_exp gradient can leave fp32), and 0 where g is 0 or not finite."""
    m = g.detach().abs().amax(dim=-1, keepdim=True)
    ok = (m > 0) & (m <= 3.0e38)
    u = torch.where(ok, g, torch.zeros_like(g)) / torch.where(ok, m, torch.ones_like(m))
    nrm = torch.linalg.vector_norm(torch.where(ok, u, torch.ones_like(u)), dim=-1, keepdim=True)
    return torch.where(ok, -u / nrm, torch.zeros_like(u))


class PairTable:
    """The pair table of two fields over ONE grid geometry (include/perf_hip_pair.h): entry e = {field 0's packed features, field 1's}, so
    that one gather per corner encodes both fields (ops.hashgrid_fwd_pair).  A half is current when it was written from the working copy
    its network holds now: keyed like tcnn.NetworkWithInputEncoding.working_copy (master's data_ptr, _version, dtype) plus the network
    itself.  A stale half is refilled (ops.pair_fill) before use, never read; the fused Adam of a network bound to a half refreshes it
    in its own launch (ops.adam_step_dev(pair=...)) and marks it current (adopted).  The plain working copies stay what every other
    consumer reads."""

    def __init__(self, grid, device):
        self.buf = ops.pair_table(grid, device)
        self.keys = [None, None]

    @staticmethod
    def _key(net):
        return (weakref.ref(net), net._w16_key)

    def refresh(self, field, net):
        w16 = net.working_copy()
        key = self._key(net)
        if self.keys[field] != key:
            ops.pair_fill(self.buf, field, w16[net.mlp.n_params:])
            self.keys[field] = key

    def adopted(self, field, net):
        """The launch that refreshed net's working copy wrote this half as well (call after net.set_working_copy)."""
        self.keys[field] = self._key(net)


class _DensityNet(tcnn.NetworkWithInputEncoding):
    """geo network whose kernel epilogue applies trunc_exp(y - shift) * selector."""

    def __init__(self, grid_cfg, exp_shift=0.0, seed=tcnn.DEFAULT_SEED, dtype=None):
        super().__init__(3, 1, grid_cfg, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None",
                                          "n_neurons": 64, "n_hidden_layers": 1}, seed=seed, dtype=dtype)
        self.mlp.output_activation = 'Exponential'
        self.mlp.exp_shift = exp_shift


class NGPNeRF(nn.Module):
    """Instant-NGP radiance field (ngp_nerf.py:68-198)."""

    def __init__(self, aabb: Union[torch.Tensor, List[float]], num_dim: int = 3, use_viewdirs: bool = False,
                 unbounded: bool = False, n_levels: int = 16, dtype=None, log2_hashmap_size: int = 18, layout: str = 'tcnn',
                 sb_shift=None, local_min_res: int = LOCAL_MIN_RES):
        """layout (not the reference's): 'tcnn' or the opt-in line-local table layouts of perf_amd.grid.GridConfig ('line_local' /
        'line_overlap', with sb_shift / local_min_res), for both fields; trained through ops.hashgrid_bwd_lines."""
        super().__init__()
        if not isinstance(aabb, torch.Tensor):
            aabb = torch.tensor(aabb, dtype=torch.float32, device='cpu')
        self.register_buffer("aabb", aabb.float().cuda())
        self._aabb_host = [float(v) for v in aabb.reshape(-1).tolist()]
        self.num_dim = num_dim
        self.use_viewdirs = use_viewdirs
        self.unbounded = unbounded
        self.n_levels = n_levels
        self.dtype_name = dtype
        # (n_levels / log2_hashmap_size beyond the reference's 16 / 18: BASELINE config 5's tables sized to HBM)
        self._layout_kw = None
        if layout != 'tcnn':
            self._layout_kw = {'layout': layout, 'local_min_res': local_min_res}
            if sb_shift is not None:
                self._layout_kw['sb_shift'] = tuple(int(v) for v in sb_shift)
        self._geo_cfg = (n_levels, log2_hashmap_size)
        self.geo_mlp = _DensityNet(_grid_cfg(n_levels, log2_hashmap_size, layout_kw=self._layout_kw), dtype=dtype)
        self.app_mlp = tcnn.NetworkWithInputEncoding(
            3, 3, _grid_cfg(n_levels, log2_hashmap_size, layout_kw=self._layout_kw),
            {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 64,
             "n_hidden_layers": 2}, dtype=dtype)

    # -- point queries (ngp_nerf.py:136-162).  Like the reference's, they normalise by the aabb whatever `unbounded` says: the
    #    reference stores that flag (ngp_nerf.py:90) and only NGPDensityField.forward (:251-252) ever contracts. ---------
    def query_density(self, x):
        shape = list(x.shape[:-1])
        x01, sel = ops.points_normalize(x.reshape(-1, 3).contiguous().float(), self._aabb_host)
        return field_apply(self.geo_mlp, x01, self.geo_mlp.params, sel).view(shape + [1])

    def query_rgb(self, x):
        shape = list(x.shape[:-1])
        x01, sel = ops.points_normalize(x.reshape(-1, 3).contiguous().float(), self._aabb_host)
        return field_apply(self.app_mlp, x01, self.app_mlp.params, sel).view(shape + [3])

    # -- ray-sample queries: positions o + d (t0+t1)/2 are formed in-kernel (nerf_renderer.py:125-127) --
    def sample_points(self, rays_o, rays_d, ray_indices, t_starts, t_ends):
        return ops.points_from_rays(rays_o, rays_d, ray_indices, t_starts, t_ends, self._aabb_host)

    def density_at(self, x01, sel, n_dev=None):
        return field_apply(self.geo_mlp, x01, self.geo_mlp.params, sel, n_dev)[:, 0]

    @torch.no_grad()
    def density_with_features(self, x01, sel, n_dev=None):
        """Density without gradient plus the level-major encoded features it was computed from -> (sigma [n], feat [L,n,2])."""
        net = self.geo_mlp
        sig, feat = ops.field_infer(net.grid, net.mlp, x01, sel, net.working_copy(), n_dev=n_dev, want_features=True)
        return sig[:, 0], feat

    # -- the pair table: both fields' grids have one geometry, a training step encodes the same positions through both ------------
    def pair_supported(self):
        """Both grids equal, in tcnn's layout, at most 16 levels, one 16-bit type: what ops.hashgrid_fwd_pair is built for."""
        ga, gb = self.geo_mlp.grid, self.app_mlp.grid
        key = lambda g: (g.n_levels, g.log2_hashmap_size, g.base_resolution, g.per_level_scale, g.interpolation, g.layout)
        return key(ga) == key(gb) and ga.layout == 'tcnn' and ga.n_levels <= 16 and self.geo_mlp.dtype_name == self.app_mlp.dtype_name

    def use_pair(self, on):
        """Bind (or unbind) the two networks to the halves of this field's pair table: a bound network's fused Adam keeps its half
        current.  -> the PairTable with both halves current, or None.  Whether a half is refilled (ops.pair_fill) is decided HERE, on
        the host, like the re-cast of a working copy: a captured step graph contains a fill only if a half was stale at capture, so a
        captured step assumes both halves current at capture time and kept current by the bound networks' Adam launches alone; a
        working copy re-cast outside the graph (reset_geo, load_state_dict) needs a new capture, as it does for the working copy."""
        if not on:
            self.geo_mlp._pair_half = self.app_mlp._pair_half = None
            return None
        pt = self.__dict__.get('_pair')
        if pt is None or pt.buf.shape[0] != self.geo_mlp.grid.total or pt.buf.device != self.geo_mlp.params.device:
            pt = self.__dict__['_pair'] = PairTable(self.geo_mlp.grid, self.geo_mlp.params.device)
        for field, net in enumerate((self.geo_mlp, self.app_mlp)):
            net._pair_half = (pt, field)
            pt.refresh(field, net)
        return pt

    @torch.no_grad()
    def density_with_pair_features(self, x01, sel, pair, n_dev=None):
        """density_with_features by ONE pair encode: -> (sigma [n], ops.PairFeat(density features, colour features)), each to the bit
        what the field's own encode gives."""
        net = self.geo_mlp
        fa, fb = ops.hashgrid_fwd_pair(net.grid, x01, pair.buf, net.dtype_name, n_dev=n_dev)
        sig = ops.mlp_fwd(net.mlp, net.working_copy()[:net.mlp.n_params], fa, sel, n_dev=n_dev)
        return sig[:, 0], ops.PairFeat(fa, fb)

    @torch.no_grad()
    def rgb_from_features(self, feat, sel, n_dev=None):
        """The colour network on already encoded colour features ([L, n, 2] or an ops.IndexedFeat), without gradient."""
        net = self.app_mlp
        return ops.mlp_fwd(net.mlp, net.working_copy()[:net.mlp.n_params], feat, sel, n_dev=n_dev)

    def _inv_extent(self):
        a = self._aabb_host
        return [1.0 / (a[3 + i] - a[i]) for i in range(3)]

    @torch.no_grad()
    def density_grad_at(self, x01, sel, n_dev=None):
        """(sigma [n], d sigma / d x [n,3] in world units) at normalised positions, one kernel on the 16-bit working copy
        (ops.field_grad_x).  Evaluation only: nothing is recorded for autograd."""
        net = self.geo_mlp
        return ops.field_grad_x(net.grid, net.mlp, x01, sel, net.working_copy(), self._inv_extent(), n_dev=n_dev)

    def density_and_grad_at(self, x01, sel, n_dev=None):
        """(sigma [n], d sigma / d x [n,3] in world units) with autograd: differentiable with respect to geo_mlp.params ONLY (a loss on
        surface normals during training) -- the forward is density_grad_at's kernel to the bit, the backward ONE fused kernel
        (ops.field_grad_x_bwd).  Positions are not trained: x01.requires_grad raises."""
        if x01.requires_grad:
            raise NotImplementedError('density_and_grad_at is differentiable with respect to geo_mlp.params only: x01.requires_grad is set '
                                      '(the second derivative with respect to positions is not built)')
        net = self.geo_mlp
        return _DensityGradFn.apply(x01, net.params, sel, net, self._inv_extent(), n_dev)

    @torch.no_grad()
    def query_normal(self, x):
        """World positions [..., 3] -> (sigma [..., 1], unit normal [..., 3]); n = -grad sigma / |grad sigma| faces the side the density
        falls towards (the camera's side of a surface: -dir . n > 0, the reference's convention), zero where the gradient is zero."""
        shape = list(x.shape[:-1])
        x01, sel = ops.points_normalize(x.reshape(-1, 3).contiguous().float(), self._aabb_host)
        sigma, g = self.density_grad_at(x01, sel)
        m = g.abs().amax(dim=-1, keepdim=True)
        u = g / torch.where(m > 0, m, torch.ones_like(m))
        nrm = torch.linalg.vector_norm(u, dim=-1, keepdim=True)
        normal = torch.where(nrm > 0, -u / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(u))
        return sigma.view(shape + [1]), normal.view(shape + [3])

    def rgb_at(self, x01, sel, n_dev=None):
        return field_apply(self.app_mlp, x01, self.app_mlp.params, sel, n_dev)

    def density_rgb_at(self, x01, sel, geo_grad=True, app_grad=False):
        """sigma [n] and rgb [n,3] at the same points with ONE shared encode pass (both grids have the same geometry).
        geo_grad / app_grad = False detach the respective parameters (nerf_renderer.py:166-179 no_grad branches)."""
        pg = self.geo_mlp.params if geo_grad else self.geo_mlp.params.detach()
        pa = self.app_mlp.params if app_grad else self.app_mlp.params.detach()
        if self.geo_mlp.grid.layout != 'tcnn':
            # (the shared-corner dual encode is tcnn-layout only: line-local tables encode each field on its own)
            return field_apply(self.geo_mlp, x01, pg, sel)[:, 0], field_apply(self.app_mlp, x01, pa, sel)
        sig, rgb = _DualFieldFn.apply(x01, pg, pa, sel, self.geo_mlp, self.app_mlp)
        return sig[:, 0], rgb

    def forward(self, positions, directions=None, contract=None):
        if self.use_viewdirs and (directions is not None):
            assert positions.shape == directions.shape, f"{positions.shape} v.s. {directions.shape}"
        density = self.query_density(positions)
        rgb = self.query_rgb(positions)
        return rgb, density

    def reset_geo(self):
        """Fresh geometry network, identical initialisation every episode (ngp_nerf.py:178-197)."""
        # (the field's own grid: levels, table size, layout -- the defaults (16, 18, tcnn) give the reference's grid bit for bit)
        self.geo_mlp = _DensityNet(_grid_cfg(*self._geo_cfg, layout_kw=self._layout_kw), dtype=self.dtype_name)


class InferenceNeRF:
    """NGPNeRF for inference only, for fields whose tables are sized to HBM (BASELINE config 5: L = 20, log2_hashmap_size
    28-30; SURVEY.md 8(e): "inference-only replicated fp16"): each network exists ONLY as its 16-bit working copy
    [MLP weights | table] -- no fp32 master, no optimizer state -- and is initialised on the device (tcnn's rule: Xavier-uniform
    MLP weights, tables U(-1e-4, 1e-4); the 10^9-entry tables are filled in chunks from a seeded device generator).  The duck
    type NeRFOCCRenderer uses (density_at / rgb_at / sample_points on kernel-made positions), like sharded.LevelShardedNeRF."""

    def __init__(self, aabb, n_levels=20, log2_hashmap_size=28, per_level_scale=PER_LEVEL_SCALE, dtype='fp16', seed=tcnn.DEFAULT_SEED,
                 table_scale=1e-4, density_bias=0.0, device=None, layout='tcnn', **layout_kw):
        """table_scale / density_bias (tests): tables U(-table_scale, table_scale) and sigma = exp(y + density_bias) instead of the
        fresh initialisation's near-constant sigma = exp(y ~ 0) -- a field with structure, dense enough for rays to terminate.
        layout: 'tcnn' (default) or the opt-in 'line_local' / 'line_overlap' table layouts of perf_amd.grid.GridConfig -- these fields exist for grids
        the reference never defines, no reference result constrains how their tables are laid out."""
        from .grid import GridConfig, MlpConfig
        import math
        if not isinstance(aabb, torch.Tensor):
            aabb = torch.tensor(aabb, dtype=torch.float32, device='cpu')
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.aabb = aabb.float().to(dev)
        self._aabb_host = [float(v) for v in aabb.reshape(-1).tolist()]
        self.training = False
        self.dtype_name = dtype
        self.grid = GridConfig(n_levels=n_levels, log2_hashmap_size=log2_hashmap_size, base_resolution=16, per_level_scale=per_level_scale,
                               layout=layout, **layout_kw)          # (layout_kw: sb_shift, local_min_res)
        t16 = ops.torch_dtype(dtype)
        self.nets = {}
        gen = torch.Generator(device=dev).manual_seed(seed)
        cg = torch.Generator(device='cpu').manual_seed(seed)
        for name, mlp in (('geo_mlp', MlpConfig(n_levels, 1, 1, 'Exponential', exp_shift=-float(density_bias))),
                          ('app_mlp', MlpConfig(n_levels, 2, 3, 'Sigmoid'))):
            n_net = mlp.n_params
            w16 = torch.empty(n_net + self.grid.n_params, dtype=t16, device=dev)
            parts = [(torch.rand(o * i, generator=cg, device='cpu') * 2 - 1) * math.sqrt(6.0 / (i + o)) for (o, i) in mlp.shapes]
            w16[:n_net].copy_(torch.cat(parts))
            chunk = 1 << 28
            for lo in range(n_net, w16.numel(), chunk):
                hi = min(lo + chunk, w16.numel())
                w16[lo:hi].copy_((torch.rand(hi - lo, device=dev, generator=gen) * 2 - 1) * table_scale)
            self.grid.canonicalize_(w16[n_net:])          # (line_overlap: the two copies of a run's shared vertex hold one value)
            self.nets[name] = (mlp, w16)

    def eval(self):
        return self

    def table_bytes(self):
        """Bytes of ONE encoder's 16-bit table."""
        return self.grid.n_params * 2

    @torch.no_grad()
    def density_at(self, x01, sel, n_dev=None):
        mlp, w16 = self.nets['geo_mlp']
        return ops.field_infer(self.grid, mlp, x01, sel, w16, n_dev=n_dev)[:, 0]

    @torch.no_grad()
    def density_grad_at(self, x01, sel, n_dev=None):
        mlp, w16 = self.nets['geo_mlp']
        a = self._aabb_host
        return ops.field_grad_x(self.grid, mlp, x01, sel, w16, [1.0 / (a[3 + i] - a[i]) for i in range(3)], n_dev=n_dev)

    @torch.no_grad()
    def rgb_at(self, x01, sel, n_dev=None):
        mlp, w16 = self.nets['app_mlp']
        return ops.field_infer(self.grid, mlp, x01, sel, w16, n_dev=n_dev)

    def sample_points(self, rays_o, rays_d, ray_indices, t_starts, t_ends):
        return ops.points_from_rays(rays_o, rays_d, ray_indices, t_starts, t_ends, self._aabb_host)


class NGPDensityField(nn.Module):
    """Proposal density field (ngp_nerf.py:200-265): sigma = trunc_exp(net(x) - 1) * selector."""

    def __init__(self, aabb, num_dim: int = 3, unbounded: bool = False, base_resolution: int = 16,
                 max_resolution: int = 128, n_levels: int = 5, log2_hashmap_size: int = 17, dtype=None):
        super().__init__()
        if not isinstance(aabb, torch.Tensor):
            aabb = torch.tensor(aabb, dtype=torch.float32, device='cpu')
        self.register_buffer("aabb", aabb.float().cuda())
        self._aabb_host = [float(v) for v in aabb.reshape(-1).tolist()]
        self.num_dim = num_dim
        self.unbounded = unbounded
        self.base_resolution = base_resolution
        self.max_resolution = max_resolution
        self.n_levels = n_levels
        self.log2_hashmap_size = log2_hashmap_size
        per_level_scale = np.exp((np.log(max_resolution) - np.log(base_resolution)) / (n_levels - 1)).tolist()
        self.mlp_base = _DensityNet(_grid_cfg(n_levels, log2_hashmap_size, base_resolution, per_level_scale),
                                    exp_shift=1.0, dtype=dtype)

    def forward(self, positions: torch.Tensor):
        shape = list(positions.shape[:-1])
        if self.unbounded:
            x01 = contract_to_unisphere(positions, self.aabb).reshape(-1, 3).contiguous().float()
            sel = ((x01 > 0.0) & (x01 < 1.0)).all(dim=-1).to(torch.uint8)
        else:
            x01, sel = ops.points_normalize(positions.reshape(-1, 3).contiguous().float(), self._aabb_host)
        return field_apply(self.mlp_base, x01, self.mlp_base.params, sel).view(shape + [1])
