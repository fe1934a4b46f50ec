"""SphereDistanceField of PeRF's geometry predictors (modules/geo_predictors/pano_joint_predictor.py:22-71, pano_geo_refiner.py:11-59) on
the fused kernels of include/perf_hip_sphere.h: a Smoothstep hash grid over the directions of the unit sphere, a 35 -> 64 -> 64 -> 1 fp32
MLP with Softplus(beta=100), and the gradient of the distance with respect to the direction -- value and gradient in ONE kernel, their
backward with respect to the parameters in ONE kernel, instead of four hash-grid launches, a torch MLP and a doubly differentiated
autograd graph.

Same constructor defaults, submodule names (hash_grid, geo_mlp.layers.{0,2,4}), state_dict keys, shapes and return contract as the
reference's two classes, which differ in three things only -- SphereDistanceField.joint() and .refiner() name them."""
import math
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import tcnn


class SphereMLP(nn.Module):
    """The reference's VanillaMLP(dim_in, 1, 64, 2, sphere_init=True, weight_norm=...) (modules/fields/networks.py:16-66), restated:
    Linear -> Softplus(beta=100) -> Linear -> Softplus(beta=100) -> Linear under `layers` (so that the parameters are
    layers.{0,2,4}.{weight,bias}, or weight_g / weight_v with weight norm), forward returns MINUS the last layer's output.  The
    geometric initialisation of a signed distance to a sphere of radius 0.5: the last layer's weights around sqrt(pi) / sqrt(fan_in) and
    its bias -0.5; the hidden layers N(0, 2 / fan_out) with zero bias; of the first layer only the three direction columns are drawn,
    the feature columns start at zero.  Needs no GPU."""

    N_NEURONS = 64

    def __init__(self, dim_in, weight_norm=False, sphere_init_radius=0.5):
        super().__init__()
        self.dim_in, self.weight_norm, self.sphere_init_radius = dim_in, weight_norm, sphere_init_radius
        w = self.N_NEURONS
        self.layers = nn.Sequential(self._linear(dim_in, w, 'first'), nn.Softplus(beta=100), self._linear(w, w, 'hidden'), nn.Softplus(beta=100),
                                    self._linear(w, 1, 'last'))

    def _linear(self, dim_in, dim_out, which):
        layer = nn.Linear(dim_in, dim_out, bias=True)
        with torch.no_grad():
            if which == 'last':
                layer.bias.fill_(-self.sphere_init_radius)
                layer.weight.normal_(mean=math.sqrt(math.pi) / math.sqrt(dim_in), std=0.0001)
            else:
                layer.bias.zero_()
                layer.weight.normal_(0.0, math.sqrt(2) / math.sqrt(dim_out))
                if which == 'first':
                    layer.weight[:, 3:].zero_()
        return nn.utils.weight_norm(layer) if self.weight_norm else layer

    def forward(self, x):
        return -self.layers(x.float())

    def effective_parameters(self):
        """(W1, b1, W2, b2, w3, b3) as the kernels see them: with weight norm W = g v / |v| (row norms), formed from weight_g and weight_v
        with differentiable torch ops -- the layer itself is not called, so the gradient reaches weight_g and weight_v through these ops."""
        out = []
        for i in (0, 2, 4):
            layer = self.layers[i]
            if self.weight_norm:
                v, g = layer.weight_v, layer.weight_g
                out.append(v * (g / v.norm(2, dim=1, keepdim=True)))
            else:
                out.append(layer.weight)
            out.append(layer.bias)
        return tuple(out)


class _SphereFieldFn(torch.autograd.Function):
    """(table, W1, b1, W2, b2, w3, b3) -> (raw, g) at fixed directions: perf_sphere_field_fwd; the backward is the one call of
    perf_sphere_field_bwd.  Saves its inputs and nothing else (under no_grad: nothing)."""

    @staticmethod
    def forward(ctx, dirs, want_grad, module, table, w1, b1, w2, b2, w3, b3):
        ctx.set_materialize_grads(False)
        net = torch.cat([w1.reshape(-1), b1.reshape(-1), w2.reshape(-1), b2.reshape(-1), w3.reshape(-1), b3.reshape(-1)]).float()
        raw, g = ops.sphere_field_fwd(module.hash_grid.grid, table.detach(), net, dirs, want_grad=want_grad)
        ctx.module = module
        ctx.save_for_backward(dirs, table, w1, b1, w2, b2, w3, b3)
        if not want_grad:
            return raw
        return raw, g

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, draw, dgrad=None):
        dirs, table, w1, b1, w2, b2, w3, b3 = ctx.saved_tensors
        if draw is None and dgrad is None:
            return (None,) * 10
        module = ctx.module
        net = torch.cat([w1.reshape(-1), b1.reshape(-1), w2.reshape(-1), b2.reshape(-1), w3.reshape(-1), b3.reshape(-1)]).float()
        grad = ops.sphere_field_bwd(module.hash_grid.grid, table.detach(), net, dirs, None if draw is None else draw.contiguous().float(),
                                    None if dgrad is None else dgrad.contiguous().float(), ws=module.bwd_workspace)
        outs, lo = [], 0
        for t in (w1, b1, w2, b2, w3, b3):
            outs.append(grad[lo:lo + t.numel()].view(t.shape))
            lo += t.numel()
        return (None, None, None, grad[lo:].view(table.shape)) + tuple(outs)


class SphereDistanceField(nn.Module):
    """distance(direction) on the unit sphere and its gradient with respect to the direction.

    forward(directions [N, 3], requires_grad=False) -> distance [N], or (distance [N], grad [N, 3]) with requires_grad=True, as the
    reference: distance = act(-(MLP([u; enc(0.49 u + 0.49)]))), grad = d distance / du with the graph kept (it can be trained on).

    fused=True (default): one kernel for (raw, d raw/du), one kernel for the whole backward with respect to the parameters; weight norm
    and the output activation (with its chain rule on the gradient) stay in torch around them.  Under torch.no_grad() nothing is kept:
    the full-panorama query costs O(N) memory.  The fused path gives NO gradient with respect to `directions`; a call whose
    directions already require a gradient takes the composed path, with one warning.
    fused=False: the composed path -- perf_amd.tcnn.Encoding's kernels, the torch MLP and torch.autograd.grad(create_graph=True), i.e.
    the reference's own formulation: the parity yardstick and the fallback.

    One stated difference from the reference: features stay in fp32 from the table to the MLP.  tiny-cuda-nn (and perf_amd.tcnn.Encoding
    by default) hands the features back as half; here hash_grid is an Encoding(dtype=torch.float32) on both paths, and the fused
    kernels never round to a 16-bit type."""

    def __init__(self, n_levels=16, log2_hashmap_size=19, base_res=16, fine_res=2048, weight_norm=False, output='softplus1', fused=True):
        super().__init__()
        if output not in ('softplus1', 'identity'):
            raise ValueError(f"output must be 'softplus1' (softplus(raw + 1)) or 'identity', got {output!r}")
        per_level_scale = math.exp(math.log(fine_res / base_res) / (n_levels - 1)) if n_levels > 1 else 1.0
        device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        self.hash_grid = tcnn.Encoding(
            n_input_dims=3,
            encoding_config={'otype': 'HashGrid', 'n_levels': n_levels, 'n_features_per_level': 2, 'log2_hashmap_size': log2_hashmap_size,
                             'base_resolution': base_res, 'per_level_scale': per_level_scale, 'interpolation': 'Smoothstep'},
            dtype=torch.float32, device=device)
        self.geo_mlp = SphereMLP(dim_in=n_levels * 2 + 3, weight_norm=weight_norm).to(device)
        self.output = output
        self.fused = fused
        self.bwd_workspace = ops.Workspace()        # scratch memory of the fused backward (plain attribute: dropped with the field)
        self._warned_dir_grad = False               # the one warning of this field when a call has to leave the fused path

    @classmethod
    def joint(cls, **kw):
        """The field of PanoJointPredictor (pano_joint_predictor.py:22-71): finest resolution 2048, no weight norm, softplus(raw + 1)."""
        return cls(**{'fine_res': 2048, 'weight_norm': False, 'output': 'softplus1', **kw})

    @classmethod
    def refiner(cls, **kw):
        """The field of PanoGeoRefiner (pano_geo_refiner.py:11-59): finest resolution 4096, weight norm, the raw output."""
        return cls(**{'fine_res': 4096, 'weight_norm': True, 'output': 'identity', **kw})

    # ---- the output activation and its chain rule on the gradient (torch: differentiable, so both are trained through) ----------------
    def _activate(self, raw, g):
        if self.output == 'identity':
            return raw, g
        distance = F.softplus(raw + 1.)
        return distance, (None if g is None else torch.sigmoid(raw + 1.)[..., None] * g)

    def forward(self, directions, requires_grad=False):
        wants_dir_grad = torch.is_tensor(directions) and directions.requires_grad and torch.is_grad_enabled()
        if self.fused and wants_dir_grad:
            if not self._warned_dir_grad:
                self._warned_dir_grad = True
                warnings.warn('SphereDistanceField: `directions` requires a gradient, which the fused kernels do not form; this call '
                              '(and every such call of this field) takes the composed path (fused=False)', stacklevel=2)
        if not self.fused or wants_dir_grad:
            return self.forward_composed(directions, requires_grad)
        shape = directions.shape[:-1]
        dirs = directions.detach().reshape(-1, 3).contiguous().float()
        out = _SphereFieldFn.apply(dirs, bool(requires_grad), self, self.hash_grid.params, *self.geo_mlp.effective_parameters())
        raw, g = out if requires_grad else (out, None)
        distance, grad = self._activate(raw, g)
        if requires_grad:
            return distance.reshape(shape), grad.reshape(*shape, 3)
        return distance.reshape(shape)

    def forward_composed(self, directions, requires_grad=False):
        """The reference's forward, statement for statement, on perf_amd.tcnn.Encoding (fp32 features)."""
        if requires_grad:
            if not self.training:
                directions = directions.clone()
            directions.requires_grad_(True)
        dir_scaled = directions * 0.49 + 0.49
        scene_feat = self.hash_grid(dir_scaled)
        raw = self.geo_mlp(torch.cat([directions, scene_feat], -1))[..., 0]
        distance = raw if self.output == 'identity' else F.softplus(raw + 1.)
        if not requires_grad:
            return distance
        grad = torch.autograd.grad(distance, directions, grad_outputs=torch.ones_like(distance), create_graph=True, retain_graph=True,
                                   only_inputs=True)[0]
        return distance, grad
