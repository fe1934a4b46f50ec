"""Training on surface normals on the GPU: perf_field_grad_x_bwd -- the backward of (sigma, grad_x sigma) with respect to the density
field's parameters -- against the oracle's DOUBLE autograd, its counts and variants, the autograd surface
(NGPNeRF.density_and_grad_at), the opt-in normal loss of the geometry step, and the room trained with and without it.

The yardstick is always oracle/perf_oracle.py, never the kernel:
    sig = O.query_density(x, p, ...);  gx = autograd.grad(sig.sum(), x, create_graph=True);
    reference = autograd.grad((gx * dg).sum() + (sig * dsigma).sum(), p)
Tolerances come from the oracle alone (e_q: what ONE set of 16-bit operand roundings does to a block of this gradient; the kernel
may take two).  Every figure is printed before it is asserted; with PERF_FIELD_NORMAL_TRAIN_REPORT=<path> the figures are also written
there as JSON (profiles/field_normal_train.json is folded from it).

Figures measured on MI355X for this file are recorded in profiles/field_normal_train.json."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import perf_oracle as O  # noqa: E402
from tests import test_gpu_exact_gradients as EG  # noqa: E402      (the exact-data construction: imported, not copied)
from tests import test_gpu_field_normal as FN  # noqa: E402         (set-up, exclusion rule and room fixture of the forward's tests)

AABB = FN.AABB
_REPORT = {}


def _report(key, value):
    _REPORT[key] = value
    path = os.environ.get('PERF_FIELD_NORMAL_TRAIN_REPORT')
    if path:
        json.dump(_REPORT, open(path, 'w'), indent=1)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _oracle_param_grad(x, p, spec, aabb, quant, dsigma, dg):
    """d [ sum(dsigma sigma) + sum(dg . d sigma / d x) ] / d p by double autograd on the oracle (world units)."""
    aabb = torch.as_tensor(aabb, dtype=x.dtype)
    pr = p.clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    sig = O.query_density(xr, pr, spec, aabb, quant=quant)[:, 0]
    (gx,) = torch.autograd.grad(sig.sum(), xr, create_graph=True)
    obj = (gx * dg).sum() + (sig * dsigma).sum()
    (gp,) = torch.autograd.grad(obj, pr)
    return gp.detach()


def _pre_activations(x, p, spec, aabb, quant):
    aabb = torch.as_tensor(aabb, dtype=x.dtype)
    with torch.no_grad():
        x01 = (x - aabb[:3]) / (aabb[3:] - aabb[:3])
        table = p[spec.n_net:].view(spec.lv.total, spec.lv.n_feat)
        feat = O.hashgrid_encode(x01, table, spec.lv, quant=quant)
        if spec.n_in > feat.shape[1]:
            feat = torch.cat([feat, feat.new_zeros(feat.shape[0], spec.n_in - feat.shape[1])], 1)
        w1 = p[:64 * spec.n_in].view(64, spec.n_in)
        return O._quant(feat, quant) @ O._quant(w1, quant).t()


def _blocks(g, spec):
    """The flat gradient cut into the blocks the bounds are stated for: W1, row 0 of Wo, each grid level."""
    n1 = 64 * spec.n_in
    out = {'W1': g[:n1], 'Wo_row0': g[n1:n1 + 64]}
    for l in range(spec.lv.n_levels):
        lo = spec.n_net + 2 * int(spec.lv.offset[l])
        out[f'level{l:02d}'] = g[lo:lo + 2 * int(spec.lv.size[l])]
    return out


def _rel(a, b):
    return float(torch.linalg.vector_norm((a - b).double()) / torch.linalg.vector_norm(b.double()))


def _field(dtype, levels):
    """(parameters, spec, aabb, grid config, mlp config): the 16-level geometry field of the forward's tests (table U(+-0.5), seed 1 /
    1337, the off-centre box) or an 8-level one on the unit cube."""
    from perf_amd.grid import GridConfig, MlpConfig
    if levels == 16:
        geo, spec = FN._geo_params()
        aabb = AABB
    else:
        lv = O.grid_levels(n_levels=levels)
        spec = O.FieldSpec(lv, 1, 1, 'None')
        geo = O.init_field_params(spec, 7)
        g = torch.Generator().manual_seed(2)
        geo[spec.n_net:] = (torch.rand(lv.n_params, generator=g) * 2 - 1) * 0.5
        aabb = [0., 0., 0., 1., 1., 1.]
    return geo, spec, aabb, GridConfig(n_levels=levels), MlpConfig(n_levels=levels, n_hidden_layers=1, n_output_dims=1, output_activation='Exponential')


@functools.lru_cache(maxsize=None)
def _case(dtype, levels):
    """One random batch per (dtype, levels), its upstream gradients and its oracle references, computed once and shared (read-only)."""
    geo, spec, aabb, cfg, mlp = _field(dtype, levels)
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    g = torch.Generator().manual_seed(1337 + levels)
    cand = lo + (hi - lo) * (torch.rand(2048, 3, generator=g) * 0.998 + 0.001)
    x_out = lo + (hi - lo) * (torch.rand(101, 3, generator=g) * 1.4 - 0.2)
    x_out = x_out[((x_out <= lo) | (x_out >= hi)).any(dim=1)]
    assert len(x_out) >= 40
    # samples with a hidden pre-activation within accumulation-order rounding of zero (the forward tests' rule, on the quantised
    # oracle) are removed from the batch before anyone sees it
    flagged = FN._near_zero_unit(_pre_activations(cand, geo, spec, aabb, dtype))
    removed = float(flagged.float().mean())
    x_in = cand[~flagged]
    if (len(x_in) + len(x_out)) % 32 == 0:
        x_in = x_in[:-1]
    x = torch.cat([x_in, x_out])
    n, n_in = len(x), len(x_in)
    dg = torch.randn(n, 3, generator=g)
    ds = torch.randn(n, generator=g)
    pre32, preq = _pre_activations(x_in, geo, spec, aabb, None), _pre_activations(x_in, geo, spec, aabb, dtype)
    agree = ((pre32 > 0) == (preq > 0)).all(dim=1)
    return {'geo': geo, 'spec': spec, 'aabb': aabb, 'cfg': cfg, 'mlp': mlp, 'x': x, 'n_in': n_in, 'dg': dg, 'ds': ds, 'agree': agree,
            'removed': removed, 'dtype': dtype}


def _noise_and_reference(c, ds, dg):
    """-> (gq: the quantised oracle's gradient on the whole batch, e_q per block: |gq - g32| / |g32| over the samples whose masks agree)."""
    x, n_in, agree = c['x'], c['n_in'], c['agree']
    xs, dss, dgs = x[:n_in][agree], ds[:n_in][agree], dg[:n_in][agree]
    g32 = _blocks(_oracle_param_grad(xs, c['geo'], c['spec'], c['aabb'], None, dss, dgs), c['spec'])
    gqs = _blocks(_oracle_param_grad(xs, c['geo'], c['spec'], c['aabb'], c['dtype'], dss, dgs), c['spec'])
    e_q = {k: _rel(gqs[k], g32[k]) for k in g32}
    gq = _oracle_param_grad(x, c['geo'], c['spec'], c['aabb'], c['dtype'], ds, dg)
    return gq, e_q


def _kernel(c, ds, dg, n=None, n_dev=None, grad=None):
    from perf_amd import ops
    n = len(c['x']) if n is None else n
    x01, sel = ops.points_normalize(c['x'][:n].cuda().contiguous(), c['aabb'])
    w16 = ops.cast_params(c['geo'].cuda(), c['dtype'])
    a = c['aabb']
    ie = [1.0 / (a[3 + i] - a[i]) for i in range(3)]
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int64, device='cuda')
    return ops.field_grad_x_bwd(c['cfg'], c['mlp'], x01, sel, w16, ie, None if ds is None else ds[:n].cuda().contiguous(),
                                None if dg is None else dg[:n].cuda().contiguous(), n_dev=nd, grad=grad).cpu()


def _check_against_oracle(c, ds, dg, what):
    gq, e_q = _noise_and_reference(c, torch.zeros(len(c['x'])) if ds is None else ds, torch.zeros(len(c['x']), 3) if dg is None else dg)
    got = _kernel(c, ds, dg)
    spec = c['spec']
    assert got.shape == gq.shape and torch.isfinite(got).all()
    kb, qb = _blocks(got, spec), _blocks(gq, spec)
    ratios = {k: _rel(kb[k], qb[k]) / e_q[k] for k in kb}
    print(f'[field_grad_x_bwd {what}] n {len(c["x"])} ({c["n_in"]} inside), removed {c["removed"]:.4%}; e_q ' +
          ', '.join(f'{k} {v:.4f}' for k, v in e_q.items()))
    print(f'[field_grad_x_bwd {what}] kernel vs quantised oracle, in units of e_q (bound 2): ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    _report(what, {'n': len(c['x']), 'removed_fraction': c['removed'], 'e_q': e_q, 'kernel_over_e_q': ratios, 'bound': '2 x e_q per block'})
    n1 = 64 * spec.n_in
    assert float(got[n1 + 64:spec.n_net].abs().max()) == 0.0, 'the padded rows of Wo'
    assert c['removed'] <= 0.01
    bad = {k: v for k, v in ratios.items() if not v <= 2.0}
    assert not bad, bad
    return got


# ---- 1. exact data -----------------------------------------------------------------------------------------------------------------
def _exact_case(dt, L, seed):
    """Integer table and weights, dyadic fractions, integer level scales: a grid whose levels all have scale 3 (base resolution 4,
    per-level scale 1), points k / 4, table entries in {-1, 0, 1}, sparse small-integer W1, small-integer Wo, the identity as output activation, a
    box whose extents are powers of two.  Features are then multiples of 1/64, their derivatives multiples of 3/16, and the upstream
    gradients (dsigma in {-2..2}, dg one axis at a time) are chosen per sample so that the directional derivative Fd = J u -- the one
    16-bit rounding of the backward -- and the combined column dsigma F + Fd are representable in the type.  Every product and sum is
    then exact in fp32 whatever its order (global fp32 atomics included), and float64 double autograd is THE answer.  The conditions
    are asserted here, on the CPU."""
    from perf_amd.grid import GridConfig, MlpConfig
    tdt, cap = EG.DT[dt]
    cfg = GridConfig(n_levels=L, log2_hashmap_size=15, base_resolution=4, per_level_scale=1.0)
    lv = O.grid_levels(L, 2, 15, 4, 1.0)
    assert lv.total == cfg.total and all(float(cfg.scale[l]) == 3.0 == float(lv.scale[l]) for l in range(L)) and not lv.hashed.any()
    mlp = MlpConfig(n_levels=L, n_hidden_layers=1, n_output_dims=1, output_activation='None')
    spec = O.FieldSpec(lv, 1, 1, 'None')
    g = torch.Generator().manual_seed(seed)
    (o1, i1), (oo, io) = mlp.shapes
    wo = torch.randint(-2, 3, (oo, io), generator=g).float()         # (every neuron feeds row 0: every level of the table gets a gradient)
    w = torch.cat([EG._sparse_int(o1, i1, 3, 2, g).reshape(-1), wo.reshape(-1)])
    table = (torch.randint(-1, 2, (lv.total, 2), generator=g) * (torch.rand(lv.total, 2, generator=g) < 0.6)).float()
    p = torch.cat([w, table.reshape(-1)]).double()
    assert p.numel() == spec.n_params == mlp.n_params + cfg.n_params
    k = torch.stack(torch.meshgrid(*[torch.arange(1, 4)] * 3, indexing='ij'), -1).reshape(-1, 3)
    x01 = torch.cat([k.repeat(7, 1).double() / 4.0, torch.tensor([[1.25, 0.5, 0.5], [0.5, -0.25, 0.75], [0.25, 0.5, 1.0], [0.0, 0.25, 0.5]] * 2).double()])
    x01 = x01[torch.randperm(len(x01), generator=g)]
    n = len(x01)
    assert n % 32 != 0 and n > 128                      # a ragged tile, more than one workgroup
    sel = ((x01 > 0) & (x01 < 1)).all(1)
    e = torch.tensor([0.5, 0.25, 1.0], dtype=torch.float64)            # 1 / (hi - lo) of the box [0, 2] x [0, 4] x [0, 1]
    # features and their directional derivatives along the axes, float64 (exact: the weights are multiples of 1/64)
    t64 = table.double()
    F = O.hashgrid_encode(x01, t64, lv)
    J = [torch.autograd.functional.jvp(lambda v: O.hashgrid_encode(v, t64, lv), x01, torch.eye(3, dtype=torch.float64)[a].expand(n, 3))[1] for a in range(3)]

    def exact16(t):
        return t.to(tdt).double() == t
    assert bool(exact16(F).all()) and float(F.abs().max()) > 0
    # per sample: the first (dsigma, axis, step) of a shuffled list whose combined column is representable
    cands = [(a, b, s) for a in (-2., -1., 0., 1., 2.) for b in range(3) for s in (-2., -1., 1., 2.)]
    order = torch.stack([torch.randperm(len(cands), generator=g) for _ in range(n)])
    ds, u = torch.zeros(n, dtype=torch.float64), torch.zeros(n, 3, dtype=torch.float64)
    for i in range(n):
        for j in order[i].tolist():
            a, b, s = cands[j]
            if bool(exact16(s * J[b][i]).all()) and bool(exact16(a * F[i] + s * J[b][i]).all()):
                ds[i] = a; u[i, b] = s
                break
        else:
            raise AssertionError(f'sample {i}: no upstream gradient gives a representable column')
    dg = u / e                                           # world units: the kernel multiplies by e again (powers of two)
    # ---- the reference: float64 double autograd through the oracle (sigma = y * sel, the identity activation)
    pr = p.clone().requires_grad_(True)
    xw = (x01 / e).clone().requires_grad_(True)
    y = O.network_with_encoding(xw * e, pr, spec)[:, 0]
    sig = y * sel.double()
    (gx,) = torch.autograd.grad(sig.sum(), xw, create_graph=True)
    obj = (gx * dg).sum() + (sig * ds).sum()
    (ref,) = torch.autograd.grad(obj, pr)
    ref = ref.detach()
    # ---- the conditions
    z = torch.cat([F, F.new_zeros(n, spec.n_in - F.shape[1])], 1) @ p[:64 * spec.n_in].view(64, spec.n_in).t()
    live = z[sel]
    assert float((live > 0).double().mean()) >= 0.2 and float((live < 0).double().mean()) >= 0.2, 'too few active / resting hidden units'
    assert bool(exact16(torch.relu(z)).all())
    yd = (gx.detach() * dg).sum(1)
    assert float((yd[sel] != 0).double().mean()) > 0.3, 'dg . g vanishes on most samples'
    assert torch.equal(ref.float().double(), ref) and float((ref * 64).abs().max()) < 2 ** 24 and torch.equal((ref * 64).round(), ref * 64)
    nb = _blocks(ref, spec)
    assert all(float(v.abs().max()) > 0 for v in nb.values()), 'a block of the reference gradient is empty'
    return cfg, mlp, p.float(), x01.float(), sel.to(torch.uint8), e.tolist(), ds.float(), dg.float(), ref.float()


@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('L', [5, 11])               # one and two k-steps of the first layer, padded inputs
def test_exact_data_gives_the_float64_double_autograd(dt, L):
    from perf_amd import ops
    cfg, mlp, p, x01, sel, ie, ds, dg, ref = _exact_case(dt, L, 40 + L)
    w16 = p.to(EG.DT[dt][0]).cuda()
    assert torch.equal(w16.float().cpu(), p)
    got = ops.field_grad_x_bwd(cfg, mlp, x01.cuda(), sel.cuda(), w16, ie, ds.cuda(), dg.cuda()).cpu()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()[:, 0]
        raise AssertionError(f'{len(bad)} of {ref.numel()} entries differ, first at {int(bad[0])} (network part: {mlp.n_params}): kernel '
                             f'{float(got[bad[0]])} reference {float(ref[bad[0]])}')
    # the same through a live count, and with every sample dead
    n = len(x01)
    nd = torch.tensor([n], dtype=torch.int64, device='cuda')
    assert torch.equal(ops.field_grad_x_bwd(cfg, mlp, x01.cuda(), sel.cuda(), w16, ie, ds.cuda(), dg.cuda(), n_dev=nd).cpu(), ref)
    dead = ops.field_grad_x_bwd(cfg, mlp, x01.cuda(), torch.zeros_like(sel).cuda(), w16, ie, ds.cuda(), dg.cuda()).cpu()
    assert float(dead.abs().max()) == 0.0


# ---- 2. random data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,levels', [('bf16', 16), ('fp16', 16), ('fp16', 8)])
def test_random_data_lies_within_two_noise_units_of_the_quantised_oracle(dtype, levels):
    """Per block (W1, row 0 of Wo, each grid level): |kernel - quantised oracle| <= 2 e_q on the whole batch, e_q = the relative L2
    distance between the quantised and the unrounded oracle gradient over the samples whose ReLU masks agree.  The factor 2 is the
    project's rule for two independent sets of 16-bit roundings (the kernel rounds the features, the hidden activations and the
    combined column; the oracle rounds the operands of every product)."""
    c = _case(dtype, levels)
    assert len(c['x']) % 32 != 0 and len(c['x']) - c['n_in'] >= 40
    _check_against_oracle(c, c['ds'], c['dg'], f'{dtype}_L{levels}')


@pytest.mark.parametrize('dtype', ['bf16'])
def test_random_data_above_and_below_the_exponential_clamp(dtype):
    """The 8-level case with its output row times -256: the network output y spreads over about +-70, a third of the samples lie
    above the clamp of the activation's derivative (a'(y) = e^15 and a''(y) = 0 there, as O.trunc_exp's backward and its derivative
    have it) and some below -15.  The scale touches neither the first layer nor the table: the removed samples and the agreeing masks
    are the 8-level case's.  Same reference, same bound.  bf16 only: the fp16 oracle rounds its dH -- e^15 times the output row -- to
    fp16, where e^15 > 65504 is inf, and its gradient is NaN at this scale (the kernels apply the activation's derivatives last, in
    fp32, and stay finite)."""
    c = dict(_case(dtype, 8))
    spec = c['spec']
    n1 = 64 * spec.n_in
    geo = c['geo'].clone()
    geo[n1:n1 + 64] *= -256.0
    c['geo'] = geo
    x_in = c['x'][:c['n_in']]
    y = O.network_with_encoding((x_in - torch.tensor(c['aabb'][:3])) / (torch.tensor(c['aabb'][3:]) - torch.tensor(c['aabb'][:3])), geo.double(), spec)[:, 0]
    above, below = float((y > 15.0).double().mean()), float((y < -15.0).double().mean())
    print(f'[field_grad_x_bwd saturated {dtype}] y in [{float(y.min()):.1f}, {float(y.max()):.1f}], {above:.1%} above the clamp, {below:.1%} below -15')
    assert 0.15 <= above <= 0.5 and below >= 0.02 and float(y.max()) < 85.0          # (the forward stays finite: expf overflows at 88.7)
    _check_against_oracle(c, c['ds'], c['dg'], f'{dtype}_L8_saturated')


# ---- 3. variants ---------------------------------------------------------------------------------------------------------------------
def test_one_upstream_gradient_at_a_time_and_their_sum():
    c = _case('fp16', 16)
    spec = c['spec']
    only_s = _check_against_oracle(c, c['ds'], None, 'fp16_L16_dsigma_only')
    only_g = _check_against_oracle(c, None, c['dg'], 'fp16_L16_dgrad_only')
    joint = _kernel(c, c['ds'], c['dg'])
    jb, sb = _blocks(joint, spec), _blocks(only_s + only_g, spec)
    worst = {}
    for k in jb:
        worst[k] = float((jb[k] - sb[k]).abs().max() / torch.linalg.vector_norm(jb[k]))
    print('[field_grad_x_bwd] |joint - (dsigma only + dgrad only)|_max / |block|: ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    _report('sum_of_the_two_calls_vs_joint', worst)
    # (the two scalars per sample stay in fp32 to the end and the 16-bit operands do not depend on dsigma: the call is linear in
    #  (dsigma, dg) up to fp32 rounding)
    assert all(v <= 1e-6 for v in worst.values()), worst


# ---- 4. counts ---------------------------------------------------------------------------------------------------------------------
def test_live_counts_tile_remainders_and_points_outside():
    c = _case('bf16', 16)
    spec = c['spec']
    n, n_net = len(c['x']), spec.n_net

    def table_close(a, b, what):
        ab, bb = _blocks(a, spec), _blocks(b, spec)
        for k in ab:
            if k.startswith('level'):
                top = float(bb[k].abs().max())
                assert float((ab[k] - bb[k]).abs().max()) <= 1e-6 * top, (what, k)

    for live in (1000, 33, 1, 31, 32, 95):
        exact = _kernel(c, c['ds'], c['dg'], n=live)
        for cap in ((n, 95) if live <= 95 else (n,)):
            got = _kernel(c, c['ds'], c['dg'], n=cap, n_dev=live, grad=torch.full((spec.n_params,), 7.0, device='cuda'))
            assert torch.equal(got[:n_net], exact[:n_net]), (live, cap)
            table_close(got, exact, (live, cap))
    # nothing live: all zeros over a buffer pre-filled with 7
    got = _kernel(c, c['ds'], c['dg'], n_dev=0, grad=torch.full((spec.n_params,), 7.0, device='cuda'))
    assert float(got.abs().max()) == 0.0
    from perf_amd import ops
    empty = ops.field_grad_x_bwd(c['cfg'], c['mlp'], torch.zeros(0, 3, device='cuda'), None, ops.cast_params(c['geo'].cuda(), 'bf16'), None,
                                 torch.zeros(0, device='cuda'), None, grad=torch.full((spec.n_params,), 7.0, device='cuda'))
    assert float(empty.abs().max()) == 0.0
    # points outside the box appended to the batch: the network part is the same to the bit
    inside = _kernel(c, c['ds'], c['dg'], n=c['n_in'])
    full = _kernel(c, c['ds'], c['dg'])
    assert torch.equal(full[:n_net], inside[:n_net])
    table_close(full, inside, 'outside')
    # and the call is repeatable in its network part
    assert torch.equal(_kernel(c, c['ds'], c['dg'])[:n_net], full[:n_net])


# ---- 5. the autograd surface ---------------------------------------------------------------------------------------------------------
def test_density_and_grad_at_is_the_forward_kernel_with_the_fused_backward():
    from perf_amd import ops
    c = _case('fp16', 16)
    nerf = FN._nerf('fp16', c['geo'], c['aabb'])
    x01, sel = ops.points_normalize(c['x'].cuda().contiguous(), nerf._aabb_host)
    s0, g0 = nerf.density_grad_at(x01, sel)
    nerf.geo_mlp.params.grad = None
    sig, grad = nerf.density_and_grad_at(x01, sel)
    assert torch.equal(sig, s0) and torch.equal(grad, g0) and sig.requires_grad and grad.requires_grad
    ds, dg = c['ds'].cuda(), c['dg'].cuda()
    ((sig * ds).sum() + (grad * dg).sum()).backward()
    net = nerf.geo_mlp
    direct = ops.field_grad_x_bwd(net.grid, net.mlp, x01, sel, net.working_copy(), nerf._inv_extent(), ds, dg)
    got = net.params.grad
    n_net = net.mlp.n_params
    assert torch.equal(got[:n_net], direct[:n_net])
    for l in range(16):                              # (the table part is scattered with atomics: the same sums in another order)
        lo, hi = n_net + 2 * int(net.grid.offset[l]), n_net + 2 * (int(net.grid.offset[l]) + int(net.grid.size[l]))
        assert float((got[lo:hi] - direct[lo:hi]).abs().max()) <= 1e-6 * float(direct[lo:hi].abs().max()), l
    # one output alone
    net.params.grad = None
    sig, grad = nerf.density_and_grad_at(x01, sel)
    (grad * dg).sum().backward()
    only_g = ops.field_grad_x_bwd(net.grid, net.mlp, x01, sel, net.working_copy(), nerf._inv_extent(), None, dg)
    assert torch.equal(net.params.grad[:n_net], only_g[:n_net])
    # positions are not trained; the evaluation-only entry stays evaluation-only
    with pytest.raises(NotImplementedError, match='geo_mlp.params only'):
        nerf.density_and_grad_at(x01.clone().requires_grad_(True), sel)
    with torch.enable_grad():
        s1, g1 = nerf.density_grad_at(x01, sel)
    assert not s1.requires_grad and not g1.requires_grad


# ---- 6. the step -----------------------------------------------------------------------------------------------------------------------
def _wall_normals(d, half=(0.9, 0.7, 0.5)):
    """The analytic room seen from its centre: the ray leaves through the wall of axis a = argmin half / |d|, whose normal towards the
    camera is -sign(d_a) e_a (tests/test_gpu_field_normal.py)."""
    h = torch.tensor(half, device=d.device)
    axis = (h / d.abs().clamp_min(1e-12)).argmin(-1)
    n = torch.zeros_like(d)
    n.scatter_(1, axis[:, None], -torch.sign(torch.gather(d, 1, axis[:, None])))
    return n


def _small_scene(weight, seed=0):
    from perf_amd import synthetic
    from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays
    torch.manual_seed(seed); np.random.seed(seed)
    scene = NeRFScene()
    rays = gen_pano_rays(torch.eye(4), 32, 64)
    dist, rgb = synthetic.room(rays.d)
    pool = SupInfoPool()
    pool.register_rays(rays.o, rays.d, rgb, dist, _wall_normals(rays.d.reshape(-1, 3)))
    scene.train_conf.pixel_loss_batch_size = 512
    if weight is not None:
        scene.train_conf.normal_loss_weight = weight
    scene.set_train(); scene.prepare_occupancy(pool); scene.nerf.reset_geo()
    return scene, pool


def _three_steps(scene, pool):
    opt = scene.make_optimizer(scene.nerf.geo_mlp, 1e-3)
    for i in range(3):
        torch.manual_seed(100 + i)
        scene.train_one_step_geo(opt, pool, progress=0.1)
    return scene.nerf.geo_mlp.params.detach().clone()


def test_geometry_step_with_and_without_the_normal_loss():
    from perf_amd.fields import unit_normals
    scene, pool = _small_scene(0.1)
    assert not scene._can_fuse()
    before = scene.nerf.geo_mlp.params.detach().clone()
    after = _three_steps(scene, pool)
    assert not torch.equal(before, after) and torch.isfinite(after).all()
    nl = float(scene.last_losses['normal_loss'])
    b = scene.last_normal_batch
    n_hat = unit_normals(b['grad'])
    n_gt = b['gt_normals'][b['ray_indices']]
    terms = b['weights'] * (1.0 - (n_hat * n_gt).sum(-1))
    again = float(terms[b['keep']].sum() / b['bs'])
    print(f'[step] normal_loss {nl:.6f}, recomputed {again:.6f}, kept samples {int(b["keep"].sum())}')
    assert np.isfinite(nl) and nl > 0 and abs(nl - again) <= 1e-5 * max(abs(again), 1e-6)
    # weight 0 and a train_conf without the attribute: the fused step, as before -- bit-equal to each other
    s0, p0 = _small_scene(0.0)
    s1, p1 = _small_scene(None)
    assert s0._can_fuse() and s1._can_fuse() and not hasattr(s1.train_conf, 'normal_loss_weight')
    a0, a1 = _three_steps(s0, p0), _three_steps(s1, p1)
    assert torch.equal(a0, a1) and 'normal_loss' not in s0.last_losses and 'normal_loss' not in s1.last_losses


# ---- 7. the room -----------------------------------------------------------------------------------------------------------------------
NORMAL_LOSS_WEIGHT = 0.05      # run B's weight: a twentieth of the depth loss' weight (both are means over the batch of O(1) terms);
                               # measured beside it: 0.005 gives +0.978 / 6.6 deg where 0.05 gives +0.997 / 2.1 deg (profiles/field_normal_train.json)


def _train_room(weight):
    from perf_amd import synthetic
    from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays
    torch.manual_seed(0); np.random.seed(0)
    scene = NeRFScene(dtype='fp16')
    rays = gen_pano_rays(torch.eye(4), 256, 512)
    dist, rgb = synthetic.room(rays.d)
    pool = SupInfoPool()
    pool.register_rays(rays.o, rays.d, rgb, dist, _wall_normals(rays.d.reshape(-1, 3)) if weight else None)
    scene.train_conf.pixel_loss_batch_size = 4096
    if weight:
        scene.train_conf.normal_loss_weight = weight
    scene.train_one_episode(pool, 150, 100)
    return scene, dist, rays


def _room_figures(scene, dist, rays):
    """The ray selection and figures of tests/test_gpu_field_normal.test_normals_face_the_camera_on_the_analytic_room."""
    half = torch.tensor((0.9, 0.7, 0.5), device='cuda')
    out = scene.render(rays, ['opacities', 'normal', 'distance'])
    d = rays.d.reshape(-1, 3)
    normal, op = out['normal'].reshape(-1, 3), out['opacities'].reshape(-1)
    t = half / d.abs().clamp_min(1e-12)
    dmin, axis = t.min(-1)
    p = d * dmin[:, None]
    inner = torch.ones_like(op, dtype=torch.bool)
    for a in range(3):
        inner &= (axis == a) | (p[:, a].abs() < 0.8 * half[a])
    pick = inner & (op > 0.9) & (torch.linalg.vector_norm(normal, dim=-1) > 0)
    cos = (normal * _wall_normals(d)).sum(-1)[pick]
    return {'rays': int(pick.sum()), 'mean_normal_dot_wall_normal': float(cos.mean()),
            'median_angular_error_deg': float(torch.rad2deg(torch.acos(cos.clamp(-1, 1))).median()),
            'distance_l1': float((out['distance'].reshape(-1) - dist.reshape(-1)).abs().mean())}


def test_room_normals_improve_with_the_normal_loss():
    """The room of the forward's tests trained twice from the same seeds: A as it is, B with the analytic wall normals in the pool and
    NORMAL_LOSS_WEIGHT.  Over the forward test's ray selection B's mean normal . n_wall must exceed A's (A is the baseline; no absolute
    figure is fixed).  Median angle and the distance map's L1 error are printed and recorded, not asserted."""
    a = _room_figures(*_train_room(None))
    b = _room_figures(*_train_room(NORMAL_LOSS_WEIGHT))
    print(f'[room A, no normal loss] {a}')
    print(f'[room B, weight {NORMAL_LOSS_WEIGHT}] {b}')
    _report('room_fp16_150+100_iterations', {'A_without': a, 'B_with': b, 'normal_loss_weight': NORMAL_LOSS_WEIGHT})
    assert a['rays'] > 1000 and b['rays'] > 1000
    assert b['mean_normal_dot_wall_normal'] > a['mean_normal_dot_wall_normal'], (a, b)
