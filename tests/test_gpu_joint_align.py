"""The joint predictor's alignment step on the GPU (include/perf_hip_joint.h, perf_amd/joint_align.py): perf_joint_sample, perf_joint_loss
and perf_joint_tv against align_step_composed in float64 under torch.autograd, with the same function in float32 on the GPU as the MEASURE
of what an fp32 evaluation may miss (the rule of the sphere field's tests).

Yardstick T: align_step_composed in float64 on the CPU around a float64 restatement of the field (oracle.perf_oracle.hashgrid_encode(...,
'Smoothstep') and the MLP, under autograd).  Measure o: align_step_composed in float32 on the GPU around the fused field.  Held, per
block (u, each record field, each loss term, d loss/d d, d loss/d g, d loss/d scale, each map's gradient, the field's parameter gradients):

    rms(kernels - T) <= 2 rms(o - T) + 2^-24 max |T|

i.e. the relative L2 error is at most twice that of o, plus 2^-24 of the block's largest magnitude (both sides of the relative form
multiplied by rms(T), so that a block that is exactly zero -- TV in the 'global' phase -- is held too).  For a scalar block this reads
|kernels - T| <= 2 |o - T| + 2^-24 |T|.

Both fp32 paths hand the field the SAME fp32 directions (align_step forms u with align_step_composed's torch ops and gives it to the
kernel: perf_amd/joint_align.py says why), so d and g are the same bits in both and the two paths differ by the head's arithmetic only;
asserted.  The rule is held on ONE draw of the inputs per shape and case for every block that is a vector, at all four shapes, and for
every block at the reference's P and B.

The exception, stated here because it departs from a single draw: the seven loss terms at the three small shapes (1, 15 and 201
samples).  Such a block is one number; both paths carry the same inherited error e of the shared fp32 (u, d, g) plus their own
arithmetic, k - T = e + a_k and o - T = e + a_o with |a_k| < |a_o| typically, and whenever a_o happens to cancel e the composed path
lands closer to T than any evaluation of fp32 inputs can be asked to (L_ref at 15 samples: 2.3e-8 against 3.0e-9 with e about 2e-8).
On one draw the rule then tests that coincidence.  These blocks are held over SIXTEEN seeded draws of the inputs, two ways: the rule on
the error pooled over the draws, and -- so that one bad draw cannot hide in the pool -- the worst draw of the kernels against the
worst draw of the composed path, max |k - T| <= 2 max |o - T| + 2^-24 max |T|.  Every draw meets the input conditions on its own.
The directions the kernel forms when it is given none are held separately (test_kernel_formed_directions).

Input conditions, checked on the CPU before either path runs: the mask channel is piecewise constant on 2 x 2 blocks with values {0, 1};
the float64 sampled mask of every sample is further than 1e-3 from 1/2 (a sample that is not is redrawn, and fewer than 1 % of a
case's samples may need it: otherwise [pm < 1/2] would compare a discontinuity, not arithmetic); no direction at a pole; no vanishing s[4:7] + nb.

Every figure is printed before it is asserted; with PERF_JOINT_ALIGN_REPORT=<path> the figures are also written there as JSON."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import perf_oracle as O  # noqa: E402

SHAPES = [(1, 1, 4, 2, 8, 16),           # one live lane
          (3, 5, 6, 4, 8, 16),
          (3, 67, 6, 2, 8, 16),          # crosses a wave; on a 2 x 2 normal map every texel collides
          (60, 256, 12, 6, 16, 32)]      # the reference's P and B on small maps
GRID = dict(n_levels=4, log2_hashmap_size=10, base_res=16, fine_res=2048)          # every level hashed: 2^10 entries collide
WEIGHTS = dict(normal_loss_weight=1e-2, normal_tv_loss_weight=1e-2)
LEAVES = ('table', 'w1', 'b1', 'w2', 'b2', 'w3', 'b3')
SCALAR_SEEDS = tuple(range(7, 7 + 16))          # the draws of the small shapes' loss terms (the first is every other block's draw)
_REPORT = {}


def _report(key, value):
    _REPORT[key] = value
    path = os.environ.get('PERF_JOINT_ALIGN_REPORT')
    if path:
        json.dump(_REPORT, open(path, 'w'), indent=1)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def _rms(x):
    return float(x.double().pow(2).mean().sqrt()) if x.numel() else 0.0


def _figures(name, kernels, o, T, key):
    T = T.detach().double().cpu().reshape(-1)
    k, o = kernels.detach().double().cpu().reshape(-1), o.detach().double().cpu().reshape(-1)
    assert k.shape == T.shape == o.shape, (name, k.shape, o.shape, T.shape)
    ek, eo, slack = _rms(k - T), _rms(o - T), 2.0 ** -24 * float(T.abs().max())
    ok = bool(torch.isfinite(k).all()) and ek <= 2 * eo + slack
    print(f'{key} {name}: kernels rms {ek:.3e} | composed fp32 rms {eo:.3e} | slack {slack:.3e} | rms(T) {_rms(T):.3e} {"" if ok else "  <-- MISSES"}')
    _report(f'{key}/{name}', {'kernels_rms': ek, 'composed_rms': eo, 'slack': slack, 'rms_T': _rms(T), 'holds': ok})
    return ok


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _hand_coords(R):
    """Exactly -1, the largest float below 1, a texel centre, a texel midpoint (of the R x R maps)."""
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    centre = lambda i: (2 * i + 1) / R - 1
    mid = lambda i: (2 * i + 2) / R - 1
    return torch.tensor([[-1., -1.], [below_one, below_one], [centre(1), centre(0)], [mid(1), mid(0)], [-1., below_one], [centre(R - 1), mid(R - 2)]],
                        dtype=torch.float32)


def _sampled64(sup, bias_n, coords, ref):
    """(the float64 sampled mask, u, s[4:7] + nb) of every sample: the input conditions' view of the draw (a torch restatement, CPU)."""
    from perf_amd.joint_align import direction_to_img_coord, img_coord_to_sample_coord
    P, B = coords.shape[:2]
    grid = coords.double().reshape(P, B, 1, 2)
    s = F.grid_sample(sup.double(), grid, padding_mode='border', align_corners=False)[:, :, :, 0].permute(0, 2, 1).reshape(-1, 7)
    nb = F.grid_sample(bias_n.double(), grid, padding_mode='border', align_corners=False)[:, :, :, 0].permute(0, 2, 1).reshape(-1, 3)
    u = s[:, :3] / s[:, :3].norm(dim=-1, keepdim=True)
    sc = img_coord_to_sample_coord(direction_to_img_coord(u))
    pm = F.grid_sample(ref.double()[None], sc[None, :, None, :], padding_mode='border', align_corners=False)[0, 1].reshape(-1)
    return pm, u, s[:, 4:] + nb


@functools.lru_cache(maxsize=None)
def _inputs(shape, seed=7):
    P, B, R, Rn, H, W = shape
    gen = torch.Generator().manual_seed(seed + 1000 * P + B)
    r = lambda *s: torch.randn(*s, generator=gen)
    base = F.normalize(r(P, 3, 1, 1) * torch.tensor([1., 1., 0.3]).view(1, 3, 1, 1), dim=1)
    sup = torch.cat([base + 0.2 * r(P, 3, R, R), 0.5 + 2.5 * torch.rand(P, 1, R, R, generator=gen), -base + 0.2 * r(P, 3, R, R)], 1)
    mask = (torch.rand(H // 2, W // 2, generator=gen) < 0.4).float().repeat_interleave(2, 0).repeat_interleave(2, 1)
    ref = torch.stack([1.0 + 0.12 * r(H, W), mask])          # (the field's distances are about 1.0 +- 0.12: both branches of smooth-L1_0.01)
    a = dict(sup=sup, ref=ref, scale=0.3 * r(P), bias_d=0.05 * r(P, 1, R, R), bias_n=0.1 * r(P, 3, Rn, Rn), ortho=r(P, B, 3))
    coords = (torch.rand(P, B, 1, 2, generator=gen) * 2 - 1).reshape(-1, 2)
    hand = _hand_coords(R)[:max(0, min(len(coords) - 1, 6))]          # (the one-lane shape keeps its random draw)
    coords[:len(hand)] = hand
    coords = coords.reshape(P, B, 1, 2)
    # ---- the input conditions
    assert set(mask.unique().tolist()) <= {0., 1.} and torch.equal(mask, mask.reshape(H // 2, 2, W // 2, 2)[:, :1, :, :1].expand(-1, 2, -1, 2).reshape(H, W))
    pm, _, _ = _sampled64(sup, a['bias_n'], coords, ref)
    close = (pm - 0.5).abs() < 1e-3
    redrawn = int(close.sum())
    for _ in range(8):
        if not bool(close.any()):
            break
        flat = coords.reshape(-1, 2)
        flat[close] = torch.rand(int(close.sum()), 2, generator=gen) * 2 - 1
        pm, _, _ = _sampled64(sup, a['bias_n'], coords, ref)
        close = (pm - 0.5).abs() < 1e-3
    pm, u, rn = _sampled64(sup, a['bias_n'], coords, ref)
    assert not bool(((pm - 0.5).abs() < 1e-3).any())
    assert float(u[:, 2].abs().max()) < 0.999 and float(rn.norm(dim=-1).min()) > 0.05
    print(f'inputs {shape}: {redrawn} of {P * B} samples redrawn; max |u_z| {float(u[:, 2].abs().max()):.4f}; min |sn + nb| {float(rn.norm(dim=-1).min()):.3f}; '
          f'masked share {float((pm >= 0.5).double().mean()):.2f}')
    a['coords'] = coords
    a['redrawn'] = redrawn
    return a


def _field(seed=11):
    """The fused field with the sphere field tests' inputs: sphere_init weights with W1[:, 3:] drawn at std 0.05, table uniform in +-0.1."""
    from perf_amd.sphere_field import SphereDistanceField
    torch.manual_seed(seed)
    f = SphereDistanceField.joint(fused=True, **GRID)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        w = f.geo_mlp.layers[0].weight
        w[:, 3:] = (torch.randn(64, w.shape[1] - 3, generator=g) * 0.05).to(w.device)
        f.hash_grid.params.copy_(((torch.rand(f.hash_grid.params.numel(), generator=g) * 2 - 1) * 0.1).to(w.device))
    f.train()
    return f


def _field_leaves(field):
    net = [p for p in field.geo_mlp.effective_parameters()]
    return dict(zip(LEAVES, [field.hash_grid.params] + net))


class _Field64:
    """The field in float64 under autograd (the yardstick's): distance = softplus(raw + 1), g = d distance / du with its graph."""

    def __init__(self, field):
        b = math.exp(math.log(GRID['fine_res'] / GRID['base_res']) / (GRID['n_levels'] - 1))
        self.lv = O.grid_levels(n_levels=GRID['n_levels'], log2_hashmap_size=GRID['log2_hashmap_size'], base_resolution=GRID['base_res'], per_level_scale=b)
        self.leaves = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in _field_leaves(field).items()}

    def __call__(self, u, requires_grad=True):
        L = self.leaves
        u = u.detach().clone().requires_grad_(True)
        f = O.hashgrid_encode(u * 0.49 + 0.49, L['table'].view(-1, 2), self.lv, 'Smoothstep')
        z1 = torch.cat([u, f], -1) @ L['w1'].t() + L['b1']
        z2 = F.softplus(z1, beta=100) @ L['w2'].t() + L['b2']
        raw = -(F.softplus(z2, beta=100) @ L['w3'].t() + L['b3'])[:, 0]
        d = F.softplus(raw + 1.)
        (g,) = torch.autograd.grad(d.sum(), u, create_graph=True)
        return d, g


def _leaf_args(a, device, dtype):
    out = {k: v.to(device=device, dtype=dtype).contiguous() for k, v in a.items() if k != 'redrawn'}
    for k in ('scale', 'bias_d', 'bias_n'):
        out[k].requires_grad_(True)
    return out


# ---- one reference per case, shared and left unchanged ---------------------------------------------------------------------------------
def _pool(cases, pick):
    """One block of a case, flattened."""
    return torch.cat([pick(c).detach().double().cpu().reshape(-1) for c in cases])


@functools.lru_cache(maxsize=None)
def _case(shape, hybrid, progress, w_reg, seed=7):
    """One draw of the inputs per shape and case (a list of one: the tests below are written over a list)."""
    redrawn = _inputs(shape, seed)['redrawn']
    assert redrawn < 0.01 * shape[0] * shape[1], (redrawn, shape)
    return [_one_case(shape, hybrid, progress, w_reg, seed)]


def _one_case(shape, hybrid, progress, w_reg, seed):
    from perf_amd.joint_align import align_step, align_step_composed
    a = _inputs(shape, seed)
    field = _field()
    kw = dict(progress=progress, hybrid=hybrid, reg_loss_weight=w_reg, **WEIGHTS)
    out = {}
    # T: float64 on the CPU
    f64 = _Field64(field)
    a64 = _leaf_args(a, 'cpu', torch.float64)
    out['T'] = (align_step_composed(f64, **a64, **kw), a64, {k: v.grad for k, v in f64.leaves.items()})
    out['d64'] = f64(out['T'][0].u)[0].detach()
    # o: the same function in float32 on the GPU, around the fused field; then the kernels, on the same draws
    for name, fn in (('o', align_step_composed), ('k', align_step)):
        field.zero_grad()
        args = _leaf_args(a, 'cuda', torch.float32)
        step = fn(field, **args, **kw)
        grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in
                 zip(LEAVES, [field.hash_grid.params] + [getattr(field.geo_mlp.layers[i], n) for i in (0, 2, 4) for n in ('weight', 'bias')])}
        out[name] = (step, args, grads)
    torch.cuda.synchronize()
    return out


CASES = [(s, h, p, w) for s in SHAPES for h in (False, True) for p in (0.0, 0.75) for w in (0.0, 0.1)]


@pytest.mark.parametrize('shape,hybrid,progress,w_reg', CASES)
def test_step_parity(shape, hybrid, progress, w_reg):
    from perf_amd.joint_align import LOSS_NAMES
    cases = _case(shape, hybrid, progress, w_reg)
    key = f'step/{"x".join(map(str, shape))}/{"hybrid" if hybrid else "global"}/p{progress}/w{w_reg}'

    def hold(name, pick):
        return _figures(name, _pool(cases, lambda c: pick(c['k'])), _pool(cases, lambda c: pick(c['o'])), _pool(cases, lambda c: pick(c['T'])), key)

    ok = [hold('u', lambda r: r[0].u)]
    ok += [hold(f'record.{f}', lambda r, f=f: r[0].record[f]) for f in ('sd', 'db', 'sn', 'nb', 'pr', 'pm')]
    if shape[0] * shape[1] >= 1000:
        ok += [hold(f'loss.{n}', lambda r, n=n: r[0].losses[n]) for n in LOSS_NAMES]
    else:            # a loss term of 1, 15 or 201 samples: sixteen draws, the pooled rule and the worst draw (module docstring)
        draws = [_case(shape, hybrid, progress, w_reg, seed)[0] for seed in SCALAR_SEEDS]
        for n in LOSS_NAMES:
            k, o, T = (_pool(draws, lambda c, w=w: c[w][0].losses[n]) for w in ('k', 'o', 'T'))
            ok.append(_figures(f'loss.{n}[{len(draws)} draws]', k, o, T, key))
            worst_k, worst_o, slack = float((k - T).abs().max()), float((o - T).abs().max()), 2.0 ** -24 * float(T.abs().max())
            print(f'{key} loss.{n}: worst draw kernels {worst_k:.3e} | composed fp32 {worst_o:.3e} | slack {slack:.3e}')
            _report(f'{key}/loss.{n}/worst', {'kernels': worst_k, 'composed': worst_o, 'slack': slack})
            ok.append(worst_k <= 2 * worst_o + slack)
    ok += [hold('dd', lambda r: r[0].dd), hold('dg', lambda r: r[0].dg), hold('dscale', lambda r: r[1]['scale'].grad)]
    if hybrid:
        ok += [hold(f'grad.{m}', lambda r, m=m: r[1][m].grad) for m in ('bias_d', 'bias_n')]
    for c in cases:
        (T, aT, _), (o, _, _), (k, ak, _) = c['T'], c['o'], c['k']
        assert torch.equal(k.u, o.u)           # the same bits go to the field in both paths
        if not hybrid:
            assert ak['bias_d'].grad is None and ak['bias_n'].grad is None          # the 'global' phase leaves the maps alone
        # the [pm < 1/2] decisions are the same in all three (the input condition at work)
        assert torch.equal(k.record['pm'].cpu() < .5, T.record['pm'] < .5) and torch.equal(o.record['pm'].cpu() < .5, T.record['pm'] < .5)
    if shape[0] * shape[1] > 10000:        # both branches of the two smooth-L1 terms are visited
        (T, aT, _), B = cases[0]['T'], shape[1]
        rd = T.record['sd'][:, 0] * F.softplus(aT['scale'].detach()).repeat_interleave(B) + T.record['db'][:, 0]
        d64 = cases[0]['d64']
        quad_d, quad_ref = float(((rd - d64).abs() < .5).double().mean()), float(((T.record['pr'][:, 0] - d64).abs() < .01).double().mean())
        print(f'{key}: quadratic branch of L_d {quad_d:.3f}, of L_ref {quad_ref:.3f}')
        assert 0.05 < quad_d < 0.95 and 0.005 < quad_ref < 0.95
    assert all(ok), key


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('hybrid', [False, True])
def test_field_gradients_are_handed_over(shape, hybrid):
    """The field's parameter gradients after align_step and after align_step_composed on the same draws, against the yardstick's."""
    cases = _case(shape, hybrid, 0.75, 0.1)
    key = f'field/{"x".join(map(str, shape))}/{"hybrid" if hybrid else "global"}'
    ok = [_figures(leaf, _pool(cases, lambda c: c['k'][2][leaf]), _pool(cases, lambda c: c['o'][2][leaf]), _pool(cases, lambda c: c['T'][2][leaf]), key)
          for leaf in LEAVES]
    assert all(float(c['T'][2]['table'].abs().max()) > 0 and float(c['T'][2]['w1'].abs().max()) > 0 for c in cases)
    assert all(ok), key


def test_sampled_fields_are_exact_on_dyadic_maps():
    """Maps of small dyadic values, coordinates at texel centres and midpoints: every bilinear weight is 1, 1/2, 1/4 or 3/4 (and their
    products), every sum is exact in fp32, and the sampled record fields equal the float64 yardstick's TO THE BIT."""
    from perf_amd import ops
    P, R, Rn, H, W = 2, 8, 4, 8, 16
    gen = torch.Generator().manual_seed(3)
    dy = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float() / 16
    sup = torch.cat([dy(1, 32, P, 3, R, R), dy(-32, 32, P, 4, R, R)], 1)
    bias_d, bias_n, ref = dy(-32, 32, P, 1, R, R), dy(-32, 32, P, 3, Rn, Rn), dy(0, 32, 2, H, W)
    ticks = torch.tensor([(k + 1) / R - 1 for k in range(2 * R - 1)])          # centres (even k) and midpoints (odd k) of the R axis, exact
    xy = torch.cartesian_prod(ticks, ticks)
    coords = xy[None].expand(P, -1, -1).contiguous()
    B = coords.shape[1]
    grid = coords.double().reshape(P, B, 1, 2)
    want = {name: F.grid_sample(m.double(), grid, padding_mode='border', align_corners=False)[:, :, :, 0].permute(0, 2, 1).reshape(P * B, -1)
            for name, m in (('s', sup), ('db', bias_d), ('nb', bias_n))}
    _, rec = ops.joint_sample(sup.cuda(), bias_d.cuda(), bias_n.cuda(), ref.cuda(), coords.cuda())
    rec = rec.cpu()
    got = {'sd': rec[:, 0:1], 'db': rec[:, 1:2], 'sn': rec[:, 2:5], 'nb': rec[:, 5:8]}
    wants = {'sd': want['s'][:, 3:4], 'db': want['db'], 'sn': want['s'][:, 4:7], 'nb': want['nb']}
    for name in got:
        assert torch.equal(wants[name].float().double(), wants[name]), name              # the yardstick's values ARE fp32 numbers
        assert torch.equal(got[name], wants[name].float()), name
        assert float(wants[name].abs().max()) > 0
    assert bool(torch.isfinite(rec).all()) and torch.equal(rec[:, 10:], torch.zeros(P * B, 2))


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_formed_directions(shape):
    """perf_joint_sample without given directions forms u itself, in double, and rounds once: every component lies within half an fp32
    ulp of 1 (2^-24) of float64, and the sampled record fields are those it writes for the same directions given back to it."""
    from perf_amd import ops
    a = _inputs(shape)
    P, B = shape[:2]
    args = {k: a[k].cuda().contiguous() for k in ('sup', 'bias_d', 'bias_n', 'ref')}
    coords = a['coords'].reshape(P, B, 2).cuda().contiguous()
    u, rec = ops.joint_sample(**args, coords=coords)
    _, u64, _ = _sampled64(a['sup'], a['bias_n'], a['coords'], a['ref'])
    err = float((u.double().cpu() - u64).abs().max())
    print(f'kernel-formed u {shape}: max abs error {err:.3e} (2^-24 = {2.0 ** -24:.3e})')
    assert err <= 2.0 ** -24 * (1 + 1e-6)
    u2, rec2 = ops.joint_sample(**args, coords=coords, u=u)
    assert u2 is u and torch.equal(rec[:, :8], rec2[:, :8]) and torch.allclose(rec[:, 8:], rec2[:, 8:], atol=1e-5)          # (pr, pm: the look-up takes the rounded u)


def test_deterministic_outputs_are_bit_identical_between_runs():
    from perf_amd.joint_align import LOSS_NAMES, align_step
    a = _inputs(SHAPES[3])
    field = _field()
    runs = []
    for _ in range(2):
        field.zero_grad()
        args = _leaf_args(a, 'cuda', torch.float32)
        step = align_step(field, **args, progress=0.75, hybrid=True, reg_loss_weight=0.1, **WEIGHTS)
        runs.append([step.losses[n].clone() for n in LOSS_NAMES] + [step.dd.clone(), step.dg.clone(), args['scale'].grad.clone(), step.u.clone()]
                    + [v.clone() for v in step.record.values()])
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert all(bool(torch.isfinite(x).all()) for x in runs[0]) and float(runs[0][7].abs().max()) > 0


@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (3, 3, 5, 7), (2, 1, 64, 65), (2, 1, 9, 64)])
def test_tv_kernel(shape):
    """perf_joint_tv: bit-identical between two runs (value and gradient map), and both held by the rule against float64 autograd.
    (1,1,2,2): every entry is a corner; (3,3,5,7) and (2,1,64,65): the scalar path, rows that are no multiple of the strip;
    (2,1,9,64): the float4 path with a strip of one row."""
    from perf_amd import ops
    from perf_amd.joint_align import _tv
    gen = torch.Generator().manual_seed(sum(shape))
    m = 0.02 * torch.randn(*shape, generator=gen)              # differences on both sides of beta = 0.01
    share = float(((m[:, :, 1:] - m[:, :, :-1]).abs() < 0.01).float().mean())
    assert shape[2] * shape[3] < 16 or 0.1 < share < 0.9
    ref = {}
    for name, t in (('T', m.double()), ('o', m.cuda())):
        t = t.clone().requires_grad_(True)
        v = _tv(t)
        (0.25 * v).backward()
        ref[name] = (v.detach(), t.grad)
    runs = []
    for _ in range(2):
        grad = torch.full(shape, float('nan'), device='cuda')          # (written in full: no zero-fill is needed)
        value, grad = ops.joint_tv(m.cuda(), 0.25, grad=grad)
        runs.append((value.clone(), grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    key = 'tv/' + 'x'.join(map(str, shape))
    ok = [_figures('value', runs[0][0], ref['o'][0], ref['T'][0], key), _figures('grad', runs[0][1], ref['o'][1], ref['T'][1], key)]
    assert all(ok), key


def test_global_phase_leaves_the_maps_gradients_alone():
    from perf_amd.joint_align import align_step
    a = _inputs(SHAPES[1])
    field = _field()
    args = _leaf_args(a, 'cuda', torch.float32)
    kept_d, kept_n = torch.full_like(args['bias_d'], 3.0), torch.full_like(args['bias_n'], -2.0)
    args['bias_d'].grad, args['bias_n'].grad = kept_d, kept_n
    align_step(field, **args, progress=0.25, hybrid=False, reg_loss_weight=0.1, **WEIGHTS)
    assert args['bias_d'].grad is kept_d and args['bias_n'].grad is kept_n
    assert bool((kept_d == 3.0).all()) and bool((kept_n == -2.0).all())
    # the hybrid phase writes the same tensors in full (no stale value survives), and the field and the scales got their gradients
    align_step(field, **args, progress=0.75, hybrid=True, reg_loss_weight=0.1, **WEIGHTS)
    assert args['bias_d'].grad is kept_d and float(kept_d.abs().max()) < 1.0 and float(kept_n.abs().max()) < 1.0
    assert args['scale'].grad is not None and field.hash_grid.params.grad is not None


# ---- a short fit -----------------------------------------------------------------------------------------------------------------------
def _fit(fused, seed, iters=40, batch=4096):
    """JointAligner on the analytic room: its 64 x 128 distance map as the panorama, three perspective views of it at R = 16 as the
    supervision (the room's distance along the view's directions over its mean, as a depth predictor's output is normalised, and the
    room's inward wall normals: a supervision the field CAN fit, so that the final loss measures the fit and not the residue of
    contradicting terms), T = 2^12, 40 + 40 iterations.

    The field is the runner's (SphereDistanceField.joint: 16 levels to resolution 2048).  The loop draws 4,096 samples per view (16 per
    texel of a 16 x 16 map), not JointAligner's default 256: at 256 the loop is not repeatable from one seed in EITHER path -- the
    order in which atomics retire (torch's grid_sample backward, the table gradient) is enough to move a final loss from 0.011 to
    0.027 -- so no fit comparison covers that regime; at 4,096 either path repeats to about 1e-4 of a final loss of 0.003-0.005."""
    from perf_amd import synthetic
    from perf_amd.joint_align import JointAligner, panorama_to_pers_directions
    from perf_amd.scene import gen_pano_rays
    from perf_amd.sphere_field import SphereDistanceField
    rays = gen_pano_rays(torch.eye(4), 64, 128)
    dist_map = synthetic.room(rays.d.reshape(-1, 3).cuda())[0][:, 0].reshape(64, 128)
    mask = torch.zeros(64, 128, device='cuda')
    mask[20:44, 30:70] = 1.0                                    # the part "to be inpainted": no panorama term there
    dirs = panorama_to_pers_directions(gen_res=16, ratio=1.1)[0][:3].cuda()          # [3, 16, 16, 3]
    dist = synthetic.room(dirs.reshape(-1, 3))[0][:, 0].reshape(3, 1, 16, 16)
    flat = dirs.reshape(-1, 3)
    axis = (torch.tensor((0.9, 0.7, 0.5), device='cuda') / flat.abs().clamp_min(1e-12)).argmin(-1)          # the wall a direction hits (synthetic.room's half extents)
    rows = torch.arange(len(flat), device='cuda')
    normals = torch.zeros_like(flat)
    normals[rows, axis] = -torch.sign(flat[rows, axis])
    sup = torch.cat([dirs.permute(0, 3, 1, 2), dist / dist.mean(), normals.reshape(3, 16, 16, 3).permute(0, 3, 1, 2)], 1).contiguous()
    torch.manual_seed(seed)
    np.random.seed(seed)
    aligner = JointAligner(field=SphereDistanceField.joint(log2_hashmap_size=12), fused=fused)
    aligner.align(sup, torch.stack([dist_map, mask]).contiguous(), iters=iters, reg_loss_weight=0.0, batch=batch, normal_res=8)
    losses = torch.stack(aligner.history).cpu()
    assert len(losses) == 2 * iters and bool(torch.isfinite(losses).all())
    return float(losses[0]), float(losses[-5:].mean())


def test_short_fit_matches_the_composed_paths_spread():
    """Fused and composed from the SAME three seeds.  On every seed the fused final loss (the mean of the last five totals; the total's
    panorama term grows with the progress, so first and final are not compared) lies no further from the composed one of that seed
    than the composed path's own finals lie apart between seeds (max - min over the three)."""
    seeds = (101, 202, 303)
    composed = [_fit(False, s) for s in seeds]
    fused = [_fit(True, s) for s in seeds]
    finals = [c[1] for c in composed]
    spread = max(finals) - min(finals)
    print(f'short fit: composed first/final {composed}, fused first/final {fused}; composed seed-to-seed spread {spread:.5f}')
    _report('fit', {'seeds': seeds, 'composed': composed, 'fused': fused, 'composed_spread': spread})
    assert spread > 0.0
    for f, c in zip(fused, composed):
        assert abs(f[1] - c[1]) < spread, (f, c, spread)
