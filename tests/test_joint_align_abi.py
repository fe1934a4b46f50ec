"""The joint predictor's alignment step (include/perf_hip_joint.h, perf_amd/joint_align.py) checked without a GPU: the header's constants and
parameter types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal happens
before a launch with a message that names its reason; the Python surface has the reference's signatures and defaults;
install_joint_predictor_shim rebinds one method on a decoy tree and nothing is rebound without the call; the torch restatement of the
iteration agrees with itself across precisions; the restated panorama look-up coordinates and perspective views reproduce the reference's
recorded outputs (tests/golden/make_joint_fixture.py), and the view set has the properties the loop relies on."""
import ctypes
import importlib
import inspect
import os
import sys
import textwrap

import numpy as np
import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

FAKE = ctypes.c_void_p(16)   # never dereferenced: every call of this file is refused before a launch


def _sample(**kw):
    a = {'sup': FAKE, 'bias_d': FAKE, 'bias_n': FAKE, 'ref': FAKE, 'coords': FAKE, 'u_given': None, 'P': 3, 'B': 5, 'R': 6, 'Rn': 4, 'H': 8, 'W': 16, 'u': FAKE, 'rec': FAKE}
    a.update(kw)
    return _call('perf_joint_sample', a['sup'], a['bias_d'], a['bias_n'], a['ref'], a['coords'], a['u_given'], a['P'], a['B'], a['R'], a['Rn'], a['H'], a['W'],
                 a['u'], a['rec'], None)


def _loss(**kw):
    a = {k: FAKE for k in ('rec', 'coords', 'scale', 'u', 'd', 'g', 'o', 'tv', 'losses', 'dd', 'dg', 'dscale', 'gbias_d', 'gbias_n', 'ws')}
    a.update({'P': 3, 'B': 5, 'R': 6, 'Rn': 4, 'ws_bytes': 1 << 30})
    a.update(kw)
    return _call('perf_joint_loss', a['rec'], a['coords'], a['scale'], a['u'], a['d'], a['g'], a['o'], a['P'], a['B'], a['R'], a['Rn'], 1.0, 0.1, 0.01, 0.01,
                 a['tv'], a['losses'], a['dd'], a['dg'], a['dscale'], a['gbias_d'], a['gbias_n'], a['ws'], a['ws_bytes'], None)


def _tv(**kw):
    a = {'map': FAKE, 'n': 3, 'C': 3, 'H': 5, 'W': 7, 'grad': FAKE, 'value': FAKE, 'ws': FAKE, 'ws_bytes': 1 << 30}
    a.update(kw)
    return _call('perf_joint_tv', a['map'], a['n'], a['C'], a['H'], a['W'], 1.0, a['grad'], a['value'], a['ws'], a['ws_bytes'], None)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [joint] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, _ = abi_units.header('joint')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_JOINT_ABI_VERSION') == _lib.JOINT_ABI_VERSION == 1
    assert list(inspect.signature(abi_units.abi_digest().digest).parameters) == ['path', 'macro']
    assert const('PERF_JOINT_RECORD') == _lib.JOINT_RECORD == 12
    assert const('PERF_JOINT_LOSSES') == _lib.JOINT_LOSSES == 8


def test_refuses_null_pointers_and_counts():
    for kw in ({'sup': None}, {'bias_d': None}, {'bias_n': None}, {'ref': None}, {'coords': None}):
        rc, msg = _sample(**kw)
        assert rc == PERF_E_INVALID and 'NULL input' in msg, (kw, msg)
    for kw in ({'u': None}, {'rec': None}):
        rc, msg = _sample(**kw)
        assert rc == PERF_E_INVALID and 'NULL output' in msg, (kw, msg)
    for kw in ({'rec': None}, {'coords': None}, {'scale': None}, {'u': None}, {'d': None}, {'g': None}, {'o': None}):
        rc, msg = _loss(**kw)
        assert rc == PERF_E_INVALID and 'NULL input' in msg, (kw, msg)
    for kw in ({'losses': None}, {'dd': None}, {'dg': None}, {'dscale': None}):
        rc, msg = _loss(**kw)
        assert rc == PERF_E_INVALID and 'NULL output' in msg, (kw, msg)
    for kw in ({'gbias_d': None}, {'gbias_n': None}):
        rc, msg = _loss(**kw)
        assert rc == PERF_E_INVALID and 'both or neither' in msg, (kw, msg)
    for call in (_sample, _loss):
        for kw, word in (({'P': -1}, 'negative'), ({'B': -1}, 'negative'), ({'P': 0}, 'empty'), ({'B': 0}, 'empty'), ({'R': 0}, 'without texels'),
                         ({'Rn': -2}, 'without texels'), ({'P': 1 << 20, 'B': 1 << 20}, '2^30')):
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and word in msg, (kw, msg)
    rc, msg = _sample(u=None, u_given=FAKE, P=0)              # (given directions: u need not exist; the call is refused for its count)
    assert rc == PERF_E_INVALID and 'empty' in msg, msg
    for call in (_sample, _loss):
        rc, msg = call(P=1, B=(1 << 20) + 1)
        assert rc == PERF_E_INVALID and '2^20' in msg, msg
    for kw in ({'H': 0}, {'W': -1}):
        rc, msg = _sample(**kw)
        assert rc == PERF_E_INVALID and 'panorama without texels' in msg, (kw, msg)
    rc, msg = _sample(rec=ctypes.c_void_p(20))
    assert rc == PERF_E_INVALID and '16-byte aligned' in msg, msg


def test_tv_refuses_small_maps_null_pointers_and_counts():
    from perf_amd import _lib
    lib = _lib.load()
    for kw in ({'H': 1}, {'W': 1}, {'H': 0}, {'W': 0}):
        rc, msg = _tv(**kw)
        assert rc == PERF_E_INVALID and 'at least 2' in msg, (kw, msg)
        assert lib.perf_joint_tv_workspace_bytes(3, 3, kw.get('H', 5), kw.get('W', 7)) == -1
    for kw in ({'n': -1}, {'C': -1}, {'H': -3}, {'W': -3}):
        rc, msg = _tv(**kw)
        assert rc == PERF_E_INVALID and 'negative' in msg, (kw, msg)
    for kw in ({'n': 0}, {'C': 0}):
        rc, msg = _tv(**kw)
        assert rc == PERF_E_INVALID and 'empty map' in msg, (kw, msg)
    rc, msg = _tv(map=None)
    assert rc == PERF_E_INVALID and 'NULL input' in msg, msg
    for kw in ({'grad': None}, {'value': None}):
        rc, msg = _tv(**kw)
        assert rc == PERF_E_INVALID and 'NULL output' in msg, (kw, msg)


def test_refuses_a_bad_workspace():
    from perf_amd import _lib
    lib = _lib.load()
    for call in (_loss, _tv):
        rc, msg = call(ws=None)
        assert rc == PERF_E_INVALID and 'NULL workspace' in msg, msg
        rc, msg = call(ws_bytes=16)
        assert rc == PERF_E_INVALID and 'workspace' in msg and 'bytes' in msg, msg
        rc, msg = call(ws=ctypes.c_void_p(20))
        assert rc == PERF_E_INVALID and '16-byte aligned' in msg, msg
    need = lib.perf_joint_loss_workspace_bytes(60, 256)
    assert need % 16 == 0 and need >= 8 * 60 * 256           # (a double per sample and the workgroups' partials)
    rc, msg = _loss(P=60, B=256, ws_bytes=need - 16)
    assert rc == PERF_E_INVALID and 'workspace' in msg, msg
    assert lib.perf_joint_loss_workspace_bytes(-1, 4) == -1 and lib.perf_joint_loss_workspace_bytes(4, 0) == -1
    tv = lib.perf_joint_tv_workspace_bytes(60, 1, 384, 384)
    assert tv % 16 == 0 and tv == lib.perf_joint_tv_workspace_bytes(1, 1, 2, 2)           # (a fixed number of partials, whatever the map)


def test_python_surface():
    import perf_amd
    from perf_amd import joint_align, ops
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items() if k != 'self']
    E = inspect.Parameter.empty
    step = [('field', E), ('sup', E), ('ref', E), ('scale', E), ('bias_d', E), ('bias_n', E), ('coords', E), ('ortho', E), ('progress', E), ('hybrid', E),
            ('reg_loss_weight', 1e-1), ('normal_loss_weight', 1e-2), ('normal_tv_loss_weight', 1e-2)]
    assert params(joint_align.align_step_composed) == step
    assert params(joint_align.align_step) == step + [('scratch', None)]
    assert params(joint_align.JointAligner.__init__) == [('field', None), ('fused', True)]
    assert params(joint_align.JointAligner.align)[:6] == [('sup', E), ('ref_distance_mask', E), ('iters', 1500), ('reg_loss_weight', 1e-1), ('normal_loss_weight', 1e-2),
                                                           ('normal_tv_loss_weight', 1e-2)]
    assert params(joint_align.PanoJointPredictor.__init__) == [('depth_predictor', E), ('normal_predictor', E), ('fused', True)]
    # the reference's __call__ (pano_joint_predictor.py:101-102): same names, same defaults
    assert params(joint_align.PanoJointPredictor.__call__) == [('img', E), ('ref_distance', E), ('mask', E), ('gen_res', 384), ('reg_loss_weight', 1e-1),
                                                                ('normal_loss_weight', 1e-2), ('normal_tv_loss_weight', 1e-2)]
    assert (joint_align.JointAligner.LR_ALPHA, joint_align.JointAligner.LR_GLOBAL, joint_align.JointAligner.LR_FIELD, joint_align.JointAligner.LR_LOCAL) == (1e-2, 1e-1, 1e-2, 1e-1)
    assert [k for k, _ in params(ops.joint_sample)] == ['sup', 'bias_d', 'bias_n', 'ref', 'coords', 'u']
    assert [k for k, _ in params(ops.joint_tv)] == ['m', 'weight', 'grad', 'value', 'ws']
    assert [k for k, _ in params(ops.joint_loss)] == ['rec', 'coords', 'scale', 'u', 'd', 'g', 'o', 'R', 'Rn', 'w_ref', 'w_reg', 'w_n', 'w_ntv', 'tv', 'gbias_d',
                                                      'gbias_n', 'ws']
    assert params(perf_amd.install_joint_predictor_shim) == [] and params(perf_amd.uninstall_joint_predictor_shim) == []
    assert list(inspect.signature(perf_amd.install_shims).parameters) == ['scene', 'sphere_field']
    import torch
    with pytest.raises(perf_amd._lib.PerfError):           # no fallback: a CPU tensor is refused
        ops.joint_tv(torch.zeros(1, 1, 4, 4))


# ---- install_joint_predictor_shim on a decoy tree --------------------------------------------------------------------------------------
DECOY = textwrap.dedent('''
    MARKER = {marker!r}


    class SphereDistanceField:
        def __init__(self, n_levels=16, log2_hashmap_size=19, base_res=16, fine_res=2048):
            self.decoy = True


    class PanoJointPredictor:
        def __init__(self):
            self.depth_predictor, self.normal_predictor = 'depth', 'normal'

        def grads_to_normal(self, grads):
            return 'decoy normals'

        def __call__(self, img, ref_distance, mask, gen_res=384):
            return 'decoy call'
''')
NAME = 'modules.geo_predictors.pano_joint_predictor'


@pytest.fixture
def decoy_tree(tmp_path):
    pkg = tmp_path / 'modules' / 'geo_predictors'
    pkg.mkdir(parents=True)
    (tmp_path / 'modules' / '__init__.py').write_text('')
    (pkg / '__init__.py').write_text('')
    (pkg / 'pano_joint_predictor.py').write_text(DECOY.format(marker='joint'))
    (pkg / 'bystander.py').write_text(DECOY.format(marker='bystander'))
    saved_path, saved_meta = list(sys.path), list(sys.meta_path)
    saved_mods = {k: v for k, v in sys.modules.items() if k == 'modules' or k.startswith('modules.')}
    for k in saved_mods:
        del sys.modules[k]
    sys.path.insert(0, str(tmp_path))
    importlib.invalidate_caches()
    yield tmp_path
    sys.path[:], sys.meta_path[:] = saved_path, saved_meta
    for k in [k for k in sys.modules if k == 'modules' or k.startswith('modules.')]:
        del sys.modules[k]
    sys.modules.update(saved_mods)


def _finders():
    import perf_amd
    return [f for f in sys.meta_path if isinstance(f, perf_amd._JointPredictorFinder)]


def test_shim_rebinds_the_one_method(decoy_tree):
    import perf_amd
    from perf_amd import joint_align
    perf_amd.install_joint_predictor_shim()
    perf_amd.install_joint_predictor_shim()        # (idempotent)
    assert len(_finders()) == 1 and sys.meta_path[0] is _finders()[0]
    mod = importlib.import_module(NAME)
    assert mod.__file__ == str(decoy_tree / 'modules' / 'geo_predictors' / 'pano_joint_predictor.py')      # loaded from its real file
    cls = mod.PanoJointPredictor
    assert cls.__call__ is joint_align.PanoJointPredictor.__call__
    assert cls.__module__ == NAME and cls.__name__ == 'PanoJointPredictor'
    inst = cls()                                   # the reference's __init__ is kept
    assert (inst.depth_predictor, inst.normal_predictor) == ('depth', 'normal') and inst.grads_to_normal(None) == 'decoy normals'
    # nothing else of the module changed, and the sphere field's global is install_shims' business, not this shim's
    assert mod.MARKER == 'joint' and mod.SphereDistanceField().decoy is True
    assert sorted(k for k in vars(mod) if not k.startswith('__')) == ['MARKER', 'PanoJointPredictor', 'SphereDistanceField']
    other = importlib.import_module('modules.geo_predictors.bystander')
    assert other.PanoJointPredictor()(None, None, None) == 'decoy call'           # a module that is not the one keeps its own method
    perf_amd.uninstall_joint_predictor_shim()
    assert not _finders() and NAME not in sys.modules
    assert importlib.import_module(NAME).PanoJointPredictor()(None, None, None) == 'decoy call'


def test_shim_composes_with_the_sphere_field_shim_and_rebinds_a_loaded_module(decoy_tree):
    import perf_amd
    from perf_amd import joint_align
    from perf_amd.sphere_field import SphereDistanceField
    perf_amd.install_shims(sphere_field=True)
    perf_amd.install_joint_predictor_shim()
    mod = importlib.import_module(NAME)
    assert mod.PanoJointPredictor.__call__ is joint_align.PanoJointPredictor.__call__ and mod.SphereDistanceField == SphereDistanceField.joint
    perf_amd.uninstall_joint_predictor_shim()
    perf_amd.uninstall_sphere_field_shims()
    mod = importlib.import_module(NAME)            # imported plain ...
    assert mod.PanoJointPredictor()(None, None, None) == 'decoy call'
    perf_amd.install_joint_predictor_shim()        # ... and rebound on the spot
    assert mod.PanoJointPredictor.__call__ is joint_align.PanoJointPredictor.__call__
    perf_amd.uninstall_joint_predictor_shim()


@pytest.mark.parametrize('kwargs', [{}, {'scene': True}, {'sphere_field': True}])
def test_without_the_call_nothing_is_rebound(decoy_tree, kwargs):
    import perf_amd
    perf_amd.install_shims(**kwargs)
    assert not _finders()
    mod = importlib.import_module(NAME)
    assert mod.PanoJointPredictor()(None, None, None) == 'decoy call' and mod.PanoJointPredictor.__call__.__module__ == NAME
    perf_amd.uninstall_sphere_field_shims()


# ---- the torch restatement against itself ------------------------------------------------------------------------------------------------
class _ToyField:
    """A smooth distance over the sphere with two parameters, any dtype: enough to carry d, g and their graph through the step."""

    def __init__(self, torch, dtype):
        self.w = torch.tensor([0.3, -0.2, 0.5], dtype=dtype, requires_grad=True)
        self.c = torch.tensor(1.2, dtype=dtype, requires_grad=True)
        self.torch = torch

    def __call__(self, u, requires_grad=False):
        torch = self.torch
        u = u.detach().clone().requires_grad_(True)
        d = torch.nn.functional.softplus(self.c + torch.sin(3.0 * (u @ self.w)) * 0.4 + 0.2 * u[:, 0] * u[:, 1])
        g, = torch.autograd.grad(d.sum(), u, create_graph=True)
        return d, g


def _toy_inputs(torch, P=3, B=7, R=6, Rn=4, H=8, W=16, seed=5):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    base = torch.nn.functional.normalize(r(P, 3, 1, 1), dim=1)
    sup = torch.cat([base + 0.3 * r(P, 3, R, R), 1.5 + torch.rand(P, 1, R, R, generator=gen), -base + 0.3 * r(P, 3, R, R)], 1)
    mask = (torch.rand(H // 2, W // 2, generator=gen) < 0.4).float().repeat_interleave(2, 0).repeat_interleave(2, 1)
    ref = torch.stack([1.5 + 0.3 * r(H, W), mask])
    return dict(sup=sup, ref=ref, scale=0.3 * r(P), bias_d=0.05 * r(P, 1, R, R), bias_n=0.1 * r(P, 3, Rn, Rn),
                coords=torch.rand(P, B, 1, 2, generator=gen) * 2 - 1, ortho=r(P, B, 3))


@pytest.mark.parametrize('hybrid', [False, True])
def test_composed_step_in_float32_agrees_with_float64(hybrid):
    import torch
    from perf_amd.joint_align import LOSS_NAMES, align_step_composed
    outs = {}
    for dtype in (torch.float64, torch.float32):
        a = {k: v.to(dtype) for k, v in _toy_inputs(torch).items()}
        for k in ('scale', 'bias_d', 'bias_n'):
            a[k].requires_grad_(True)
        field = _ToyField(torch, dtype)
        step = align_step_composed(field, progress=0.75, hybrid=hybrid, **a)
        outs[dtype] = (step, a, field)
    (s64, a64, f64), (s32, a32, f32) = outs[torch.float64], outs[torch.float32]
    assert list(s64.losses) == list(LOSS_NAMES) and s64.u.shape == (21, 3) and s64.dd.shape == (21,) and s64.dg.shape == (21, 3)
    pairs = [(s32.losses[k], s64.losses[k]) for k in LOSS_NAMES] + [(s32.u, s64.u), (s32.dd, s64.dd), (s32.dg, s64.dg)]
    pairs += [(s32.record[k], s64.record[k]) for k in s64.record]
    pairs += [(a32[k].grad, a64[k].grad) for k in ('scale', 'bias_d', 'bias_n')] + [(f32.w.grad, f64.w.grad), (f32.c.grad, f64.c.grad)]
    for got, want in pairs:
        assert float((got.double() - want).norm()) <= 2e-5 * float(want.norm()) + 1e-12, (got, want)
    # the terms are the stated ones: the total is their weighted sum, TV only in the hybrid phase, and the maps get a gradient
    L = {k: float(v) for k, v in s64.losses.items()}
    assert abs(L['total'] - (20 * 0.75 * L['ref'] + L['distance'] + 0.1 * L['reg'] + 0.01 * L['normal'] + L['tv_distance'] + 0.01 * L['tv_normal'])) < 1e-12
    assert (L['tv_distance'] > 0 and L['tv_normal'] > 0) if hybrid else (L['tv_distance'] == 0 and L['tv_normal'] == 0)
    assert all(L[k] > 0 for k in ('distance', 'normal', 'reg', 'ref')) and float(a64['bias_d'].grad.abs().sum()) > 0


# ---- the reference's recorded outputs (tests/golden/make_joint_fixture.py) ---------------------------------------------------------------
def test_look_up_coordinates_reproduce_the_reference(golden_dir):
    import torch
    from perf_amd.joint_align import direction_to_img_coord
    fx = np.load(os.path.join(golden_dir, 'joint_align.npz'))
    dirs, want = torch.from_numpy(fx['dirs']), fx['img_coord']
    assert dirs.shape == (256, 3) and float(dirs[:, 2].abs().max()) < 1.0              # near, not at, the poles
    assert int(((want[:, 1] < 1e-3) | (want[:, 1] > 1 - 1e-3)).sum()) >= 16             # next to the seam, either side
    got = direction_to_img_coord(dirs).numpy()
    err = np.abs(got - want).max()
    print(f'direction_to_img_coord: max abs difference {err:.3e}')
    assert got.dtype == np.float32 and err <= 4 * 2.0 ** -24           # values in [0, 1]: a few roundings of half an fp32 ulp of 1


def test_views_reproduce_the_reference(golden_dir):
    from perf_amd.joint_align import verts_to_dirs
    fx = np.load(os.path.join(golden_dir, 'joint_align.npz'))
    for k in range(3):
        for ratio in (1.1, 1.7):
            got = verts_to_dirs(*[p.copy() for p in fx[f'tri/{k}']], gen_res=4, ratio=ratio)
            for name, v in zip(('dirs', 'ratios', 'to_vec', 'down_vec', 'right_vec'), got):
                want = fx[f'verts/{k}/{ratio}/{name}']
                assert v.numpy().shape == want.shape and v.numpy().dtype == np.float32
                assert np.abs(v.numpy() - want).max() <= 4 * 2.0 ** -24 * max(1.0, np.abs(want).max()), (k, ratio, name)
    with pytest.raises(ValueError):
        verts_to_dirs(np.float32([0, 0, 1]), np.float32([1, 0, 0.5]), np.float32([0, 1, 0]), 4, 1.1)


def test_view_set_properties():
    import torch
    from perf_amd import joint_align as J
    vertices, faces = J.icosahedron()
    assert vertices.shape == (12, 3) and vertices.dtype == np.float32 and faces.shape == (20, 3)
    assert np.abs(np.linalg.norm(vertices, axis=1) - 1).max() < 1e-6 and np.abs(vertices[:, 2]).max() > 1 - 1e-6          # one vertex is the pole
    edges = {tuple(sorted((f[i], f[(i + 1) % 3]))) for f in faces for i in range(3)}
    assert len(edges) == 30 and sorted(np.bincount(faces.reshape(-1))) == [5] * 12                                       # a closed icosahedron
    centres = vertices[faces].mean(1)
    np.random.seed(3)
    views = [J.panorama_to_pers_directions(gen_res=4, ratio=r, ex_rot='rand') for r in (1.1, 1.4, 1.7)]
    assert sum(v[0].shape[0] for v in views) == 60 and all(v[0].shape == (20, 4, 4, 3) and v[1].shape == (20, 4, 4, 1) for v in views)
    for ratio in (1.1, 1.4, 1.7):
        dirs, ratios, to_vecs, down_vecs, right_vecs = J.panorama_to_pers_directions(gen_res=4, ratio=ratio)
        assert np.abs(to_vecs.numpy() - centres).max() < 1e-6                       # the to_vecs of one ratio are the 20 face centres
        assert float((to_vecs * down_vecs).sum(-1).abs().max()) < 1e-6 and float((to_vecs * right_vecs).sum(-1).abs().max()) < 1e-6
        assert float((down_vecs * right_vecs).sum(-1).abs().max()) < 1e-6 and float((dirs.norm(dim=-1) - 1).abs().max()) < 1e-6
        assert float(ratios.min()) >= 1.0 - 1e-6
        assert torch.allclose(down_vecs.norm(dim=-1), right_vecs.norm(dim=-1), rtol=1e-5)
    # the random turn is about z and shared by the five outputs
    turned = J.panorama_to_pers_directions(gen_res=4, ratio=1.1, ex_rot=0.7)
    plain = J.panorama_to_pers_directions(gen_res=4, ratio=1.1)
    assert torch.allclose(turned[2][:, 2], plain[2][:, 2]) and torch.allclose(turned[1], plain[1])
    assert torch.allclose(turned[2][:, 0], np.cos(0.7) * plain[2][:, 0] - np.sin(0.7) * plain[2][:, 1], atol=1e-6)
    # every direction of a 64 x 128 panorama falls inside at least one view at ratio 1.1 (direction_to_pers_img_coord's inside test)
    _, _, to_vecs, down_vecs, right_vecs = plain
    pano = J.img_coord_to_pano_direction(J.img_coord_from_hw(64, 128)).reshape(-1, 3)
    covered = torch.zeros(len(pano), dtype=torch.bool)
    for t, dn, ri in zip(to_vecs, down_vecs, right_vecs):
        length = t.norm()
        along = (pano * t / length).sum(-1)
        q = pano / along.clamp_min(1e-5)[:, None] * length
        i, j = ((q - t) * dn).sum(-1) / dn.norm() ** 2, ((q - t) * ri).sum(-1) / ri.norm() ** 2
        covered |= (along > 1e-5) & (i.abs() <= 1.) & (j.abs() <= 1.)
    assert bool(covered.all())
