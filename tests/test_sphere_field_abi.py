"""The sphere distance field (include/perf_hip_sphere.h, perf_amd/sphere_field.py) checked without a GPU: the header's constants and parameter
types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal happens before a launch
with a message that names its reason; the MLP half is pinned on the reference's VanillaMLP; install_shims(sphere_field=True) rebinds one
global."""
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


def _desc(n_levels=16, interpolation='Smoothstep', **kw):
    from perf_amd.grid import GridConfig
    return GridConfig(n_levels=n_levels, interpolation=interpolation, **kw).desc()


def _fwd(gd, n=64, **kw):
    a = {'table': FAKE, 'net': FAKE, 'dirs': FAKE, 'raw': FAKE, 'grad': FAKE}
    a.update(kw)
    return _call('perf_sphere_field_fwd', ctypes.byref(gd) if gd is not None else None, a['table'], a['net'], a['dirs'], a['raw'], a['grad'], n, None)


def _bwd(gd, n=64, **kw):
    a = {'table': FAKE, 'net': FAKE, 'dirs': FAKE, 'draw': FAKE, 'dgrad': FAKE, 'grad': FAKE, 'ws': FAKE, 'ws_bytes': 1 << 30}
    a.update(kw)
    return _call('perf_sphere_field_bwd', ctypes.byref(gd) if gd is not None else None, a['table'], a['net'], a['dirs'], a['draw'], a['dgrad'],
                 a['grad'], a['ws'], a['ws_bytes'], n, None)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [sphere] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, _ = abi_units.header('sphere')
    assert abi_units.const(header, 'PERF_SPHERE_ABI_VERSION') == _lib.SPHERE_ABI_VERSION == 1
    assert list(inspect.signature(abi_units.abi_digest().digest).parameters) == ['path', 'macro']


def test_refuses_null_pointers_and_counts():
    gd = _desc()
    for call in (_fwd, _bwd):
        rc, msg = call(None)
        assert rc == PERF_E_INVALID and 'NULL descriptor' in msg, msg
        rc, msg = call(gd, n=-1)
        assert rc == PERF_E_INVALID and 'n < 0' in msg, msg
        for kw in ({'table': None}, {'net': None}, {'dirs': None}):
            rc, msg = call(gd, **kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (kw, msg)
    rc, msg = _fwd(gd, raw=None)
    assert rc == PERF_E_INVALID and 'NULL output' in msg, msg
    rc, msg = _bwd(gd, grad=None)
    assert rc == PERF_E_INVALID and 'NULL output' in msg, msg
    rc, msg = _bwd(gd, n=0, grad=None)          # (an empty call zero-fills grad_out: it must exist)
    assert rc == PERF_E_INVALID and 'NULL output' in msg, msg
    rc, msg = _bwd(gd, draw=None, dgrad=None)
    assert rc == PERF_E_INVALID and 'both upstream gradients are NULL' in msg, msg


def test_bwd_refuses_a_bad_workspace():
    from perf_amd import _lib, ops
    gd = _desc()
    rc, msg = _bwd(gd, ws=None)
    assert rc == PERF_E_INVALID and 'NULL workspace' in msg, msg
    rc, msg = _bwd(gd, ws_bytes=16)
    assert rc == PERF_E_INVALID and 'workspace' in msg and 'bytes' in msg, msg
    rc, msg = _bwd(gd, ws=ctypes.c_void_p(20))
    assert rc == PERF_E_INVALID and '16-byte aligned' in msg, msg
    lib = _lib.load()
    need = lib.perf_sphere_field_bwd_workspace_bytes(ctypes.byref(gd), 1 << 15)
    assert need % 16 == 0 and need >= 256 * 4 * ops.sphere_net_params(16)
    assert need == lib.perf_sphere_field_bwd_workspace_bytes(ctypes.byref(gd), 1)       # (a fixed number of partials, whatever n)
    assert lib.perf_sphere_field_bwd_workspace_bytes(ctypes.byref(gd), -1) == -1
    assert ops.sphere_net_params(16) == 64 * 35 + 64 + 64 * 64 + 64 + 64 + 1


def test_refuses_what_is_not_built():
    from perf_amd import _lib
    lib = _lib.load()
    cases = [(_desc(interpolation='Linear'), ('Linear',)),
             (_desc(layout='line_local', sb_shift=(3, 3, 2)), ('layout', 'tcnn')),
             (_desc(layout='line_overlap', sb_shift=(3, 3, 2)), ('layout', 'tcnn')),
             (_desc(n_levels=20), ('16 levels',))]
    for gd, words in cases:
        for call in (_fwd, _bwd):
            rc, msg = call(gd)
            assert rc == PERF_E_INVALID and all(w in msg for w in words), msg
        assert lib.perf_sphere_field_bwd_workspace_bytes(ctypes.byref(gd), 64) == -1


# ---- the MLP half, pinned on the reference's VanillaMLP (tests/golden/make_sphere_fixture.py) -------------------------------------
@pytest.mark.parametrize('tag,weight_norm', [('plain', False), ('wn', True)])
def test_mlp_restatement_reproduces_the_reference(golden_dir, tag, weight_norm):
    import torch
    from perf_amd.sphere_field import SphereMLP
    fx = np.load(os.path.join(golden_dir, 'sphere_mlp.npz'))
    torch.manual_seed(0)
    mlp = SphereMLP(35, weight_norm=weight_norm)
    assert list(mlp.state_dict().keys()) == [str(k) for k in fx[f'{tag}/keys']]
    mlp.load_state_dict({str(k): torch.from_numpy(fx[f'{tag}/sd/{k}']) for k in fx[f'{tag}/keys']})
    x = torch.from_numpy(fx['x']).requires_grad_(True)
    y = mlp(x)
    gx, = torch.autograd.grad(y.sum(), x)
    for got, want in ((y.detach().numpy(), fx[f'{tag}/y']), (gx.numpy(), fx[f'{tag}/gx'])):
        assert got.shape == want.shape
        assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want)
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    # the effective weights the kernels get are the layer's own: the same outputs from plain matrix products
    w1, b1, w2, b2, w3, b3 = mlp.effective_parameters()
    sp = torch.nn.Softplus(beta=100)
    y2 = -(sp(sp(x.detach() @ w1.T + b1) @ w2.T + b2) @ w3.T + b3)
    assert np.abs(y2.detach().numpy() - fx[f'{tag}/y']).max() <= 1e-6 * np.abs(fx[f'{tag}/y']).max()
    assert all(p.requires_grad for p in (w1, w2, w3))


def test_mlp_initialisation_is_the_sphere_of_radius_one_half():
    import torch
    from perf_amd.sphere_field import SphereMLP
    torch.manual_seed(1)
    mlp = SphereMLP(35)
    first, hidden, last = mlp.layers[0], mlp.layers[2], mlp.layers[4]
    assert float(first.weight[:, 3:].abs().max()) == 0.0 and float(first.bias.abs().max()) == 0.0 and float(hidden.bias.abs().max()) == 0.0
    assert abs(float(first.weight[:, :3].std()) - (2 / 64) ** 0.5) < 0.03 and abs(float(hidden.weight.std()) - (2 / 64) ** 0.5) < 0.01
    assert abs(float(last.weight.mean()) - (np.pi / 64) ** 0.5) < 1e-3 and float(last.bias) == -0.5
    # at initialisation the network is close to |u| - 0.5 of its first three inputs, and forward returns MINUS the last layer
    u = torch.nn.functional.normalize(torch.randn(256, 3), dim=-1)
    y = mlp(torch.cat([u, torch.zeros(256, 32)], -1))[:, 0]
    assert float((y + 0.5).abs().mean()) < 0.35 and float(y.mean()) < 0.0


def test_python_surface():
    from perf_amd import ops, sphere_field
    assert list(inspect.signature(ops.sphere_field_fwd).parameters) == ['grid', 'table', 'net', 'dirs', 'want_grad']
    assert list(inspect.signature(ops.sphere_field_bwd).parameters) == ['grid', 'table', 'net', 'dirs', 'draw', 'dgrad', 'grad', 'ws']
    sig = inspect.signature(sphere_field.SphereDistanceField.__init__)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != 'self'] == [
        ('n_levels', 16), ('log2_hashmap_size', 19), ('base_res', 16), ('fine_res', 2048), ('weight_norm', False), ('output', 'softplus1'), ('fused', True)]
    assert list(inspect.signature(sphere_field.SphereDistanceField.forward).parameters) == ['self', 'directions', 'requires_grad']
    assert 'fp32' in sphere_field.SphereDistanceField.__doc__ and 'half' in sphere_field.SphereDistanceField.__doc__


# ---- install_shims(sphere_field=True) on a decoy tree ------------------------------------------------------------------------------
DECOY = textwrap.dedent('''
    MARKER = {marker!r}


    class SphereDistanceField:
        def __init__(self, n_levels=16, log2_hashmap_size=19, base_res=16, fine_res={fine}):
            self.decoy = True


    class Other:
        pass


    def make(**kw):
        return SphereDistanceField(**kw)
''')
SERVED = {'pano_joint_predictor': ('joint', 2048, False, 'softplus1'), 'pano_geo_refiner': ('refiner', 4096, True, 'identity')}


@pytest.fixture
def decoy_tree(tmp_path):
    pkg = tmp_path / 'modules' / 'geo_predictors'
    pkg.mkdir(parents=True)
    (tmp_path / 'modules' / '__init__.py').write_text('')
    (pkg / '__init__.py').write_text('')
    for name, (_, fine, _, _) in SERVED.items():
        (pkg / f'{name}.py').write_text(DECOY.format(marker=name, fine=fine))
    (pkg / 'bystander.py').write_text(DECOY.format(marker='bystander', fine=1))
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


def test_shim_rebinds_the_one_global(decoy_tree):
    import perf_amd
    from perf_amd.sphere_field import SphereDistanceField
    perf_amd.install_shims(sphere_field=True)
    perf_amd.install_shims(sphere_field=True)        # (idempotent)
    assert sum(isinstance(f, perf_amd._SphereFieldFinder) for f in sys.meta_path) == 1
    for name, (variant, fine, weight_norm, output) in SERVED.items():
        mod = importlib.import_module(f'modules.geo_predictors.{name}')
        assert mod.__file__ == str(decoy_tree / 'modules' / 'geo_predictors' / f'{name}.py')      # loaded from its real file
        assert mod.SphereDistanceField == getattr(SphereDistanceField, variant)
        field = mod.make(log2_hashmap_size=8)         # (the function instantiates by the global name; a small table: this is a CPU test)
        assert type(field) is SphereDistanceField and not hasattr(field, 'decoy')
        assert field.fused and field.geo_mlp.weight_norm is weight_norm and field.output == output
        want = np.exp(np.log(fine / 16) / 15)
        assert abs(field.hash_grid.encoding_config['per_level_scale'] - want) < 1e-12
        assert ('geo_mlp.layers.0.weight_g' in field.state_dict()) is weight_norm and 'hash_grid.params' in field.state_dict()
        # nothing else of the module changed
        assert mod.MARKER == name and mod.Other.__module__ == mod.__name__ and mod.make.__globals__ is mod.__dict__
        assert sorted(k for k in vars(mod) if not k.startswith('__')) == ['MARKER', 'Other', 'SphereDistanceField', 'make']
    other = importlib.import_module('modules.geo_predictors.bystander')
    assert other.make().decoy is True                 # a module that is not one of the two keeps its own class
    perf_amd.uninstall_sphere_field_shims()
    assert not any(isinstance(f, perf_amd._SphereFieldFinder) for f in sys.meta_path)


@pytest.mark.parametrize('kwargs', [{}, {'scene': True}])
def test_without_the_flag_nothing_is_rebound(decoy_tree, kwargs):
    import perf_amd
    assert list(inspect.signature(perf_amd.install_shims).parameters) == ['scene', 'sphere_field']
    assert inspect.signature(perf_amd.install_shims).parameters['sphere_field'].default is False
    perf_amd.install_shims(**kwargs)
    assert not any(isinstance(f, perf_amd._SphereFieldFinder) for f in sys.meta_path)
    for name in SERVED:
        mod = importlib.import_module(f'modules.geo_predictors.{name}')
        assert mod.make().decoy is True and mod.SphereDistanceField.__module__ == mod.__name__
