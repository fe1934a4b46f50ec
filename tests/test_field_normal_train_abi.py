"""The backward of the density gradient (include/perf_hip_ext.h: perf_field_grad_x_bwd) and its Python surface, checked without a GPU: the
header's constants and parameter types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's);
every refusal happens before a launch with a message that names its reason; the geometry step leaves the fused path only when a normal loss
is asked for."""
import ctypes
import inspect
from types import SimpleNamespace

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

FAKE = ctypes.c_void_p(16)   # never dereferenced: every call of this file is refused -- or is an empty call -- before a launch


def _descs(n_levels=16, n_hidden=1, **grid_kw):
    from perf_amd.grid import GridConfig, MlpConfig
    g = GridConfig(n_levels=n_levels, **grid_kw)
    m = MlpConfig(n_levels=n_levels, n_hidden_layers=n_hidden, n_output_dims=1 if n_hidden == 1 else 3,
                  output_activation='Exponential' if n_hidden == 1 else 'Sigmoid')
    return g.desc(), m.desc()


def _bwd(gd, md, n=64, dtype=0, **kw):
    a = {'x01': FAKE, 'table': FAKE, 'w': FAKE, 'dsigma': FAKE, 'dgrad': FAKE, 'grad': FAKE, 'ws': FAKE, 'ws_bytes': 1 << 30}
    a.update(kw)
    return _call('perf_field_grad_x_bwd', ctypes.byref(gd) if gd is not None else None, ctypes.byref(md) if md is not None else None, a['x01'], None,
                 a['table'], a['w'], None, a['dsigma'], a['dgrad'], a['grad'], a['ws'], a['ws_bytes'], n, None, dtype, None)


def test_extension_header_binding_record_and_library_agree():
    """(the agreement every unit owes is tests/test_abi_units.py's, [ext]; this is what is the extension's own)"""
    from perf_amd import _lib
    header, _ = abi_units.header('ext')
    assert abi_units.const(header, 'PERF_EXT_ABI_VERSION') == _lib.EXT_ABI_VERSION == 1
    # the extension's names are not in the core's frozen table
    assert not set(_lib._SIGS_EXT) & set(_lib.exported_symbols())


def test_bwd_refuses_null_pointers_counts_and_dtypes():
    gd, md = _descs()
    rc, msg = _bwd(None, md)
    assert rc == PERF_E_INVALID and 'NULL descriptor' in msg, msg
    rc, msg = _bwd(gd, None)
    assert rc == PERF_E_INVALID and 'NULL descriptor' in msg, msg
    rc, msg = _bwd(gd, md, n=-1)
    assert rc == PERF_E_INVALID and 'n < 0' in msg, msg
    rc, msg = _bwd(gd, md, dtype=7)
    assert rc == PERF_E_INVALID and 'dtype' in msg, msg
    rc, msg = _bwd(gd, md, grad=None)
    assert rc == PERF_E_INVALID and 'NULL output' in msg, msg
    for kw in ({'x01': None}, {'table': None}, {'w': None}):
        rc, msg = _bwd(gd, md, **kw)
        assert rc == PERF_E_INVALID and 'NULL input' in msg, (kw, msg)
    rc, msg = _bwd(gd, md, dsigma=None, dgrad=None)
    assert rc == PERF_E_INVALID and 'both upstream gradients are NULL' in msg, msg
    rc, msg = _bwd(gd, md, ws=None)
    assert rc == PERF_E_INVALID and 'workspace' in msg, msg
    rc, msg = _bwd(gd, md, ws_bytes=16)
    assert rc == PERF_E_INVALID and 'workspace' in msg and 'bytes' in msg, msg
    rc, msg = _bwd(gd, md, ws=ctypes.c_void_p(20))
    assert rc == PERF_E_INVALID and '16-byte aligned' in msg, msg


def test_bwd_empty_call_is_refused_only_for_a_null_gradient():
    """n == 0 is a valid call that zero-fills grad: the inputs may be NULL (an empty tensor's pointer is), grad may not."""
    gd, md = _descs()
    rc, msg = _bwd(gd, md, n=0, grad=None, x01=None, table=None, w=None, dsigma=None, dgrad=None, ws=None, ws_bytes=0)
    assert rc == PERF_E_INVALID and 'NULL output' in msg, msg
    # (with a gradient the call goes on to the zero-fill -- which this file, without a device, does not issue: the workspace query
    #  answers for the same arguments instead)
    from perf_amd import _lib
    lib = _lib.load()
    assert lib.perf_field_grad_x_bwd_workspace_bytes(ctypes.byref(gd), ctypes.byref(md), 0) > 0
    n_net = 64 * 32 + 16 * 64
    assert lib.perf_field_grad_x_bwd_workspace_bytes(ctypes.byref(gd), ctypes.byref(md), 1 << 20) % (4 * n_net) == 0
    assert lib.perf_field_grad_x_bwd_workspace_bytes(ctypes.byref(gd), ctypes.byref(md), -1) == -1


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
def test_bwd_refuses_the_line_layouts(layout):
    gd, md = _descs(layout=layout, sb_shift=(3, 3, 2))
    rc, msg = _bwd(gd, md)
    assert rc == PERF_E_INVALID and 'layout' in msg and 'tcnn' in msg, msg
    from perf_amd import _lib
    assert _lib.load().perf_field_grad_x_bwd_workspace_bytes(ctypes.byref(gd), ctypes.byref(md), 64) == -1


def test_bwd_refuses_what_is_not_built():
    gd, md = _descs(interpolation='Smoothstep')
    rc, msg = _bwd(gd, md)
    assert rc == PERF_E_INVALID and 'Smoothstep' in msg, msg
    gd, md = _descs(n_levels=20)
    rc, msg = _bwd(gd, md)
    assert rc == PERF_E_INVALID and '16 levels' in msg, msg
    gd, md = _descs(n_hidden=2)
    rc, msg = _bwd(gd, md)
    assert rc == PERF_E_INVALID and 'hidden layer' in msg, msg
    gd, _ = _descs(n_levels=16)
    _, md = _descs(n_levels=8)
    rc, msg = _bwd(gd, md)
    assert rc == PERF_E_INVALID and 'the MLP takes 8 levels, the grid has 16' in msg, msg


def test_python_surface():
    from perf_amd import fields, ops, scene
    assert list(inspect.signature(ops.field_grad_x_bwd).parameters) == ['grid', 'mlp', 'x01', 'sel', 'w16', 'inv_extent', 'dsigma', 'dgrad',
                                                                       'n_dev', 'grad', 'ws']
    assert list(inspect.signature(fields.NGPNeRF.density_and_grad_at).parameters) == ['self', 'x01', 'sel', 'n_dev']
    # the evaluation-only surface is what it was
    assert list(inspect.signature(fields.NGPNeRF.density_grad_at).parameters) == ['self', 'x01', 'sel', 'n_dev']
    assert list(inspect.signature(fields.NGPNeRF.query_normal).parameters) == ['self', 'x']
    assert callable(fields.unit_normals) and callable(scene.normals_to_world) and callable(scene.NeRFScene._normal_loss)
    assert not hasattr(scene.default_train_conf(), 'normal_loss_weight')        # (opt-in: read with getattr(..., 0.))
    assert 'WORLD-frame' in scene.SupInfoPool.register_rays.__doc__ and 'normals_to_world' in scene.SupInfoPool.register_sup_info.__doc__


def test_unit_normals_and_the_world_frame():
    import torch
    from perf_amd import fields, scene
    g = torch.tensor([[3.0, 0.0, -4.0], [0.0, 0.0, 0.0], [float('inf'), 1.0, 0.0], [float('nan'), 1.0, 0.0], [1e30, -2e30, 2e30]], requires_grad=True)
    n = fields.unit_normals(g)
    assert torch.allclose(n[0], torch.tensor([-0.6, 0.0, 0.8])) and torch.allclose(n[4], torch.tensor([-1.0, 2.0, -2.0]) / 3.0)
    assert float(n.detach()[1:4].abs().max()) == 0.0
    n.sum().backward()
    assert torch.isfinite(g.grad).all() and float(g.grad[1:4].abs().max()) == 0.0
    gen = torch.Generator().manual_seed(3)
    v = torch.nn.functional.normalize(torch.randn(6, 3, generator=gen), dim=-1)
    a = 0.7
    pose = torch.eye(4)
    pose[:3, :3] = torch.tensor([[1, 0, 0], [0, torch.cos(torch.tensor(a)), -torch.sin(torch.tensor(a))], [0, torch.sin(torch.tensor(a)), torch.cos(torch.tensor(a))]])
    assert torch.allclose(scene.normals_to_camera(scene.normals_to_world(v, pose), pose), v, atol=1e-6)
    assert torch.allclose(scene.normals_to_world(v, pose), torch.matmul(pose[:3, :3], v[..., None])[..., 0], atol=1e-6)


def test_a_normal_loss_takes_the_eager_geometry_step():
    from perf_amd import scene
    conf = scene.default_train_conf()
    host = SimpleNamespace(fused_steps=True, train_conf=conf)
    base = scene.NeRFScene._can_fuse(host)
    assert base is True
    conf.normal_loss_weight = 0.0
    assert scene.NeRFScene._can_fuse(host) is True
    conf.normal_loss_weight = 0.1
    assert scene.NeRFScene._can_fuse(host) is False
    del conf.normal_loss_weight
    assert scene.NeRFScene._can_fuse(host) is base
