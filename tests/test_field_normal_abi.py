"""The density-gradient entry points (ABI 16: perf_field_grad_x, perf_normal_composite) and their Python surface, checked without a GPU: the
symbols are exported and declared in the header, and every refusal happens before a launch with a message that names its reason."""
import ctypes
import inspect
import re

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call


def _descs(n_levels=16, n_hidden=1, **grid_kw):
    from perf_amd.grid import GridConfig, MlpConfig
    g = GridConfig(n_levels=n_levels, **grid_kw)
    m = MlpConfig(n_levels=n_levels, n_hidden_layers=n_hidden, n_output_dims=1 if n_hidden == 1 else 3,
                  output_activation='Exponential' if n_hidden == 1 else 'Sigmoid')
    return g.desc(), m.desc()


def _grad_x(gd, md, grad, sigma=None, n=64, x01=ctypes.c_void_p(16), table=ctypes.c_void_p(16), w=ctypes.c_void_p(16)):
    # (the fake pointers are never dereferenced: every call of this file is refused -- or returns for n == 0 -- before a launch)
    return _call('perf_field_grad_x', ctypes.byref(gd), ctypes.byref(md), x01, None, table, w, None, grad, sigma, n, None, 0, None)


def test_abi_16_header_binding_and_record_agree():
    from perf_amd import _lib
    header, _ = abi_units.header('core')
    lib = _lib.load()
    assert abi_units.const(header, 'PERF_ABI_VERSION') == _lib.ABI_VERSION == 16          # (the record and the library: tests/test_abi_units.py)
    for name in ('perf_field_grad_x', 'perf_normal_composite'):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name


def test_grad_x_refuses_null_outputs_and_inputs():
    gd, md = _descs()
    fake = ctypes.c_void_p(16)
    rc, msg = _grad_x(gd, md, None, fake)
    assert rc == PERF_E_INVALID and 'NULL output' in msg, msg
    for kw in ({'x01': None}, {'table': None}, {'w': None}):
        rc, msg = _grad_x(gd, md, fake, **kw)
        assert rc == PERF_E_INVALID and 'NULL input' in msg, (kw, msg)
    rc, msg = _call('perf_field_grad_x', None, ctypes.byref(md), fake, None, fake, fake, None, fake, None, 64, None, 0, None)
    assert rc == PERF_E_INVALID and 'NULL descriptor' in msg
    rc, msg = _grad_x(gd, md, fake, n=-1)
    assert rc == PERF_E_INVALID and 'n < 0' in msg
    rc, msg = _call('perf_field_grad_x', ctypes.byref(gd), ctypes.byref(md), fake, None, fake, fake, None, fake, None, 64, None, 7, None)
    assert rc == PERF_E_INVALID and 'dtype' in msg
    # n == 0 is a valid, empty call (an empty tensor's pointer is NULL)
    rc, msg = _grad_x(gd, md, None, None, n=0, x01=None)
    assert rc == 0, msg


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
def test_grad_x_refuses_the_line_layouts(layout):
    gd, md = _descs(layout=layout, sb_shift=(3, 3, 2))
    rc, msg = _grad_x(gd, md, ctypes.c_void_p(16))
    assert rc == PERF_E_INVALID and 'layout' in msg and 'tcnn' in msg, msg


def test_grad_x_refuses_what_is_not_built():
    fake = ctypes.c_void_p(16)
    gd, md = _descs(interpolation='Smoothstep')
    rc, msg = _grad_x(gd, md, fake)
    assert rc == PERF_E_INVALID and 'Smoothstep' in msg, msg
    gd, md = _descs(n_levels=20)
    rc, msg = _grad_x(gd, md, fake)
    assert rc == PERF_E_INVALID and '16 levels' in msg, msg
    gd, md = _descs(n_hidden=2)
    rc, msg = _grad_x(gd, md, fake)
    assert rc == PERF_E_INVALID and 'hidden layer' in msg, msg
    gd, _ = _descs(n_levels=16)
    _, md = _descs(n_levels=8)
    rc, msg = _grad_x(gd, md, fake)
    assert rc == PERF_E_INVALID and 'the MLP takes 8 levels, the grid has 16' in msg, msg


def test_normal_composite_refuses_null_pointers():
    fake = ctypes.c_void_p(16)
    rc, msg = _call('perf_normal_composite', fake, fake, fake, 8, None, None)
    assert rc == PERF_E_INVALID and 'NULL output' in msg, msg
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        rc, msg = _call('perf_normal_composite', *args, 8, fake, None)
        assert rc == PERF_E_INVALID and 'NULL input' in msg, msg
    rc, msg = _call('perf_normal_composite', None, None, None, 0, None, None)
    assert rc == 0, msg


def test_python_surface():
    from perf_amd import fields, ops, renderer, scene, sharded
    assert list(inspect.signature(ops.field_grad_x).parameters)[:5] == ['grid', 'mlp', 'x01', 'sel', 'w16']
    assert list(inspect.signature(fields.NGPNeRF.density_grad_at).parameters) == ['self', 'x01', 'sel', 'n_dev']
    assert list(inspect.signature(fields.NGPNeRF.query_normal).parameters) == ['self', 'x']
    assert inspect.signature(renderer.NeRFOCCRenderer.stage_composite).parameters['with_normal'].default is False
    assert inspect.signature(renderer.NeRFOCCRenderer.render).parameters['with_normal'].default is False
    assert callable(scene.normals_to_camera)
    with pytest.raises(NotImplementedError, match='level-sharded'):
        sharded.LevelShardedNeRF.density_grad_at(None, None, None)


def test_normals_to_camera_is_the_transpose_of_apply_rot():
    import numpy as np
    import torch
    from perf_amd import scene
    g = torch.Generator().manual_seed(3)
    n = torch.nn.functional.normalize(torch.randn(5, 7, 3, generator=g), dim=-1)
    assert torch.equal(scene.normals_to_camera(n, torch.eye(4)), n)
    a, b = 0.7, -0.4
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    pose = torch.eye(4)
    pose[:3, :3] = torch.from_numpy(rz @ rx).float()
    pose[:3, 3] = torch.tensor([0.3, -0.2, 0.1])            # (the translation does not touch a direction)
    world = torch.matmul(pose[:3, :3], n[..., None])[..., 0]            # apply_rot (utils/camera_utils.py:44-46)
    assert torch.allclose(scene.normals_to_camera(world, pose), n, atol=1e-6)
