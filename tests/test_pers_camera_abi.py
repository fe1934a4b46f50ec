"""The perspective camera's C entry points and Python surface, checked without a GPU: the argument checks of
perf_pers_raygen(_dev) refuse before anything is launched, and the Python signatures carry the reference's defaults
(core_exp_runner.py:223, 235; utils/camera_utils.py:237)."""
import ctypes
import inspect

import numpy as np
import pytest

from tests.abi_units import PERF_E_INVALID, refused as _refused


def test_pers_raygen_refuses_bad_fovy_and_null_pointers():
    pose = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    fake = ctypes.c_void_p(16)              # never dereferenced: every call below is refused before a launch
    for fovy in (0.0, -0.5, np.pi, 3.5, float('nan'), float('inf')):
        for name, p in (('perf_pers_raygen', pose), ('perf_pers_raygen_dev', fake)):
            rc, msg = _refused(name, p, 64, 64, fovy, 0, 64, fake, fake, None)
            assert rc == PERF_E_INVALID and 'fovy' in msg, (name, fovy, msg)
    rc, msg = _refused('perf_pers_raygen', None, 64, 64, 1.0, 0, 64, fake, fake, None)
    assert rc == PERF_E_INVALID and 'NULL' in msg
    rc, msg = _refused('perf_pers_raygen_dev', None, 64, 64, 1.0, 0, 64, fake, fake, None)
    assert rc == PERF_E_INVALID and 'NULL' in msg
    for out in ((None, fake), (fake, None)):
        rc, msg = _refused('perf_pers_raygen', pose, 64, 64, 1.0, 0, 64, *out, None)
        assert rc == PERF_E_INVALID and 'NULL' in msg


def test_pers_camera_signatures_carry_the_reference_defaults():
    from perf_amd import ops, scene, traverse
    p = inspect.signature(traverse.render_dense).parameters
    assert p['cam_type'].default == 'pano' and p['fov'].default == np.deg2rad(75.) and p['res'].default == 512
    assert p['height'].default == 512 and p['width'].default == 1024          # the panorama's, unchanged
    assert list(inspect.signature(scene.gen_pers_rays).parameters) == ['pose', 'fov', 'res', 'device']
    assert inspect.signature(scene.NeRFScene.make_graphed_render).parameters['fovy'].default is None
    assert list(inspect.signature(ops.pers_raygen).parameters) == ['pose', 'height', 'width', 'fovy', 'row0', 'nrows', 'device']
    assert list(inspect.signature(ops.pers_raygen_dev).parameters) == ['pose_dev', 'height', 'width', 'fovy', 'row0', 'nrows', 'out']


def test_pers_raygen_ops_refuse_bad_poses():
    from perf_amd import _lib, ops
    with pytest.raises(_lib.PerfError, match='pose'):
        ops._pose16(np.eye(3, dtype=np.float32))
    assert list(ops._pose16(np.eye(4)[:3]))[12:] == [0.0] * 4
