"""The connected components of a triangle mesh (include/perf_hip_meshcc.h, perf_amd/mesh.py) checked without a GPU: the header's constants and
parameter types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal happens
before a launch with a message that names its reason (the fake pointers are never dereferenced); the workspace has the documented size; the
Python surface has the documented signatures and refuses CPU tensors."""
import ctypes
import inspect
import os
import re

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
BIG = 1 << 40


def _label(**kw):
    a = {'faces': FAKE, 'F': 10, 'V': 8, 'vc': FAKE, 'counts': FAKE, 'ws': FAKE, 'ws_bytes': BIG}
    a.update(kw)
    return _call('perf_meshcc_label', a['faces'], a['F'], a['V'], a['vc'], a['counts'], a['ws'], a['ws_bytes'], None)


def _stats(**kw):
    a = {'faces': FAKE, 'F': 10, 'vertices': FAKE, 'V': 8, 'vc': FAKE, 'C': 2, 'per_faces': FAKE, 'per_vertices': FAKE, 'volume': FAKE}
    a.update(kw)
    return _call('perf_meshcc_stats', a['faces'], a['F'], a['vertices'], a['V'], a['vc'], a['C'], a['per_faces'], a['per_vertices'], a['volume'], None)


def _filter_count(**kw):
    a = {'faces': FAKE, 'F': 10, 'vc': FAKE, 'V': 8, 'keep': FAKE, 'C': 2, 'ws': FAKE, 'ws_bytes': BIG, 'counts': FAKE}
    a.update(kw)
    return _call('perf_meshcc_filter_count', a['faces'], a['F'], a['vc'], a['V'], a['keep'], a['C'], a['ws'], a['ws_bytes'], a['counts'], None)


def _filter_write(**kw):
    a = {'faces': FAKE, 'F': 10, 'vc': FAKE, 'V': 8, 'keep': FAKE, 'C': 2, 'vertices': FAKE, 'ws': FAKE, 'ws_bytes': BIG, 'vertices_out': FAKE, 'index': FAKE, 'vcap': 8,
         'faces_out': FAKE, 'fcap': 10}
    a.update(kw)
    return _call('perf_meshcc_filter_write', a['faces'], a['F'], a['vc'], a['V'], a['keep'], a['C'], a['vertices'], a['ws'], a['ws_bytes'], a['vertices_out'], a['index'],
                 a['vcap'], a['faces_out'], a['fcap'], None)


ALL = (_label, _stats, _filter_count, _filter_write)
WITH_COMPONENTS = (_stats, _filter_count, _filter_write)
WITH_WORKSPACE = (_label, _filter_count, _filter_write)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [meshcc] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, plain = abi_units.header('meshcc')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_MESHCC_ABI_VERSION') == _lib.MESHCC_ABI_VERSION == 1
    assert list(inspect.signature(abi_units.abi_digest().digest).parameters) == ['path', 'macro']
    assert const('PERF_MESHCC_MAX_VERTICES') == _lib.MESHCC_MAX_VERTICES == _lib.MESH_MAX_CELLS == 1 << 30          # the mesh ABI's ceiling
    assert const('PERF_MESHCC_MAX_FACES') == _lib.MESHCC_MAX_FACES == 1 << 38 and _lib.MESHCC_MAX_FACES > 1 << 31
    # face counts and offsets are 64-bit at the boundary
    for name in ('perf_meshcc_label', 'perf_meshcc_stats', 'perf_meshcc_filter_count', 'perf_meshcc_filter_write'):
        params = abi_units.params(plain, name)
        assert 'int64_t n_faces' in params and 'int64_t n_vertices' in params, name


def test_the_header_states_the_termination_argument():
    comment = re.search(r'/\*.*?\*/', open(os.path.join(ROOT, 'include', 'perf_hip_meshcc.h')).read(), re.S).group(0)
    comment = re.sub(r'\s*\n \*\s*', ' ', comment)
    for phrase in ('only ever decreases', 'Termination.', 'FROM THAT RETURNED VALUE', 'agent-scope relaxed atomic load', 'No thread waits',
                   'MAY DEPEND ON THE ORDER OF SUMMATION'):
        assert phrase in comment, phrase


def test_refuses_null_pointers():
    for call, kws in ((_label, ({'faces': None},)), (_stats, ({'faces': None}, {'vc': None})), (_filter_count, ({'faces': None}, {'vc': None}, {'keep': None})),
                      (_filter_write, ({'faces': None}, {'vc': None}, {'keep': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_label, ({'vc': None}, {'counts': None})), (_stats, ({'per_faces': None}, {'per_vertices': None}, {'volume': None})),
                      (_filter_count, ({'counts': None},)), (_filter_write, ({'vertices_out': None}, {'index': None}, {'faces_out': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL output' in msg, (call.__name__, kw, msg)
    for kw in ({'vcap': -1}, {'fcap': -1}):
        rc, msg = _filter_write(**kw)
        assert rc == PERF_E_INVALID and 'negative capacity' in msg, (kw, msg)
    for call in WITH_WORKSPACE:
        rc, msg = call(ws=None)
        assert rc == PERF_E_INVALID and 'NULL workspace' in msg, msg


def test_refuses_counts():
    from perf_amd import _lib
    lib = _lib.load()
    for call in ALL:
        rc, msg = call(V=-1)
        assert rc == PERF_E_INVALID and 'negative number of vertices' in msg, (call.__name__, msg)
        rc, msg = call(F=-1)
        assert rc == PERF_E_INVALID and 'negative number of faces' in msg, (call.__name__, msg)
        rc, msg = call(V=(1 << 30) + 1)
        assert rc == PERF_E_INVALID and '2^30' in msg, (call.__name__, msg)
        rc, msg = call(F=(1 << 38) + 1)
        assert rc == PERF_E_INVALID and '2^38' in msg, (call.__name__, msg)
    for call in WITH_COMPONENTS:
        rc, msg = call(C=-1)
        assert rc == PERF_E_INVALID and 'negative number of components' in msg, (call.__name__, msg)
        rc, msg = call(C=9)
        assert rc == PERF_E_INVALID and 'the mesh has 8 vertices' in msg, (call.__name__, msg)
    assert lib.perf_meshcc_workspace_bytes(-1, 0) == -1 and lib.perf_meshcc_workspace_bytes(0, -1) == -1
    assert lib.perf_meshcc_workspace_bytes((1 << 30) + 1, 0) == -1 and lib.perf_meshcc_workspace_bytes(0, (1 << 38) + 1) == -1
    assert lib.perf_meshcc_workspace_bytes(1 << 30, 1 << 38) > 0


def test_refuses_a_bad_workspace_and_sizes_it_as_documented():
    from perf_amd import _lib
    lib = _lib.load()
    for V, F in ((0, 0), (5, 0), (0, 7), (1, 1), (256, 256), (257, 65537), (65536, 65536), (65537, 131070), (3_700_000, 7_400_000), (14_700_000, 29_400_000),
                 (1 << 30, 1 << 31), (1 << 30, (1 << 31) + 12345), (1 << 30, 1 << 38)):
        words = V + abi_units.group_words(V) + abi_units.group_words(F) + 4
        need = lib.perf_meshcc_workspace_bytes(V, F)
        assert need == 8 * (words + words % 2) and need % 16 == 0, (V, F)
    assert lib.perf_meshcc_workspace_bytes(14_700_000, 29_400_000) < 8.1 * 14_700_000          # 8 bytes per vertex, 1/32 byte per face, and the levels
    for call in WITH_WORKSPACE:
        need = lib.perf_meshcc_workspace_bytes(8, 10)
        rc, msg = call(ws_bytes=need - 8)
        assert rc == PERF_E_INVALID and 'workspace' in msg and 'bytes' in msg, msg
        rc, msg = call(ws=ctypes.c_void_p(72))
        assert rc == PERF_E_INVALID and '16-byte aligned' in msg, msg


def test_python_surface():
    import torch
    import perf_amd
    from perf_amd import mesh, ops, scene
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    names = lambda f: [k for k, _ in params(f)]
    E = inspect.Parameter.empty
    assert mesh.Mesh._fields == ('vertices', 'faces', 'colors', 'normals')
    assert mesh.Components._fields == ('vertex_component', 'faces', 'vertices', 'signed_volume')
    assert params(mesh.connected_components) == [('mesh_or_faces', E), ('n_vertices', None), ('vertices', None)]
    assert params(mesh.select_components) == [('components', E), ('min_faces', 0), ('keep_largest', None), ('orientation', None)]
    assert params(mesh.filter_mesh) == [('mesh', E), ('components', E), ('keep', E)]
    assert params(mesh.clean_mesh) == [('mesh', E), ('min_faces', 0), ('keep_largest', None), ('orientation', None)]
    assert names(scene.NeRFScene.clean_mesh) == ['self', 'mesh', 'kw']
    # the extraction paths keep their exact signatures
    assert params(mesh.extract_mesh) == [('scene', E), ('resolution', 256), ('threshold', None), ('use_occupancy', True), ('colors', False), ('normals', False)]
    assert params(mesh.extract_mesh_sparse) == [('scene', E), ('resolution', 1024), ('threshold', None), ('colors', False), ('normals', False)]
    assert names(scene.NeRFScene.extract_mesh) == ['self', 'kw'] and names(scene.NeRFScene.extract_mesh_sparse) == ['self', 'kw']
    assert names(ops.meshcc_label) == ['faces', 'n_vertices', 'ws'] and names(ops.meshcc_stats) == ['faces', 'vertex_component', 'n_components', 'vertices']
    assert names(ops.meshcc_filter_count) == ['faces', 'vertex_component', 'keep', 'ws']
    assert names(ops.meshcc_filter_write) == ['faces', 'vertex_component', 'keep', 'ws', 'n_vertices_kept', 'n_faces_kept', 'vertices']
    vertices, faces = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cpu = mesh.Mesh(vertices, faces)
    comps = mesh.Components(torch.zeros(3, dtype=torch.int32), torch.ones(1, dtype=torch.int64), torch.full((1,), 3, dtype=torch.int32), torch.zeros(1, dtype=torch.float64))
    with pytest.raises(perf_amd._lib.PerfError):           # no fallback: CPU tensors are refused
        mesh.connected_components(cpu)
    with pytest.raises(perf_amd._lib.PerfError):
        mesh.connected_components(faces, n_vertices=3)
    with pytest.raises(perf_amd._lib.PerfError):
        mesh.select_components(comps)
    with pytest.raises(perf_amd._lib.PerfError):
        mesh.filter_mesh(cpu, comps, torch.ones(1, dtype=torch.bool))
    with pytest.raises(perf_amd._lib.PerfError):
        mesh.clean_mesh(cpu, min_faces=1)
    with pytest.raises(perf_amd._lib.PerfError):
        ops.meshcc_label(faces, 3)
    with pytest.raises(perf_amd._lib.PerfError):           # the number of vertices has to come from somewhere
        mesh.connected_components(faces)


def test_extract_mesh_tool_has_the_cleaning_options():
    text = open(os.path.join(ROOT, 'tools', 'extract_mesh.py')).read()
    for option in ("'--min-component-faces'", "'--keep-largest'", "'--orientation', choices=['inward', 'outward']"):
        assert option in text, option
    assert text.index('extract_mesh_sparse(') < text.index('scene.clean_mesh(') and text.index('scene.extract_mesh(') < text.index('scene.clean_mesh(')
