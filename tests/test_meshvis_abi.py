"""The cull of the faces no registered panorama saw (include/perf_hip_meshvis.h, perf_amd/mesh.py) checked without a GPU: the header's
constants and parameter types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal
happens before a launch with a message that names its reason (the fake pointers are never dereferenced); the workspace has the documented
size; the Python surface has the documented signatures and refuses CPU tensors; the extraction tool applies the cull before the component
cleaning."""
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


def _sizes(k, height=16, width=32):
    return (ctypes.c_int32 * (2 * max(k, 1)))(*([height, width] * max(k, 1)))


def _bits(**kw):
    a = {'vertices': FAKE, 'V': 8, 'views': FAKE, 'K': 2, 'tol': 1 / 256, 'free_tol': 1 / 256, 'visible': FAKE, 'free': FAKE}
    a.update(kw)
    a.setdefault('sizes', _sizes(a['K']) if 0 <= a['K'] <= 64 else _sizes(1))
    return _call('perf_meshvis_vertex_bits', a['vertices'], a['V'], a['views'], a['sizes'], a['K'], a['tol'], a['free_tol'], a['visible'], a['free'], None)


def _face_keep(**kw):
    a = {'faces': FAKE, 'F': 10, 'vertices': FAKE, 'V': 8, 'visible': FAKE, 'free': FAKE, 'centres': FAKE, 'K': 2, 'facing': 1, 'min_views': 1, 'carve': 1,
         'keep': FAKE, 'flag': FAKE}
    a.update(kw)
    return _call('perf_meshvis_face_keep', a['faces'], a['F'], a['vertices'], a['V'], a['visible'], a['free'], a['centres'], a['K'], a['facing'], a['min_views'],
                 a['carve'], a['keep'], a['flag'], None)


def _filter_count(**kw):
    a = {'faces': FAKE, 'F': 10, 'V': 8, 'keep': FAKE, 'ws': FAKE, 'ws_bytes': BIG, 'counts': FAKE}
    a.update(kw)
    return _call('perf_meshvis_filter_count', a['faces'], a['F'], a['V'], a['keep'], a['ws'], a['ws_bytes'], a['counts'], None)


def _filter_write(**kw):
    a = {'faces': FAKE, 'F': 10, 'V': 8, 'keep': FAKE, 'vertices': FAKE, 'ws': FAKE, 'ws_bytes': BIG, 'vertices_out': FAKE, 'index': FAKE, 'vcap': 8, 'faces_out': FAKE,
         'fcap': 10}
    a.update(kw)
    return _call('perf_meshvis_filter_write', a['faces'], a['F'], a['V'], a['keep'], a['vertices'], a['ws'], a['ws_bytes'], a['vertices_out'], a['index'], a['vcap'],
                 a['faces_out'], a['fcap'], None)


WITH_FACES = (_face_keep, _filter_count, _filter_write)
WITH_WORKSPACE = (_filter_count, _filter_write)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [meshvis] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, plain = abi_units.header('meshvis')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_MESHVIS_ABI_VERSION') == _lib.MESHVIS_ABI_VERSION == 1
    assert const('PERF_MESHVIS_MAX_VERTICES') == _lib.MESHVIS_MAX_VERTICES == _lib.MESHCC_MAX_VERTICES == 1 << 30
    assert const('PERF_MESHVIS_MAX_FACES') == _lib.MESHVIS_MAX_FACES == _lib.MESHCC_MAX_FACES == 1 << 38
    assert const('PERF_MESHVIS_MAX_VIEWS') == _lib.MESHVIS_MAX_VIEWS == 64
    assert _lib.load().perf_meshvis_sizeof_view() == _lib.MESHVIS_VIEW_BYTES == 64
    # vertex and face counts are 64-bit at the boundary
    for name in ('perf_meshvis_face_keep', 'perf_meshvis_filter_count', 'perf_meshvis_filter_write'):
        params = abi_units.params(plain, name)
        assert 'int64_t n_faces' in params and 'int64_t n_vertices' in params, name
    assert 'int64_t n_vertices' in abi_units.params(plain, 'perf_meshvis_vertex_bits')


def test_the_header_states_the_face_rule_and_what_it_does_not_do():
    comment = re.search(r'/\*.*?\*/', open(os.path.join(ROOT, 'include', 'perf_hip_meshvis.h')).read(), re.S).group(0)
    comment = re.sub(r'\s*\n \*\s*', ' ', comment)
    for phrase in ('RESTATED LINE FOR LINE', 'e1 = b - a, e2 = c - a', 's  = (n.x g.x + n.y g.y) + n.z g.z', 'iff s > 0', 'no atomics', 'THE ONE HOST READ-BACK',
                   'no occlusion test against the mesh itself', 'no colours are taken from the panoramas', 'more than 64 views are refused',
                   'ceil(V / 2) + S(V) + S(F) + 4'):
        assert phrase in comment, phrase


def test_the_unit_is_built_with_its_own_header_only():
    from perf_amd import build
    assert 'meshvis.hip' in build.SOURCES and len(set(build.SOURCES)) == len(build.SOURCES)
    assert os.path.join(ROOT, 'include', 'perf_hip_meshvis.h') in abi_units.build_deps()
    users = [s for s in build.SOURCES if any(p.endswith(os.sep + 'perf_hip_meshvis.h') for p in build._includes(os.path.join(build.CSRC, s)))]
    assert users == ['meshvis.hip', 'meshcolor.hip'], users          # the units that include the header, by their #include lines, are the ones rebuilt for it


def test_refuses_null_pointers():
    for call, kws in ((_bits, ({'vertices': None}, {'views': None}, {'sizes': None})), (_face_keep, ({'faces': None}, {'visible': None}, {'free': None}, {'vertices': None},
                                                                                                       {'centres': None})),
                      (_filter_count, ({'faces': None}, {'keep': None})), (_filter_write, ({'faces': None}, {'keep': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_bits, ({'visible': None}, {'free': None})), (_face_keep, ({'keep': None}, {'flag': None})), (_filter_count, ({'counts': None},)),
                      (_filter_write, ({'vertices_out': None}, {'index': None}, {'faces_out': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL output' in msg, (call.__name__, kw, msg)
    for kw in ({'vcap': -1}, {'fcap': -1}):
        rc, msg = _filter_write(**kw)
        assert rc == PERF_E_INVALID and 'negative capacity' in msg, (kw, msg)
    for call in WITH_WORKSPACE:
        rc, msg = call(ws=None)
        assert rc == PERF_E_INVALID and 'NULL workspace' in msg, msg
    rc, msg = _bits(views=ctypes.c_void_p(68))
    assert rc == PERF_E_INVALID and '8-byte aligned' in msg, msg


def test_refuses_counts_views_and_tolerances():
    from perf_amd import _lib
    lib = _lib.load()
    for call in (_bits,) + WITH_FACES:
        rc, msg = call(V=-1)
        assert rc == PERF_E_INVALID and 'negative number of vertices' in msg, (call.__name__, msg)
        rc, msg = call(V=(1 << 30) + 1)
        assert rc == PERF_E_INVALID and '2^30' in msg, (call.__name__, msg)
    for call in WITH_FACES:
        rc, msg = call(F=-1)
        assert rc == PERF_E_INVALID and 'negative number of faces' in msg, (call.__name__, msg)
        rc, msg = call(F=(1 << 38) + 1)
        assert rc == PERF_E_INVALID and '2^38' in msg, (call.__name__, msg)
    for call in (_bits, _face_keep):
        rc, msg = call(K=65)
        assert rc == PERF_E_INVALID and '65 views are more than 64' in msg, (call.__name__, msg)
        rc, msg = call(K=-1)
        assert rc == PERF_E_INVALID and 'negative number of views' in msg, (call.__name__, msg)
    for sizes in (_sizes(2, 0, 32), _sizes(2, 16, 0), _sizes(2, -3, 32)):
        rc, msg = _bits(sizes=sizes)
        assert rc == PERF_E_INVALID and 'a map dimension below 1' in msg, msg
    for name in ('tol', 'free_tol'):
        for bad in (-1e-6, float('inf'), float('nan'), -float('inf')):
            rc, msg = _bits(**{name: bad})
            assert rc == PERF_E_INVALID and name + ' ' in msg and 'negative or not finite' in msg, (name, bad, msg)
    for bad in (0, -1):
        rc, msg = _face_keep(min_views=bad)
        assert rc == PERF_E_INVALID and 'min_views' in msg and 'below 1' in msg, msg
    for kw in ({'facing': 2}, {'carve': -1}):
        rc, msg = _face_keep(**kw)
        assert rc == PERF_E_INVALID and 'are 0 or 1' in msg, msg
    assert lib.perf_meshvis_workspace_bytes(-1, 0) == -1 and lib.perf_meshvis_workspace_bytes(0, -1) == -1
    assert lib.perf_meshvis_workspace_bytes((1 << 30) + 1, 0) == -1 and lib.perf_meshvis_workspace_bytes(0, (1 << 38) + 1) == -1
    assert lib.perf_meshvis_workspace_bytes(1 << 30, 1 << 38) > 0


def test_refuses_a_bad_workspace_and_sizes_it_as_documented():
    from perf_amd import _lib
    lib = _lib.load()
    for V, F in ((0, 0), (5, 0), (0, 7), (1, 1), (256, 256), (257, 65537), (65536, 65536), (65537, 131070), (3_700_000, 7_400_000), (14_700_000, 29_400_000),
                 (1 << 30, 1 << 31), (1 << 30, (1 << 31) + 12345), (1 << 30, 1 << 38)):          # the sizes of tests/test_meshcc_abi.py
        words = -(-V // 2) + abi_units.group_words(V) + abi_units.group_words(F) + 4
        need = lib.perf_meshvis_workspace_bytes(V, F)
        assert need == 8 * (words + words % 2) and need % 16 == 0, (V, F)
    assert lib.perf_meshvis_workspace_bytes(14_700_000, 29_400_000) < 4.1 * 14_700_000          # 4 bytes per vertex, 1/32 byte per face, and the levels
    for call in WITH_WORKSPACE:
        need = lib.perf_meshvis_workspace_bytes(8, 10)
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
    assert mesh.Visibility._fields == ('visible', 'free', 'n_views')
    assert params(mesh.vertex_visibility) == [('vertices', E), ('views', E), ('tol', 1 / 256), ('free_tol', None)]
    assert params(mesh.visible_faces) == [('mesh', E), ('visibility', E), ('views', E), ('facing', True), ('min_views', 1), ('carve', False)]
    assert params(mesh.filter_faces) == [('mesh', E), ('face_keep', E)]
    assert params(mesh.cull_unseen) == [('mesh', E), ('views', E), ('tol', 1 / 256), ('free_tol', None), ('facing', True), ('min_views', 1), ('carve', False)]
    assert names(scene.NeRFScene.cull_unseen_mesh) == ['self', 'mesh', 'sup_pool', 'kw']
    assert names(ops.meshvis_views) == ['poses', 'maps'] and names(ops.meshvis_vertex_bits) == ['vertices', 'views', 'sizes', 'tol', 'free_tol']
    assert names(ops.meshvis_face_keep) == ['faces', 'vertices', 'visible_bits', 'free_bits', 'centres', 'facing', 'min_views', 'carve', 'flag']
    assert names(ops.meshvis_filter_count) == ['faces', 'n_vertices', 'face_keep', 'ws', 'counts']
    assert names(ops.meshvis_filter_write) == ['faces', 'n_vertices', 'face_keep', 'ws', 'n_vertices_kept', 'n_faces_kept', 'vertices']
    # no fallback: CPU tensors are refused
    vertices, faces = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cpu = mesh.Mesh(vertices, faces)
    views = [{'pose': torch.eye(4), 'distance_map': torch.ones(4, 8, 1), 'mask': torch.ones(4, 8, 1, dtype=torch.bool)}]
    bits = mesh.Visibility(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), 1)
    for call in (lambda: mesh.vertex_visibility(vertices, views), lambda: mesh.visible_faces(cpu, bits, views), lambda: mesh.filter_faces(cpu, torch.ones(1, dtype=torch.uint8)),
                 lambda: mesh.cull_unseen(cpu, views), lambda: ops.meshvis_views([torch.eye(4)], [torch.ones(4, 8)]),
                 lambda: ops.meshvis_vertex_bits(vertices, torch.zeros(0, 16, dtype=torch.int32), [], 0.0, 0.0),
                 lambda: ops.meshvis_filter_count(faces, 3, torch.ones(1, dtype=torch.uint8))):
        with pytest.raises(perf_amd._lib.PerfError):
            call()
    with pytest.raises(perf_amd._lib.PerfError, match='65 views are more than 64'):
        ops.meshvis_views([torch.eye(4)] * 65, [torch.ones(4, 8)] * 65)


def test_extract_mesh_tool_culls_before_it_cleans():
    text = open(os.path.join(ROOT, 'tools', 'extract_mesh.py')).read()
    options = ["'--seen-by-panoramas'", "'--visibility-tol'", "'--carve'"]
    for option in options + ["'--sup-pool'"]:
        assert option in text, option
    assert text.index(options[0]) < text.index(options[1]) < text.index(options[2])
    cull, clean = text.index('scene.cull_unseen_mesh('), text.index('scene.clean_mesh(')
    assert text.index('extract_mesh_sparse(') < cull < clean and text.index('scene.extract_mesh(') < cull
