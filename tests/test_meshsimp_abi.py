"""The simplification by vertex clustering (include/perf_hip_meshsimp.h, perf_amd/mesh.py) checked without a GPU: the header's constants and
parameter types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal happens
before a launch with a message that names its reason (the fake pointers are never dereferenced); the workspace has the documented size; the
Python surface has the documented signatures and refuses CPU tensors; the extraction tool simplifies after the component cleaning."""
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


def _lo(*values):
    return (ctypes.c_float * 3)(*(values or (0.0, 0.0, 0.0)))


def _bounds(**kw):
    a = {'vertices': FAKE, 'V': 8, 'bounds': FAKE}
    a.update(kw)
    return _call('perf_meshsimp_bounds', a['vertices'], a['V'], a['bounds'], None)


def _cluster(**kw):
    a = {'vertices': FAKE, 'V': 8, 'F': 10, 'lo': _lo(), 'h': 0.25, 'n': (4, 4, 4), 'cluster': FAKE, 'counts': FAKE, 'ws': FAKE, 'ws_bytes': BIG}
    a.update(kw)
    return _call('perf_meshsimp_cluster', a['vertices'], a['V'], a['F'], a['lo'], a['h'], *a['n'], a['cluster'], a['counts'], a['ws'], a['ws_bytes'], None)


def _place(**kw):
    a = {'vertices': FAKE, 'V': 8, 'lo': _lo(), 'h': 0.25, 'n': (4, 4, 4), 'cluster': FAKE, 'C': 5, 'placement': 0, 'out': FAKE, 'rep': FAKE, 'ws': FAKE,
         'ws_bytes': BIG}
    a.update(kw)
    return _call('perf_meshsimp_place', a['vertices'], a['V'], a['lo'], a['h'], *a['n'], a['cluster'], a['C'], a['placement'], a['out'], a['rep'], a['ws'],
                 a['ws_bytes'], None)


def _faces(**kw):
    a = {'faces': FAKE, 'F': 10, 'cluster': FAKE, 'V': 8, 'dedupe': 1, 'out': FAKE, 'keep': FAKE, 'flag': FAKE, 'ws': FAKE, 'ws_bytes': BIG}
    a.update(kw)
    return _call('perf_meshsimp_faces', a['faces'], a['F'], a['cluster'], a['V'], a['dedupe'], a['out'], a['keep'], a['flag'], a['ws'], a['ws_bytes'], None)


WITH_GRID = (_cluster, _place)
WITH_WORKSPACE = (_cluster, _faces)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [meshsimp] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, plain = abi_units.header('meshsimp')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_MESHSIMP_ABI_VERSION') == _lib.MESHSIMP_ABI_VERSION == 1
    assert const('PERF_MESHSIMP_MAX_VERTICES') == _lib.MESHSIMP_MAX_VERTICES == 1 << 30
    assert const('PERF_MESHSIMP_MAX_FACES') == _lib.MESHSIMP_MAX_FACES == (1 << 31) - 1
    assert const('PERF_MESHSIMP_MAX_CELLS') == _lib.MESHSIMP_MAX_CELLS == 1 << 21
    assert {k: const('PERF_MESHSIMP_PLACE_' + k.upper()) for k in ('mean', 'member')} == _lib.MESHSIMP_PLACEMENT
    assert {None if k == 'NONE' else k.lower(): const('PERF_MESHSIMP_DEDUPE_' + k) for k in ('NONE', 'ORIENTED', 'UNORIENTED')} == _lib.MESHSIMP_DEDUPE
    # vertex and face counts are 64-bit at the boundary
    for name in ('perf_meshsimp_cluster', 'perf_meshsimp_faces'):
        params = abi_units.params(plain, name)
        assert 'int64_t n_faces' in params and 'int64_t n_vertices' in params, name
    assert 'int64_t n_vertices' in abi_units.params(plain, 'perf_meshsimp_place')


def test_the_header_states_the_rule_and_what_it_does_not_do():
    comment = re.search(r'/\*.*?\*/', open(os.path.join(ROOT, 'include', 'perf_hip_meshsimp.h')).read(), re.S).group(0)
    comment = re.sub(r'\s*\n \*\s*', ' ', comment)
    for phrase in ('t = ((double)x - (double)lo) / (double)h', 'i = min((int64)floor(t), n - 1)', 'q = llrint(f * 2^32)', 'key = ix << 42 | iy << 21 | iz',
                   'S / (count * 2^32)', 'p = (double)lo + ((double)i + m) * (double)h', 'd2 = (dx dx + dy dy) + dz dz', 'ties go to the smaller index',
                   'no floating-point atomics', 'THE ONE HOST READ-BACK', 'one more read-back', 'FROM THE VALUE THE COMPARE-AND-SWAP RETURNED',
                   'hash(key) = (key * M) >> (64 - b)', 'M = 0x9E3779B97F4A7C15', 'No thread waits for another thread', 'no manifold repair',
                   'more than 2^21 cells per axis are refused', '16 V + 4 T(V) + 4 F\' + 4 T(F) + 8 S(V) + 32', '48 bytes per cluster'):
        assert phrase in comment, phrase


def test_the_unit_is_built_with_its_own_header_only():
    from perf_amd import build
    assert 'meshsimp.hip' in build.SOURCES and len(set(build.SOURCES)) == len(build.SOURCES)
    assert os.path.join(ROOT, 'include', 'perf_hip_meshsimp.h') in abi_units.build_deps()
    users = [s for s in build.SOURCES if any(p.endswith(os.sep + 'perf_hip_meshsimp.h') for p in build._includes(os.path.join(build.CSRC, s)))]
    assert users == ['meshsimp.hip'], users          # the units that include the header, by their #include lines, are the ones rebuilt for it


def test_refuses_null_pointers():
    for call, kws in ((_bounds, ({'vertices': None},)), (_cluster, ({'vertices': None}, {'lo': None})), (_place, ({'vertices': None}, {'cluster': None}, {'lo': None})),
                      (_faces, ({'faces': None}, {'cluster': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_bounds, ({'bounds': None},)), (_cluster, ({'cluster': None}, {'counts': None})), (_place, ({'out': None}, {'rep': None})),
                      (_faces, ({'out': None}, {'keep': None}, {'flag': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL output' in msg, (call.__name__, kw, msg)
    for call in WITH_WORKSPACE + (_place,):
        rc, msg = call(ws=None)
        assert rc == PERF_E_INVALID and 'NULL workspace' in msg, msg


def test_refuses_counts_and_grids():
    from perf_amd import _lib
    lib = _lib.load()
    for call in (_bounds, _cluster, _place, _faces):
        rc, msg = call(V=-1)
        assert rc == PERF_E_INVALID and 'negative number of vertices' in msg, (call.__name__, msg)
        rc, msg = call(V=(1 << 30) + 1)
        assert rc == PERF_E_INVALID and '2^30' in msg, (call.__name__, msg)
    for call in (_cluster, _faces):
        rc, msg = call(F=-1)
        assert rc == PERF_E_INVALID and 'negative number of faces' in msg, (call.__name__, msg)
        rc, msg = call(F=1 << 31)
        assert rc == PERF_E_INVALID and '2^31 - 1' in msg, (call.__name__, msg)
    for call in WITH_GRID:
        for bad in (0.0, -0.25, float('inf'), float('nan'), -float('inf')):
            rc, msg = call(h=bad)
            assert rc == PERF_E_INVALID and 'cell edge h' in msg and 'not positive or not finite' in msg, (call.__name__, bad, msg)
        for bad in ((0, 4, 4), (4, -1, 4), (4, 4, (1 << 21) + 1)):
            rc, msg = call(n=bad)
            assert rc == PERF_E_INVALID and 'outside 1 .. 2^21' in msg, (call.__name__, bad, msg)
        rc, msg = call(lo=_lo(0.0, float('nan'), 0.0))
        assert rc == PERF_E_INVALID and 'origin lo is not finite' in msg, msg
        assert call(n=(1, 1, 1 << 21), V=-1)[1].count('negative number of vertices') == 1          # (the largest grid is none of the reasons)
    for bad, reason in ((-1, 'negative number of clusters'), (9, '9 clusters, the mesh has 8 vertices')):
        rc, msg = _place(C=bad)
        assert rc == PERF_E_INVALID and reason in msg, msg
    for bad in (-1, 2):
        rc, msg = _place(placement=bad)
        assert rc == PERF_E_INVALID and 'neither mean (0) nor member (1)' in msg, msg
    for bad in (-1, 3):
        rc, msg = _faces(dedupe=bad)
        assert rc == PERF_E_INVALID and 'none of none (0), oriented (1), unoriented (2)' in msg, msg
    assert lib.perf_meshsimp_workspace_bytes(-1, 0) == -1 and lib.perf_meshsimp_workspace_bytes(0, -1) == -1
    assert lib.perf_meshsimp_workspace_bytes((1 << 30) + 1, 0) == -1 and lib.perf_meshsimp_workspace_bytes(0, 1 << 31) == -1
    assert lib.perf_meshsimp_workspace_bytes(1 << 30, (1 << 31) - 1) > 0
    assert lib.perf_meshsimp_table_slots(-1) == -1 and lib.perf_meshsimp_table_slots(1 << 31) == -1


def test_refuses_a_bad_workspace_and_sizes_it_as_documented():
    from perf_amd import _lib
    lib = _lib.load()
    for n in (0, 1, 127, 128, 129, 4096, 4097, 65536, 65537, 14_700_000, 1 << 30, (1 << 31) - 1):
        assert lib.perf_meshsimp_table_slots(n) == abi_units.slots(n) >= 2 * n
    for V, F in ((0, 0), (5, 0), (0, 7), (1, 1), (256, 256), (257, 65537), (65536, 65536), (65537, 131070), (3_700_000, 7_400_000), (14_700_000, 29_400_000),
                 (1 << 30, 1 << 30), (1 << 30, (1 << 31) - 1)):
        need = 16 * V + 4 * abi_units.slots(V) + 4 * (F + F % 2) + 4 * abi_units.slots(F) + 8 * abi_units.group_words(V) + 32
        assert lib.perf_meshsimp_workspace_bytes(V, F) == -(-need // 16) * 16, (V, F)
    assert 24 * 14_700_000 < lib.perf_meshsimp_workspace_bytes(14_700_000, 0) < 32.1 * 14_700_000          # 24 to 32 bytes per vertex, and the levels
    assert 12 * 29_400_000 < lib.perf_meshsimp_workspace_bytes(0, 29_400_000) < 20.1 * 29_400_000          # 12 to 20 bytes per face
    for call in WITH_WORKSPACE:
        need = lib.perf_meshsimp_workspace_bytes(8, 10)
        rc, msg = call(ws_bytes=need - 8)
        assert rc == PERF_E_INVALID and 'workspace' in msg and 'bytes' in msg, msg
        rc, msg = call(ws=ctypes.c_void_p(72))
        assert rc == PERF_E_INVALID and '16-byte aligned' in msg, msg
    rc, msg = _place(ws_bytes=48 * 5 - 8)
    assert rc == PERF_E_INVALID and 'the scratch holds 232 bytes, 240 are needed' in msg, msg
    rc, msg = _place(ws=ctypes.c_void_p(72))
    assert rc == PERF_E_INVALID and '16-byte aligned' in msg, msg


def test_python_surface():
    import torch
    import perf_amd
    from perf_amd import mesh, ops, scene
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    names = lambda f: [k for k, _ in params(f)]
    E = inspect.Parameter.empty
    assert mesh.Clusters._fields == ('vertex_cluster', 'n_clusters', 'vertices', 'representative')
    assert params(mesh.cluster_vertices) == [('vertices', E), ('cell', E), ('box', None), ('placement', 'mean')]
    assert params(mesh.cluster_faces) == [('faces', E), ('clusters', E), ('dedupe', 'oriented')]
    assert params(mesh.simplify_mesh) == [('mesh', E), ('cell', E), ('box', None), ('placement', 'mean'), ('dedupe', 'oriented')]
    assert names(scene.NeRFScene.simplify_mesh) == ['self', 'mesh', 'cell', 'kw']
    assert names(ops.meshsimp_bounds) == ['vertices'] and names(ops.meshsimp_cluster) == ['vertices', 'lo', 'h', 'n', 'n_faces', 'ws', 'counts']
    assert names(ops.meshsimp_place) == ['vertices', 'lo', 'h', 'n', 'vertex_cluster', 'n_clusters', 'placement']
    assert names(ops.meshsimp_faces) == ['faces', 'vertex_cluster', 'dedupe', 'ws', 'flag']
    # no fallback: CPU tensors are refused
    vertices, faces = torch.rand(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cpu = mesh.Mesh(vertices, faces)
    box = ((0, 0, 0), (1, 1, 1))
    clusters = mesh.Clusters(torch.zeros(3, dtype=torch.int32), 1, vertices[:1], torch.zeros(1, dtype=torch.int32))
    for call in (lambda: mesh.cluster_vertices(vertices, 0.5, box), lambda: mesh.cluster_vertices(vertices, 0.5), lambda: mesh.cluster_faces(faces, clusters),
                 lambda: mesh.simplify_mesh(cpu, 0.5, box), lambda: ops.meshsimp_bounds(vertices), lambda: ops.meshsimp_cluster(vertices, [0, 0, 0], 0.5, [2, 2, 2]),
                 lambda: ops.meshsimp_place(vertices, [0, 0, 0], 0.5, [2, 2, 2], clusters.vertex_cluster, 1),
                 lambda: ops.meshsimp_faces(faces, clusters.vertex_cluster)):
        with pytest.raises(perf_amd._lib.PerfError):
            call()


def test_extract_mesh_tool_simplifies_after_it_cleans():
    text = open(os.path.join(ROOT, 'tools', 'extract_mesh.py')).read()
    options = ["'--simplify-cell'", "'--simplify-placement'", "'--simplify-dedupe'"]
    for option in options:
        assert option in text, option
    assert text.index(options[0]) < text.index(options[1]) < text.index(options[2])
    older = ["'--min-component-faces'", "'--keep-largest'", "'--orientation'", "'--seen-by-panoramas'", "'--visibility-tol'", "'--carve'", "'--sup-pool'"]
    assert [text.index(o) for o in older] == sorted(text.index(o) for o in older) and text.index(older[-1]) < text.index(options[0])
    cull, clean, simplify = text.index('scene.cull_unseen_mesh('), text.index('scene.clean_mesh('), text.index('scene.simplify_mesh(')
    assert cull < clean < simplify < text.index('write_ply(args.out')
