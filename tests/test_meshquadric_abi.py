"""The quadric error placement (include/perf_hip_meshquadric.h, perf_amd/mesh.py) checked without a GPU: the header's constants and parameter
types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); the header states the rule; the unit
lives where the build and the other units' tests need it; every refusal happens before a launch with a message that names its reason (the
fake pointers are never dereferenced); the Python surface has the documented signatures and refuses CPU tensors; the extraction tool offers
'quadric'."""
import ctypes
import inspect
import os
import re

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
NAMES = ['perf_meshquadric_place', 'perf_meshquadric_sums', 'perf_meshquadric_version']
ARITY = {'perf_meshquadric_version': 0, 'perf_meshquadric_sums': 15, 'perf_meshquadric_place': 13}


def _lo(values):
    return (ctypes.c_float * 3)(*values) if values is not None else None


def _sums(**kw):
    a = {'vertices': FAKE, 'V': 8, 'faces': FAKE, 'F': 10, 'lo': (0.0, 0.0, 0.0), 'h': 0.25, 'n': (4, 4, 4), 'vc': FAKE, 'C': 3, 'acc': FAKE, 'bad': FAKE, 'skipped': FAKE}
    a.update(kw)
    return _call('perf_meshquadric_sums', a['vertices'], a['V'], a['faces'], a['F'], _lo(a['lo']), a['h'], *a['n'], a['vc'], a['C'], a['acc'], a['bad'], a['skipped'], None)


def _place(**kw):
    a = {'vertices': FAKE, 'V': 8, 'lo': (0.0, 0.0, 0.0), 'h': 0.25, 'n': (4, 4, 4), 'anchor': FAKE, 'rep': FAKE, 'acc': FAKE, 'C': 3, 'out': FAKE}
    a.update(kw)
    return _call('perf_meshquadric_place', a['vertices'], a['V'], _lo(a['lo']), a['h'], *a['n'], a['anchor'], a['rep'], a['acc'], a['C'], a['out'], None)


ALL = (_sums, _place)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [meshquadric] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, plain = abi_units.header('meshquadric')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_MESHQUADRIC_ABI_VERSION') == _lib.MESHQUADRIC_ABI_VERSION == 1
    assert const('PERF_MESHQUADRIC_MAX_VERTICES') == _lib.MESHQUADRIC_MAX_VERTICES == _lib.MESHSIMP_MAX_VERTICES == 1 << 30
    assert const('PERF_MESHQUADRIC_MAX_FACES') == _lib.MESHQUADRIC_MAX_FACES == _lib.MESHSIMP_MAX_FACES == (1 << 31) - 1
    assert const('PERF_MESHQUADRIC_MAX_CELLS') == _lib.MESHQUADRIC_MAX_CELLS == _lib.MESHSIMP_MAX_CELLS == 1 << 21
    assert const('PERF_MESHQUADRIC_TERMS') == _lib.MESHQUADRIC_TERMS == 9
    assert const('PERF_MESHQUADRIC_FRACTION_BITS') == _lib.MESHQUADRIC_FRACTION_BITS == 40
    assert const('PERF_MESHQUADRIC_SKIP_BITS') == _lib.MESHQUADRIC_SKIP_BITS == 60
    assert const('PERF_MESHQUADRIC_REGULARISER_BITS') == _lib.MESHQUADRIC_REGULARISER_BITS == 10
    # the header stands alone
    assert '#include "perf_hip' not in header and 'typedef struct' not in header and '#include <stdint.h>' in header
    assert {name: len(args) for name, (_, args) in _lib._SIGS_MESHQUADRIC.items()} == ARITY
    for name in NAMES[:2]:
        params = abi_units.params(plain, name)
        assert 'int64_t n_vertices' in params and 'const float* lo' in params and 'float h' in params and 'int64_t n_clusters' in params and 'void* stream' in params, name
    # 'quadric' is the wrapper's: the clustering unit's placements are what they were
    assert _lib.MESHSIMP_PLACEMENT == {'mean': 0, 'member': 1}


def test_the_header_states_the_rule_and_what_it_does_not_do():
    comment = re.search(r'/\*.*?\*/', open(os.path.join(ROOT, 'include', 'perf_hip_meshquadric.h')).read(), re.S).group(0)
    comment = re.sub(r'\s*\n \*\s*', ' ', comment)
    for phrase in ('Each operation rounds once and nothing is contracted', 'No square root and no division happen before a quantisation',
                   'only + - * / and llrint are used', 't = ((double)x - (double)lo) / (double)h', 'i = min((int64)floor(t), n - 1)', 'f = t - (double)i',
                   'e1 = (b - a) / h and e2 = (c - a) / h', 'n = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)', 'n is unnormalised',
                   'squared area in cell units', 'xx, xy, xz, yy, yz, zz', 'qA_ij = llrint(n_i n_j * 2^40), ties to even', 'magnitude >= 2^60, the face contributes nothing',
                   'goes to skipped_face_dev', 'one 64-bit integer atomicMin per such face', 'The flag is information, not a refusal', 'r = f - 0.5',
                   'd = (n_x r_x + n_y r_y) + n_z r_z', 'qb_i = llrint((n_i d) * 2^40)', '64-bit integer atomicAdd', 'acc is int64 [C, 9], zeroed by the call',
                   'A face counts once per corner', 'gets it twice', 'the sum of per-vertex quadrics', 'goes to bad_face_dev', 'a cluster id of -1',
                   'exact in any order and any grouping', 'They wrap modulo 2^64', 'terms near 2^32', 'A_ij = (double)acc_ij * 2^-40', 'tr = (A_xx + A_yy) + A_zz',
                   'If tr is not > 0, the output row is anchor\'s row, bit for bit', 'm_c = ((double)anchor_c - lo_c) / h - ((double)i_c + 0.5)',
                   'lambda = tr * 2^-10', 'M = A + lambda I', 'g_c = b_c + lambda m_c', 'on a plane the vertex is the mean moved onto the plane',
                   'at a corner it is the corner', 'c00 = Myy Mzz - Myz Myz', 'c01 = Mxz Myz - Mxy Mzz', 'c02 = Mxy Myz - Mxz Myy', 'c11 = Mxx Mzz - Mxz Mxz',
                   'c12 = Mxy Mxz - Mxx Myz', 'c22 = Mxx Myy - Mxy Mxy', 'det = (Mxx c00 + Mxy c01) + Mxz c02', 'If det is not > 0 or not finite',
                   'x_x = ((c00 g_x + c01 g_y) + c02 g_z) / det', 'x_y = ((c01 g_x + c11 g_y) + c12 g_z) / det', 'x_z = ((c02 g_x + c12 g_y) + c22 g_z) / det',
                   'A component that is not finite gives the anchor\'s row', 'x_c = min(max(x_c, -0.5), 0.5)', 'p_c = (double)lo_c + (((double)i_c + 0.5) + x_c) * (double)h',
                   'The output is (float)p_c', 'no face budget', 'no manifold repair', 'no boundary or feature constraints', 'no attribute quadrics',
                   'skipped by the 2^60 rule', 'V above 2^30, F above 2^31 - 1, C above V', 'a dimension outside 1 .. 2^21', 'no floating-point atomics',
                   'sends 9 atomics, not 27', 'every lane on one 72-byte row', 'no thread waits on another'):
        assert phrase in comment, phrase


def test_the_code_lives_where_the_older_abi_tests_need_it():
    from perf_amd import build
    includes = lambda name: build._includes(os.path.join(build.CSRC, name))
    reaches = lambda name, header: any(p.endswith(os.sep + header) for p in includes(name))
    assert build.SOURCES.count('meshquadric.hip') == 1 and len(set(build.SOURCES)) == len(build.SOURCES)
    assert os.path.join(ROOT, 'include', 'perf_hip_meshquadric.h') in abi_units.build_deps()
    assert [s for s in build.SOURCES if reaches(s, 'perf_hip_meshquadric.h')] == ['meshquadric.hip']
    assert [s for s in build.SOURCES if reaches(s, 'perf_hip_meshsimp.h')] == ['meshsimp.hip']
    for header in ('perf_hip_meshsimp.h', 'perf_hip_meshvis.h', 'perf_hip_meshcolor.h', 'perf_hip_meshray.h', 'perf_hip_meshtex.h', 'meshtex_device.hpp'):
        assert not reaches('meshquadric.hip', header), header
    unit = open(os.path.join(build.CSRC, 'meshquadric.hip')).read()
    for name in NAMES:
        assert re.search(r'extern "C" \w+ ' + name + r'\(', unit), name
    assert unit.count('#pragma clang fp contract(off)') >= 3
    assert not re.search(r'atomic\w*\s*\(\s*\(?\s*(float|double)', unit)          # no floating-point atomics
    for name in ('sqrt', 'fmaf(', 'fma(', '__fma', 'unsafeAtomicAdd', '__syncthreads', 'while ('):
        assert name not in unit, name


def test_refuses_null_pointers():
    for call, kws in ((_sums, ({'vertices': None}, {'faces': None}, {'vc': None}, {'lo': None})), (_place, ({'vertices': None}, {'lo': None}, {'anchor': None}, {'rep': None}, {'acc': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_sums, ({'acc': None}, {'bad': None}, {'skipped': None})), (_place, ({'out': None},))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL output' in msg, (call.__name__, kw, msg)


def test_refuses_counts_and_the_grid():
    for call in ALL:
        rc, msg = call(V=-1)
        assert rc == PERF_E_INVALID and 'negative number of vertices' in msg, (call.__name__, msg)
        rc, msg = call(V=(1 << 30) + 1)
        assert rc == PERF_E_INVALID and '2^30' in msg, (call.__name__, msg)
        rc, msg = call(C=-1)
        assert rc == PERF_E_INVALID and 'negative number of clusters' in msg, (call.__name__, msg)
        rc, msg = call(C=9)
        assert rc == PERF_E_INVALID and '9 clusters, the mesh has 8 vertices' in msg, (call.__name__, msg)
        for bad in (0.0, -0.25, float('inf'), float('nan')):
            rc, msg = call(h=bad)
            assert rc == PERF_E_INVALID and 'cell edge h' in msg and 'not positive or not finite' in msg, (call.__name__, bad, msg)
        for bad in ((float('nan'), 0.0, 0.0), (0.0, float('inf'), 0.0), (0.0, 0.0, -float('inf'))):
            rc, msg = call(lo=bad)
            assert rc == PERF_E_INVALID and 'origin lo is not finite' in msg, (call.__name__, msg)
        for bad in ((0, 4, 4), (4, -1, 4), (4, 4, (1 << 21) + 1)):
            rc, msg = call(n=bad)
            assert rc == PERF_E_INVALID and 'outside 1 .. 2^21' in msg, (call.__name__, bad, msg)
    rc, msg = _sums(F=-1)
    assert rc == PERF_E_INVALID and 'negative number of faces' in msg, msg
    rc, msg = _sums(F=1 << 31)
    assert rc == PERF_E_INVALID and '2^31 - 1' in msg, msg


def test_python_surface():
    import torch
    import perf_amd
    from perf_amd import mesh, ops, scene
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    names = lambda f: [k for k, _ in params(f)]
    E = inspect.Parameter.empty
    assert mesh.QuadricPlacement._fields == ('vertices', 'skipped')
    assert params(mesh.quadric_placement) == [('mesh', E), ('clusters', E), ('cell', E), ('box', None)]
    assert params(mesh.simplify_mesh) == [('mesh', E), ('cell', E), ('box', None), ('placement', 'mean'), ('dedupe', 'oriented')]
    assert params(mesh.cluster_vertices) == [('vertices', E), ('cell', E), ('box', None), ('placement', 'mean')]
    assert mesh.Clusters._fields == ('vertex_cluster', 'n_clusters', 'vertices', 'representative')
    assert params(scene.NeRFScene.simplify_mesh) == [('self', E), ('mesh', E), ('cell', E), ('kw', E)]
    assert names(ops.meshquadric_sums) == ['vertices', 'faces', 'lo', 'h', 'n', 'vertex_cluster', 'n_clusters', 'flags']
    assert names(ops.meshquadric_place) == ['vertices', 'lo', 'h', 'n', 'anchor', 'representative', 'acc']
    assert names(ops.meshsimp_place) == ['vertices', 'lo', 'h', 'n', 'vertex_cluster', 'n_clusters', 'placement']
    for doc in (mesh.simplify_mesh.__doc__, mesh.cluster_vertices.__doc__, scene.NeRFScene.simplify_mesh.__doc__):
        assert 'quadric' in doc
    # the placements are named, all three, where one is refused
    with pytest.raises(perf_amd._lib.PerfError, match="'mean', 'member' or 'quadric'"):
        mesh._check_placement('who', 'median')
    mesh._check_placement('who', 'quadric')
    # no fallback: CPU tensors are refused
    vertices, faces = torch.rand(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cpu = mesh.Mesh(vertices, faces)
    clusters = mesh.Clusters(torch.zeros(3, dtype=torch.int32), 1, torch.zeros(1, 3), torch.zeros(1, dtype=torch.int32))
    for call in (lambda: mesh.simplify_mesh(cpu, 0.5, placement='quadric'), lambda: mesh.quadric_placement(cpu, clusters, 0.5),
                 lambda: ops.meshquadric_sums(vertices, faces, (0, 0, 0), 0.5, (2, 2, 2), clusters.vertex_cluster, 1),
                 lambda: ops.meshquadric_place(vertices, (0, 0, 0), 0.5, (2, 2, 2), clusters.vertices, clusters.representative, torch.zeros(1, 9, dtype=torch.int64))):
        with pytest.raises(perf_amd._lib.PerfError):
            call()
    # the clustering alone has no faces to read: it says who has
    with pytest.raises(perf_amd._lib.PerfError, match='quadric_placement'):
        mesh.cluster_vertices(torch.rand(3, 3), 0.5, placement='quadric')


def test_extract_mesh_tool_offers_quadric():
    text = open(os.path.join(ROOT, 'tools', 'extract_mesh.py')).read()
    assert "choices=['mean', 'member', 'quadric']" in text and '--simplify-placement mean|member|quadric' in text
    assert 'quadric error' in text.split("'--simplify-placement'")[1].split('ap.add_argument')[0]
    assert 'placement=args.simplify_placement' in text
