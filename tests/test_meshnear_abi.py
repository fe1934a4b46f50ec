"""The closest point of a mesh (include/staged/perf_hip_meshnear.h, perf_amd/mesh.py) checked without a GPU.  The unit is STAGED: it is
not in the pinned table of tests/test_abi_units.py, so what that file checks for a pinned unit is checked here for this one -- the
header's macro, the binding, the record and the library agree, the digest is current, the declared names are the binding's, disjoint
from every pinned unit's, the build depends on the header -- beside what is particular to it: the header's statement, every refusal
before a launch with its message (the fake pointers are never dereferenced), and the Python surface."""
import ctypes
import inspect
import json
import os
import re

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

ROOT = abi_units.ROOT
HEADER = os.path.join(ROOT, 'include', 'staged', 'perf_hip_meshnear.h')
FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
ARITY = {'perf_meshnear_version': 0, 'perf_meshnear_query': 18}
BASE = {'vertices': FAKE, 'V': 8, 'faces': FAKE, 'F': 10, 'origin': (0.0, 0.0, 0.0), 'cell': 0.5, 'dims': (4, 3, 2), 'offsets': FAKE, 'refs': FAKE, 'R': 30,
        'points': FAKE, 'N': 5, 'max_distance': float('inf'), 'dist2': FAKE, 'face': FAKE, 'u': FAKE, 'v': FAKE}


def _query(**kw):
    a = dict(BASE)
    a.update(kw)
    origin = (ctypes.c_float * 3)(*a['origin']) if a['origin'] is not None else None
    dims = (ctypes.c_int32 * 3)(*a['dims']) if a['dims'] is not None else None
    return _call('perf_meshnear_query', a['vertices'], a['V'], a['faces'], a['F'], origin, a['cell'], dims, a['offsets'], a['refs'], a['R'], a['points'], a['N'],
                 a['max_distance'], a['dist2'], a['face'], a['u'], a['v'], None)


def _text():
    text = open(HEADER).read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_header_binding_record_and_library_agree():
    from perf_amd import _lib
    abi_digest = abi_units.abi_digest()
    assert [u.name for u in _lib._STAGED_UNITS] == ['meshnear']
    unit = _lib._STAGED_UNITS[0]
    assert (unit.header, unit.record, unit.macro, unit.version_fn) == ('staged/perf_hip_meshnear.h', 'staged/perf_hip_meshnear.abi.json', 'PERF_MESHNEAR_ABI_VERSION',
                                                                     'perf_meshnear_version')
    assert type(unit) is type(_lib._UNITS[0])
    text, plain = _text()
    record = json.load(open(abi_digest.record_path('meshnear')))
    lib = _lib.load()
    assert abi_units.const(text, unit.macro) == _lib.MESHNEAR_ABI_VERSION == unit.version == record['version'] == lib.perf_meshnear_version() == 1
    now = abi_digest.digest(HEADER, unit.macro)
    assert now == record == abi_digest.digest_unit('meshnear'), 'the header changed: bump PERF_MESHNEAR_ABI_VERSION, then `python tools/abi_digest.py --meshnear --write`'
    assert abi_digest.header_path('meshnear') == HEADER
    declared = sorted(set(re.findall(r'\b(perf_[a-z0-9_]+)\s*\(', plain)))
    assert declared == sorted(unit.sigs) == sorted(ARITY)
    for fn, (_, args) in unit.sigs.items():
        params = abi_units.params(plain, fn).strip()
        assert (0 if params in ('', 'void') else len(params.split(','))) == len(args) == ARITY[fn], fn
        assert hasattr(lib, fn) and len(getattr(lib, fn).argtypes or []) == len(args), fn
    assert next(iter(unit.sigs)) == unit.version_fn
    # the constants, and the counts are 64-bit at the boundary
    const = lambda name: abi_units.const(text, name)
    assert const('PERF_MESHNEAR_MAX_CELLS') == _lib.MESHNEAR_MAX_CELLS == _lib.MESHRAY_MAX_CELLS == 1 << 24
    assert const('PERF_MESHNEAR_MAX_VERTICES') == _lib.MESHNEAR_MAX_VERTICES == _lib.MESHRAY_MAX_VERTICES == 1 << 30
    assert const('PERF_MESHNEAR_MAX_FACES') == _lib.MESHNEAR_MAX_FACES == _lib.MESHRAY_MAX_FACES == (1 << 31) - 1
    params = abi_units.params(plain, 'perf_meshnear_query')
    for piece in ('int64_t n_vertices', 'int64_t n_faces', 'int64_t n_refs', 'int64_t n_points', 'float max_distance', 'double* dist2_out', 'void* stream'):
        assert piece in params, piece
    # the grid's arguments are perf_meshray_cast's, type for type: one RayGrid serves both
    assert unit.sigs['perf_meshnear_query'][1][:10] == _lib._SIGS_MESHRAY['perf_meshray_cast'][1][:10]
    assert '#include "perf_hip' not in text and 'typedef struct' not in text          # it stands alone


def test_the_staged_names_are_disjoint_from_every_pinned_unit():
    from perf_amd import _lib
    staged = set(_lib._STAGED_UNITS[0].sigs)
    assert len(_lib._UNITS) == 15
    for unit in _lib._UNITS:
        assert not (staged & set(unit.sigs)), unit.name
    assert 'meshnear' not in [u.name for u in _lib._UNITS]
    # the pinned table's own view of include/ does not see the staged folder
    assert not [n for n in os.listdir(os.path.join(ROOT, 'include')) if 'meshnear' in n]
    assert sorted(os.listdir(os.path.join(ROOT, 'include', 'staged'))) == ['perf_hip_meshnear.abi.json', 'perf_hip_meshnear.h']


def test_the_unit_is_built_with_its_own_header_alone():
    from perf_amd import build
    assert build.SOURCES.count('meshnear.hip') == 1 and len(set(build.SOURCES)) == len(build.SOURCES)
    assert os.path.normpath(HEADER) in abi_units.build_deps()
    reached = build._includes(os.path.join(build.CSRC, 'meshnear.hip'))
    public = sorted(os.path.relpath(p, os.path.join(ROOT, 'include')) for p in reached if os.path.normpath(p).startswith(os.path.join(ROOT, 'include')))
    # no public header but its own, beside the core's error codes every unit gets through common.hpp
    assert public == ['perf_hip.h', os.path.join('staged', 'perf_hip_meshnear.h')], public
    assert '#include "../../include/perf_hip.h"' in open(os.path.join(build.CSRC, 'common.hpp')).read()
    assert [s for s in build.SOURCES if os.path.normpath(HEADER) in {os.path.normpath(p) for p in build._includes(os.path.join(build.CSRC, s))}] == ['meshnear.hip']
    assert any(p.endswith(os.sep + 'mesh_check_host.hpp') for p in reached)             # the counts' checks are the shared ones
    unit = open(os.path.join(ROOT, 'perf_amd', 'csrc', 'meshnear.hip')).read()
    assert '#include "../../include/staged/perf_hip_meshnear.h"' in unit and 'mesh_counts_check(' in unit
    assert unit.count('#pragma clang fp contract(off)') >= 3 and "'-ffp-contract=off'" in open(os.path.join(ROOT, 'perf_amd', 'build.py')).read()
    for name in ('atomic', 'fmaf(', 'fma(', '__fma', 'sqrt', '__syncthreads', '__shared__'):
        assert name not in unit.replace('No atomics', ''), name
    # the protection against a hang: the bounded loops say what bounds them
    for phrase in ('At most max(nx, ny, nz) shells', 'Nothing here waits on another thread', 'Bounded by the cell\'s count', 'before anything is read',
                   'validated when the grid was', 'every denominator is tested first', 'at least D + m away'):
        assert phrase in unit, phrase


def test_the_header_states_the_rule_the_search_and_what_it_does_not_do():
    comment = re.search(r'/\*.*?\*/', open(HEADER).read(), re.S).group(0)
    comment = re.sub(r'\s*\n \*\s*', ' ', comment)
    for phrase in ('every value is a DOUBLE formed from the fp32 inputs', 'each operation rounds once', 'nothing is contracted', 'x . y = (xx yx + xy yy) + xz yz',
                   'ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c', 'd1 = ab . ap, d2 = ac . ap, d3 = ab . bp, d4 = ac . bp, d5 = ab . cp, d6 = ac . cp',
                   'vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, e = d4 - d3, g = d5 - d6', 'the FIRST of these tests that holds',
                   'every comparison false on NaN', 'd1 <= 0 and d2 <= 0', 'd3 >= 0 and d4 <= d3', 'd6 >= 0 and d5 <= d6',
                   'vc <= 0 and d1 >= 0 and d3 <= 0 and (d1 - d3) > 0', 'u = d1 / (d1 - d3), v = 0', 'vb <= 0 and d2 >= 0 and d6 <= 0 and (d2 - d6) > 0',
                   'va <= 0 and e >= 0 and g >= 0 and (e + g) > 0', 'v = e / (e + g), u = 1 - v', 'va > 0 and vb > 0 and vc > 0',
                   'den = (va + vb) + vc, u = vb / den, v = vc / den', 'the first of equals', 'q = (a + u ab) + v ac, r = p - q', 'dist2 = (rx rx + ry ry) + rz rz',
                   'Every division\'s denominator is tested first', 'with dist2 == 0 exactly', 'A degenerate face', 'is never the answer', 'No square root is taken',
                   'the lexicographic minimum of (dist2, face index) over ALL faces', 'never "over the cells visited"', '+inf, -1, 0, 0', 'reads nothing',
                   '(double)max_distance * (double)max_distance', 'm = cell / 8', 'shells of growing Chebyshev radius', 'may be tested more than once',
                   'not the grid\'s own boundary', 'best dist2 <= D * D, or D > max_distance, or the block is the whole grid', 'at most max(nx, ny, nz) shells',
                   'at least D + m from the point', 'many orders below m', 'neither win nor tie', 'does not depend on cell or dims', 'bit-identical from run to run',
                   'O((d / cell)^3)', 'max_distance is the way to bound it', 'no BVH', 'no sparse or two-level grid', 'no empty-space skipping', 'no signed distance',
                   'no exact (unsampled) Hausdorff distance', 'max_distance NaN or negative'):
        assert phrase in comment, phrase


def test_refuses_null_pointers():
    for kw in ({'vertices': None}, {'faces': None}, {'origin': None}, {'dims': None}, {'offsets': None}, {'refs': None}, {'points': None}):
        rc, msg = _query(**kw)
        assert rc == PERF_E_INVALID and 'perf_meshnear_query: NULL input' in msg, (kw, msg)
    for kw in ({'dist2': None}, {'face': None}):
        rc, msg = _query(**kw)
        assert rc == PERF_E_INVALID and 'NULL output (dist2_out or face_out)' in msg, (kw, msg)
    # u and v are optional: the refusal that remains is the one asked for
    rc, msg = _query(u=None, v=None, max_distance=-1.0)
    assert rc == PERF_E_INVALID and 'max_distance' in msg, msg


def test_refuses_the_box_with_the_ray_units_messages():
    for bad in (0.0, -0.5, float('inf'), float('nan')):
        rc, msg = _query(cell=bad)
        assert rc == PERF_E_INVALID and 'cell edge' in msg and 'not positive or not finite' in msg, (bad, msg)
    for bad in ((0, 3, 2), (4, -1, 2), (4, 3, 0)):
        rc, msg = _query(dims=bad)
        assert rc == PERF_E_INVALID and 'is below 1' in msg, (bad, msg)
    for bad in ((257, 256, 256), (1 << 24, 2, 1), (2048, 2048, 2048)):
        rc, msg = _query(dims=bad)
        assert rc == PERF_E_INVALID and 'more than 2^24 cells' in msg, (bad, msg)
    rc, msg = _query(origin=(0.0, float('nan'), 0.0))
    assert rc == PERF_E_INVALID and 'origin[1]' in msg and 'not finite' in msg, msg


def test_refuses_counts_and_the_limit():
    for kw, reason in (({'V': -1}, 'negative number of vertices'), ({'F': -1}, 'negative number of faces'), ({'V': (1 << 30) + 1}, '2^30'), ({'F': 1 << 31}, '2^31 - 1'),
                       ({'R': -1}, 'negative number of references'), ({'R': 1 << 31}, '2^31 or more'), ({'N': -1}, 'negative number of points'),
                       ({'N': (1 << 38) + 1}, 'more than 2^38'), ({'max_distance': float('nan')}, 'max_distance (nan) is NaN or negative'),
                       ({'max_distance': -0.5}, 'max_distance (-0.5) is NaN or negative')):
        rc, msg = _query(**kw)
        assert rc == PERF_E_INVALID and reason in msg and msg.startswith('perf_meshnear_query: '), (kw, msg)
    # nothing to do is not a refusal, whatever the pointers are: no points
    rc, msg = _query(N=0, points=None, dist2=None, face=None, u=None, v=None)
    assert rc == 0, msg


def test_python_surface():
    import torch
    import perf_amd
    from perf_amd import mesh, ops, scene
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    names = lambda f: [k for k, _ in params(f)]
    E, inf = inspect.Parameter.empty, float('inf')
    assert mesh.NearestHits._fields == ('dist2', 'distance', 'face', 'u', 'v')
    assert mesh.Deviation._fields[:7] == ('max', 'mean', 'rms', 'p90', 'argmax_point', 'argmax_face_of_b', 'n_samples')
    assert mesh.Deviation._fields[7:] == ('n_beyond', 'a_to_b', 'b_to_a')
    assert params(mesh.closest_point) == [('mesh', E), ('grid', E), ('points', E), ('max_distance', inf)]
    assert params(mesh.surface_samples) == [('mesh', E), ('order', 2)]
    assert params(mesh.mesh_deviation) == [('a', E), ('b', E), ('order', 2), ('symmetric', True), ('cell', None), ('max_distance', inf)]
    assert params(mesh.simplify_to_tolerance) == [('mesh', E), ('tol', E), ('cells', None), ('placement', 'quadric'), ('order', 2), ('kw', E)]
    assert params(mesh.transfer_vertex_values) == [('src_mesh', E), ('values', E), ('hits', E)]
    assert names(scene.NeRFScene.mesh_deviation) == ['self', 'a', 'b', 'kw'] and names(scene.NeRFScene.simplify_mesh_to_tolerance) == ['self', 'mesh', 'tol', 'kw']
    assert names(ops.meshnear_query) == ['vertices', 'faces', 'origin', 'cell', 'dims', 'offsets', 'refs', 'points', 'max_distance', 'uv']
    assert mesh._lattice(1) == [] and mesh._lattice(2) == [(1, 0, 1), (1, 1, 0), (0, 1, 1)] and len(mesh._lattice(5)) == 21 - 3
    # no fallback: CPU tensors are refused
    vertices, faces = torch.rand(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cpu = mesh.Mesh(vertices, faces)
    grid = mesh.RayGrid((0.0, 0.0, 0.0), 1.0, (1, 1, 1), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 3, 1, -1)
    hits = mesh.NearestHits(torch.zeros(3, dtype=torch.float64), torch.zeros(3), torch.zeros(3, dtype=torch.int32), torch.zeros(3), torch.zeros(3))
    for call in (lambda: mesh.closest_point(cpu, grid, vertices), lambda: mesh.surface_samples(cpu), lambda: mesh.mesh_deviation(cpu, cpu),
                 lambda: mesh.simplify_to_tolerance(cpu, 0.1), lambda: mesh.transfer_vertex_values(cpu, vertices, hits),
                 lambda: ops.meshnear_query(vertices, faces, (0, 0, 0), 1.0, (1, 1, 1), grid.offsets, grid.refs, vertices)):
        with pytest.raises(perf_amd._lib.PerfError):
            call()


def test_extract_mesh_tool_takes_the_tolerance_and_the_report():
    text = open(os.path.join(ROOT, 'tools', 'extract_mesh.py')).read()
    assert "'--simplify-tolerance'" in text and "'--report-deviation'" in text and 'are exclusive' in text
    assert text.index('scene.simplify_mesh(') < text.index('scene.simplify_mesh_to_tolerance(') < text.index('write_ply(args.out')
    assert text.count("report('") == 5          # the two culls, the cleaning, the two simplifications


def test_the_documents_name_the_staged_unit():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'staged unit' in integration and '_STAGED_UNITS' in integration and 'include/staged/' in integration
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '5.6.8' in design and 'perf_meshnear_query' in design
