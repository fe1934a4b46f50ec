"""Rays against a mesh on a uniform grid (include/perf_hip_meshray.h, perf_amd/mesh.py) checked without a GPU: the header's constants and
parameter types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal happens
before a launch with a message that names its reason (the fake pointers are never dereferenced); the header states the rule; the Python
surface has the documented signatures and refuses CPU tensors; the extraction tool takes --occlusion."""
import ctypes
import inspect
import os
import re

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
NAMES = ['perf_meshray_cast', 'perf_meshray_grid_count', 'perf_meshray_grid_write', 'perf_meshray_occluded', 'perf_meshray_version']
ARITY = {'perf_meshray_version': 0, 'perf_meshray_grid_count': 10, 'perf_meshray_grid_write': 13, 'perf_meshray_cast': 22, 'perf_meshray_occluded': 15}


def _box(a):
    origin = (ctypes.c_float * 3)(*a['origin']) if a['origin'] is not None else None
    dims = (ctypes.c_int32 * 3)(*a['dims']) if a['dims'] is not None else None
    return a['vertices'], a['V'], a['faces'], a['F'], origin, a['cell'], dims


BASE = {'vertices': FAKE, 'V': 8, 'faces': FAKE, 'F': 10, 'origin': (0.0, 0.0, 0.0), 'cell': 0.5, 'dims': (4, 3, 2)}


def _count(**kw):
    a = dict(BASE, counts=FAKE, flag=FAKE)
    a.update(kw)
    return _call('perf_meshray_grid_count', *_box(a), a['counts'], a['flag'], None)


def _write(**kw):
    a = dict(BASE, counts=FAKE, offsets=FAKE, R=30, refs=FAKE, capacity=30)
    a.update(kw)
    return _call('perf_meshray_grid_write', *_box(a), a['counts'], a['offsets'], a['R'], a['refs'], a['capacity'], None)


def _cast(**kw):
    a = dict(BASE, offsets=FAKE, refs=FAKE, R=30, rays_o=FAKE, rays_d=FAKE, N=5, t_min=0.0, t_max=float('inf'), any_hit=0, t=FAKE, face=FAKE, u=FAKE, v=FAKE, hit=FAKE)
    a.update(kw)
    return _call('perf_meshray_cast', *_box(a), a['offsets'], a['refs'], a['R'], a['rays_o'], a['rays_d'], a['N'], a['t_min'], a['t_max'], a['any_hit'], a['t'], a['face'],
                 a['u'], a['v'], a['hit'], None)


def _occluded(**kw):
    a = dict(BASE, offsets=FAKE, refs=FAKE, R=30, centres=FAKE, K=2, mask=FAKE, out=FAKE)
    a.update(kw)
    return _call('perf_meshray_occluded', *_box(a), a['offsets'], a['refs'], a['R'], a['centres'], a['K'], a['mask'], a['out'], None)


ALL = (_count, _write, _cast, _occluded)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [meshray] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, plain = abi_units.header('meshray')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_MESHRAY_ABI_VERSION') == _lib.MESHRAY_ABI_VERSION == 1
    assert const('PERF_MESHRAY_MAX_CELLS') == _lib.MESHRAY_MAX_CELLS == 1 << 24
    assert const('PERF_MESHRAY_MAX_VIEWS') == _lib.MESHRAY_MAX_VIEWS == _lib.MESHVIS_MAX_VIEWS == 64
    assert const('PERF_MESHRAY_MAX_VERTICES') == _lib.MESHRAY_MAX_VERTICES == 1 << 30
    assert const('PERF_MESHRAY_MAX_FACES') == _lib.MESHRAY_MAX_FACES == (1 << 31) - 1
    assert '#include "perf_hip' not in header and 'typedef struct' not in header          # it stands alone: the other headers do not change
    assert {name: len(args) for name, (_, args) in _lib._SIGS_MESHRAY.items()} == ARITY
    # counts are 64-bit at the boundary
    for name in NAMES[:4]:
        params = abi_units.params(plain, name)
        assert 'int64_t n_vertices' in params and 'int64_t n_faces' in params and 'void* stream' in params, name
    assert 'int64_t n_rays' in plain and 'int64_t n_refs' in plain and 'int64_t ref_capacity' in plain and 'int64_t n_refs_counted' in plain


def test_the_header_states_the_rule_and_what_it_does_not_do():
    comment = re.search(r'/\*.*?\*/', open(os.path.join(ROOT, 'include', 'perf_hip_meshray.h')).read(), re.S).group(0)
    comment = re.sub(r'\s*\n \*\s*', ' ', comment)
    for phrase in ('e1 = b - a, e2 = c - a', 'p  = (dy e2z - dz e2y,  dz e2x - dx e2z,  dx e2y - dy e2x)', 'det = (e1x px + e1y py) + e1z pz', 'det == 0 or NaN: no hit',
                   's  = o - a', 'u  = ((sx px + sy py) + sz pz) / det', 'q  = (sy e1z - sz e1y,  sz e1x - sx e1z,  sx e1y - sy e1x)',
                   'v  = ((dx qx + dy qy) + dz qz) / det', 't  = ((e2x qx + e2y qy) + e2z qz) / det',
                   'hit  <=>  u >= 0 and v >= 0 and (u + v) <= 1 and t_min <= t <= t_max', 'every comparison false on NaN', 'two-sided: no backface culling',
                   'NOT WATERTIGHT along shared edges', 'the lexicographic minimum of (t, face index) over ALL faces', 'never "over the cells visited"',
                   '+inf, -1, 0, 0', 'STRICT 0 < t < 1', 'faces that name index v are not tested', 'a subset of the mask', 'bits >= K are 0', 'm = cell / 8',
                   '[floor((min - m - origin) / cell), floor((max + m - origin) / cell)]', 'a face wholly outside the box is listed nowhere',
                   'integer atomicAdd only', 'The order of the references inside a cell is unspecified', 'R >= 2^31 is refused',
                   '64 MiB of int32 counts and 64 MiB of int32 offsets', 'at most nx + ny + nz + 2 steps', 'a hit point lies in its face\'s bounding box',
                   'many orders below m', 'No floating-point atomics', 'bit-identical from run to run', 'no BVH', 'no sparse or two-level grid', 'no texture bake',
                   'no occlusion in the colouring of perf_hip_meshcolor.h', 't_min or t_max NaN', 'K outside 0 .. 64'):
        assert phrase in comment, phrase


def test_the_unit_is_built_with_its_own_header():
    from perf_amd import build
    assert 'meshray.hip' in build.SOURCES and len(set(build.SOURCES)) == len(build.SOURCES)
    assert os.path.join(ROOT, 'include', 'perf_hip_meshray.h') in abi_units.build_deps()
    text = open(os.path.join(ROOT, 'perf_amd', 'build.py')).read()
    users = [s for s in build.SOURCES if any(p.endswith(os.sep + 'perf_hip_meshray.h') for p in build._includes(os.path.join(build.CSRC, s)))]
    assert users == ['meshray.hip'], users          # the units that include the header, by their #include lines, are the ones rebuilt for it
    assert "'-ffp-contract=off'" in text
    unit = open(os.path.join(ROOT, 'perf_amd', 'csrc', 'meshray.hip')).read()
    assert '#include "../../include/perf_hip_meshray.h"' in unit
    assert unit.count('#pragma clang fp contract(off)') >= 4          # the ranges, the rule, the walk, the segments
    assert not re.search(r'atomic\w*\s*\(\s*\(?\s*(float|double)', unit) and 'atomicAdd(counts' in unit          # integer atomics only
    for name in ('unsafeAtomicAdd', 'atomicAdd_system', 'fmaf(', 'fma(', '__fma'):
        assert name not in unit, name
    # the protection against a hang: the bounded loops say what bounds them
    for phrase in ('At most nx + ny + nz + 2 steps', 'Nothing here waits on another thread', 'bounded by the cell\'s count', 'no inf * 0',
                   'before anything is read', 'validated when the grid was'):
        assert phrase in unit, phrase


def test_refuses_null_pointers():
    for call in ALL:
        for kw in ({'vertices': None}, {'faces': None}, {'origin': None}, {'dims': None}):
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_count, ()), (_write, ({'counts': None}, {'offsets': None})), (_cast, ({'offsets': None}, {'refs': None}, {'rays_o': None}, {'rays_d': None})),
                      (_occluded, ({'offsets': None}, {'refs': None}, {'centres': None}, {'mask': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_count, ({'counts': None}, {'flag': None})), (_write, ({'refs': None},)), (_cast, ({'t': None}, {'face': None}, {'hit': None, 'any_hit': 1})),
                      (_occluded, ({'out': None},))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL output' in msg, (call.__name__, kw, msg)


def test_refuses_the_box():
    for call in ALL:
        for bad in (0.0, -0.5, float('inf'), float('nan')):
            rc, msg = call(cell=bad)
            assert rc == PERF_E_INVALID and 'cell edge' in msg and 'not positive or not finite' in msg, (call.__name__, bad, msg)
        for bad in ((0, 3, 2), (4, -1, 2), (4, 3, 0)):
            rc, msg = call(dims=bad)
            assert rc == PERF_E_INVALID and 'is below 1' in msg, (call.__name__, bad, msg)
        for bad in ((257, 256, 256), (1 << 24, 2, 1), (2048, 2048, 2048)):
            rc, msg = call(dims=bad)
            assert rc == PERF_E_INVALID and 'more than 2^24 cells' in msg, (call.__name__, bad, msg)
        rc, msg = call(origin=(0.0, float('nan'), 0.0))
        assert rc == PERF_E_INVALID and 'origin[1]' in msg and 'not finite' in msg, (call.__name__, msg)


def test_refuses_counts_and_parameters():
    for call in ALL:
        rc, msg = call(V=-1)
        assert rc == PERF_E_INVALID and 'negative number of vertices' in msg, (call.__name__, msg)
        rc, msg = call(F=-1)
        assert rc == PERF_E_INVALID and 'negative number of faces' in msg, (call.__name__, msg)
        rc, msg = call(V=(1 << 30) + 1)
        assert rc == PERF_E_INVALID and '2^30' in msg, (call.__name__, msg)
        rc, msg = call(F=1 << 31)
        assert rc == PERF_E_INVALID and '2^31 - 1' in msg, (call.__name__, msg)
    rc, msg = _write(capacity=29)
    assert rc == PERF_E_INVALID and 'room for 29 references, 30 were counted' in msg, msg
    rc, msg = _write(R=-1)
    assert rc == PERF_E_INVALID and 'negative number of counted references' in msg, msg
    rc, msg = _write(R=1 << 31, capacity=1 << 31)
    assert rc == PERF_E_INVALID and '2^31 or more' in msg, msg
    for call in (_cast, _occluded):
        rc, msg = call(R=-1)
        assert rc == PERF_E_INVALID and 'negative number of references' in msg, (call.__name__, msg)
        rc, msg = call(R=1 << 31)
        assert rc == PERF_E_INVALID and '2^31 or more' in msg, (call.__name__, msg)
    rc, msg = _cast(N=-1)
    assert rc == PERF_E_INVALID and 'negative number of rays' in msg, msg
    for kw in ({'t_min': float('nan')}, {'t_max': float('nan')}):
        rc, msg = _cast(**kw)
        assert rc == PERF_E_INVALID and 'is NaN' in msg, (kw, msg)
    for bad in (-1, 2):
        rc, msg = _cast(any_hit=bad)
        assert rc == PERF_E_INVALID and 'any_hit' in msg and 'is 0 or 1' in msg, msg
    rc, msg = _occluded(K=-1)
    assert rc == PERF_E_INVALID and 'negative number of views' in msg, msg
    rc, msg = _occluded(K=65)
    assert rc == PERF_E_INVALID and '65 views are more than 64' in msg, msg
    # u and v are optional, and the outputs of the other mode are not asked for: the refusal that remains is the one asked for
    rc, msg = _cast(u=None, v=None, hit=None, t_min=float('nan'))
    assert rc == PERF_E_INVALID and 'is NaN' in msg, msg
    rc, msg = _cast(any_hit=1, t=None, face=None, u=None, v=None, t_max=float('nan'))
    assert rc == PERF_E_INVALID and 'is NaN' in msg, msg


def test_python_surface():
    import torch
    import perf_amd
    from perf_amd import mesh, ops, scene
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    names = lambda f: [k for k, _ in params(f)]
    E = inspect.Parameter.empty
    inf = float('inf')
    assert mesh.RayGrid._fields == ('origin', 'cell', 'dims', 'offsets', 'refs', 'n_vertices', 'n_faces', 'bad_face')
    assert mesh.RayHits._fields == ('t', 'face', 'u', 'v')
    assert params(mesh.build_ray_grid) == [('mesh', E), ('cell', None)]
    assert params(mesh.cast_rays) == [('mesh', E), ('grid', E), ('origins', E), ('directions', E), ('t_min', 0.0), ('t_max', inf), ('any_hit', False)]
    assert params(mesh.vertex_occlusion) == [('mesh', E), ('grid', E), ('views', E), ('visibility', E)]
    assert params(mesh.cull_occluded) == [('mesh', E), ('views', E), ('tol', 1 / 256), ('free_tol', None), ('facing', True), ('min_views', 1), ('carve', False), ('cell', None)]
    assert params(mesh.mesh_distance) == [('mesh', E), ('grid', E), ('rays_o', E), ('rays_d', E)]
    assert params(mesh.cull_occluded)[:7] == params(mesh.cull_unseen)          # the cull's own keywords, unchanged
    assert names(scene.NeRFScene.cull_occluded_mesh) == ['self', 'mesh', 'sup_pool', 'kw']
    assert names(scene.NeRFScene.render_mesh_distance)[:3] == ['self', 'mesh', 'rays']
    assert names(ops.meshray_grid_count) == ['vertices', 'faces', 'origin', 'cell', 'dims', 'flag']
    assert names(ops.meshray_grid_write) == ['vertices', 'faces', 'origin', 'cell', 'dims', 'counts', 'offsets', 'n_refs']
    assert names(ops.meshray_cast)[:9] == ['vertices', 'faces', 'origin', 'cell', 'dims', 'offsets', 'refs', 'rays_o', 'rays_d']
    assert names(ops.meshray_occluded) == ['vertices', 'faces', 'origin', 'cell', 'dims', 'offsets', 'refs', 'centres', 'mask_bits']
    # the default cell: round(cbrt(2 F)) cells along the longest axis, in 1 .. 255 (256^3 = 2^24 cells with the margins' extra cell)
    assert [mesh._default_cells(f) for f in (0, 1, 4, 2964, 800000, 1 << 40)] == [1, 1, 2, 18, 117, 255]
    assert (255 + 1) ** 3 == perf_amd._lib.MESHRAY_MAX_CELLS
    # no fallback: CPU tensors are refused
    vertices, faces = torch.rand(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cpu = mesh.Mesh(vertices, faces)
    grid = mesh.RayGrid((0.0, 0.0, 0.0), 1.0, (1, 1, 1), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 3, 1, -1)
    view = {'pose': torch.eye(4), 'distance_map': torch.ones(4, 8)}
    bits = mesh.Visibility(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), 1)
    for call in (lambda: mesh.build_ray_grid(cpu), lambda: mesh.build_ray_grid(cpu, 0.5), lambda: mesh.cast_rays(cpu, grid, vertices, vertices),
                 lambda: mesh.cast_rays(cpu, grid, vertices, vertices, any_hit=True), lambda: mesh.vertex_occlusion(cpu, grid, [view], bits),
                 lambda: mesh.cull_occluded(cpu, [view]), lambda: mesh.mesh_distance(cpu, grid, vertices, vertices),
                 lambda: ops.meshray_grid_count(vertices, faces, (0, 0, 0), 1.0, (1, 1, 1)),
                 lambda: ops.meshray_grid_write(vertices, faces, (0, 0, 0), 1.0, (1, 1, 1), grid.offsets, grid.offsets, 1),
                 lambda: ops.meshray_cast(vertices, faces, (0, 0, 0), 1.0, (1, 1, 1), grid.offsets, grid.refs, vertices, vertices),
                 lambda: ops.meshray_occluded(vertices, faces, (0, 0, 0), 1.0, (1, 1, 1), grid.offsets, grid.refs, vertices, bits.visible)):
        with pytest.raises(perf_amd._lib.PerfError):
            call()


def test_extract_mesh_tool_takes_the_occlusion_flag():
    text = open(os.path.join(ROOT, 'tools', 'extract_mesh.py')).read()
    assert "'--occlusion'" in text and text.index("'--carve'") < text.index("'--occlusion'") < text.index("'--sup-pool'")
    occluded, unseen, clean = (text.index(c) for c in ('scene.cull_occluded_mesh(', 'scene.cull_unseen_mesh(', 'scene.clean_mesh('))
    assert text.index('if args.occlusion') < occluded < unseen < clean
