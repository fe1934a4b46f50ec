"""The colouring from the registered panoramas (include/perf_hip_meshcolor.h, perf_amd/mesh.py) checked without a GPU: the header's constants
and parameter types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal happens
before a launch with a message that names its reason (the fake pointers are never dereferenced); the Python surface has the documented
signatures and refuses CPU tensors; the extraction tool colours after the cleaning and before the simplification."""
import ctypes
import inspect
import os
import re

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch


def _sums(**kw):
    a = {'vertices': FAKE, 'V': 8, 'faces': FAKE, 'F': 10, 's': 36, 'acc': FAKE, 'flag': FAKE}
    a.update(kw)
    return _call('perf_meshcolor_normal_sums', a['vertices'], a['V'], a['faces'], a['F'], a['s'], a['acc'], a['flag'], None)


def _normals(**kw):
    a = {'acc': FAKE, 'V': 8, 'normals': FAKE}
    a.update(kw)
    return _call('perf_meshcolor_normals', a['acc'], a['V'], a['normals'], None)


def _blend(**kw):
    a = {'vertices': FAKE, 'normals': FAKE, 'V': 8, 'views': FAKE, 'maps': FAKE, 'sizes': (16, 32, 7, 5), 'K': 2, 'tol': 1 / 256, 'facing': 1, 'power': 2, 'select': 0,
         'fallback': None, 'fill': (0.5, 0.5, 0.5), 'colors': FAKE, 'weight': FAKE, 'used': FAKE, 'best': FAKE}
    a.update(kw)
    sizes = (ctypes.c_int32 * len(a['sizes']))(*a['sizes']) if a['sizes'] is not None else None
    fill = (ctypes.c_float * 3)(*a['fill']) if a['fill'] is not None else None
    return _call('perf_meshcolor_blend', a['vertices'], a['normals'], a['V'], a['views'], a['maps'], sizes, a['K'], a['tol'], a['facing'], a['power'], a['select'],
                 a['fallback'], fill, a['colors'], a['weight'], a['used'], a['best'], None)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [meshcolor] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, plain = abi_units.header('meshcolor')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_MESHCOLOR_ABI_VERSION') == _lib.MESHCOLOR_ABI_VERSION == 1
    assert const('PERF_MESHCOLOR_MAX_VIEWS') == _lib.MESHCOLOR_MAX_VIEWS == _lib.MESHVIS_MAX_VIEWS == 64
    assert const('PERF_MESHCOLOR_MAX_VERTICES') == _lib.MESHCOLOR_MAX_VERTICES == 1 << 30
    assert const('PERF_MESHCOLOR_MAX_FACES') == _lib.MESHCOLOR_MAX_FACES == (1 << 31) - 1
    assert const('PERF_MESHCOLOR_MAX_POWER') == _lib.MESHCOLOR_MAX_POWER == 8
    assert {k: const('PERF_MESHCOLOR_SELECT_' + k.upper()) for k in ('blend', 'best')} == _lib.MESHCOLOR_SELECT
    assert '#include "perf_hip_meshvis.h"' in header and 'typedef struct' not in header          # the view descriptor is the cull's, unchanged
    # vertex and face counts are 64-bit at the boundary
    params = abi_units.params(plain, 'perf_meshcolor_normal_sums')
    assert 'int64_t n_faces' in params and 'int64_t n_vertices' in params
    for name in ('perf_meshcolor_normals', 'perf_meshcolor_blend'):
        assert 'int64_t n_vertices' in abi_units.params(plain, name), name


def test_the_header_states_the_rule_and_what_it_does_not_do():
    comment = re.search(r'/\*.*?\*/', open(os.path.join(ROOT, 'include', 'perf_hip_meshcolor.h')).read(), re.S).group(0)
    comment = re.sub(r'\s*\n \*\s*', ' ', comment)
    for phrase in ('e1 = b - a, e2 = c - a', 'n  = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)', 'q_c = llrint(n_c * 2^s)', 'magnitude >= 2^62',
                   '64-bit integer atomicAdd', 'no floating-point atomics', 'bit-identical from run to run', 'wrap modulo 2^64', 'a valence of 2^23 faces',
                   's = 40 - ceil(log2(D^2))', 'len = sqrt((Ax Ax + Ay Ay) + Az Az)', 'normal_c = (float)(A_c / len)', 'exactly 0 where len == 0',
                   'RESTATED LINE FOR LINE', 'nw / ne / sw / se order', 'dist < proj + tol', 'dist > 0 and dist is finite', 'g = t_k - p',
                   's = (Nx gx + Ny gy) + Nz gz', 'cos = s / (sqrt((Nx Nx + Ny Ny) + Nz Nz) * sqrt((gx gx + gy gy) + gz gz))',
                   'w_k = cos^power / ((double)dist * (double)dist)', 'footprint on the surface grows as dist^2 / cos', 'num += w_k * (double)c_k, den += w_k',
                   '(float)(num / den)', 'weight = (float)den', 'ties go to the smaller k', 'best_view = -1', 'the fallback row if fallback is given, else fill',
                   'plain vector stores; no atomics', 'makes it index outside a map', "the reference's own grid_sample behaviour",
                   'no occlusion test against the mesh itself', 'no texture atlas, colours are per vertex', 'no exposure matching between views',
                   'no wrap at the seam', 'more than 64 views are refused', 'scale_log2 outside -200 .. 200'):
        assert phrase in comment, phrase


def test_the_unit_is_built_with_its_own_header():
    from perf_amd import build
    assert 'meshcolor.hip' in build.SOURCES and len(set(build.SOURCES)) == len(build.SOURCES)
    assert os.path.join(ROOT, 'include', 'perf_hip_meshcolor.h') in abi_units.build_deps()
    users = [s for s in build.SOURCES if any(p.endswith(os.sep + 'perf_hip_meshcolor.h') for p in build._includes(os.path.join(build.CSRC, s)))]
    assert users == ['meshcolor.hip'], users          # the units that include the header, by their #include lines, are the ones rebuilt for it
    unit = open(os.path.join(ROOT, 'perf_amd', 'csrc', 'meshcolor.hip')).read()
    assert '#include "../../include/perf_hip_meshcolor.h"' in unit
    # the panorama look-up is stated once: the three units that run it include the header, and no other file of csrc holds its asinf
    for name in ('visibility.hip', 'meshvis.hip', 'meshcolor.hip'):
        assert any(p.endswith(os.sep + 'pano_lookup_device.hpp') for p in build._includes(os.path.join(build.CSRC, name))), name
    holders = sorted(f for f in os.listdir(build.CSRC) if 'asinf(' in open(os.path.join(build.CSRC, f)).read())
    assert holders == ['pano_lookup_device.hpp'], holders
    assert unit.count('#pragma clang fp contract(off)') >= 3 and 'atomicAdd(acc' in unit
    assert not re.search(r'atomicAdd\s*\(\s*\(?\s*(float|double)', unit)          # no floating-point atomics


def test_refuses_null_pointers():
    for call, kws in ((_sums, ({'vertices': None}, {'faces': None})), (_normals, ({'acc': None},)),
                      (_blend, ({'vertices': None}, {'views': None}, {'maps': None}, {'sizes': None}, {'fill': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_sums, ({'acc': None}, {'flag': None})), (_normals, ({'normals': None},)),
                      (_blend, ({'colors': None}, {'weight': None}, {'used': None}, {'best': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL output' in msg, (call.__name__, kw, msg)
    rc, msg = _blend(normals=None)
    assert rc == PERF_E_INVALID and 'NULL input (normals) with facing' in msg, msg
    rc, msg = _blend(views=ctypes.c_void_p(68))
    assert rc == PERF_E_INVALID and '8-byte aligned' in msg, msg


def test_refuses_counts_and_parameters():
    for call in (_sums, _normals, _blend):
        rc, msg = call(V=-1)
        assert rc == PERF_E_INVALID and 'negative number of vertices' in msg, (call.__name__, msg)
        rc, msg = call(V=(1 << 30) + 1)
        assert rc == PERF_E_INVALID and '2^30' in msg, (call.__name__, msg)
    rc, msg = _sums(F=-1)
    assert rc == PERF_E_INVALID and 'negative number of faces' in msg, msg
    rc, msg = _sums(F=1 << 31)
    assert rc == PERF_E_INVALID and '2^31 - 1' in msg, msg
    for bad in (-201, 201, 1 << 20):
        rc, msg = _sums(s=bad)
        assert rc == PERF_E_INVALID and 'scale_log2' in msg and 'outside -200 .. 200' in msg, msg
    rc, msg = _blend(K=-1)
    assert rc == PERF_E_INVALID and 'negative number of views' in msg, msg
    rc, msg = _blend(K=65, sizes=(4, 4) * 65)
    assert rc == PERF_E_INVALID and '65 views are more than 64' in msg, msg
    for bad in ((0, 32, 7, 5), (16, 32, 7, -1)):
        rc, msg = _blend(sizes=bad)
        assert rc == PERF_E_INVALID and 'a map dimension below 1' in msg, msg
    for bad in (-1 / 256, float('inf'), float('nan'), -float('inf')):
        rc, msg = _blend(tol=bad)
        assert rc == PERF_E_INVALID and 'tol' in msg and 'negative or not finite' in msg, (bad, msg)
    for bad in (0, 9, -1):
        rc, msg = _blend(power=bad)
        assert rc == PERF_E_INVALID and 'power' in msg and 'outside 1 .. 8' in msg, msg
    for bad in (-1, 2):
        rc, msg = _blend(select=bad)
        assert rc == PERF_E_INVALID and 'neither blend (0) nor best (1)' in msg, msg
    # power is read only with facing, normals likewise: without it neither is a reason (the refusal that remains is the one asked for)
    rc, msg = _blend(facing=0, power=0, normals=None, select=7)
    assert rc == PERF_E_INVALID and 'neither blend (0) nor best (1)' in msg, msg


def test_python_surface():
    import torch
    import perf_amd
    from perf_amd import mesh, ops, scene
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    names = lambda f: [k for k, _ in params(f)]
    E = inspect.Parameter.empty
    assert mesh.PanoramaColors._fields == ('colors', 'weight', 'used', 'best_view')
    assert params(mesh.face_normals) == [('mesh', E), ('box', None)]
    assert params(mesh.panorama_colors) == [('vertices', E), ('views', E), ('normals', None), ('tol', 1 / 256), ('facing', True), ('power', 2), ('select', 'blend'),
                                            ('fallback', None), ('fill', (0.5, 0.5, 0.5))]
    assert params(mesh.color_from_panoramas) == [('mesh', E), ('views', E), ('normals', 'faces'), ('kw', E)]
    assert names(scene.NeRFScene.color_mesh_from_panoramas) == ['self', 'mesh', 'sup_pool', 'kw']
    assert names(ops.meshcolor_normal_sums) == ['vertices', 'faces', 'scale_log2', 'flag'] and names(ops.meshcolor_normals) == ['acc']
    assert names(ops.meshcolor_maps) == ['color_maps', 'sizes']
    assert names(ops.meshcolor_blend) == ['vertices', 'normals', 'views', 'sizes', 'map_pointers', 'tol', 'facing', 'power', 'select', 'fallback', 'fill']
    # the scale of the fixed point: 40 - ceil(log2(D^2)), 0 for a box of no extent
    assert mesh._normal_scale(((-1, -1, -1), (1, 1, 1))) == 36 and mesh._normal_scale(((0, 0, 0), (0, 0, 0))) == 0
    assert mesh._normal_scale(((0, 0, 0), (2, 0, 0))) == 38 and mesh._normal_scale(((0, 0, 0), (2.0001, 0, 0))) == 37
    # no fallback: CPU tensors are refused
    vertices, faces = torch.rand(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cpu = mesh.Mesh(vertices, faces)
    view = {'pose': torch.eye(4), 'distance_map': torch.ones(4, 8), 'color_map': torch.ones(4, 8, 3)}
    for call in (lambda: mesh.face_normals(cpu), lambda: mesh.face_normals(cpu, ((0, 0, 0), (1, 1, 1))), lambda: mesh.panorama_colors(vertices, [view], facing=False),
                 lambda: mesh.color_from_panoramas(cpu, [view]), lambda: ops.meshcolor_normal_sums(vertices, faces, 36),
                 lambda: ops.meshcolor_normals(torch.zeros(3, 3, dtype=torch.int64)), lambda: ops.meshcolor_maps([view['color_map']], [(4, 8)]),
                 lambda: ops.meshcolor_blend(vertices, None, torch.zeros(0, 16, dtype=torch.int32), [], torch.zeros(0, dtype=torch.int64), 1 / 256, facing=False)):
        with pytest.raises(perf_amd._lib.PerfError):
            call()


def test_extract_mesh_tool_colours_between_the_cleaning_and_the_simplification():
    text = open(os.path.join(ROOT, 'tools', 'extract_mesh.py')).read()
    options = ["'--colors-from-panoramas'", "'--color-select'", "'--color-power'"]
    for option in options:
        assert option in text, option
    assert text.index("'--simplify-dedupe'") < text.index(options[0]) < text.index(options[1]) < text.index(options[2])
    assert "choices=['blend', 'best']" in text
    cull, clean, colour, simplify = (text.index(c) for c in ('scene.cull_unseen_mesh(', 'scene.clean_mesh(', 'scene.color_mesh_from_panoramas(', 'scene.simplify_mesh('))
    assert cull < clean < colour < simplify < text.index('write_ply(args.out')
