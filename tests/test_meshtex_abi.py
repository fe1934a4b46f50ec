"""The texture atlas (include/perf_hip_meshtex.h, perf_amd/mesh.py) checked without a GPU: the header's constants and parameter types are the
binding's (that header, binding, record and library agree is tests/test_abi_units.py's); the code lives where the build and the other units'
tests need it; every refusal happens before a launch with a message that names its reason (the fake pointers are never dereferenced); the
Python surface has the documented signatures and refuses CPU tensors; the extraction tool bakes after the simplification."""
import ctypes
import inspect
import os
import re

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
NAMES = ['perf_meshtex_bake', 'perf_meshtex_points', 'perf_meshtex_uv', 'perf_meshtex_version']
ARITY = {'perf_meshtex_version': 0, 'perf_meshtex_uv': 5, 'perf_meshtex_points': 13, 'perf_meshtex_bake': 23}


def _uv(**kw):
    a = {'F': 10, 'S': 64, 'T': 8, 'uv': FAKE}
    a.update(kw)
    return _call('perf_meshtex_uv', a['F'], a['S'], a['T'], a['uv'], None)


def _points(**kw):
    a = {'vertices': FAKE, 'V': 8, 'normals': None, 'faces': FAKE, 'F': 10, 'S': 64, 'T': 8, 'points': FAKE, 'point_normals': FAKE, 'face_of': FAKE, 'coverage': FAKE,
         'flag': FAKE}
    a.update(kw)
    return _call('perf_meshtex_points', a['vertices'], a['V'], a['normals'], a['faces'], a['F'], a['S'], a['T'], a['points'], a['point_normals'], a['face_of'],
                 a['coverage'], a['flag'], None)


def _bake(**kw):
    a = {'vertices': FAKE, 'V': 8, 'normals': None, 'faces': FAKE, 'F': 10, 'S': 64, 'T': 8, 'views': FAKE, 'maps': FAKE, 'sizes': (16, 32, 7, 5), 'K': 2, 'tol': 1 / 256,
         'facing': 1, 'power': 2, 'select': 0, 'fallback': None, 'fill': (0.5, 0.5, 0.5), 'image': FAKE, 'weight': FAKE, 'used': FAKE, 'coverage': FAKE, 'flag': FAKE}
    a.update(kw)
    sizes = (ctypes.c_int32 * len(a['sizes']))(*a['sizes']) if a['sizes'] is not None else None
    fill = (ctypes.c_float * 3)(*a['fill']) if a['fill'] is not None else None
    return _call('perf_meshtex_bake', a['vertices'], a['V'], a['normals'], a['faces'], a['F'], a['S'], a['T'], a['views'], a['maps'], sizes, a['K'], a['tol'], a['facing'],
                 a['power'], a['select'], a['fallback'], fill, a['image'], a['weight'], a['used'], a['coverage'], a['flag'], None)


ALL = (_uv, _points, _bake)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [meshtex] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, plain = abi_units.header('meshtex')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_MESHTEX_ABI_VERSION') == _lib.MESHTEX_ABI_VERSION == 1
    assert const('PERF_MESHTEX_MIN_SIZE') == _lib.MESHTEX_MIN_SIZE == 64 and const('PERF_MESHTEX_MAX_SIZE') == _lib.MESHTEX_MAX_SIZE == 16384
    assert const('PERF_MESHTEX_MIN_TILE') == _lib.MESHTEX_MIN_TILE == 4
    assert const('PERF_MESHTEX_MAX_VIEWS') == _lib.MESHTEX_MAX_VIEWS == _lib.MESHCOLOR_MAX_VIEWS == 64
    assert const('PERF_MESHTEX_MAX_VERTICES') == _lib.MESHTEX_MAX_VERTICES == 1 << 30
    assert const('PERF_MESHTEX_MAX_POWER') == _lib.MESHTEX_MAX_POWER == _lib.MESHCOLOR_MAX_POWER == 8
    assert {k: const('PERF_MESHTEX_COVER_' + k.upper()) for k in ('none', 'inside', 'gutter')} == _lib.MESHTEX_COVER
    # the header stands alone: the views are a const void*, said in words to be the cull's array
    assert '#include "perf_hip_' not in header and 'typedef struct' not in header and 'const void* views_dev' in header
    assert {name: len(args) for name, (_, args) in _lib._SIGS_MESHTEX.items()} == ARITY
    for name in NAMES[:3]:
        params = abi_units.params(plain, name)
        assert 'int64_t n_faces' in params and 'int32_t size' in params and 'int32_t tile' in params and 'void* stream' in params, name


def test_the_header_states_the_rule_and_what_it_does_not_do():
    comment = re.search(r'/\*.*?\*/', open(os.path.join(ROOT, 'include', 'perf_hip_meshtex.h')).read(), re.S).group(0)
    comment = re.sub(r'\s*\n \*\s*', ' ', comment)
    for phrase in ('64 <= S <= 16384', '4 <= T <= S', 'n = S / T tiles fit per row', 't = f >> 1 as half h = f & 1', '(X0, Y0) = ((t % n) T, (t / n) T)',
                   'Capacity is 2 n^2 faces', 'm = T - 3', 'a (X0, Y0),  b (X0 + m, Y0),  c (X0, Y0 + m)', 'rotated 180 degrees about the tile centre',
                   'a (X0 + T - 1, Y0 + T - 1),  b (X0 + T - 1 - m, Y0 + T - 1),  c (X0 + T - 1, Y0 + T - 1 - m)', 'u = (i + 0.5) / S, v = (j + 0.5) / S in fp32',
                   'a corner sits on a texel centre', 'element j S + i', 'h = (i + j >= T)', '(li, lj) = (T - 1 - i, T - 1 - j)',
                   'Half 0 therefore owns li + lj <= m + 2 and half 1 owns li + lj <= m + 1', 'exactly one owner', '1 li + lj <= m, inside the triangle', '2 gutter',
                   'beta = li / m, gamma = lj / m in DOUBLE', 'alpha = (1 - beta) - gamma', 'EXTRAPOLATED, NOT CLAMPED', 'alpha can be negative there',
                   'P = (a + beta (b - a)) + gamma (c - a)', 'rounded to fp32 once', 'm + 1 uniformly spaced samples',
                   'n = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)', 'len = sqrt((nx nx + ny ny) + nz nz)', 'exactly 0 where len == 0',
                   '(alpha Na + beta Nb) + gamma Nc', 'NOT normalised', 'point 0, normal 0, face_of = -1, coverage 0', 'one 64-bit integer atomicMin per such face',
                   'STAGE B OF perf_hip_meshcolor.h, UNCHANGED', 'bit for bit the colors, weight and used_bits perf_meshcolor_blend gives',
                   '(alpha Ca + beta Cb) + gamma Cc', 'fill, weight 0, bits 0, coverage 0', 'runs are bit-identical', 'an 8 x 8 block of texels',
                   'no area-proportional charts, no chart merging', 'no mip-safe padding between tiles', 'no exposure matching between views',
                   'more than 64 views are refused', 'S outside 64 .. 16384', 'T below 4 or above S', 'F above 2 n^2', 'not 8-byte aligned'):
        assert phrase in comment, phrase


def test_the_code_lives_where_the_older_abi_tests_need_it():
    from perf_amd import build
    includes = lambda name: build._includes(os.path.join(build.CSRC, name))
    reaches = lambda name, header: any(p.endswith(os.sep + header) for p in includes(name))
    assert 'meshtex.hip' in build.SOURCES and 'meshtex_device.hpp' in build.HEADERS and len(set(build.SOURCES)) == len(build.SOURCES)
    assert os.path.join(ROOT, 'include', 'perf_hip_meshtex.h') in abi_units.build_deps()
    users = sorted(s for s in build.SOURCES if reaches(s, 'perf_hip_meshtex.h'))
    assert users == ['meshcolor.hip', 'meshtex.hip'], users
    assert sorted(s for s in build.SOURCES if reaches(s, 'meshtex_device.hpp')) == ['meshcolor.hip', 'meshtex.hip']
    # the unit of the layout names no view: it reaches neither the cull's header nor the colouring's, directly or through a device header
    for header in ('perf_hip_meshvis.h', 'perf_hip_meshcolor.h', 'pano_lookup_device.hpp'):
        assert not reaches('meshtex.hip', header), header
    assert [s for s in build.SOURCES if reaches(s, 'perf_hip_meshvis.h')] == ['meshvis.hip', 'meshcolor.hip']
    assert [s for s in build.SOURCES if reaches(s, 'perf_hip_meshcolor.h')] == ['meshcolor.hip']
    unit, color, device = (open(os.path.join(build.CSRC, n)).read() for n in ('meshtex.hip', 'meshcolor.hip', 'meshtex_device.hpp'))
    for name in ('perf_meshtex_version', 'perf_meshtex_uv', 'perf_meshtex_points'):
        assert re.search(r'extern "C" \w+ ' + name + r'\(', unit) and not re.search(r'extern "C" \w+ ' + name + r'\(', color), name
    assert re.search(r'extern "C" int perf_meshtex_bake\(', color) and 'perf_meshtex_bake' not in unit
    # the rule is stated once, in the device header; both kernels of the blend's unit call one per-point function
    for name in ('tex_owner', 'tex_bary', 'tex_point', 'tex_rows', 'tex_flat_normal', 'tex_layout_check'):
        assert len(re.findall(r'\b' + name + r'\(', device)) >= 1 and name + '(' not in unit.split('namespace perf {')[0], name
    assert 'tex_owner(' in unit and 'tex_owner(' in color and 'li / m' not in unit and 'li / m' not in color
    assert len(re.findall(r'\bcol_blend_point\(', color)) == 3          # the definition and the two kernels' calls
    assert color.count('for (int k = 0; k < n_views; ++k) {') == 1          # one loop over the views
    assert unit.count('#pragma clang fp contract(off)') >= 2 and device.count('#pragma clang fp contract(off)') >= 4
    for text_ in (unit, device):
        assert not re.search(r'atomic\w*\s*\(\s*\(?\s*(float|double)', text_)          # no floating-point atomics
        for name in ('asinf(', 'atan2f(', 'fmaf(', 'fma(', '__fma', 'unsafeAtomicAdd'):
            assert name not in text_, name


def test_refuses_null_pointers():
    for call, kws in ((_points, ({'vertices': None}, {'faces': None})), (_bake, ({'vertices': None}, {'faces': None}, {'views': None}, {'maps': None}, {'sizes': None}, {'fill': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_uv, ({'uv': None},)), (_points, ({'points': None}, {'point_normals': None}, {'face_of': None}, {'coverage': None}, {'flag': None})),
                      (_bake, ({'image': None}, {'weight': None}, {'used': None}, {'coverage': None}, {'flag': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL output' in msg, (call.__name__, kw, msg)
    for kw in ({'views': ctypes.c_void_p(68)}, {'maps': ctypes.c_void_p(68)}):
        rc, msg = _bake(**kw)
        assert rc == PERF_E_INVALID and '8-byte aligned' in msg, msg


def test_refuses_the_layout_before_anything_else():
    for call in ALL:
        for f, s, t in ((129, 64, 8), (513, 64, 4), (3, 64, 64), (2 * 4096 * 4096 + 1, 16384, 4)):
            rc, msg = call(F=f, S=s, T=t)
            assert rc == PERF_E_INVALID and f'{f} faces are more than the' in msg and '2 n^2' in msg, (call.__name__, msg)
        rc, msg = call(F=-1)
        assert rc == PERF_E_INVALID and 'negative number of faces' in msg, (call.__name__, msg)
        for bad in (3, 0, -8):
            rc, msg = call(T=bad)
            assert rc == PERF_E_INVALID and 'is below 4' in msg, (call.__name__, msg)
        rc, msg = call(T=65)
        assert rc == PERF_E_INVALID and 'larger than the atlas' in msg, (call.__name__, msg)
        for bad in (63, 0, -64, 16385, 1 << 20):
            rc, msg = call(S=bad)
            assert rc == PERF_E_INVALID and 'outside 64 .. 16384' in msg, (call.__name__, bad, msg)


def test_refuses_counts_and_parameters():
    for call in (_points, _bake):
        rc, msg = call(V=-1)
        assert rc == PERF_E_INVALID and 'negative number of vertices' in msg, (call.__name__, msg)
        rc, msg = call(V=(1 << 30) + 1)
        assert rc == PERF_E_INVALID and '2^30' in msg, (call.__name__, msg)
    rc, msg = _bake(K=-1)
    assert rc == PERF_E_INVALID and 'negative number of views' in msg, msg
    rc, msg = _bake(K=65, sizes=(4, 4) * 65)
    assert rc == PERF_E_INVALID and '65 views are more than 64' in msg, msg
    for bad in ((0, 32, 7, 5), (16, 32, 7, -1)):
        rc, msg = _bake(sizes=bad)
        assert rc == PERF_E_INVALID and 'a map dimension below 1' in msg, msg
    for bad in (-1 / 256, float('inf'), float('nan'), -float('inf')):
        rc, msg = _bake(tol=bad)
        assert rc == PERF_E_INVALID and 'tol' in msg and 'negative or not finite' in msg, (bad, msg)
    for bad in (0, 9, -1):
        rc, msg = _bake(power=bad)
        assert rc == PERF_E_INVALID and 'power' in msg and 'outside 1 .. 8' in msg, msg
    for bad in (-1, 2):
        rc, msg = _bake(select=bad)
        assert rc == PERF_E_INVALID and 'neither blend (0) nor best (1)' in msg, msg
    for bad in (-1, 2):
        rc, msg = _bake(facing=bad)
        assert rc == PERF_E_INVALID and 'facing' in msg and 'is 0 or 1' in msg, msg
    # power is read only with facing: without it, it is no reason (the refusal that remains is the one asked for)
    rc, msg = _bake(facing=0, power=0, select=7)
    assert rc == PERF_E_INVALID and 'neither blend (0) nor best (1)' in msg, msg


def test_python_surface():
    import torch
    import perf_amd
    from perf_amd import mesh, ops, scene
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    names = lambda f: [k for k, _ in params(f)]
    E = inspect.Parameter.empty
    assert mesh.Atlas._fields == ('size', 'tile', 'uv', 'image', 'coverage', 'weight', 'used')
    assert params(mesh.atlas_layout) == [('n_faces', E), ('size', None), ('tile', None)]
    assert names(mesh.atlas_uv)[:3] == ['n_faces', 'size', 'tile']
    assert params(mesh.atlas_points) == [('mesh', E), ('size', E), ('tile', E), ('normals', 'flat')]
    assert params(mesh.bake_panorama_texture) == [('mesh', E), ('views', E), ('size', None), ('tile', None), ('normals', 'flat'), ('kw', E)]
    assert params(mesh.bake_field_texture)[:4] == [('scene', E), ('mesh', E), ('size', None), ('tile', None)]
    assert names(mesh.sample_atlas) == ['atlas', 'face_ids', 'bary'] and names(mesh.write_obj) == ['path', 'mesh', 'atlas']
    assert params(scene.NeRFScene.bake_mesh_texture) == [('self', E), ('mesh', E), ('sup_pool', None), ('kw', E)]
    assert names(ops.meshtex_uv)[:3] == ['n_faces', 'size', 'tile']
    assert names(ops.meshtex_points) == ['vertices', 'faces', 'size', 'tile', 'normals', 'flag']
    assert names(ops.meshtex_bake) == ['vertices', 'faces', 'size', 'tile', 'views', 'sizes', 'map_pointers', 'tol', 'normals', 'facing', 'power', 'select', 'fallback',
                                       'fill', 'flag']
    # no fallback: CPU tensors are refused
    vertices, faces = torch.rand(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    cpu = mesh.Mesh(vertices, faces)
    view = {'pose': torch.eye(4), 'distance_map': torch.ones(4, 8), 'color_map': torch.ones(4, 8, 3)}
    for call in (lambda: mesh.atlas_points(cpu, 64, 8), lambda: mesh.bake_panorama_texture(cpu, [view]), lambda: mesh.bake_field_texture(None, cpu),
                 lambda: mesh.atlas_uv(1, 64, 8, device='cpu'), lambda: ops.meshtex_points(vertices, faces, 64, 8),
                 lambda: ops.meshtex_bake(vertices, faces, 64, 8, torch.zeros(0, 16, dtype=torch.int32), [], torch.zeros(0, dtype=torch.int64), 1 / 256)):
        with pytest.raises(perf_amd._lib.PerfError):
            call()
    # and what does not fit is refused in Python before the library is asked
    for call in (lambda: ops.meshtex_uv(129, 64, 8), lambda: ops.meshtex_uv(1, 32, 8), lambda: ops.meshtex_uv(1, 64, 3)):
        with pytest.raises(perf_amd._lib.PerfError):
            call()


def test_extract_mesh_tool_bakes_after_the_simplification():
    text = open(os.path.join(ROOT, 'tools', 'extract_mesh.py')).read()
    options = ["'--texture'", "'--texture-source'", "'--texture-tile'"]
    for option in options:
        assert option in text, option
    assert text.index("'--color-power'") < text.index(options[0]) < text.index(options[1]) < text.index(options[2])
    assert "choices=['panoramas', 'field']" in text
    simplify, bake, obj = (text.index(c) for c in ('scene.simplify_mesh(', 'scene.bake_mesh_texture(', 'write_obj(args.out'))
    assert simplify < bake < obj and "+ '.obj'" in text
