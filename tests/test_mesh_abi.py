"""Surface nets on a dense lattice (include/perf_hip_mesh.h, perf_amd/mesh.py) checked without a GPU: the header's constants and parameter
types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal happens before a launch
with a message that names its reason (the fake pointers are never dereferenced); the workspace has the documented size; write_ply's files
read back."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
F3 = ctypes.c_float * 3


def _count(**kw):
    a = {'field': FAKE, 'nx': 4, 'ny': 5, 'nz': 6, 'thr': 0.5, 'ws': FAKE, 'ws_bytes': 1 << 40, 'counts': FAKE}
    a.update(kw)
    return _call('perf_mesh_count', a['field'], a['nx'], a['ny'], a['nz'], a['thr'], a['ws'], a['ws_bytes'], a['counts'], None)


def _write(**kw):
    a = {'field': FAKE, 'nx': 4, 'ny': 5, 'nz': 6, 'thr': 0.5, 'lo': F3(-1, -1, -1), 'hi': F3(1, 1, 1), 'ws': FAKE, 'ws_bytes': 1 << 40,
         'vertices': FAKE, 'vcap': 10, 'faces': FAKE, 'fcap': 10}
    a.update(kw)
    return _call('perf_mesh_write', a['field'], a['nx'], a['ny'], a['nz'], a['thr'], a['lo'], a['hi'], a['ws'], a['ws_bytes'], a['vertices'], a['vcap'],
                 a['faces'], a['fcap'], None)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [mesh] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, _ = abi_units.header('mesh')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_MESH_ABI_VERSION') == _lib.MESH_ABI_VERSION == 1
    assert list(inspect.signature(abi_units.abi_digest().digest).parameters) == ['path', 'macro']
    assert const('PERF_MESH_MAX_CELLS') == _lib.MESH_MAX_CELLS == 1 << 30


def test_refuses_null_pointers():
    for kw in ({'field': None},):
        rc, msg = _count(**kw)
        assert rc == PERF_E_INVALID and 'NULL input' in msg, (kw, msg)
    rc, msg = _count(counts=None)
    assert rc == PERF_E_INVALID and 'NULL output' in msg, msg
    for kw in ({'field': None}, {'lo': None}, {'hi': None}):
        rc, msg = _write(**kw)
        assert rc == PERF_E_INVALID and 'NULL input' in msg, (kw, msg)
    for kw in ({'vertices': None}, {'faces': None}):
        rc, msg = _write(**kw)
        assert rc == PERF_E_INVALID and 'NULL output' in msg, (kw, msg)
    for kw in ({'vcap': -1}, {'fcap': -1}):
        rc, msg = _write(**kw)
        assert rc == PERF_E_INVALID and 'negative capacity' in msg, (kw, msg)
    for call in (_count, _write):
        rc, msg = call(ws=None)
        assert rc == PERF_E_INVALID and 'NULL workspace' in msg, msg


def test_refuses_dimensions_threshold_and_box():
    from perf_amd import _lib
    lib = _lib.load()
    for call in (_count, _write):
        for kw in ({'nx': 0}, {'ny': 0}, {'nz': 0}, {'nx': -3}):
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'dimension below 1' in msg, (kw, msg)
        for kw in ({'nx': 1025, 'ny': 1024, 'nz': 1024}, {'nx': 1 << 20, 'ny': 1 << 20, 'nz': 1}, {'nx': 1 << 30, 'ny': 1, 'nz': 2}):
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and '2^30' in msg, (kw, msg)
        for thr in (float('nan'), float('inf'), -float('inf')):
            rc, msg = call(thr=thr)
            assert rc == PERF_E_INVALID and 'not finite' in msg, (thr, msg)
    assert lib.perf_mesh_workspace_bytes(0, 4, 4) == -1 and lib.perf_mesh_workspace_bytes(1025, 1024, 1024) == -1
    assert lib.perf_mesh_workspace_bytes(1024, 1024, 1024) > 0
    for lo, hi in ((F3(-1, -1, -1), F3(1, -1, 1)), (F3(0, 0, 2), F3(1, 1, 1)), (F3(0, 0, 0), F3(1, float('nan'), 1)), (F3(0, 0, 0), F3(float('inf'), 1, 1))):
        rc, msg = _write(lo=lo, hi=hi)
        assert rc == PERF_E_INVALID and 'hi > lo' in msg, (list(lo), list(hi), msg)


def _words(nx, ny, nz):
    """The documented layout: masks and ranks of the chunks, the scan's levels of 256, two totals."""
    chunks = nx * ny * -(-nz // 64)
    words, n = 2 * chunks + 2, chunks
    while True:
        n = -(-n // 256)
        words += n
        if n == 1:
            return words


def test_refuses_a_bad_workspace_and_sizes_it_as_documented():
    from perf_amd import _lib
    lib = _lib.load()
    for shape in ((1, 1, 1), (4, 5, 6), (3, 3, 64), (3, 3, 65), (70, 70, 70), (160, 160, 160), (1024, 1024, 1024), (1 << 15, 1 << 15, 1)):
        need = lib.perf_mesh_workspace_bytes(*shape)
        assert need == 8 * (_words(*shape) + _words(*shape) % 2) and need % 16 == 0, shape           # (rounded up to 16 bytes)
    assert lib.perf_mesh_workspace_bytes(1024, 1024, 1024) < 0.26 * 1024 ** 3           # a quarter of a byte per cell
    need = lib.perf_mesh_workspace_bytes(4, 5, 6)
    for call in (_count, _write):
        rc, msg = call(ws_bytes=need - 8)
        assert rc == PERF_E_INVALID and 'workspace' in msg and 'bytes' in msg, msg
        rc, msg = call(ws=ctypes.c_void_p(72))
        assert rc == PERF_E_INVALID and '16-byte aligned' in msg, msg


def test_python_surface():
    import torch
    import perf_amd
    from perf_amd import mesh, ops, scene
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert mesh.Mesh._fields == ('vertices', 'faces', 'colors', 'normals') and mesh.Mesh(1, 2) == (1, 2, None, None)
    assert params(mesh.surface_nets) == [('field', E), ('thr', E), ('lo', E), ('hi', E)]
    assert params(mesh.density_lattice) == [('scene', E), ('resolution', E), ('use_occupancy', True), ('chunk', 1 << 22)]
    assert params(mesh.extract_mesh) == [('scene', E), ('resolution', 256), ('threshold', None), ('use_occupancy', True), ('colors', False), ('normals', False)]
    assert [k for k, _ in params(scene.NeRFScene.extract_mesh)] == ['self', 'kw']
    assert [k for k, _ in params(ops.mesh_count)] == ['field', 'thr', 'ws'] and [k for k, _ in params(ops.mesh_write)] == ['field', 'thr', 'lo', 'hi', 'ws', 'n_vertices', 'n_faces']
    with pytest.raises(perf_amd._lib.PerfError):           # no fallback: a CPU tensor is refused
        mesh.surface_nets(torch.zeros(3, 3, 3), 0.5, [0, 0, 0], [1, 1, 1])
    with pytest.raises(perf_amd._lib.PerfError):           # a lattice has a cell on every axis
        ops.mesh_count(torch.zeros(3, 1, 3), 0.5)


def _read_ply(path):
    """A reader for what write_ply writes: -> {property: array} of the vertices, faces [F, 3]."""
    raw = open(path, 'rb').read()
    head, body = raw[:raw.index(b'end_header\n')].decode('ascii').split('\n'), raw[raw.index(b'end_header\n') + 11:]
    assert head[0] == 'ply' and head[1] == 'format binary_little_endian 1.0'
    counts, props, element = {}, {}, None
    for line in head[2:]:
        w = line.split()
        if w and w[0] == 'element':
            element = w[1]; counts[element] = int(w[2]); props[element] = []
        elif w and w[0] == 'property':
            props[element].append(w[1:])
    types = {'float': '<f4', 'uchar': 'u1', 'int': '<i4'}
    vdt = np.dtype([(p[1], types[p[0]]) for p in props['vertex']])
    verts = np.frombuffer(body, dtype=vdt, count=counts['vertex'])
    assert props['face'] == [['list', 'uchar', 'int', 'vertex_indices']]
    fdt = np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
    faces = np.frombuffer(body, dtype=fdt, count=counts['face'], offset=vdt.itemsize * counts['vertex'])
    assert len(body) == vdt.itemsize * counts['vertex'] + fdt.itemsize * counts['face'] and (faces['n'] == 3).all()
    return verts, faces['i']


@pytest.mark.parametrize('with_normals,with_colors', [(False, False), (True, True), (False, True)])
def test_write_ply_round_trips(tmp_path, with_normals, with_colors):
    import torch
    from perf_amd.mesh import Mesh, write_ply
    g = torch.Generator().manual_seed(3)
    v = torch.randn(17, 3, generator=g)
    f = torch.randint(0, 17, (29, 3), generator=g, dtype=torch.int32)
    n = torch.nn.functional.normalize(torch.randn(17, 3, generator=g), dim=1) if with_normals else None
    c = torch.randint(0, 256, (17, 3), generator=g).float() / 255.0 if with_colors else None
    path = str(tmp_path / 'm.ply')
    write_ply(path, Mesh(v, f, c, n))
    verts, faces = _read_ply(path)
    names = ['x', 'y', 'z'] + (['nx', 'ny', 'nz'] if with_normals else []) + (['red', 'green', 'blue'] if with_colors else [])
    assert list(verts.dtype.names) == names
    assert np.array_equal(np.stack([verts[k] for k in 'xyz'], 1), v.numpy()) and np.array_equal(faces, f.numpy())
    if with_normals:
        assert np.array_equal(np.stack([verts[k] for k in ('nx', 'ny', 'nz')], 1), n.numpy())
    if with_colors:
        assert np.array_equal(np.stack([verts[k] for k in ('red', 'green', 'blue')], 1), np.rint(c.numpy() * 255).astype(np.uint8))
    write_ply(path, Mesh(v[:0], f[:0]))                     # an empty mesh is a valid file
    verts, faces = _read_ply(path)
    assert len(verts) == 0 and faces.shape == (0, 3)
