"""Surface nets on the live bricks of a lattice (include/perf_hip_brickmesh.h, perf_amd/mesh.py) checked without a GPU: the header's constants
and parameter types are the binding's (that header, binding, record and library agree is tests/test_abi_units.py's); every refusal happens
before a launch with a message that names its reason (the fake pointers are never dereferenced); the workspace has the documented size; the
Python surface has the documented signatures and refuses CPU tensors."""
import ctypes
import inspect

import pytest

from tests import abi_units
from tests.abi_units import PERF_E_INVALID, refused as _call

FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
F3 = ctypes.c_float * 3
BIG = 1 << 40


def _select(**kw):
    a = {'binaries': FAKE, 'occ_res': 16, 'nx': 8, 'ny': 16, 'nz': 24, 'table': FAKE, 'n_live': FAKE, 'ws': FAKE, 'ws_bytes': BIG}
    a.update(kw)
    return _call('perf_brickmesh_select', a['binaries'], a['occ_res'], a['nx'], a['ny'], a['nz'], a['table'], a['n_live'], a['ws'], a['ws_bytes'], None)


def _list(**kw):
    a = {'table': FAKE, 'nx': 8, 'ny': 16, 'nz': 24, 'ids': FAKE, 'n_bricks': 3}
    a.update(kw)
    return _call('perf_brickmesh_list', a['table'], a['nx'], a['ny'], a['nz'], a['ids'], a['n_bricks'], None)


def _corners(**kw):
    a = {'ids': FAKE, 'n_bricks': 3, 'first': 0, 'm': 3, 'nx': 8, 'ny': 16, 'nz': 24, 'binaries': FAKE, 'occ_res': 16, 'x01': FAKE, 'sel': FAKE, 'interior': FAKE}
    a.update(kw)
    return _call('perf_brickmesh_corners', a['ids'], a['n_bricks'], a['first'], a['m'], a['nx'], a['ny'], a['nz'], a['binaries'], a['occ_res'], a['x01'], a['sel'],
                 a['interior'], None)


def _count(**kw):
    a = {'values': FAKE, 'ids': FAKE, 'table': FAKE, 'n_bricks': 3, 'nx': 8, 'ny': 16, 'nz': 24, 'thr': 0.5, 'fill': 0.0, 'ws': FAKE, 'ws_bytes': BIG, 'counts': FAKE}
    a.update(kw)
    return _call('perf_brickmesh_count', a['values'], a['ids'], a['table'], a['n_bricks'], a['nx'], a['ny'], a['nz'], a['thr'], a['fill'], a['ws'], a['ws_bytes'],
                 a['counts'], None)


def _write(**kw):
    a = {'values': FAKE, 'ids': FAKE, 'table': FAKE, 'n_bricks': 3, 'nx': 8, 'ny': 16, 'nz': 24, 'thr': 0.5, 'fill': 0.0, 'lo': F3(-1, -1, -1), 'hi': F3(1, 1, 1), 'ws': FAKE,
         'ws_bytes': BIG, 'vertices': FAKE, 'vcap': 10, 'faces': FAKE, 'fcap': 10, 'cells': FAKE}
    a.update(kw)
    return _call('perf_brickmesh_write', a['values'], a['ids'], a['table'], a['n_bricks'], a['nx'], a['ny'], a['nz'], a['thr'], a['fill'], a['lo'], a['hi'], a['ws'],
                 a['ws_bytes'], a['vertices'], a['vcap'], a['faces'], a['fcap'], a['cells'], None)


ALL = (_select, _list, _corners, _count, _write)
WITH_BRICKS = (_list, _corners, _count, _write)


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [brickmesh] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, _ = abi_units.header('brickmesh')
    const = lambda name: abi_units.const(header, name)
    assert const('PERF_BRICKMESH_ABI_VERSION') == _lib.BRICKMESH_ABI_VERSION == 1
    assert list(inspect.signature(abi_units.abi_digest().digest).parameters) == ['path', 'macro']
    assert const('PERF_BRICKMESH_EDGE') == _lib.BRICKMESH_EDGE == 8
    assert const('PERF_BRICKMESH_MAX_DIM') == _lib.BRICKMESH_MAX_DIM == 4096
    assert const('PERF_BRICKMESH_MAX_BRICKS') == _lib.BRICKMESH_MAX_BRICKS == 1 << 21


def test_refuses_null_pointers():
    for call, kws in ((_select, ({'binaries': None},)), (_list, ({'table': None},)), (_corners, ({'ids': None}, {'binaries': None})),
                      (_count, ({'values': None}, {'ids': None}, {'table': None})), (_write, ({'values': None}, {'ids': None}, {'table': None}, {'lo': None}, {'hi': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL input' in msg, (call.__name__, kw, msg)
    for call, kws in ((_select, ({'table': None}, {'n_live': None})), (_list, ({'ids': None},)), (_corners, ({'x01': None}, {'sel': None})), (_count, ({'counts': None},)),
                      (_write, ({'vertices': None}, {'faces': None}))):
        for kw in kws:
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'NULL output' in msg, (call.__name__, kw, msg)
    for kw in ({'vcap': -1}, {'fcap': -1}):
        rc, msg = _write(**kw)
        assert rc == PERF_E_INVALID and 'negative capacity' in msg, (kw, msg)
    for call in (_select, _count, _write):
        rc, msg = call(ws=None)
        assert rc == PERF_E_INVALID and 'NULL workspace' in msg, msg


def test_refuses_dimensions_and_brick_counts():
    from perf_amd import _lib
    lib = _lib.load()
    for call in ALL:
        for kw in ({'nx': 0}, {'ny': 0}, {'nz': 0}, {'nx': -8}, {'nz': 7}):
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'dimension below 8' in msg, (call.__name__, kw, msg)
        for kw in ({'nx': 12}, {'ny': 17}, {'nz': 4100}, {'nx': 100}):
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'not a multiple of 8' in msg, (call.__name__, kw, msg)
        for kw in ({'nx': 4104}, {'ny': 8192}, {'nz': 1 << 30}):
            rc, msg = call(**kw)
            assert rc == PERF_E_INVALID and 'above 4096' in msg, (call.__name__, kw, msg)
    for call in WITH_BRICKS:
        rc, msg = call(n_bricks=-1)
        assert rc == PERF_E_INVALID and 'negative number of bricks' in msg, (call.__name__, msg)
        rc, msg = call(n_bricks=(1 << 21) + 1, nx=4096, ny=4096, nz=4096)
        assert rc == PERF_E_INVALID and '2^21' in msg, (call.__name__, msg)
        rc, msg = call(n_bricks=7)                              # (8, 16, 24) cells are 6 bricks
        assert rc == PERF_E_INVALID and 'the lattice has 6' in msg, (call.__name__, msg)
    for kw in ({'first': -1}, {'m': -1}, {'first': 2, 'm': 2}):
        rc, msg = _corners(**kw)
        assert rc == PERF_E_INVALID and 'not within' in msg, (kw, msg)
    for call in (_select, _corners):
        for res in (0, -4, 4097):
            rc, msg = call(occ_res=res)
            assert rc == PERF_E_INVALID and 'occupancy resolution' in msg, (call.__name__, res, msg)
    assert lib.perf_brickmesh_workspace_bytes(0, 8, 8, 0) == -1 and lib.perf_brickmesh_workspace_bytes(8, 8, 12, 0) == -1
    assert lib.perf_brickmesh_workspace_bytes(4104, 8, 8, 0) == -1 and lib.perf_brickmesh_workspace_bytes(8, 8, 8, 2) == -1
    assert lib.perf_brickmesh_workspace_bytes(4096, 4096, 4096, (1 << 21) + 1) == -1 and lib.perf_brickmesh_workspace_bytes(4096, 4096, 4096, 1 << 21) > 0


def test_refuses_threshold_fill_and_box():
    for call in (_count, _write):
        for thr in (float('nan'), float('inf'), -float('inf')):
            rc, msg = call(thr=thr)
            assert rc == PERF_E_INVALID and 'threshold is not finite' in msg, (thr, msg)
        for fill in (float('nan'), float('inf'), -float('inf')):
            rc, msg = call(fill=fill)
            assert rc == PERF_E_INVALID and 'fill value is not finite' in msg, (fill, msg)
        for thr, fill in ((0.5, 0.5), (0.5, 0.75), (-1.0, 0.0)):
            rc, msg = call(thr=thr, fill=fill)
            assert rc == PERF_E_INVALID and 'below the threshold' in msg, (thr, fill, msg)
    for lo, hi in ((F3(-1, -1, -1), F3(1, -1, 1)), (F3(0, 0, 2), F3(1, 1, 1)), (F3(0, 0, 0), F3(1, float('nan'), 1)), (F3(0, 0, 0), F3(float('inf'), 1, 1))):
        rc, msg = _write(lo=lo, hi=hi)
        assert rc == PERF_E_INVALID and 'hi > lo' in msg, (list(lo), list(hi), msg)


def _words(nx, ny, nz, m):
    groups = -(-(nx // 8) * (ny // 8) * (nz // 8) // 256)
    select = groups + abi_units.levels(groups)
    count = 3 * 8 * m + 2 * abi_units.levels(8 * m) + 4 if m else 4
    return max(select, count)


def test_refuses_a_bad_workspace_and_sizes_it_as_documented():
    from perf_amd import _lib
    lib = _lib.load()
    for shape, m in (((8, 8, 8), 0), ((8, 8, 8), 1), ((8, 16, 24), 6), ((48, 48, 48), 100), ((256, 256, 256), 32), ((256, 256, 256), 33), ((256, 256, 256), 32768),
                     ((1024, 1024, 1024), 0), ((1024, 1024, 1024), 8193), ((2048, 2048, 2048), 1 << 20), ((4096, 4096, 4096), 0), ((4096, 4096, 4096), 1 << 21), ((4096, 8, 8), 5)):
        need = lib.perf_brickmesh_workspace_bytes(*shape, m)
        assert need == 8 * (_words(*shape, m) + _words(*shape, m) % 2) and need % 16 == 0, (shape, m)           # (rounded up to 16 bytes)
    assert lib.perf_brickmesh_workspace_bytes(4096, 4096, 4096, 1 << 21) < 0.38 * 512 * (1 << 21)          # 0.375 bytes per cell of a live brick, and the levels
    for call, m in ((_select, 0), (_count, 3), (_write, 3)):
        need = lib.perf_brickmesh_workspace_bytes(8, 16, 24, m)
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
    assert params(mesh.select_bricks) == [('binaries', E), ('n', E)]
    assert params(mesh.density_bricks) == [('scene', E), ('n', E), ('chunk_bricks', 8192)]
    assert params(mesh.surface_nets_bricks) == [('values', E), ('ids', E), ('table', E), ('shape', E), ('thr', E), ('fill', E), ('lo', E), ('hi', E)]
    assert params(mesh.extract_mesh_sparse) == [('scene', E), ('resolution', 1024), ('threshold', None), ('colors', False), ('normals', False)]
    assert names(scene.NeRFScene.extract_mesh_sparse) == ['self', 'kw']
    assert names(ops.brickmesh_select) == ['binaries', 'shape', 'ws'] and names(ops.brickmesh_list) == ['table', 'n_bricks']
    assert names(ops.brickmesh_corners) == ['ids', 'first', 'm', 'shape', 'binaries']
    assert names(ops.brickmesh_count) == ['values', 'ids', 'table', 'shape', 'thr', 'fill', 'ws']
    assert names(ops.brickmesh_write) == ['values', 'ids', 'table', 'shape', 'thr', 'fill', 'lo', 'hi', 'ws', 'n_vertices', 'n_faces']
    values, ids, table = torch.zeros(1, 8, 8, 8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, 1, dtype=torch.int32)
    occ = torch.ones(16, 16, 16, dtype=torch.bool)
    with pytest.raises(perf_amd._lib.PerfError):           # no fallback: CPU tensors are refused
        mesh.surface_nets_bricks(values, ids, table, (8, 8, 8), 0.5, 0.0, [0, 0, 0], [1, 1, 1])
    with pytest.raises(perf_amd._lib.PerfError):
        mesh.select_bricks(occ, 8)
    with pytest.raises(perf_amd._lib.PerfError):
        ops.brickmesh_corners(ids, 0, 1, (8, 8, 8), occ)
    with pytest.raises(perf_amd._lib.PerfError):
        ops.brickmesh_list(table, 1)
    for bad in (12, 4104, 0, (8, 8), (8, 8, 9)):           # the lattice's shape is checked before anything else
        with pytest.raises(perf_amd._lib.PerfError):
            mesh.select_bricks(occ, bad)
