"""Surface nets on the live bricks of a lattice (include/perf_hip_brickmesh.h, perf_amd/mesh.py) on the GPU.  The yardstick is the
float64 numpy restatement tests/mesh_reference.py run on the VIRTUAL field -- `fill` everywhere but at the stored corners --, with the
non-cubic box of tests/test_gpu_mesh.py: the device vertices sorted by their cells must be a permutation onto the restatement's linear
cell order, the faces relabelled through it and lexsorted must be EQUAL rows, the vertices within 1 ulp of max(|lo|, |hi|) of float64
(the dense test's bound and its reasoning: one fp32 rounding of a double-carried value) and BIT-EQUAL to the dense device unit run on
the same virtual field.  Then the selection against a numpy restatement of the box rule, and the scene path against the dense path.
With PERF_BRICKMESH_REPORT=<path> the figures of the 1024^3 extraction are also written there as JSON."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_reference as R

pytestmark = pytest.mark.gpu

LO, HI = [-1.0, -1.25, -0.5], [1.0, 0.75, 1.0]           # (the box of tests/test_gpu_mesh.py: the three axes scale differently)


def _ulp(m):
    return float(np.spacing(np.float32(m)))


# ---- numpy: brick sets and the virtual field ----------------------------------------------------------------------------------------------
def _closure(virtual, live, thr):
    """live plus the bricks of the eight cells around every corner of `virtual` that is >= thr."""
    shape = np.array(virtual.shape) - 1
    with np.errstate(invalid='ignore'):
        corners = np.stack(np.nonzero(virtual >= np.float32(thr)), axis=1)
    out = live.copy()
    for d in np.ndindex(2, 2, 2):
        cell = np.clip(corners - np.array(d), 0, shape - 1)
        out[tuple((cell >> 3).T)] = True
    return out


def _brick_set(field, store, thr, fill, close=True, closure_from_field=False):
    """field: fp32 [nx+1, ny+1, nz+1]; store: bool [Bx, By, Bz], the bricks that take their corners from it.  close: the bricks of the
    eight cells around every stored corner >= thr are added, with all their corners at `fill` (they bring no inside corner, so one
    pass closes the set) or, closure_from_field, with the field's values (the caller's field has no inside corner there: asserted).
    -> ids int32 [M], table int32 [Bx, By, Bz], values fp32 [M, 8, 8, 8], virtual fp32 like field."""
    def fill_from_field(bricks):
        for b in zip(*np.nonzero(bricks)):
            sl = tuple(slice(8 * c, 8 * c + 8) for c in b)
            virtual[sl] = field[sl]
    virtual = np.full(field.shape, fill, dtype=np.float32)
    fill_from_field(store)
    live = store.copy()
    if close:
        live = _closure(virtual, live, thr)
        if closure_from_field:
            fill_from_field(live)
            assert np.array_equal(_closure(virtual, live, thr), live)
    ids = np.nonzero(live.reshape(-1))[0].astype(np.int32)
    table = np.full(live.shape, -1, dtype=np.int32)
    table.reshape(-1)[ids] = np.arange(len(ids), dtype=np.int32)
    values = np.empty((len(ids), 8, 8, 8), dtype=np.float32)
    for s, b in enumerate(zip(*np.nonzero(live))):
        values[s] = virtual[tuple(slice(8 * c, 8 * c + 8) for c in b)]
    return ids, table, values, virtual


def _active_cells(virtual, thr):
    """The linear indices (i ny + j) nz + k of the restatement's active cells, ascending: its vertex order."""
    nx, ny, nz = (s - 1 for s in virtual.shape)
    with np.errstate(invalid='ignore'):
        inside = virtual >= np.float32(thr)
    n_in = sum(inside[dx:dx + nx, dy:dy + ny, dz:dz + nz].astype(np.int32) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    return np.nonzero(((n_in > 0) & (n_in < 8)).reshape(-1))[0]


def _sorted_rows(f):
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def _device(ids, table, values, shape, thr, fill, lo=LO, hi=HI):
    from perf_amd.mesh import surface_nets_bricks
    mesh, cells = surface_nets_bricks(torch.from_numpy(values).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(table).cuda(), shape, thr, fill, lo, hi)
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32 and cells.dtype == torch.int64
    return mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), cells.cpu().numpy()


def _check_order(cells, faces, ids, table, shape):
    """The statement's order: vertices ascend in (slot, local cell); faces come in pairs that share their first vertex."""
    nx, ny, nz = shape
    i, j, k = cells // (ny * nz), (cells // nz) % ny, cells % nz
    key = table[i >> 3, j >> 3, k >> 3].astype(np.int64) * 512 + ((i & 7) * 8 + (j & 7)) * 8 + (k & 7)
    assert (table[i >> 3, j >> 3, k >> 3] >= 0).all() and (np.diff(key) > 0).all()
    assert len(faces) % 2 == 0 and np.array_equal(faces[0::2, 0], faces[1::2, 0]) and np.array_equal(faces[0::2, 2], faces[1::2, 1])


def _compare(ids, table, values, virtual, thr, fill, lo=LO, hi=HI, label=''):
    from perf_amd.mesh import surface_nets
    shape = tuple(s - 1 for s in virtual.shape)
    want_v, want_f = R.surface_nets(virtual, thr, lo, hi)
    got_v, got_f, cells = _device(ids, table, values, shape, thr, fill, lo, hi)
    assert got_v.shape == want_v.shape and got_f.shape == want_f.shape, (label, got_v.shape, want_v.shape, got_f.shape, want_f.shape)
    order = np.argsort(cells, kind='stable')
    assert np.array_equal(cells[order], _active_cells(virtual, thr)), label             # a permutation onto the linear cell order
    _check_order(cells, got_f, ids, table, shape)
    new = np.empty(len(cells), dtype=np.int64)
    new[order] = np.arange(len(cells))
    assert got_f.min(initial=0) >= 0 and got_f.max(initial=-1) < len(cells)
    assert np.array_equal(_sorted_rows(new[got_f]), _sorted_rows(want_f)), label
    bound = _ulp(max(abs(v) for v in list(lo) + list(hi)))
    err = float(np.abs(got_v[order].astype(np.float64) - want_v).max()) if len(want_v) else 0.0
    print(f'[brickmesh {label}] bricks {len(ids)} of {table.size}; V {len(want_v)} F {len(want_f)}; max |vertex - float64 restatement| {err:.3e} = {err / bound:.3f} ulp '
          'of the box (bound 1)')
    assert np.isfinite(got_v).all() and err <= bound, (label, err, bound)
    dense = surface_nets(torch.from_numpy(virtual).cuda(), thr, lo, hi)
    assert got_v[order].tobytes() == dense.vertices.cpu().numpy().tobytes(), label      # the dense unit's bits
    assert np.array_equal(_sorted_rows(new[got_f]), _sorted_rows(dense.faces.cpu().numpy())), label
    return got_v, got_f, cells


def _random_field(shape, seed):
    return np.random.default_rng(seed).random(tuple(s + 1 for s in shape), dtype=np.float32)


def _store(bricks, *which):
    s = np.zeros(bricks, dtype=bool)
    for b in which:
        s[b] = True
    return s


# ---- against the restatement ---------------------------------------------------------------------------------------------------------------
def test_one_brick_alone():
    field = _random_field((8, 8, 8), 1)
    ids, table, values, virtual = _brick_set(field, np.ones((1, 1, 1), dtype=bool), 0.5, 0.0)
    assert len(ids) == 1 and (virtual[8] == 0).all() and (virtual[:, 8] == 0).all() and (virtual[:, :, 8] == 0).all()
    _compare(ids, table, values, virtual, 0.5, 0.0, label='one brick')


PAIRS = [((16, 16, 16), (0, 1, 1), (1, 1, 1), 'face-x'), ((16, 16, 16), (1, 1, 0), (1, 1, 1), 'face-z'), ((16, 16, 16), (0, 0, 1), (1, 1, 1), 'edge-xy'),
         ((16, 16, 16), (0, 1, 0), (1, 1, 1), 'edge-xz'), ((16, 16, 16), (0, 0, 0), (1, 1, 1), 'corner'), ((16, 16, 16), (1, 0, 0), (0, 1, 1), 'corner-mixed'),
         ((8, 16, 24), (0, 0, 1), (0, 1, 1), 'face-y'), ((8, 16, 24), (0, 0, 1), (0, 1, 2), 'edge-yz')]


@pytest.mark.parametrize('shape,a,b,kind', PAIRS, ids=[p[3] + '-' + 'x'.join(map(str, p[0])) for p in PAIRS])
def test_two_bricks_and_a_ball_on_what_they_share(shape, a, b, kind):
    """A ball centred (slightly off, so that no value is exactly 0) on the middle of what the two bricks share -- a face, an edge, a
    corner -- crosses every seam between them and the seams to the closure bricks around them, which hold `fill`."""
    centre = tuple((8.0 * max(p, q) if p != q else 8.0 * p + 4.0) + e for p, q, e in zip(a, b, (0.3, -0.4, 0.2)))
    field = R.ball(shape, centre, 5.7)
    bricks = tuple(s // 8 for s in shape)
    ids, table, values, virtual = _brick_set(field, _store(bricks, a, b), 0.0, -1.0)
    assert len(ids) > 2
    got_v, got_f, _ = _compare(ids, table, values, virtual, 0.0, -1.0, label=f'{kind} {shape}')
    assert len(got_f) > 0


def test_all_bricks_live():
    shape = (16, 24, 8)
    field = _random_field(shape, 2)
    ids, table, values, virtual = _brick_set(field, np.ones((2, 3, 1), dtype=bool), 0.5, 0.0)
    assert len(ids) == 6 and np.array_equal(virtual[:16, :24, :8], field[:16, :24, :8]) and (virtual[16] == 0).all() and (virtual[:, 24] == 0).all() and (virtual[:, :, 8] == 0).all()
    _compare(ids, table, values, virtual, 0.5, 0.0, label='all live (16, 24, 8)')


def test_all_bricks_live_with_two_scan_levels():
    """40 bricks are 320 slabs, more than one scan workgroup's 256: the scan over the slabs takes a second level."""
    shape = (40, 32, 16)
    ids, table, values, virtual = _brick_set(_random_field(shape, 6), np.ones((5, 4, 2), dtype=bool), 0.5, 0.0)
    assert len(ids) == 40 and 8 * len(ids) > 256
    _compare(ids, table, values, virtual, 0.5, 0.0, label='all live (40, 32, 16)')


def _random_half(close):
    shape = (24, 24, 24)
    rng = np.random.default_rng(7)
    store = np.zeros(27, dtype=bool)
    store[rng.permutation(27)[:13]] = True
    return shape, _brick_set(_random_field(shape, 3), store.reshape(3, 3, 3), 0.5, 0.0, close=close)


def test_a_random_half_of_the_bricks_closed():
    shape, (ids, table, values, virtual) = _random_half(True)
    assert 13 < len(ids) < 27
    _compare(ids, table, values, virtual, 0.5, 0.0, label='random half (24, 24, 24), closed')


def test_a_set_that_is_not_closed_is_counted_and_refused():
    """Without the closure bricks: the count pass counts the quads of the virtual field's mesh that need a cell of a missing brick, both
    passes leave exactly those out, the Python layer raises, and the raw ops stay in range and leave no error on the device."""
    from perf_amd import _lib, ops
    from perf_amd.mesh import surface_nets_bricks
    shape, (ids, table, values, virtual) = _random_half(False)
    assert len(ids) == 13
    dv, di, dt = torch.from_numpy(values).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(table).cuda()
    with pytest.raises(_lib.PerfError, match='not in the set'):
        surface_nets_bricks(dv, di, dt, shape, 0.5, 0.0, LO, HI)
    counts, ws = ops.brickmesh_count(dv, di, dt, shape, 0.5, 0.0)
    nv, nf, bad = counts.tolist()
    vertices, faces, cells = ops.brickmesh_write(dv, di, dt, shape, 0.5, 0.0, LO, HI, ws, nv, nf)
    torch.cuda.synchronize()
    v, f, c = vertices.cpu().numpy(), faces.cpu().numpy(), cells.cpu().numpy()
    want_v, want_f = R.surface_nets(virtual, 0.5, LO, HI)
    print(f'[brickmesh not closed] V {nv} of {len(want_v)}, F {nf} of {len(want_f)}, violations {bad}')
    assert bad > 0 and nv > 0 and nf > 0 and np.isfinite(v).all() and f.min() >= 0 and f.max() < nv
    assert (v >= np.array(LO, dtype=np.float32)).all() and (v <= np.array(HI, dtype=np.float32)).all()
    # exactly the active cells that lie in live bricks have a vertex, and exactly the violating quads are missing
    active = _active_cells(virtual, 0.5)
    i, j, k = active // (24 * 24), (active // 24) % 24, active % 24
    assert np.array_equal(np.sort(c), active[table[i >> 3, j >> 3, k >> 3] >= 0])
    assert nf + 2 * bad == len(want_f)
    order = np.argsort(c)
    new = np.full(len(want_v), -1, dtype=np.int64)
    new[np.searchsorted(active, c)] = np.arange(nv)
    kept = new[want_f]
    kept = kept[(kept >= 0).all(axis=1)]                 # the restatement's faces whose three cells are live, in the device's numbering
    assert set(map(tuple, f.tolist())) <= set(map(tuple, kept.tolist()))
    assert np.abs(v[order].astype(np.float64) - want_v[np.searchsorted(active, c[order])]).max() <= _ulp(1.25)


def test_zero_bricks():
    from perf_amd import ops
    values = torch.empty(0, 8, 8, 8, device='cuda')
    ids = torch.empty(0, dtype=torch.int32, device='cuda')
    table = torch.full((2, 1, 3), -1, dtype=torch.int32, device='cuda')
    counts, ws = ops.brickmesh_count(values, ids, table, (16, 8, 24), 0.5, 0.0)
    assert counts.tolist() == [0, 0, 0]
    vertices, faces, cells = ops.brickmesh_write(values, ids, table, (16, 8, 24), 0.5, 0.0, LO, HI, ws, 0, 0)       # zero capacities, NULL outputs
    assert vertices.shape == (0, 3) and faces.shape == (0, 3) and cells.shape == (0,)


def test_values_at_the_threshold_are_inside():
    rng = np.random.default_rng(5)
    field = rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=(17, 9, 25))
    ids, table, values, virtual = _brick_set(field, np.ones((2, 1, 3), dtype=bool), 0.5, 0.0)
    _, faces, _ = _compare(ids, table, values, virtual, 0.5, 0.0, label='values in {0, thr, 1}')
    above = np.where(values == 0.5, np.float32(1.0), values)                    # the same inside set, by construction
    assert np.array_equal(_device(ids, table, above, (16, 8, 24), 0.5, 0.0)[1], faces) and len(faces) > 0


def test_nan_and_infinite_corners():
    shape = (16, 16, 24)
    rng = np.random.default_rng(11)
    field = _random_field(shape, 4)
    pick = rng.random(field.shape)
    field[pick < 0.05] = np.nan
    field[(pick >= 0.05) & (pick < 0.10)] = np.inf
    field[(pick >= 0.10) & (pick < 0.12)] = -np.inf
    store = np.ones((2, 2, 3), dtype=bool)
    store[1, 0, 2] = store[0, 1, 0] = False               # (and two bricks the closure has to bring back, holding `fill`)
    ids, table, values, virtual = _brick_set(field, store, 0.5, 0.0)
    assert np.isnan(values).any() and np.isposinf(values).any() and np.isneginf(values).any()
    vertices, faces, _ = _compare(ids, table, values, virtual, 0.5, 0.0, label='NaN and inf corners')
    assert np.isfinite(vertices).all() and len(faces) > 0


def _ball_set():
    shape = (48, 48, 48)
    field = R.ball(shape, (24.3, 23.6, 24.4), 17.3)
    store = np.zeros((6, 6, 6), dtype=bool)
    inside = np.stack(np.nonzero(field[:48, :48, :48] >= 0), axis=1)
    store[tuple((inside >> 3).T)] = True
    ids, table, values, virtual = _brick_set(field, store, 0.0, -1.0, closure_from_field=True)
    # the virtual field is the ball wherever a cell is active and -1 (outside, like the ball there) elsewhere: the ball's own mesh
    return shape, ids, table, values, virtual


def test_ball_from_its_closed_live_bricks_is_a_closed_manifold():
    shape, ids, table, values, virtual = _ball_set()
    assert 0 < len(ids) < 216
    vertices, faces, _ = _compare(ids, table, values, virtual, 0.0, -1.0, [0, 0, 0], list(shape), label='ball r=17.3')
    assert R.is_closed_oriented_manifold(faces) and not R.has_repeated_index(faces)
    ratio = R.signed_volume(vertices, faces) / (4.0 / 3.0 * np.pi * 17.3 ** 3)
    print(f'[brickmesh ball r=17.3] live bricks {len(ids)} of 216; signed volume / ball volume {ratio:.4f}')
    assert abs(ratio - 1.0) <= 0.03                      # (the bound of tests/test_cpu_mesh_reference.py for a ball of this size)


def test_capacities_below_the_counts_are_refused():
    from perf_amd import _lib, ops
    shape, (ids, table, values, virtual) = _random_half(True)
    dv, di, dt = torch.from_numpy(values).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(table).cuda()
    counts, ws = ops.brickmesh_count(dv, di, dt, shape, 0.5, 0.0)
    nv, nf, bad = counts.tolist()
    assert nv > 0 and nf > 0 and bad == 0
    with pytest.raises(_lib.PerfError, match='vertices'):
        ops.brickmesh_write(dv, di, dt, shape, 0.5, 0.0, LO, HI, ws, nv - 1, nf)
    with pytest.raises(_lib.PerfError, match='faces'):
        ops.brickmesh_write(dv, di, dt, shape, 0.5, 0.0, LO, HI, ws, nv, nf - 1)
    vertices, faces, cells = ops.brickmesh_write(dv, di, dt, shape, 0.5, 0.0, LO, HI, ws, nv + 3, nf + 5)    # room to spare: the rows past the counts are not written
    exact = ops.brickmesh_write(dv, di, dt, shape, 0.5, 0.0, LO, HI, ws, nv, nf)
    assert torch.equal(vertices[:nv], exact[0]) and torch.equal(faces[:nf], exact[1]) and torch.equal(cells[:nv], exact[2])


def test_two_runs_are_bit_identical():
    shape, (ids, table, values, virtual) = _random_half(True)
    a, b = _device(ids, table, values, shape, 0.5, 0.0), _device(ids, table, values, shape, 0.5, 0.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    shape, ids, table, values, virtual = _ball_set()
    a, b = _device(ids, table, values, shape, 0.0, -1.0), _device(ids, table, values, shape, 0.0, -1.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- which bricks are live -----------------------------------------------------------------------------------------------------------------
def _occ_cell(i, n, res, exact):
    """c(i, n), every step in fp32.  exact: from the correctly rounded i / n; otherwise from fl32(i) * fl32(1 / n), the header's x(i, n):
    what the dense lattice's division of a device tensor by a host scalar evaluates to."""
    i = np.asarray(i, dtype=np.float32)
    x = i / np.float32(n) if exact else i * (np.float32(1.0) / np.float32(n))
    return (np.clip(x, np.float32(0.0005), np.float32(0.9995)) * np.float32(res)).astype(np.int64)


def _select_reference(occ, shape, exact):
    res = occ.shape[0]
    bricks = tuple(n // 8 for n in shape)
    lo = [_occ_cell(8 * np.arange(b), n, res, exact) for b, n in zip(bricks, shape)]
    hi = [_occ_cell(np.minimum(8 * np.arange(b) + 8, n), n, res, exact) for b, n in zip(bricks, shape)]
    live = np.zeros(bricks, dtype=bool)
    for b in np.ndindex(*bricks):
        live[b] = occ[lo[0][b[0]]:hi[0][b[0]] + 1, lo[1][b[1]]:hi[1][b[1]] + 1, lo[2][b[2]]:hi[2][b[2]] + 1].any()
    table = np.full(bricks, -1, dtype=np.int32)
    table[live] = np.arange(int(live.sum()), dtype=np.int32)
    return table


@pytest.mark.parametrize('res', [16, 32])
@pytest.mark.parametrize('n', [8, 24, 64, 136, (24, 136, 64)], ids=str)
def test_select_bricks_follows_the_box_rule(n, res):
    from perf_amd.mesh import select_bricks
    shape = (n,) * 3 if isinstance(n, int) else n
    rng = np.random.default_rng(100 * res + sum(shape))
    for share in (0.01, 0.2):
        occ = rng.random((res, res, res)) < share
        occ[0, 0, 0] = occ[-1, -1, -1] = share > 0.1
        ids, table = select_bricks(torch.from_numpy(occ).cuda(), n)
        want = _select_reference(occ, shape, exact=True)
        assert np.array_equal(want, _select_reference(occ, shape, exact=False))      # (the two forms of x(i, n) agree on every box here)
        assert table.dtype == torch.int32 and ids.dtype == torch.int32
        assert np.array_equal(table.cpu().numpy(), want), (shape, res, share)
        assert np.array_equal(ids.cpu().numpy(), np.nonzero(want.reshape(-1) >= 0)[0]) and (np.diff(ids.cpu().numpy()) > 0).all()
    ids, table = select_bricks(torch.zeros(res, res, res, dtype=torch.bool, device='cuda'), n)
    assert ids.numel() == 0 and bool((table == -1).all())
    ids, table = select_bricks(torch.ones(1, res, res, res, dtype=torch.bool, device='cuda'), n)           # (the estimator's [1, R, R, R] too)
    assert ids.numel() == table.numel() and torch.equal(table.reshape(-1), torch.arange(table.numel(), dtype=torch.int32, device='cuda'))


# ---- end to end: the trained analytic room (the set-up of tests/test_gpu_mesh.py) ------------------------------------------------------------
HALF = (0.9, 0.7, 0.5)           # perf_amd.synthetic.room's half extents, before it normalises its distances


def _room_distance(d):
    """The distance from the origin to the room's walls along unit directions d [..., 3], NOT normalised."""
    return (torch.tensor(HALF, device=d.device) / d.abs().clamp_min(1e-12)).amin(-1)


@pytest.fixture(scope='module')
def trained_scene():
    """The synthetic room, trained from one 256x512 panorama at the origin."""
    from perf_amd import synthetic
    from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays
    torch.manual_seed(0); np.random.seed(0)
    scene = NeRFScene(dtype='fp16')
    rays = gen_pano_rays(torch.eye(4), 256, 512)
    dist, rgb = synthetic.room(rays.d)
    pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
    scene.train_conf.pixel_loss_batch_size = 4096
    scene.train_one_episode(pool, 150, 100)
    # synthetic.room divides its distances by (their largest) * 1.05: in the scene's units the walls stand at HALF / unit
    unit = float(_room_distance(rays.d).max()) * 1.05
    assert float((dist[..., 0] * unit - _room_distance(rays.d)).abs().max()) < 1e-5
    return scene, unit


def _distance_to_walls(v, unit):
    q = np.abs(v.astype(np.float64)) - np.array(HALF) / unit
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.abs(np.minimum(q.max(axis=1), 0.0))


def _stored_index(ids, table):
    """The corner indices [M, 8, 8, 8] per axis of the bricks `ids` of a table [Bx, By, Bz]."""
    by, bz = table.shape[1], table.shape[2]
    b = ids.long()
    g = torch.arange(8, device=ids.device)
    i = (8 * (b // (by * bz)))[:, None, None, None] + g[None, :, None, None]
    j = (8 * ((b // bz) % by))[:, None, None, None] + g[None, None, :, None]
    k = (8 * (b % bz))[:, None, None, None] + g[None, None, None, :]
    return torch.broadcast_tensors(i, j, k)


@pytest.mark.parametrize('n', [128, 200, 256])
def test_density_bricks_are_the_dense_lattices_values(trained_scene, n):
    """To the bit at the stored corners; every corner that is not stored is exactly 0 in the dense lattice.  n = 200 makes i / n inexact."""
    from perf_amd.mesh import density_bricks, density_lattice, select_bricks
    scene = trained_scene[0]
    ids, table, values = density_bricks(scene, n, chunk_bricks=1000)                # (several chunks, the last one short)
    ids2, table2 = select_bricks(scene.estimator.binaries, n)
    assert torch.equal(ids, ids2) and torch.equal(table, table2) and values.shape == (ids.numel(), 8, 8, 8) and values.dtype == torch.float32
    assert 0 < ids.numel() < table.numel() and torch.equal(values, density_bricks(scene, n)[2])
    dense = density_lattice(scene, n)
    i, j, k = _stored_index(ids, table)
    # the coordinates are the dense lattice's own expression, to the bit
    from perf_amd import ops
    few = min(int(ids.numel()), 300)
    x01, sel, interior = ops.brickmesh_corners(ids, 0, few, (n,) * 3, scene.estimator.binaries)
    want = torch.stack([i[:few], j[:few], k[:few]], dim=-1).reshape(-1, 3).float() / float(n)
    assert torch.equal(x01, want) and torch.equal(interior.bool(), ((want > 0) & (want < 1)).all(dim=1)) and bool((sel <= interior).all())
    assert torch.equal(values, dense[i, j, k])
    stored = torch.zeros_like(dense, dtype=torch.bool)
    stored[i, j, k] = True
    assert float(dense[~stored].abs().max()) == 0.0 and float(values.max()) > 0.0
    print(f'[brickmesh density {n}] live bricks {ids.numel()} of {table.numel()}: {ids.numel() * 512 / (n + 1) ** 3:.4f} of the lattice\'s corners')


@pytest.mark.parametrize('n', [128, 200])
def test_sparse_extraction_is_the_dense_extraction_reordered(trained_scene, n):
    from perf_amd.mesh import density_bricks, surface_nets_bricks
    scene = trained_scene[0]
    thr = math.log(2.0) / float(scene.renderer.render_step_size)
    aabb = scene.nerf._aabb_host
    dense = scene.extract_mesh(resolution=n, colors=True, normals=True)
    sparse = scene.extract_mesh_sparse(resolution=n, colors=True, normals=True)
    ids, table, values = density_bricks(scene, n)
    again, cells = surface_nets_bricks(values, ids, table, (n,) * 3, thr, 0.0, aabb[:3], aabb[3:])        # the same call, for the cells
    assert torch.equal(again.vertices, sparse.vertices) and torch.equal(again.faces, sparse.faces)
    V = len(dense.vertices)
    assert V > 0 and len(sparse.vertices) == V and len(sparse.faces) == len(dense.faces) and len(torch.unique(cells)) == V
    order = torch.argsort(cells)
    assert torch.equal(sparse.vertices[order], dense.vertices)                          # bit-equal, in linear cell order
    new = torch.empty(V, dtype=torch.int64, device='cuda')
    new[order] = torch.arange(V, device='cuda')
    assert np.array_equal(_sorted_rows(new[sparse.faces.long()].cpu().numpy()), _sorted_rows(dense.faces.cpu().numpy()))
    assert torch.equal(sparse.colors[order], dense.colors) and torch.equal(sparse.normals[order], dense.normals)
    plain = scene.extract_mesh_sparse(resolution=n)
    assert plain.colors is None and plain.normals is None and torch.equal(plain.vertices, sparse.vertices) and torch.equal(plain.faces, sparse.faces)


def test_mesh_of_the_trained_room_at_1024(trained_scene):
    """A resolution the dense path has never run (a 4.3 GB lattice)."""
    from perf_amd.mesh import select_bricks
    from perf_amd.scene import gen_pano_rays
    scene, unit = trained_scene
    res = 1024
    mesh = scene.extract_mesh_sparse(resolution=res)
    V, F = len(mesh.vertices), len(mesh.faces)
    assert V > 0 and F > 0 and mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32 and mesh.vertices.is_cuda
    assert bool(torch.isfinite(mesh.vertices).all()) and float(mesh.vertices.min()) >= -1.0 and float(mesh.vertices.max()) <= 1.0
    assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < V
    f = mesh.faces
    assert not bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any())
    again = scene.extract_mesh_sparse(resolution=res)
    assert torch.equal(again.vertices, mesh.vertices) and torch.equal(again.faces, mesh.faces)
    ids, table = select_bricks(scene.estimator.binaries, res)
    share = ids.numel() * 512 / (res + 1) ** 3
    rays = gen_pano_rays(torch.eye(4), 64, 128)
    rendered = scene.render(rays, ['distance'])['distance'].reshape(-1).cpu().numpy()
    analytic = (_room_distance(rays.d) / unit).reshape(-1).cpu().numpy()
    e = float(np.percentile(np.abs(rendered - analytic), 90))
    d90 = float(np.percentile(_distance_to_walls(mesh.vertices.cpu().numpy(), unit), 90))
    occ_diag = math.sqrt(3.0) * 2.0 / 256            # an occupancy cell's diagonal
    lat_diag = math.sqrt(3.0) * 2.0 / res            # a lattice cell's diagonal
    bound = e + 2 * occ_diag + lat_diag
    print(f'[brickmesh room 1024] V {V} F {F}; live bricks {ids.numel()} of {table.numel()}; {share:.4f} of the (n+1)^3 corners evaluated; p90 |rendered - analytic '
          f'distance| {e:.4f}; p90 vertex distance to the nearest wall {d90:.4f}; bound {bound:.4f}')
    path = os.environ.get('PERF_BRICKMESH_REPORT')
    if path:
        json.dump({'resolution': res, 'vertices': V, 'faces': F, 'live_bricks': ids.numel(), 'bricks': table.numel(), 'share_of_corners_evaluated': share,
                   'p90_abs_rendered_minus_analytic_distance': e, 'p90_vertex_distance_to_nearest_wall': d90, 'bound': bound}, open(path, 'w'), indent=1)
    assert d90 <= bound
