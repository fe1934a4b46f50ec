"""Surface nets on the GPU (include/perf_hip_mesh.h, perf_amd/mesh.py) against the float64 numpy restatement of tests/mesh_reference.py:
faces and the vertex count exactly, vertices to one fp32 ulp; analytic balls; values at the threshold, empty and full fields, NaN and
infinite corners; determinism; and a mesh of the trained analytic room whose distance to the walls is bounded by what the same model
renders.

The vertex bound.  The kernel carries a vertex in double between the fp32 corner loads and its fp32 store: the same
formula as the restatement, whose double rounding errors (~1e-16 relative, on either side) are nothing beside the ONE fp32 rounding of
the store, half an ulp of the coordinate.  A coordinate is at most max(|lo|, |hi|) =: M in magnitude, so the bound asserted is 1 ulp of
M (half an ulp for the store, rounded up to the next whole ulp for the double noise that can move a value across a rounding boundary).
With PERF_MESH_REPORT=<path> the end-to-end figures are also written there as JSON (profiles/mesh.json is folded from it)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_reference as R

pytestmark = pytest.mark.gpu

LO, HI = [-1.0, -1.25, -0.5], [1.0, 0.75, 1.0]           # (not a cube, not centred: the three axes scale differently)
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 7, 9), (33, 17, 65), (3, 3, 63), (3, 3, 64), (3, 3, 65), (70, 70, 70), (160, 160, 160)]
_REPORT = {}


def _report(key, value):
    _REPORT[key] = value
    path = os.environ.get('PERF_MESH_REPORT')
    if path:
        json.dump(_REPORT, open(path, 'w'), indent=1)


def _field(shape, kind, seed=0):
    rng = np.random.default_rng(1000 * seed + sum(s * 7 ** i for i, s in enumerate(shape)))
    f = rng.random(tuple(s + 1 for s in shape), dtype=np.float32)
    if kind == 'sparse':                        # 1 % of the corners above thr = 0.5
        f = np.where(f > 0.99, np.float32(0.75), f * np.float32(0.5)).astype(np.float32)
    return f


def _ulp(m):
    return float(np.spacing(np.float32(m)))


def _device_mesh(field, thr, lo=LO, hi=HI):
    from perf_amd.mesh import surface_nets
    m = surface_nets(torch.from_numpy(field).cuda(), thr, lo, hi)
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy()


def _compare(field, thr, lo=LO, hi=HI, label=''):
    want_v, want_f = R.surface_nets(field, thr, lo, hi)
    got_v, got_f = _device_mesh(field, thr, lo, hi)
    assert got_v.dtype == np.float32 and got_f.dtype == np.int32
    assert got_v.shape == want_v.shape and got_f.shape == want_f.shape, (label, got_v.shape, want_v.shape, got_f.shape, want_f.shape)
    assert np.array_equal(got_f, want_f), label
    bound = _ulp(max(abs(v) for v in list(lo) + list(hi)))
    err = float(np.abs(got_v.astype(np.float64) - want_v).max()) if len(want_v) else 0.0
    print(f'[mesh {label}] V {len(want_v)} F {len(want_f)}; max |vertex - float64 restatement| {err:.3e} = {err / bound:.3f} ulp of the box (bound 1)')
    assert np.isfinite(got_v).all() and err <= bound, (label, err, bound)
    return got_v, got_f


@pytest.mark.parametrize('kind', ['random', 'sparse'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_matches_the_restatement(shape, kind):
    _compare(_field(shape, kind), 0.5, label=f'{shape} {kind}')


def test_four_scan_levels():
    """256^3 = 2^24 chunks is where the scan needs a fourth level; with nz = 1 every cell is a chunk, so a flat lattice gets there."""
    shape = (4100, 4100, 1)
    assert shape[0] * shape[1] > 256 ** 3
    _compare(_field(shape, 'sparse'), 0.5, label=f'{shape} sparse')


@pytest.mark.parametrize('shape,centre,radius', [((24, 26, 28), (12.3, 13.6, 14.4), 9.7), ((16, 18, 20), (8.3, 9.6, 10.4), 6.2)])
def test_ball_is_a_closed_manifold_of_the_balls_volume(shape, centre, radius):
    vertices, faces = _compare(R.ball(shape, centre, radius), 0.0, [0, 0, 0], list(shape), label=f'ball r={radius}')
    if radius == 9.7:
        assert vertices.shape == (1770, 3) and faces.shape == (3536, 3)
    assert R.is_closed_oriented_manifold(faces) and not R.has_repeated_index(faces)
    ratio = R.signed_volume(vertices, faces) / (4.0 / 3.0 * np.pi * radius ** 3)
    print(f'[mesh ball r={radius}] signed volume / ball volume {ratio:.4f}')
    assert (abs(ratio - 1.0) <= 0.03) if radius == 9.7 else (0.95 <= ratio <= 1.0)         # (the bounds of tests/test_cpu_mesh_reference.py)


def test_values_at_the_threshold_are_inside():
    rng = np.random.default_rng(5)
    field = rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=(12, 10, 70))
    vertices, faces = _compare(field, 0.5, label='values in {0, thr, 1}')
    below = np.where(field == 0.5, np.float32(1.0), field)                      # the same inside set, by construction
    assert np.array_equal(_device_mesh(below, 0.5)[1], faces) and len(faces) > 0


@pytest.mark.parametrize('value', [0.0, 1.0, 0.5], ids=['empty', 'full', 'equal-to-thr'])
def test_empty_and_full_fields(value):
    from perf_amd import ops
    field = torch.full((8, 6, 71), value, device='cuda')
    counts, ws = ops.mesh_count(field, 0.5)
    assert counts.tolist() == [0, 0]
    vertices, faces = ops.mesh_write(field, 0.5, LO, HI, ws, 0, 0)              # zero capacities, NULL outputs
    assert vertices.shape == (0, 3) and faces.shape == (0, 3)


def test_capacities_below_the_counts_are_refused():
    from perf_amd import _lib, ops
    field = torch.from_numpy(_field((5, 7, 9), 'random')).cuda()
    counts, ws = ops.mesh_count(field, 0.5)
    nv, nf = counts.tolist()
    assert nv > 0 and nf > 0
    with pytest.raises(_lib.PerfError, match='vertices'):
        ops.mesh_write(field, 0.5, LO, HI, ws, nv - 1, nf)
    with pytest.raises(_lib.PerfError, match='faces'):
        ops.mesh_write(field, 0.5, LO, HI, ws, nv, nf - 1)
    vertices, faces = ops.mesh_write(field, 0.5, LO, HI, ws, nv + 3, nf + 5)    # room to spare: the rows past the counts are not written
    want_v, want_f = R.surface_nets(field.cpu().numpy(), 0.5, LO, HI)
    assert np.array_equal(faces[:nf].cpu().numpy(), want_f) and len(want_v) == nv


def test_nan_and_infinite_corners():
    rng = np.random.default_rng(11)
    field = _field((9, 11, 67), 'random', seed=3)
    pick = rng.random(field.shape)
    field[pick < 0.05] = np.nan
    field[(pick >= 0.05) & (pick < 0.10)] = np.inf
    field[(pick >= 0.10) & (pick < 0.12)] = -np.inf
    vertices, faces = _compare(field, 0.5, label='NaN and inf corners')
    assert np.isfinite(vertices).all() and len(faces) > 0


def test_two_runs_are_bit_identical():
    for shape, kind in (((70, 70, 70), 'random'), ((33, 17, 65), 'sparse')):
        field = _field(shape, kind, seed=2)
        (v1, f1), (v2, f2) = _device_mesh(field, 0.5), _device_mesh(field, 0.5)
        assert v1.tobytes() == v2.tobytes() and f1.tobytes() == f2.tobytes()


# ---- end to end: the trained analytic room ----------------------------------------------------------------------------------------------
HALF = (0.9, 0.7, 0.5)           # perf_amd.synthetic.room's half extents, before it normalises its distances


def _room_distance(d):
    """The distance from the origin to the room's walls along unit directions d [..., 3], NOT normalised."""
    return (torch.tensor(HALF, device=d.device) / d.abs().clamp_min(1e-12)).amin(-1)


@pytest.fixture(scope='module')
def trained_scene():
    """The set-up of tests/test_gpu_field_normal.py: the synthetic room, trained from one 256x512 panorama at the origin."""
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


def test_density_lattice(trained_scene):
    from perf_amd.mesh import density_lattice
    scene = trained_scene[0]
    res = 32                          # (a power of two: i / res, and the world coordinate made from it, are exact)
    plain = density_lattice(scene, res, use_occupancy=False, chunk=5000)          # (several chunks, the last one short)
    assert plain.shape == (res + 1,) * 3 and plain.dtype == torch.float32 and torch.equal(plain, density_lattice(scene, res, use_occupancy=False))
    border = torch.ones_like(plain, dtype=torch.bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert float(plain[border].abs().max()) == 0.0 and float(plain[~border].max()) > 0.0
    # corner (i, j, k) is the world point lo + (i, j, k) / res * (hi - lo): the density query there
    ijk = torch.tensor([[3, 5, 7], [16, 16, 16], [31, 1, 20]], device='cuda')
    world = ijk.float() / res * 2.0 - 1.0
    assert torch.equal(plain[ijk[:, 0], ijk[:, 1], ijk[:, 2]], scene.nerf.query_density(world)[:, 0].float())
    # the occupancy zeroes what lies in an empty cell and keeps the rest: the cell of x01 is int(x01 * 256) away from the border
    masked = density_lattice(scene, res)
    g = torch.arange(res + 1, device='cuda')
    cell = (g.float() / res).clamp(0.0005, 0.9995).mul(256).long()
    occ = scene.estimator.binaries[0][cell[:, None, None], cell[None, :, None], cell[None, None, :]]
    assert torch.equal(masked, torch.where(occ, plain, torch.zeros_like(plain))) and 0 < int(occ.sum()) < occ.numel()


def test_mesh_of_the_trained_room(trained_scene):
    from perf_amd.scene import gen_pano_rays
    scene, unit = trained_scene
    res = 128
    mesh = scene.extract_mesh(resolution=res)
    V, F = len(mesh.vertices), len(mesh.faces)
    assert V > 0 and F > 0 and mesh.colors is None and mesh.normals is None
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32 and mesh.vertices.is_cuda
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    assert np.isfinite(v).all() and (v >= -1.0).all() and (v <= 1.0).all()
    assert f.min() >= 0 and f.max() < V and not R.has_repeated_index(f)
    again = scene.extract_mesh(resolution=res)
    assert torch.equal(again.vertices, mesh.vertices) and torch.equal(again.faces, mesh.faces)
    full = scene.extract_mesh(resolution=res, colors=True, normals=True)
    assert torch.equal(full.vertices, mesh.vertices) and torch.equal(full.faces, mesh.faces)
    assert full.colors.shape == (V, 3) and full.normals.shape == (V, 3)
    assert bool(torch.isfinite(full.colors).all()) and bool(torch.isfinite(full.normals).all())
    assert float(full.colors.min()) >= 0.0 and float(full.colors.max()) <= 1.0
    ln = torch.linalg.vector_norm(full.normals, dim=-1)
    assert bool((((ln - 1).abs() < 1e-5) | (ln == 0)).all())
    # geometry, measured on the same model: the panorama's distance error against the vertices' distance to the nearest wall
    rays = gen_pano_rays(torch.eye(4), 64, 128)
    rendered = scene.render(rays, ['distance'])['distance'].reshape(-1).cpu().numpy()
    analytic = (_room_distance(rays.d) / unit).reshape(-1).cpu().numpy()
    e = float(np.percentile(np.abs(rendered - analytic), 90))
    d90 = float(np.percentile(_distance_to_walls(v, unit), 90))
    occ_diag = math.sqrt(3.0) * 2.0 / 256            # an occupancy cell's diagonal
    lat_diag = math.sqrt(3.0) * 2.0 / res            # a lattice cell's diagonal
    bound = e + 2 * occ_diag + lat_diag
    print(f'[mesh room] V {V} F {F}; p90 |rendered - analytic distance| {e:.4f}; p90 vertex distance to the nearest wall {d90:.4f}; bound {bound:.4f}')
    _report('room_fp16_150+100_iterations', {'resolution': res, 'threshold': math.log(2.0) / scene.renderer.render_step_size, 'vertices': V, 'faces': F,
                                             'p90_abs_rendered_minus_analytic_distance': e, 'p90_vertex_distance_to_nearest_wall': d90, 'bound': bound})
    assert d90 <= bound
