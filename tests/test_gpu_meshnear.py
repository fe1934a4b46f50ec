"""The closest point of a mesh on the device (include/staged/perf_hip_meshnear.h, perf_amd/mesh.py) against the float64 restatement of
tests/meshnear_reference.py: dist2, face, u and v TO THE BIT (the rule is + - * / in double with contraction off, and the restatement
performs the same operations in the same order) on four grids from the default cell to one cell, the limit, the grid it shares with the
rays, and the deviation, the tolerance search and the value transfer built on it."""
import math

import numpy as np
import pytest
import torch

from tests import meshnear_reference as N
from tests import meshray_reference as M
from tests import meshvis_reference as V

pytestmark = pytest.mark.gpu
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cached inputs are read-only)


def _mesh(vertices, faces):
    from perf_amd.mesh import Mesh
    return Mesh(_dev(np.asarray(vertices, dtype=np.float32).reshape(-1, 3)), _dev(np.asarray(faces, dtype=np.int32).reshape(-1, 3)))


def _bits(t):
    """The words of a result: floats compared as integers, so that a NaN, the sign of a zero and the last bit all count."""
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want):
    """got: NearestHits; want: (dist2, face, u, v) of the restatement."""
    assert got.dist2.dtype == torch.float64 and got.face.dtype == torch.int32 and got.u.dtype == got.v.dtype == got.distance.dtype == torch.float32
    for name, g, w in zip(('dist2', 'face', 'u', 'v'), (got.dist2, got.face, got.u, got.v), want):
        g, w = _bits(g), _bits(w)
        differ = np.nonzero(g != w)[0]
        assert not len(differ), (name, len(differ), differ[:5], g[differ[:5]], w[differ[:5]])
    assert np.array_equal(_bits(got.distance), _bits(np.sqrt(want[0]).astype(np.float32)))


def _four_grids(mesh, cells):
    """The mesh's grid at four cells, the first the default (None), the last so large that the grid is one cell: brute force on the device."""
    from perf_amd.mesh import build_ray_grid
    grids = [build_ray_grid(mesh, cell) for cell in cells]
    assert cells[0] is None and grids[-1].dims == (1, 1, 1) and len(grids) == 4
    return grids


def _on_four_grids(vertices, faces, points, cells, max_distance=np.inf, want=None):
    """The device's answers on the four grids, equal to the restatement's brute force and to each other, and again from run to run."""
    from perf_amd.mesh import closest_point
    mesh = _mesh(vertices, faces)
    want = N.closest(vertices, faces, points, max_distance) if want is None else want
    query = _dev(np.asarray(points, dtype=np.float32).reshape(-1, 3))
    grids = _four_grids(mesh, cells)
    for grid in grids + grids[:1]:
        _same(closest_point(mesh, grid, query, max_distance), want)
    return want, grids


SMALL_CELLS = [None, 0.5, 0.3, 64.0]


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------------
def test_hand_points_in_every_region_on_the_boundaries_and_at_the_vertices():
    vertices, faces = N.TRIANGLE
    points = np.array([p for p, _ in N.HAND_POINTS], dtype=np.float32)
    want, _ = _on_four_grids(vertices, faces, points, SMALL_CELLS)
    for n, (p, (dist2, u, v)) in enumerate(N.HAND_POINTS):          # the restatement's answers are the hand-computed ones
        assert (want[0][n], want[1][n], want[2][n], want[3][n]) == (dist2, 0, u, v), p
    assert want[0][7] == 2.0 ** -6 and not want[0][-3:].any()        # 2^-3 above the interior; the vertices themselves: 0 exactly


def test_degenerate_faces():
    vertices, faces, points = N.degenerate_mesh()
    want, _ = _on_four_grids(vertices, faces, points, SMALL_CELLS)
    assert np.isfinite(want[0]).all()
    for face, cases in N.DEGENERATE:                                 # each face alone: the hand-computed answers
        pts = np.array([p for p, _ in cases], dtype=np.float32)
        alone, _ = _on_four_grids(np.array(face, dtype=np.float32), [[0, 1, 2]], pts, SMALL_CELLS)
        assert [(alone[0][n], alone[2][n], alone[3][n]) for n in range(len(cases))] == [w for _, w in cases], face


def test_on_a_shared_edge_the_tie_goes_to_the_smaller_face_index():
    vertices, faces = N.TETRAHEDRON
    want, _ = _on_four_grids(vertices, faces, N.TETRAHEDRON_POINTS, [None, 0.25, 0.11, 8.0])
    # (0.1, 0, 0) is the midpoint of the edge 0-1 of the faces 0 = (0, 2, 1) and 1 = (0, 1, 3): both give dist2 = 0 exactly; face 0 wins,
    # where the point is the midpoint of its edge a-c
    assert (want[0][0], want[1][0], want[2][0], want[3][0]) == (0.0, 0, 0.0, 0.5)
    assert (want[0][1], want[1][1]) == (0.0, 0) and (want[0][2], want[1][2]) == (0.0, 1)          # the vertices 0 (faces 0, 1, 3) and 3 (faces 1, 2, 3)


# ---- 2. the search -------------------------------------------------------------------------------------------------------------------------
def _fixture(which):
    if which not in _CACHE:
        if which == 'hollow_sphere':
            (vertices, faces), points = V.reference_mesh('hollow_sphere'), N.sphere_points()
        else:
            (vertices, faces), points = M.random_triangles(), N.triangle_points()
        _CACHE[which] = (vertices, faces, points)
    return _CACHE[which]


@pytest.mark.parametrize('which', ['hollow_sphere', 'triangles'])
def test_random_points_equal_brute_force_on_every_grid_and_within_every_limit(which):
    from perf_amd.mesh import build_ray_grid, closest_point
    vertices, faces, points = _fixture(which)
    want = N.expected_closest(which)
    longest = float((vertices.max(axis=0) - vertices.min(axis=0)).max())
    mesh = _mesh(vertices, faces)
    default = build_ray_grid(mesh)
    cells = [None, 2 * default.cell, 7.3 * default.cell, 4 * longest]
    _, grids = _on_four_grids(vertices, faces, points, cells, want=want)
    assert max(grids[0].dims) > 8 and len({g.dims for g in grids}) == 4 and int(grids[3].refs.numel()) == len(faces)
    if which == 'hollow_sphere':
        assert len(faces) == 768 + 2196 and len(points) == 4096 + 64
        far = np.sqrt(want[0][4096:])
        assert far.min() > 8.0 and (want[1][4096:] >= 0).all()          # the points at ten times the box's size have their answers too
        inside = np.abs(points[:4096]).max(axis=1) < 1.0
        assert 0.2 < inside.mean() < 0.9                                 # points inside the box and outside it
    # a finite limit: exactly the brute-force answer where dist2 <= max^2, and +inf, -1, 0, 0 elsewhere (the restatement applies the limit
    # to the same brute force; dist2 == max^2 is within)
    query = _dev(points)
    for limit in (0.05, 0.25, float(np.float32(np.sqrt(np.median(want[0])))), 0.0):
        cut = N.limited(want, limit)
        assert limit == 0.0 or 0 < int((cut[1] >= 0).sum()) < len(points)
        for grid in grids:
            _same(closest_point(mesh, grid, query, limit), cut)


def test_points_that_are_not_finite_faces_that_are_never_the_answer_and_empty_inputs():
    from perf_amd.mesh import build_ray_grid, closest_point
    vertices, faces = M.SMALL                                        # face 0 has a NaN vertex, face 1 an index outside [0, V)
    want, grids = _on_four_grids(vertices, faces, N.EDGE_POINTS, [None, 1.0, 0.25, 64.0])
    assert grids[0].bad_face == 0 and not np.isin(want[1], (0, 1)).any()
    assert want[1][1:4].tolist() == [-1, -1, -1] and np.isinf(want[0][1:4]).all() and not want[2][1:4].any()          # NaN and infinite points
    assert want[1][4] == 2 and want[0][4] == 0.25                    # three faces tie between the sheets: the smallest index
    _on_four_grids(vertices, faces, N.EDGE_POINTS, [None, 1.0, 0.25, 64.0], max_distance=0.5)
    # a hand-made grid that lists the two bad faces: they are still never the answer
    from perf_amd.mesh import RayGrid
    mesh = _mesh(vertices, faces)
    listed = RayGrid((-1.0, -1.0, -1.0), 8.0, (1, 1, 1), torch.zeros(1, dtype=torch.int32, device='cuda'), torch.arange(5, dtype=torch.int32, device='cuda'), 7, 5, 0)
    _same(closest_point(mesh, listed, _dev(N.EDGE_POINTS)), want)
    # N = 0, and the empty mesh
    none = closest_point(mesh, grids[0], torch.zeros(0, 3, device='cuda'))
    assert [tuple(t.shape) for t in none] == [(0,)] * 5
    empty = _mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    grid = build_ray_grid(empty)
    assert grid.dims == (1, 1, 1) and grid.refs.numel() == 0
    _same(closest_point(empty, grid, _dev(N.EDGE_POINTS)), N.closest(np.zeros((0, 3)), np.zeros((0, 3)), N.EDGE_POINTS))
    no_faces = _mesh(vertices, np.zeros((0, 3), np.int32))
    got = closest_point(no_faces, build_ray_grid(no_faces), _dev(N.EDGE_POINTS))
    assert (got.face == -1).all() and torch.isinf(got.dist2).all() and torch.isinf(got.distance).all() and not got.u.any() and not got.v.any()


def test_a_point_count_that_is_no_multiple_of_the_group():
    from perf_amd.mesh import build_ray_grid, closest_point
    vertices, faces = M.SMALL
    rng = np.random.default_rng(65537)
    points = rng.uniform(-1, 5, size=(65537, 3)).astype(np.float32)
    points[:len(N.EDGE_POINTS)] = N.EDGE_POINTS
    mesh = _mesh(vertices, faces)
    _same(closest_point(mesh, build_ray_grid(mesh, 1.0), _dev(points)), N.closest(vertices, faces, points))


# ---- 3. one grid, two units ----------------------------------------------------------------------------------------------------------------
def test_one_ray_grid_serves_the_rays_and_the_closest_points():
    """The grid is described twice, in meshray.hip and in meshnear.hip: ONE RayGrid of build_ray_grid fed to both gives each unit's brute
    force.  And a ray's hit point fed back as a query is as close to the mesh as fp32 lets it be: the exact hit point o + t d lies in its
    face; t is rounded to fp32 (|dt| <= 2^-24 t, which moves the point by at most 2^-24 t |d|) and so is each coordinate of the point
    (at most 2^-24 |h|_inf each, sqrt(3) of that together); the double operations in between add 2^-50 of the same.  So the distance to
    the mesh is at most 2^-24 (t |d| + sqrt(3) |h|_inf) (1 + 2^-20)."""
    from perf_amd.mesh import build_ray_grid, cast_rays, closest_point
    vertices, faces, points = _fixture('hollow_sphere')
    mesh = _mesh(vertices, faces)
    grid = build_ray_grid(mesh)
    o, d = M.sphere_rays()
    hits = cast_rays(mesh, grid, _dev(o), _dev(d))
    for name, g, w in zip(('t', 'face', 'u', 'v'), hits, M.expected_cast('hollow_sphere')):
        assert np.array_equal(_bits(g), _bits(w)), name
    _same(closest_point(mesh, grid, _dev(points)), N.expected_closest('hollow_sphere'))
    t = hits.t.cpu().numpy().astype(np.float64)
    hit = np.isfinite(t)
    assert hit.sum() > 1000
    o64, d64 = o[hit].astype(np.float64), d[hit].astype(np.float64)
    point = (o64 + t[hit, None] * d64).astype(np.float32)
    got = closest_point(mesh, grid, _dev(point))
    bound = 2.0 ** -24 * (t[hit] * np.linalg.norm(d64, axis=1) + math.sqrt(3) * np.abs(point).max(axis=1)) * (1 + 2.0 ** -20)
    dist2 = got.dist2.cpu().numpy()
    assert (got.face.cpu().numpy() >= 0).all() and (dist2 <= bound * bound).all(), float((np.sqrt(dist2) / bound).max())


# ---- 4. the deviation ------------------------------------------------------------------------------------------------------------------------
def _ball():
    """The device's surface-nets mesh of the rays' ball (radius 0.6, lattice spacing 0.1), made once, with its host copy."""
    if 'ball' not in _CACHE:
        from perf_amd.mesh import surface_nets
        from tests import meshcc_reference as CC
        mesh = surface_nets(_dev(M.ball_field()), 0.0, CC.SPHERE_LO, CC.SPHERE_HI)
        _CACHE['ball'] = (mesh, (mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()))
    return _CACHE['ball']


def _host(mesh):
    return mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()


def _same_deviation(got, want):
    """max, p90, the argmax and the counts exactly (a maximum, an order statistic and a correctly rounded square root); mean and rms are
    float64 sums of n terms added in another order than numpy's: n 2^-52 of the largest term, relative."""
    assert (got.max, got.p90, got.argmax_point, got.argmax_face_of_b, got.n_samples, got.n_beyond) == (
        want['max'], want['p90'], want['argmax_point'], want['argmax_face_of_b'], want['n_samples'], want['n_beyond'])
    slack = want['n_samples'] * 2.0 ** -52 * max(want['max'], 1e-300) if math.isfinite(want['max']) else 1e-9
    assert abs(got.mean - want['mean']) <= slack and abs(got.rms - want['rms']) <= slack, (got.mean, want['mean'], got.rms, want['rms'])


def test_surface_samples_equal_the_restatement():
    from perf_amd.mesh import surface_samples
    mesh, (vertices, faces) = _ball()
    for order in (1, 2, 3):
        points, face = surface_samples(mesh, order)
        want = N.surface_samples(vertices, faces, order)
        assert np.array_equal(_bits(points), _bits(want[0])) and np.array_equal(face.cpu().numpy(), want[1]) and face.dtype == torch.int32
    assert len(surface_samples(mesh, 1)[0]) == len(vertices) and len(surface_samples(mesh, 2)[0]) == len(vertices) + 3 * len(faces)
    bad = _mesh(*M.SMALL)                                            # the samples of a face with an index outside [0, V) are NaN, not a fault
    points, face = surface_samples(bad, 2)
    assert torch.isnan(points[7 + 3:7 + 6]).all() and not torch.isnan(points[7 + 6:]).any()


def test_mesh_deviation_equals_the_restatements_statistics():
    from perf_amd.mesh import mesh_deviation, simplify_mesh
    mesh, ball = _ball()
    same = mesh_deviation(mesh, mesh, order=1)
    assert same.max == 0.0 and same.mean == 0.0 and same.n_beyond == 0 and same.n_samples == len(ball[0])          # exactly
    small = simplify_mesh(mesh, 0.25, placement='quadric')[0]
    assert 0 < len(small.faces) < len(ball[1]) // 2
    want = N.deviation(_host(small), ball)
    got = mesh_deviation(small, mesh)
    _same_deviation(got, want)
    _same_deviation(got.a_to_b, want['a_to_b'])
    _same_deviation(got.b_to_a, want['b_to_a'])
    assert got.max == max(got.a_to_b.max, got.b_to_a.max) and 0.0 < got.max < 0.25 * math.sqrt(3) and got.mean <= got.rms <= got.max and got.p90 <= got.max
    one_way = mesh_deviation(small, mesh, order=3, symmetric=False, cell=0.2)
    _same_deviation(one_way, N.deviation(_host(small), ball, order=3, symmetric=False))
    assert one_way.a_to_b is None
    # samples beyond the limit are counted and make max +inf: they are not dropped from it
    limit = float(np.float32(want['b_to_a']['p90']))
    cut = mesh_deviation(small, mesh, max_distance=limit)
    _same_deviation(cut.b_to_a, N.deviation(ball, _host(small), symmetric=False, max_distance=limit))
    assert cut.max == math.inf and 0 < cut.b_to_a.n_beyond < cut.b_to_a.n_samples // 5 and cut.b_to_a.argmax_face_of_b == -1


def test_simplify_to_tolerance_returns_the_first_cell_of_the_ladder_within_the_tolerance():
    """The tolerance is one lattice spacing of the ball (0.1).  The ladder starts at 16 median edge lengths, more than the ball's diameter: that
    cell leaves at most 8 vertices and cannot pass; whichever cell is returned, its reported deviation is within the tolerance and is the
    restatement's, and the ladder's next coarser cell, simplified again here, is beyond it by the restatement's own measure."""
    from perf_amd.mesh import median_edge_length, simplify_mesh, simplify_to_tolerance, tolerance_ladder
    mesh, ball = _ball()
    tol = M.BALL_SPACING
    ladder = tolerance_ladder(mesh)
    corners = ball[0][ball[1]].astype(np.float64)
    edges = np.sort(np.linalg.norm(corners - np.roll(corners, -1, axis=1), axis=2).reshape(-1))
    assert abs(median_edge_length(mesh) - edges[(len(edges) - 1) // 2]) <= 1e-12
    assert len(ladder) == 10 and ladder[0] == 16 * median_edge_length(mesh) > 2 * M.BALL_RADIUS
    assert all(abs(b / a - math.sqrt(0.5)) < 1e-12 for a, b in zip(ladder, ladder[1:]))
    small, cell, deviation = simplify_to_tolerance(mesh, tol)
    k = ladder.index(cell)
    assert k > 0 and deviation.max <= tol and len(small.faces) < len(ball[1])
    _same_deviation(deviation, N.deviation(_host(small), ball))
    again = simplify_mesh(mesh, cell, placement='quadric')[0]
    assert torch.equal(again.vertices.view(torch.int32), small.vertices.view(torch.int32)) and torch.equal(again.faces, small.faces)
    coarser = simplify_mesh(mesh, ladder[k - 1], placement='quadric')[0]
    assert N.deviation(_host(coarser), ball)['max'] > tol
    # cells given by hand are scanned in their order, and when none passes the finest comes back with a warning
    with pytest.warns(RuntimeWarning, match='no cell'):
        _, cell, deviation = simplify_to_tolerance(mesh, 1e-6, cells=[ladder[0], ladder[1]], placement='mean')
    assert cell == ladder[1] and deviation.max > 1e-6


def test_transfer_vertex_values_reproduces_a_linear_function_of_position():
    """g(x) = w . x + c at the closest points.  The transfer forms ((1 - u - v) g_a + u g_b) + v g_c from the fp32 values g_a, g_b, g_c of the
    face's vertices; for a linear g that is g(q) at q = (1 - u - v) a + u b + v c, up to the rounding of the three values to fp32 (2^-24 G
    each, G the largest |g| at a vertex, the weights being non-negative and summing to 1) and of the result to fp32 (2^-24 G again); the
    float64 operations add 2^-50 G.  Bound: 2 * 2^-24 * G * (1 + 2^-20)."""
    from perf_amd.mesh import build_ray_grid, closest_point, transfer_vertex_values
    mesh, (vertices, faces) = _ball()
    w, c = np.array([[0.5, -1.25, 2.0], [3.0, 0.75, -0.5]]), np.array([0.25, -1.0])
    g = lambda x: x.astype(np.float64) @ w.T + c
    values = g(vertices).astype(np.float32)
    points = N.sphere_points()[:4096:4]          # (a quarter of them well inside the ball, the others all over the box and beyond it)
    hits = closest_point(mesh, build_ray_grid(mesh), _dev(points))
    got = transfer_vertex_values(mesh, _dev(values), hits)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1024, 2)
    face, u, v = hits.face.cpu().numpy(), hits.u.cpu().numpy().astype(np.float64)[:, None], hits.v.cpu().numpy().astype(np.float64)[:, None]
    assert (face >= 0).all()
    a, b, cc = (vertices[faces[face, k]].astype(np.float64) for k in range(3))
    q = ((1.0 - u) - v) * a + u * b + v * cc
    bound = 2 * 2.0 ** -24 * np.abs(values).max() * (1 + 2.0 ** -20)
    assert np.abs(got.cpu().numpy().astype(np.float64) - g(q)).max() <= bound
    # the closest points are where the restatement puts them, and a point without an answer carries NaN
    _same(hits, N.closest(vertices, faces, points))
    cut = closest_point(mesh, build_ray_grid(mesh), _dev(points), 0.05)
    out = transfer_vertex_values(mesh, _dev(values), cut)
    assert torch.equal(torch.isnan(out).all(dim=1), cut.face < 0) and (cut.face < 0).any() and (cut.face >= 0).any()
