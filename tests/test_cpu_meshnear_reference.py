"""The float64 restatement of include/staged/perf_hip_meshnear.h (tests/meshnear_reference.py) pinned without a GPU: the hand-computed
answers in each of the seven regions and on their boundaries, the degenerate faces, vertices as queries, and about 2,000 random
point-triangle pairs against an independent formulation in longdouble, to the bound meshnear_reference.dist2_bound derives."""
import numpy as np

from tests import meshnear_reference as N
from tests import meshray_reference as M


def _one(face, p):
    got = N.closest(np.array(face, dtype=np.float32), [[0, 1, 2]], [p])
    return float(got[0][0]), int(got[1][0]), float(got[2][0]), float(got[3][0])


def test_hand_points_in_every_region_and_on_their_boundaries():
    vertices, faces = N.TRIANGLE
    regions = set()
    for p, want in N.HAND_POINTS:
        got = N.closest(vertices, faces, [p])
        assert (float(got[0][0]), float(got[2][0]), float(got[3][0])) == want and got[1][0] == 0, (p, got)
        assert abs(N.independent_dist2(p, *vertices) - want[0]) <= 1e-15, p
        a, b, c = (vertices[k].astype(np.float64) for k in range(3))
        regions.add(int(N.rule(np.array(p, dtype=np.float64), a, b, c)[3]))
    assert regions == {0, 1, 2, 4, 5, 6, 7}
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32 and got[2].dtype == got[3].dtype == np.float32


def test_degenerate_faces_are_answered_by_their_vertices_and_edges():
    for face, cases in N.DEGENERATE:
        for p, want in cases:
            dist2, index, u, v = _one(face, p)
            assert (dist2, u, v) == want and index == 0, (face, p, dist2, u, v)
            assert abs(N.independent_dist2(p, *face) - dist2) <= 1e-15, (face, p)
    # nothing is divided by zero: every value of the restatement is finite on them, and the same faces in one mesh give the same answers
    vertices, faces, points = N.degenerate_mesh()
    got = N.closest(vertices, faces, points)
    assert np.isfinite(got[0]).all() and (got[1] >= 0).all()
    for n, p in enumerate(points):
        assert got[0][n] == min(_one(vertices[3 * k:3 * k + 3], p)[0] for k in range(len(faces)))


def test_random_pairs_against_the_independent_formulation():
    rng = np.random.default_rng(17)
    checked, regions, worst = 0, np.zeros(9, dtype=np.int64), 0.0
    while checked < 2000:
        a, b, c = rng.uniform(-1, 1, size=(3, 3)).astype(np.float32)
        ab, ac, bc = (b - a).astype(np.float64), (c - a).astype(np.float64), (c - b).astype(np.float64)
        longest2 = max(ab @ ab, ac @ ac, bc @ bc)
        n = np.cross(ab, ac)
        if n @ n < 2.0 ** -6 * longest2 * longest2:          # (the bound is derived for such triangles; the slivers are the degenerate cases' business)
            continue
        # a point of the face's plane pushed out of it, a point near an edge, or anywhere in the box
        kind = checked % 3
        if kind == 0:
            w = rng.dirichlet(np.ones(3))
            p = w[0] * a + w[1] * b + w[2] * c + rng.normal() * 0.3 * n / np.sqrt(n @ n)
        elif kind == 1:
            t = rng.uniform(-0.2, 1.2)
            p = a + t * ab + rng.normal(size=3) * 0.05
        else:
            p = rng.uniform(-2, 2, size=3)
        p = p.astype(np.float32)
        dist2, u, v, region = N.rule(p.astype(np.float64), a.astype(np.float64), b.astype(np.float64), c.astype(np.float64))
        want, bound = N.independent_dist2(p, a, b, c), N.dist2_bound(p, a, b, c)
        assert abs(float(dist2) - want) <= bound, (a, b, c, p, float(dist2), want, bound)
        assert 0.0 <= u <= 1.0 and 0.0 <= v <= 1.0 and u + v <= 1.0 + 2.0 ** -52
        worst = max(worst, abs(float(dist2) - want) / bound)
        regions[int(region)] += 1
        checked += 1
    assert (regions[[0, 1, 2, 4, 5, 6, 7]] >= 20).all(), regions          # every region is met
    assert worst < 1.0


def test_vertices_as_queries_give_zero_exactly():
    for vertices, faces in (M.random_triangles(), N.TETRAHEDRON):
        vertices, faces = vertices[:600], faces[:200] if len(faces) > 4 else faces
        got = N.closest(vertices, faces, vertices)
        assert (got[0] == 0.0).all() and (got[1] >= 0).all()
    # also where b - a is not exact in double: the vertex test comes first
    face = np.array([[1e10, 1, 0], [1e-10, 0, 0], [0, 1e-10, 0]], dtype=np.float32)
    for k in range(3):
        dist2, index, u, v = _one(face, face[k])
        assert dist2 == 0.0 and (u, v) == ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))[k]


def test_the_minimum_is_over_dist2_then_the_face_index():
    vertices, faces = N.TETRAHEDRON
    got = N.closest(vertices, faces, N.TETRAHEDRON_POINTS)
    assert got[0][0] == 0.0 and got[1][0] == 0 and (float(got[2][0]), float(got[3][0])) == (0.0, 0.5)          # the shared edge 0-1: face 0 before face 1
    alone = N.closest(vertices, faces[1:2], N.TETRAHEDRON_POINTS[:1])
    assert alone[0][0] == 0.0 and (float(alone[2][0]), float(alone[3][0])) == (0.5, 0.0)                       # face 1 ties exactly
    # faces that are never the answer, points that are not finite, the limit
    got = N.closest(*M.SMALL, N.EDGE_POINTS)
    assert not np.isin(got[1], (0, 1)).any() and got[1][1:4].tolist() == [-1, -1, -1] and np.isinf(got[0][1:4]).all()
    assert got[1][4] == 2 and got[0][4] == 0.25          # between the sheets: the coincident faces 2 and 3 and the face 4 tie; the smallest index
    cut = N.closest(*M.SMALL, N.EDGE_POINTS, max_distance=0.5)
    assert cut[1].tolist() == [-1, -1, -1, -1, 2, 2, 4, -1, -1, 2] and cut[0][6] == 0.25          # dist2 == max^2 is within
    none = N.closest(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), N.EDGE_POINTS)
    assert (none[1] == -1).all() and np.isinf(none[0]).all() and not none[2].any() and not none[3].any()


def test_surface_samples_and_statistics():
    vertices, faces = N.TRIANGLE
    points, face = N.surface_samples(vertices, faces, 1)
    assert np.array_equal(points, vertices) and face.tolist() == [-1, -1, -1]
    points, face = N.surface_samples(vertices, faces, 2)
    assert points[3:].tolist() == [[0, 2, 1], [2, 0, 1], [2, 2, 1]] and face.tolist() == [-1, -1, -1, 0, 0, 0]          # (1,0,1) ac, (1,1,0) ab, (0,1,1) bc
    assert len(N.surface_samples(vertices, faces, 3)[0]) == 3 + 7 and len(N.surface_samples(*N.TETRAHEDRON, 4)[0]) == 4 + 4 * 12
    same = N.deviation(N.TETRAHEDRON, N.TETRAHEDRON, order=1)
    assert same['max'] == 0.0 and same['n_beyond'] == 0 and same['n_samples'] == 4
    assert N.deviation(N.TETRAHEDRON, N.TETRAHEDRON, order=3)['max'] <= 2.0 ** -24          # (the inner samples are rounded to fp32: half an ulp of 1 off the face)
    lifted = (vertices + np.array([0, 0, 0.5], np.float32), faces)
    d = N.deviation(lifted, N.TRIANGLE)
    assert (d['max'], d['mean'], d['rms'], d['p90'], d['n_samples'], d['argmax_face_of_b']) == (0.5, 0.5, 0.5, 0.5, 6, 0) and d['argmax_point'] == (0.0, 0.0, 1.5)
    d = N.deviation(lifted, N.TRIANGLE, max_distance=0.25)
    assert d['max'] == np.inf and d['n_beyond'] == 6 and d['argmax_face_of_b'] == -1
