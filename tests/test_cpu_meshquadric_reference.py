"""The numpy restatement of the quadric error placement (tests/meshquadric_reference.py, the yardstick of tests/test_gpu_meshquadric.py)
pinned without a GPU: against an independently written one (loops over the faces, Python integers for the sums, Python floats for the
arithmetic), its solve against np.linalg.solve of the un-quantised system within a bound derived from each cluster's own numbers, and the
properties the rule is built for on a tessellated box and on dyadic planes, where the 'mean' placement is shown to be told apart."""
import math

import numpy as np

from tests import meshquadric_reference as Q

EPS = 2.0 ** -52
# What the solve itself may lose, in cell units, relative to max(1, |x|): M = A + lambda I has a condition number up to 3 * 2^10 + 1 (the
# largest eigenvalue is at most tr, the smallest at least lambda = tr 2^-10); cofactors and determinant are a dozen operations of double:
# 2^12 (condition) * 64 (ulps) * 2^-52.
SOLVE_SLACK = 2.0 ** 18 * EPS


def _wrap(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def _cell_loop(x, lo, h, n):
    t = (float(x) - float(lo)) / float(h)
    t = min(max(t, 0.0), float(n))
    i = min(int(math.floor(t)), n - 1)
    return i, t - float(i)


def _round_half_even(x):
    return int(round(x))          # (Python's round of a float: ties to even, exact for |x| < 2^63)


def loop_sums(vertices, faces, lo, h, n, vertex_cluster, C):
    """Stage A written apart from the restatement: one face at a time, Python floats (IEEE doubles) and Python integers."""
    v = [[float(c) for c in row] for row in np.asarray(vertices, dtype=np.float32).reshape(-1, 3)]
    lo = [float(np.float32(c)) for c in lo]
    h = float(np.float32(h))
    acc = [[0] * 9 for _ in range(C)]
    bad = skipped = -1
    for index, face in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if any(k < 0 or k >= len(v) for k in face):
            bad = index if bad < 0 else bad
            continue
        cl = [int(vertex_cluster[k]) for k in face]
        if any(c < 0 or c >= C for c in cl):
            continue
        a, b, c = (v[k] for k in face)
        try:
            e1 = [(b[i] - a[i]) / h for i in range(3)]
            e2 = [(c[i] - a[i]) / h for i in range(3)]
            nrm = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            scaled = [(nrm[i] * nrm[j]) * Q.SCALE for i, j in Q.PAIRS]
        except OverflowError:
            scaled = [math.inf]
        if not all(abs(s) < Q.SKIP for s in scaled):
            skipped = index if skipped < 0 else skipped
            continue
        qa = [_round_half_even(s) for s in scaled]
        for k, vertex in enumerate(face):
            r = [_cell_loop(v[vertex][i], lo[i], h, n[i])[1] - 0.5 for i in range(3)]
            d = (nrm[0] * r[0] + nrm[1] * r[1]) + nrm[2] * r[2]
            row = qa + [_round_half_even((nrm[i] * d) * Q.SCALE) for i in range(3)]
            acc[cl[k]] = [x + y for x, y in zip(acc[cl[k]], row)]
    return np.array([[_wrap(x) for x in row] for row in acc], dtype=np.int64).reshape(C, 9), bad, skipped


def _random_mesh(V, F, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    vertices = (rng.random((V, 3)) * spread).astype(np.float32)
    base = rng.integers(0, V, F)
    faces = np.stack([base, (base + rng.integers(1, 6, F)) % V, (base + rng.integers(6, 12, F)) % V], axis=1).astype(np.int32)
    return vertices, faces


def _local_mesh(V, F, seed):
    """Faces about a cell wide: vertices along a jittered sheet, each face of three neighbours in the vertex order."""
    rng = np.random.default_rng(seed)
    u = np.arange(V) / V
    vertices = np.stack([u, 0.5 + 0.3 * np.sin(7 * u), 0.5 + 0.3 * np.cos(5 * u)], axis=1) + rng.normal(0, 0.02, (V, 3))
    base = rng.integers(0, V - 12, F)
    faces = np.stack([base, base + rng.integers(1, 6, F), base + rng.integers(6, 12, F)], axis=1)
    return vertices.astype(np.float32), faces.astype(np.int32)


GRID = (np.array([0.0, 0.0, 0.0], np.float32), np.float32(0.125), [8, 8, 8])


def test_the_restatement_agrees_with_loops_over_the_faces():
    for vertices, faces in (_random_mesh(200, 700, 1), _local_mesh(400, 900, 2), Q.box_mesh()[:1] + (Q.box_mesh()[1][::37],)):
        grid = Q.BOX_GRID if len(vertices) > 1000 else GRID
        faces = faces.copy()
        faces[5, 1], faces[3, 2] = len(vertices), -1          # two faces that are not followed
        vertices = vertices.copy()
        vertices[7, 0] = np.nan                               # a vertex that joins nothing
        vc, C, anchor, rep = Q.labelled(vertices, *grid)
        acc, bad, skipped = Q.sums(vertices, faces, *grid, vc, C)
        acc2, bad2, skipped2 = loop_sums(vertices, faces, *grid, vc, C)
        assert bad == bad2 == 3 and skipped == skipped2 == -1
        assert np.array_equal(acc, acc2) and np.abs(acc).sum() > 0


def test_the_skip_rule_and_the_ties_agree_with_the_loops():
    # a face of 32 x 32 cells sits exactly on 2^60 (skipped), one a fraction of a cell smaller is summed; products of 2^-41 are ties
    h = np.float32(1 / 64)
    vertices = np.array([[0, 0, 0], [32 / 64, 0, 0], [0, 32 / 64, 0], [0, (32 - 2.0 ** -10) / 64, 0], [64, 0, 0], [0, 64, 0.25]], dtype=np.float32)
    faces = np.array([[0, 1, 3], [0, 1, 2], [0, 4, 5]], dtype=np.int32)
    grid = (np.zeros(3, np.float32), h, [4096, 4096, 1])
    vc, C, _, _ = Q.labelled(vertices, *grid)
    acc, bad, skipped = Q.sums(vertices, faces, *grid, vc, C)
    acc2, bad2, skipped2 = loop_sums(vertices, faces, *grid, vc, C)
    assert (bad, skipped) == (bad2, skipped2) == (-1, 1) and np.array_equal(acc, acc2)
    _, scaled, fits, _ = Q.face_terms(vertices, faces, *grid)
    assert fits.tolist() == [True, False, False] and scaled[1, 5] == 2.0 ** 60 and 2.0 ** 59 < scaled[0, 5] < 2.0 ** 60
    vertices, faces = ties_mesh()
    grid = (np.zeros(3, np.float32), np.float32(1.0), [1, 1, 1])
    _, scaled, fits, q = Q.face_terms(vertices, faces, *grid)
    half = np.abs(scaled - np.trunc(scaled)) == 0.5
    assert fits.all() and (half & (scaled > 0)).any() and (half & (scaled < 0)).any()
    assert np.array_equal(q[:, 0, :6][half] % 2, np.zeros(half.sum(), dtype=np.int64))          # ties went to even
    vc, C, _, _ = Q.labelled(vertices, *grid)
    assert np.array_equal(Q.sums(vertices, faces, *grid, vc, C)[0], loop_sums(vertices, faces, *grid, vc, C)[0])


def ties_mesh():
    """Faces with the normal (2^-20, +-k 2^-21, 0), k odd: n_x n_y * 2^40 = +-k / 2, a tie of either sign."""
    s = 2.0 ** -10
    vertices, faces = [], []
    for k in (1, 3, 5, 7, -1, -3, -5, -7):
        a = np.array([0.5, 0.5, 0.5])
        base = len(vertices)
        vertices += [a, a + [0, 0, s], a + [k * 2.0 ** -11, -s, 0]]          # e1 = (0, 0, s), e2 = (k 2^-11, -s, 0): n = (s^2, k 2^-21, 0)
        faces.append([base, base + 1, base + 2])
    return np.array(vertices, dtype=np.float32), np.array(faces, dtype=np.int32)


def test_the_solve_agrees_with_linalg_solve_of_the_unquantised_system():
    checked = 0
    for vertices, faces, grid in ((*_local_mesh(3000, 9000, 3), GRID), (*_local_mesh(500, 4000, 4), GRID), (*Q.box_mesh(), Q.BOX_GRID)):
        out, acc, _, _, info, (vc, C, anchor, rep) = Q.placement(vertices, faces, *grid)
        nrm, _, fits, _ = Q.face_terms(vertices, faces, *grid)
        v64 = vertices.astype(np.float64)
        A, b, terms = np.zeros((C, 3, 3)), np.zeros((C, 3)), np.zeros(C)
        for k in range(3):          # the same sums, never quantised
            _, frac = Q.fractions(v64[faces[:, k]], *grid)
            d = np.einsum('fi,fi->f', nrm, frac - 0.5)
            np.add.at(A, vc[faces[fits, k]], np.einsum('fi,fj->fij', nrm, nrm)[fits])
            np.add.at(b, vc[faces[fits, k]], (nrm * d[:, None])[fits])
            np.add.at(terms, vc[faces[fits, k]], 1.0)
        for c in np.nonzero(info['solved'])[0]:
            lam = np.trace(A[c]) * Q.REGULARISER
            x = np.linalg.solve(A[c] + lam * np.eye(3), b[c] + lam * info['m'][c])
            # every entry of A and b is a sum of N roundings of at most 2^-41 each: |dA|_F, |db| <= 3 N 2^-41; lambda moves by the
            # trace's part of that times 2^-10, in M and in g; the smallest eigenvalue of M is at least lambda
            dA = 3 * terms[c] * 2.0 ** -41 * (1 + Q.REGULARISER)
            db = 3 * terms[c] * 2.0 ** -41 * (1 + Q.REGULARISER * np.linalg.norm(info['m'][c]))
            bound = (dA * np.linalg.norm(x) + db) / lam + SOLVE_SLACK * max(1.0, np.linalg.norm(x))
            assert np.linalg.norm(info['x'][c] - x) <= bound, (c, info['x'][c], x, bound)
            checked += 1
    assert checked > 300          # (the three meshes have some 400 clusters with a face: the loop is not empty)


def test_the_box_keeps_its_corners_and_the_mean_does_not():
    vertices, faces = Q.box_mesh()
    lo, h, n = Q.BOX_GRID
    out, acc, bad, skipped, info, (vc, C, anchor, rep) = Q.placement(vertices, faces, lo, h, n)
    assert (bad, skipped) == (-1, -1) and info['solved'].all() and info['clamped'] == 0
    lo64, h64 = lo.astype(np.float64), float(h)
    worst_bound = 0.0
    for corner in Q.box_corners():
        c = int(vc[np.argmin(np.abs(vertices.astype(np.float64) - corner).sum(axis=1))])          # the cluster of the corner's own vertex
        star = (corner - lo64) / h64 - info['centre'][c]                    # the corner in the cell's centred coordinates: (+-0.25) x 3
        assert np.abs(star).max() == 0.25
        A = info['M'][c] - info['lam'][c] * np.eye(3)
        sigma = np.linalg.eigvalsh(A)[0]
        assert sigma > 0                                                      # three planes meet in this cell
        lam = info['lam'][c]
        # x - x* = lambda (A + lambda I)^-1 (m - x*), since A x* = b exactly (every face of the cluster passes through x*)
        bound = lam / (sigma + lam) * np.linalg.norm(info['m'][c] - star) + SOLVE_SLACK
        assert np.linalg.norm(info['x'][c] - star) <= bound, (corner, info['x'][c], star, bound)
        # the fp32 vertex: half an ulp of fp32 at a coordinate below 1/2 on top
        assert np.linalg.norm(out[c].astype(np.float64) - corner) <= bound * h64 + math.sqrt(3) * 2.0 ** -26
        # the mean is told apart: it misses the corner by more than ten times what the quadric is allowed
        assert np.linalg.norm(anchor[c].astype(np.float64) - corner) > 10 * bound * h64
        worst_bound = max(worst_bound, bound)
    assert worst_bound < 0.01                                                 # (cells: the bound is not vacuous)
    # every vertex lies on the box's surface (the largest distance of a vertex's outermost coordinate to it, in cells) within the
    # corners' bound; the mean of an edge cell, whose two strips are a quarter and three quarters of a cell wide, lies a twelfth of a
    # cell inside the box
    def off_surface(p):
        q = np.abs(p.astype(np.float64))
        return np.abs(q.max(axis=1) - Q.BOX_HALF).max() / h64
    # (a plane that holds a share s of a cluster's trace is missed by at most 2^-10 / (s + 2^-10) |m - x*|; no share here is below 1/10)
    assert off_surface(out) < 0.01 < 0.08 < off_surface(anchor)


def test_on_a_dyadic_plane_the_vertex_is_the_mean_on_the_plane():
    grid = (np.zeros(3, np.float32), np.float32(0.125), [8, 8, 8])
    flat = Q.join([Q.patch((1 / 64, 1 / 64, 0.40625), (1 / 64, 0, 0), (0, 1 / 64, 0), 60, 60)])          # z = 13/32
    oblique = Q.join([Q.patch((1 / 64, 1 / 64, 1 / 64), (1 / 64, 0, 1 / 64), (0, 1 / 64, 0), 40, 60)])    # z = x
    for (vertices, faces), normal in ((flat, (0.0, 0.0, 1.0)), (oblique, (-1.0, 0.0, 1.0))):
        out, acc, bad, skipped, info, (vc, C, anchor, rep) = Q.placement(vertices, faces, *grid)
        assert info['solved'].all() and C > 30
        nrm = np.asarray(normal) / np.linalg.norm(normal)
        # the members lie on the plane, so their mean does (to the 2^-32 of the mean's fixed point), b = A m' for any m' on the plane,
        # and the minimiser of the regularised quadric is m itself: on the plane, with the mean's in-plane coordinates
        gap = np.abs(info['x'] - info['m']).max()
        assert gap <= 3 * 2.0 ** -32 + SOLVE_SLACK, gap
        assert np.abs((info['x'] - info['m']) @ nrm).max() <= 3 * 2.0 ** -32 + SOLVE_SLACK
        assert np.abs(out.astype(np.float64) - anchor.astype(np.float64)).max() <= 2.0 ** -24          # an ulp of fp32 below 1
    # two such planes that meet inside a row of cells: a ridge z = |x - 17/32| + 5/32, the line at fractions (0.25, 0.25) of its cells.
    # The planes are orthogonal and share the cell 3 : 1, so the smaller eigenvalue of A in their span is tr / 4 and the vertex is
    # within lambda / (tr / 4 + lambda) |m - x*| < 0.004 cells of the line; the mean of such a cell lies on neither plane
    rx, rz = 17 / 32, 5 / 32
    ridge = Q.join([Q.patch((rx, 1 / 64, rz), (1 / 64, 0, 1 / 64), (0, 1 / 64, 0), 24, 60), Q.patch((rx, 1 / 64, rz), (0, 1 / 64, 0), (-1 / 64, 0, 1 / 64), 60, 24)])
    out, acc, bad, skipped, info, (vc, C, anchor, rep) = Q.placement(*ridge, *grid)
    on_ridge = np.unique(vc[ridge[0][:, 0] == np.float32(rx)])
    assert len(on_ridge) == 8
    dist = lambda p: np.hypot(p[:, 0].astype(np.float64) - rx, p[:, 2].astype(np.float64) - rz)
    assert dist(out[on_ridge]).max() < 0.004 * 0.125 < 0.1 * 0.125 < dist(anchor[on_ridge]).min()


def test_empty_and_degenerate_inputs():
    grid = GRID
    vertices = np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.6, 0.6, 0.6], [0.9, 0.9, 0.9]], dtype=np.float32)
    for faces in (np.zeros((0, 3), np.int32), np.array([[0, 0, 1], [1, 1, 1]], np.int32)):          # no faces; faces without area
        out, acc, bad, skipped, info, (vc, C, anchor, rep) = Q.placement(vertices, faces, *grid)
        assert C == 4 and not acc.any() and not info['solved'].any() and np.array_equal(out.view(np.int32), anchor.view(np.int32))
    out, acc, bad, skipped, info, lab = Q.placement(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), *grid)
    assert out.shape == (0, 3) and acc.shape == (0, 9) and (bad, skipped) == (-1, -1)
