"""The closest point of a triangle mesh as include/staged/perf_hip_meshnear.h states it, in numpy float64: the per-face rule operation for
operation in the header's order (numpy does not contract), the answer by BRUTE FORCE over all faces with the (dist2, face index) minimum,
the surface samples and the deviation statistics of perf_amd/mesh.py.  The yardstick of tests/test_cpu_meshnear_reference.py and
tests/test_gpu_meshnear.py, written from the statement, not from the kernel.  Also the inputs both files use."""
import functools
import math

import numpy as np

from tests import meshray_reference as M
from tests import meshvis_reference as V

_CHUNK = 128                             # points per block of the brute force


def _f64(x, shape):
    return np.asarray(x, dtype=np.float32).astype(np.float64).reshape(shape)


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def rule(p, a, b, c):
    """The header's lines, each operation rounded once.  p, a, b, c: sequences of three float64 arrays (x, y, z) that broadcast ->
    (dist2, u, v, region) float64 and int8; region: 0, 1, 2 the vertices a, b, c; 4, 5, 6 the edges ab, ac, bc; 7 the interior."""
    with np.errstate(all='ignore'):
        ab, ac = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
        ap, bp, cp = [p[k] - a[k] for k in range(3)], [p[k] - b[k] for k in range(3)], [p[k] - c[k] for k in range(3)]
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va, e, g = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4, d4 - d3, d5 - d6
        at = [(x[0] == 0) & (x[1] == 0) & (x[2] == 0) for x in (ap, bp, cp)]
        ra, rb, rc = _dot(ap, ap), _dot(bp, bp), _dot(cp, cp)
        nearest = np.where(rc < np.minimum(ra, rb), 2, np.where(rb < ra, 1, 0))          # 8: the first of equals
        region = np.select(
            [at[0], at[1], at[2],                                                       # 0
             (d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6),       # 1, 2, 3
             (vc <= 0) & (d1 >= 0) & (d3 <= 0) & ((d1 - d3) > 0),                        # 4
             (vb <= 0) & (d2 >= 0) & (d6 <= 0) & ((d2 - d6) > 0),                        # 5
             (va <= 0) & (e >= 0) & (g >= 0) & ((e + g) > 0),                            # 6
             (va > 0) & (vb > 0) & (vc > 0)],                                           # 7
            [0, 1, 2, 0, 1, 2, 4, 5, 6, 7], default=-1)
        region = np.where(region < 0, nearest, region)
        den = (va + vb) + vc
        v6 = e / (e + g)
        u = np.select([region == 1, region == 4, region == 6, region == 7], [1.0, d1 / (d1 - d3), 1.0 - v6, vb / den], default=0.0)
        v = np.select([region == 2, region == 5, region == 6, region == 7], [1.0, d2 / (d2 - d6), v6, vc / den], default=0.0)
        r = [np.select([region == 0, region == 1, region == 2], [ap[k], bp[k], cp[k]], default=p[k] - ((a[k] + u * ab[k]) + v * ac[k])) for k in range(3)]
        dist2 = _dot(r, r)
    return dist2, u, v, region.astype(np.int8)


def closest(vertices, faces, points, max_distance=np.inf):
    """The answer for N points over ALL valid faces: the lexicographic minimum of (dist2, face index) -> (dist2 float64 [N], face int32 [N],
    u float32 [N], v float32 [N]); +inf, -1, 0, 0 for a point that is not finite, without a valid face, and beyond max_distance."""
    vt = _f64(vertices, (-1, 3))
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    index = np.nonzero(M.valid_faces(vertices, faces))[0]
    f = f[index]
    pt = _f64(points, (-1, 3))
    n = len(pt)
    dist2_out, face_out = np.full(n, np.inf, np.float64), np.full(n, -1, np.int32)
    u_out, v_out = np.zeros(n, np.float32), np.zeros(n, np.float32)
    finite = np.isfinite(pt).all(axis=1)
    if len(f) and finite.any():
        a, b, c = ([vt[f[:, corner], k][None] for k in range(3)] for corner in range(3))
        rows_all = np.nonzero(finite)[0]
        for first in range(0, len(rows_all), _CHUNK):
            rows = rows_all[first:first + _CHUNK]
            dist2, u, v, _ = rule([pt[rows, k][:, None] for k in range(3)], a, b, c)
            best = np.argmin(dist2, axis=1)                  # (the first of equal minima: the smallest face index)
            r = np.arange(len(rows))
            dist2_out[rows], face_out[rows] = dist2[r, best], index[best].astype(np.int32)
            u_out[rows], v_out[rows] = u[r, best].astype(np.float32), v[r, best].astype(np.float32)
    return limited((dist2_out, face_out, u_out, v_out), max_distance)


def limited(answer, max_distance):
    """The answer with everything beyond (double)max_distance^2 replaced by +inf, -1, 0, 0 (max_distance as the fp32 the library takes)."""
    dist2, face, u, v = answer
    limit = float(np.float32(max_distance))
    with np.errstate(over='ignore'):
        keep = (face >= 0) & (dist2 <= limit * limit)
    return np.where(keep, dist2, np.inf), np.where(keep, face, -1).astype(np.int32), np.where(keep, u, 0).astype(np.float32), np.where(keep, v, 0).astype(np.float32)


def independent_dist2(p, a, b, c):
    """The squared distance of ONE point to ONE triangle by another formulation, in longdouble: the minimum over the interior projection
    (when it falls inside) and the three edge projections clamped to [0, 1].  Not the header's rule: no regions, no order of tests."""
    L = np.longdouble
    p, a, b, c = (np.asarray(x, dtype=np.float32).astype(L) for x in (p, a, b, c))
    best = L(np.inf)
    for x, y in ((a, b), (b, c), (c, a)):
        d = y - x
        dd = d @ d
        t = min(max((p - x) @ d / dd, L(0)), L(1)) if dd > 0 else L(0)
        r = p - (x + t * d)
        best = min(best, r @ r)
    ab, ac, ap = b - a, c - a, p - a
    n = np.cross(ab, ac)
    nn = n @ n
    if nn > 0:
        u, v = np.cross(ap, ac) @ n / nn, np.cross(ab, ap) @ n / nn
        if u >= 0 and v >= 0 and u + v <= 1:
            h = n @ ap
            best = min(best, h * h / nn)
    return float(best)


def dist2_bound(p, a, b, c):
    """|rule's dist2 - the true one| for a triangle whose |ab x ac|^2 is at least 2^-6 of its longest edge to the fourth.  T: the largest
    of the coordinates' magnitudes and of the distances from p to the vertices; u = 2^-53.  The closest point q is formed as
    (a + u ab) + v ac with six roundings per coordinate, each at most u T (ab and ac, the two products, the two sums), and r = p - q adds
    one: |dr| <= 7 sqrt(3) u T.  An error of u and v moves q INSIDE the face's plane or edge, where dist2 is stationary: it enters
    squared, and for such a triangle it is below 2^12 u T, so its square is far below u T^2; a point classified into the neighbouring
    region meets the same continuity.  dist2 = |r|^2 then errs by 2 |r| |dr| + 3 u |r|^2 <= (14 sqrt(3) + 3) u T^2 < 28 u T^2; stated
    with room as 32 * 2^-52 * T^2."""
    pts = np.asarray([p, a, b, c], dtype=np.float64)
    t = max(np.abs(pts).max(), np.sqrt(((pts[1:] - pts[0]) ** 2).sum(axis=1)).max())
    return 32 * 2.0 ** -52 * t * t


def surface_samples(vertices, faces, order=2):
    """perf_amd.mesh.surface_samples: the vertices with face -1, then per face the lattice points (i, j, k) / order that are not corners,
    j ascending, then k, each ((i a + j b) + k c) / order in float64 rounded once -> (points float32 [M, 3], face int32 [M])."""
    vt = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lattice = [(order - j - k, j, k) for j in range(order + 1) for k in range(order + 1 - j) if order not in (order - j - k, j, k)]
    if not lattice or not len(f) or not len(vt):
        return vt.copy(), np.full(len(vt), -1, np.int32)
    a, b, c = (vt[f[:, corner]].astype(np.float64) for corner in range(3))
    inner = np.stack([((i * a + j * b) + k * c) / order for i, j, k in lattice], axis=1).astype(np.float32).reshape(-1, 3)
    return np.concatenate([vt, inner]), np.concatenate([np.full(len(vt), -1, np.int32), np.repeat(np.arange(len(f), dtype=np.int32), len(lattice))])


def statistics(points, answer):
    """The fields of perf_amd.mesh.Deviation of one direction, from the samples and their answers."""
    dist2, face = answer[0], answer[1]
    n = len(dist2)
    if n == 0:
        return dict(max=0.0, mean=0.0, rms=0.0, p90=0.0, argmax_point=None, argmax_face_of_b=-1, n_samples=0, n_beyond=0)
    within = face >= 0
    m = int(within.sum())
    top = int(np.argmax(dist2))                              # (the first of equal maxima)
    inside = np.sort(dist2[within])
    return dict(max=math.sqrt(dist2[top]), mean=float(np.sqrt(inside).sum() / max(m, 1)), rms=math.sqrt(inside.sum() / max(m, 1)),
                p90=math.sqrt(inside[(9 * m + 9) // 10 - 1]) if m else 0.0, argmax_point=tuple(float(x) for x in np.asarray(points, dtype=np.float32)[top]),
                argmax_face_of_b=int(face[top]), n_samples=n, n_beyond=n - m)


def deviation(a, b, order=2, symmetric=True, max_distance=np.inf):
    """perf_amd.mesh.mesh_deviation of the meshes a, b = (vertices, faces) by brute force -> the statistics of a to b, with symmetric
    those of the direction with the larger max (a to b when equal) and both under 'a_to_b' and 'b_to_a'."""
    sa = surface_samples(*a, order)[0]
    forward = statistics(sa, closest(*b, sa, max_distance))
    if not symmetric:
        return forward
    sb = surface_samples(*b, order)[0]
    backward = statistics(sb, closest(*a, sb, max_distance))
    return dict(forward if forward['max'] >= backward['max'] else backward, a_to_b=forward, b_to_a=backward)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
TRIANGLE = M.TRIANGLE                    # a = (0, 0, 1), b = (4, 0, 1), c = (0, 4, 1)
HAND_POINTS = (                          # point -> (dist2, u, v), computed by hand
    ((-1, -1, 1), (2.0, 0.0, 0.0)),                          # the region of the vertex a
    ((6, -1, 1), (5.0, 1.0, 0.0)),                           # of b
    ((-1, 6, 1), (5.0, 0.0, 1.0)),                           # of c
    ((1, -2, 1), (4.0, 0.25, 0.0)),                          # of the edge ab: q = (1, 0, 1)
    ((-2, 1, 1), (4.0, 0.0, 0.25)),                          # of the edge ac: q = (0, 1, 1)
    ((3, 3, 1), (2.0, 0.5, 0.5)),                            # of the edge bc: q = (2, 2, 1)
    ((1, 1, 3), (4.0, 0.25, 0.25)),                          # the interior: q = (1, 1, 1)
    ((1, 1, 1.125), (2.0 ** -6, 0.25, 0.25)),                # 2^-3 above the interior
    ((1, 1, 1), (0.0, 0.25, 0.25)),                          # in the face
    ((2, 0, 1), (0.0, 0.5, 0.0)),                            # on the edge ab: vc = 0 is the edge's
    ((0, -1, 1), (1.0, 0.0, 0.0)),                           # between the regions of a and ab: d1 = 0 is a's
    ((4, -1, 1), (1.0, 1.0, 0.0)),                           # between ab and b: d3 = 0 is b's
    ((1, 5, 1), (2.0, 0.0, 1.0)),                            # between bc and c: d5 = d6 is c's
    ((2, 2, 2), (1.0, 0.5, 0.5)),                            # above the edge bc: va = 0 is the edge's
    ((0, 0, 1), (0.0, 0.0, 0.0)), ((4, 0, 1), (0.0, 1.0, 0.0)), ((0, 4, 1), (0.0, 0.0, 1.0)),          # the vertices themselves
)
# degenerate faces: (a, b, c) and points with their (dist2, u, v) by hand
DEGENERATE = (
    (((0, 0, 0), (4, 0, 0), (4, 0, 0)), (((2, 1, 0), (1.0, 0.5, 0.0)), ((5, 1, 0), (2.0, 1.0, 0.0)), ((-1, 0, 0), (1.0, 0.0, 0.0)), ((4, 0, 0), (0.0, 1.0, 0.0)))),          # a != b = c
    (((1, 1, 1), (1, 1, 1), (1, 1, 1)), (((1, 1, 3), (4.0, 0.0, 0.0)), ((1, 1, 1), (0.0, 0.0, 0.0)), ((0, -1, 3), (9.0, 0.0, 0.0)))),                                      # a = b = c
    (((0, 0, 0), (2, 0, 0), (4, 0, 0)), (((3, 1, 0), (1.0, 0.0, 0.75)), ((5, 1, 0), (2.0, 0.0, 1.0)), ((1, 1, 0), (1.0, 0.5, 0.0)), ((-2, 0, 0), (4.0, 0.0, 0.0)))),         # collinear, b between
    (((0, 0, 0), (4, 0, 0), (2, 0, 0)), (((3, 1, 0), (1.0, 0.75, 0.0)), ((2, 0, 0), (0.0, 0.0, 1.0)), ((6, 0, 2), (8.0, 1.0, 0.0)))),                                       # collinear, c between
)
# the tetrahedron of tests/test_gpu_mesh_binding_checks.py; (0.1, 0, 0) lies on the edge 0-1 its faces 0 and 1 share: both give dist2 = 0
TETRAHEDRON = (np.array([[0, 0, 0], [0.2, 0, 0], [0, 0.2, 0], [1, 0, 0.3]], dtype=np.float32), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32))
TETRAHEDRON_POINTS = np.array([[0.1, 0, 0], [0, 0, 0], [1, 0, 0.3], [0.05, 0.05, 0.5], [0.3, 0.1, -0.2], [2, 2, 2], [0.05, 0.05, 0.01]], dtype=np.float32)


def degenerate_mesh():
    """The faces of DEGENERATE as one mesh, with the points of all of them."""
    vertices = np.array([corner for face, _ in DEGENERATE for corner in face], dtype=np.float32)
    faces = np.arange(len(vertices), dtype=np.int32).reshape(-1, 3)
    points = np.array([p for _, cases in DEGENERATE for p, _ in cases], dtype=np.float32)
    return vertices, faces, points


@functools.lru_cache(maxsize=None)
def sphere_points(n=4096, far=64, seed=7):
    """n points for the hollow sphere (the origins of the rays' fixture: inside, between the skins, outside the box) and `far` more at ten
    times the box's size."""
    rng = np.random.default_rng(seed + 1)
    direction = rng.normal(size=(far, 3))
    away = (direction / np.linalg.norm(direction, axis=1, keepdims=True) * rng.uniform(10.0, 20.0, size=(far, 1))).astype(np.float32)
    points = np.concatenate([M.sphere_rays(n, seed)[0], away])
    points.setflags(write=False)
    return points


@functools.lru_cache(maxsize=None)
def triangle_points(n=4096):
    return M.triangle_rays(n)[0]


@functools.lru_cache(maxsize=None)
def expected_closest(which):
    """The brute-force answers of the two large inputs, computed once: 'hollow_sphere' (sphere_points against the cull's fixture) or
    'triangles' (triangle_points against the rays' random triangles)."""
    if which == 'hollow_sphere':
        (vertices, faces), points = V.reference_mesh('hollow_sphere'), sphere_points()
    else:
        (vertices, faces), points = M.random_triangles(), triangle_points()
    out = closest(vertices, faces, points)
    for a in out:
        a.setflags(write=False)
    return out


# the edge inputs: five faces of which two are never the answer (M.SMALL: a NaN vertex, an index outside [0, V)), points that are not finite
EDGE_POINTS = np.array([[1, 1, 0], [np.nan, 1, 0], [1, np.inf, 0], [-np.inf, 0, 0], [1, 1, 1.5], [1, 1, 1.75], [0, 0, 0.5], [3e38, 0, 0], [100, 100, 100], [0.5, 0.25, 2]],
                       dtype=np.float32)
