"""Rays against a triangle mesh as include/perf_hip_meshray.h states them, in numpy float64: the per-face rule operation for operation in
the header's order (numpy does not contract), the closest hit, the any hit and the segment occlusion by BRUTE FORCE over all faces, and
the cell lists of the uniform grid as sets per cell.  The yardstick of tests/test_cpu_meshray_reference.py and tests/test_gpu_meshray.py,
written from the statement, not from the kernels.  Also the inputs both files use."""
import functools

import numpy as np

from tests import meshvis_reference as V

VIEW = (0.13, -0.05, 0.07)               # the off-centre view inside the hollow sphere
_CHUNK = 256                             # rays per block of the brute force


def _f64(x, shape):
    return np.asarray(x, dtype=np.float32).astype(np.float64).reshape(shape)


def valid_faces(vertices, faces):
    """bool [F]: every index in [0, V) and every coordinate of the three vertices finite.  A face that is not valid can never be hit and is
    listed in no cell."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    if len(v):
        ok &= np.isfinite(v[np.clip(f, 0, len(v) - 1)].astype(np.float64)).all(axis=(1, 2))
    return ok


def rule(o, d, a, b, c, t_lo, t_hi, strict=False):
    """The header's lines, each operation rounded once, broadcasting over the leading axes -> (hit bool, t, u, v float64)."""
    with np.errstate(all='ignore'):
        e1, e2 = b - a, c - a
        px = d[..., 1] * e2[..., 2] - d[..., 2] * e2[..., 1]
        py = d[..., 2] * e2[..., 0] - d[..., 0] * e2[..., 2]
        pz = d[..., 0] * e2[..., 1] - d[..., 1] * e2[..., 0]
        det = (e1[..., 0] * px + e1[..., 1] * py) + e1[..., 2] * pz
        s = o - a
        u = ((s[..., 0] * px + s[..., 1] * py) + s[..., 2] * pz) / det
        qx = s[..., 1] * e1[..., 2] - s[..., 2] * e1[..., 1]
        qy = s[..., 2] * e1[..., 0] - s[..., 0] * e1[..., 2]
        qz = s[..., 0] * e1[..., 1] - s[..., 1] * e1[..., 0]
        v = ((d[..., 0] * qx + d[..., 1] * qy) + d[..., 2] * qz) / det
        t = ((e2[..., 0] * qx + e2[..., 1] * qy) + e2[..., 2] * qz) / det
        inside = (det != 0) & (u >= 0) & (v >= 0) & ((u + v) <= 1)              # (every comparison is false on a NaN; det NaN makes u NaN)
        within = ((t > t_lo) & (t < t_hi)) if strict else ((t >= t_lo) & (t <= t_hi))
    return inside & within, t, u, v


def cast(vertices, faces, origins, directions, t_min=0.0, t_max=np.inf):
    """Closest hit of N rays over ALL valid faces: the lexicographic minimum of (t, face index) -> (t float32 [N], face int32 [N],
    u float32 [N], v float32 [N]); +inf, -1, 0, 0 where nothing is hit."""
    vt = _f64(vertices, (-1, 3))
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    index = np.nonzero(valid_faces(vertices, faces))[0]
    f = f[index]
    o, d = _f64(origins, (-1, 3)), _f64(directions, (-1, 3))
    n = len(o)
    t_lo, t_hi = float(np.float32(t_min)), float(np.float32(t_max))
    t_out, face_out = np.full(n, np.inf, np.float32), np.full(n, -1, np.int32)
    u_out, v_out = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if not len(f):
        return t_out, face_out, u_out, v_out
    a, b, c = vt[f[:, 0]][None], vt[f[:, 1]][None], vt[f[:, 2]][None]
    for first in range(0, n, _CHUNK):
        rows = slice(first, min(first + _CHUNK, n))
        hit, t, u, v = rule(o[rows, None, :], d[rows, None, :], a, b, c, t_lo, t_hi)
        key = np.where(hit, t, np.inf)
        best = np.argmin(key, axis=1)                        # (the first of equal minima: the smallest face index)
        any_ = hit.any(axis=1)
        r = np.arange(len(best))
        with np.errstate(over='ignore'):
            t_out[rows] = np.where(any_, t[r, best], np.inf).astype(np.float32)
            u_out[rows] = np.where(any_, u[r, best], 0.0).astype(np.float32)
            v_out[rows] = np.where(any_, v[r, best], 0.0).astype(np.float32)
        face_out[rows] = np.where(any_, index[best], -1).astype(np.int32)
    return t_out, face_out, u_out, v_out


def any_hit(vertices, faces, origins, directions, t_min=0.0, t_max=np.inf):
    """uint8 [N]: some valid face is hit."""
    return (cast(vertices, faces, origins, directions, t_min, t_max)[1] >= 0).astype(np.uint8)


def occluded(vertices, faces, centres, mask_bits):
    """int64 [V]: bit k is set iff bit k of mask_bits[v] is set (k < K) and some valid face that does not name index v is hit by the segment
    o = p_v, d = c_k - p_v at a STRICT 0 < t < 1."""
    vt = _f64(vertices, (-1, 3))
    f_all = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f_all[valid_faces(vertices, faces)]
    cs = _f64(centres, (-1, 3))
    mask = np.asarray(mask_bits).astype(np.uint64).reshape(-1)
    out = np.zeros(len(vt), dtype=np.uint64)
    if not len(f):
        return out.view(np.int64)
    a, b, c = vt[f[:, 0]][None], vt[f[:, 1]][None], vt[f[:, 2]][None]
    for k in range(len(cs)):
        bit = np.uint64(1) << np.uint64(k)
        for first in range(0, len(vt), _CHUNK):
            ids = np.arange(first, min(first + _CHUNK, len(vt)))
            ids = ids[(mask[ids] & bit) != 0]
            if not len(ids):
                continue
            o = vt[ids][:, None, :]
            with np.errstate(all='ignore'):
                d = cs[k][None, None, :] - o
            hit = rule(o, d, a, b, c, 0.0, 1.0, strict=True)[0]
            hit &= (f[None, :, :] != ids[:, None, None]).all(axis=2)            # faces that name the vertex are not tested
            out[ids[hit.any(axis=1)]] |= bit
    return out.view(np.int64)


def cell_range(lo, hi, origin, cell, dims):
    """Per axis, the clamped index range [floor((min - m - origin) / cell), floor((max + m - origin) / cell)] of a face with bounds lo, hi
    (float64 [3] from fp32), in double; None when the face lies wholly outside the box."""
    origin = _f64(origin, 3)
    cell = float(np.float32(cell))
    m = cell / 8.0
    first = np.floor(((lo - m) - origin) / cell)
    last = np.floor(((hi + m) - origin) / cell)
    dims = np.asarray(dims, dtype=np.int64)
    if (last < 0).any() or (first > dims - 1).any():
        return None
    return np.maximum(first, 0).astype(np.int64), np.minimum(last, dims - 1).astype(np.int64)


def cell_lists(vertices, faces, origin, cell, dims):
    """-> (lists, bad): lists = {linear cell (i ny + j) nz + k: set of face indices} of the non-empty cells; bad = the smallest index of a
    face that is not valid, or -1."""
    vt = _f64(vertices, (-1, 3))
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = valid_faces(vertices, faces)
    bad = int(np.nonzero(~ok)[0][0]) if (~ok).any() else -1
    ny, nz = int(dims[1]), int(dims[2])
    lists = {}
    for n in np.nonzero(ok)[0]:
        tri = vt[f[n]]
        r = cell_range(tri.min(axis=0), tri.max(axis=0), origin, cell, dims)
        if r is None:
            continue
        for i in range(r[0][0], r[1][0] + 1):
            for j in range(r[0][1], r[1][1] + 1):
                for k in range(r[0][2], r[1][2] + 1):
                    lists.setdefault((i * ny + j) * nz + k, set()).add(int(n))
    return lists, bad


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
# one dyadic triangle in the plane z = 1 and the rays whose answers are computed by hand (tests/test_cpu_meshray_reference.py)
TRIANGLE = (np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32))
HAND_RAYS = (                            # (origin, direction, t_min, t_max) -> (t, face, u, v)
    (((1, 1, 0), (0, 0, 1), 0.0, np.inf), (1.0, 0, 0.25, 0.25)),             # the centre region, from below
    (((1, 1, 3), (0, 0, -1), 0.0, np.inf), (2.0, 0, 0.25, 0.25)),            # from behind: two-sided
    (((2, 0, 0), (0, 0, 2), 0.0, np.inf), (0.5, 0, 0.5, 0.0)),               # exactly on the edge a-b: v = 0 is inside
    (((2, 2, 0), (0, 0, 1), 0.0, np.inf), (1.0, 0, 0.5, 0.5)),               # exactly on the edge b-c: u + v = 1 is inside
    (((0, 0, 0), (0, 0, 1), 0.0, np.inf), (1.0, 0, 0.0, 0.0)),               # exactly on the vertex a
    (((4, 0, 0), (0, 0, 1), 0.0, np.inf), (1.0, 0, 1.0, 0.0)),               # exactly on the vertex b
    (((1, 1, 0), (1, 0, 0), 0.0, np.inf), (np.inf, -1, 0.0, 0.0)),           # parallel to the plane: det = 0
    (((1, 1, 1), (1, 0, 0), 0.0, np.inf), (np.inf, -1, 0.0, 0.0)),           # in the plane itself: det = 0
    (((2.5, 2, 0), (0, 0, 1), 0.0, np.inf), (np.inf, -1, 0.0, 0.0)),         # just outside the edge b-c
    (((1, 1, 0), (0, 0, 1), 1.0, 2.0), (1.0, 0, 0.25, 0.25)),                # t == t_min: a hit
    (((1, 1, 0), (0, 0, 1), 0.5, 1.0), (1.0, 0, 0.25, 0.25)),                # t == t_max: a hit
    (((1, 1, 0), (0, 0, 1), 1.25, 2.0), (np.inf, -1, 0.0, 0.0)),             # t below t_min
    (((1, 1, 0), (0, 0, 1), 0.0, 0.75), (np.inf, -1, 0.0, 0.0)),             # t above t_max
    (((1, 1, 2), (0, 0, 1), 0.0, np.inf), (np.inf, -1, 0.0, 0.0)),           # the plane lies behind the origin: t = -1
    (((1, 1, 0), (0, 0, 0), 0.0, np.inf), (np.inf, -1, 0.0, 0.0)),           # d = 0
)


@functools.lru_cache(maxsize=None)
def sphere_rays(n=4096, seed=7):
    """n rays for the hollow sphere of the cull's fixtures: origins inside, in the shell's gap and outside the box, random directions."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.3, 1.3, size=(n, 3)).astype(np.float32)
    o[: n // 4] *= np.float32(0.25)                           # a quarter start well inside the inner skin
    d = rng.normal(size=(n, 3)).astype(np.float32)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def random_triangles(n_faces=3000, seed=11):
    """n_faces loose triangles in [-1, 1]^3 with edges up to 0.5: several cells of the default grid large."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, size=(n_faces, 1, 3))
    vertices = (base + rng.uniform(-0.25, 0.25, size=(n_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)
    vertices.setflags(write=False)
    faces.setflags(write=False)
    return vertices, faces


@functools.lru_cache(maxsize=None)
def triangle_rays(n=4096, seed=13):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def expected_cast(which):
    """The brute-force closest hits of the two large inputs, computed once: 'hollow_sphere' (sphere_rays against the cull's fixture) or
    'triangles' (triangle_rays against random_triangles)."""
    if which == 'hollow_sphere':
        (vertices, faces), (o, d) = V.reference_mesh('hollow_sphere'), sphere_rays()
    else:
        (vertices, faces), (o, d) = random_triangles(), triangle_rays()
    out = cast(vertices, faces, o, d)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def skin_occlusion(which, centre):
    """(occluded bool [V], faces with no occluded vertex bool [F]) of 'hollow_sphere' or 'tunnel' for ONE view at centre whose mask passes
    every vertex."""
    vertices, faces = V.reference_mesh(which)
    bits = occluded(vertices, faces, [centre], np.ones(len(vertices), dtype=np.int64))
    occ = bits != 0
    keep = ~occ[faces.astype(np.int64)].any(axis=1)
    return occ, keep


# five faces of which two can never be hit (a NaN vertex, an index outside [0, V)), two coincide and the nearest is listed last
SMALL = (np.array([[0, 0, 2], [4, 0, 2], [0, 4, 2], [0, 0, 1], [4, 0, 1], [0, 4, 1], [np.nan, 0, 0.5]], dtype=np.float32),
         np.array([[0, 1, 6], [0, 1, 9], [2, 1, 0], [0, 1, 2], [3, 4, 5]], dtype=np.int32))

# a solid ball of radius 6 cells on a lattice of 20^3 cells of edge 0.1 over [-1, 1]^3, centred at lattice (10.3, 9.8, 10.1)
BALL_CENTRE, BALL_RADIUS, BALL_SPACING = (0.03, -0.02, 0.01), 0.6, 0.1


def ball_field():
    from tests import mesh_reference as R
    return R.ball((20, 20, 20), (10.3, 9.8, 10.1), 6.0)


@functools.lru_cache(maxsize=None)
def ball_rays(n=4096, seed=5):
    """n rays from the ball's centre along random unit directions (fp32)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.tile(np.array(BALL_CENTRE, dtype=np.float32), (n, 1))
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


# rays that run IN cell-boundary planes, ALONG cell edges and THROUGH cell corners of a grid whose origin and cell are dyadic (the corner at
# the origin or at (-1, -1, -1), cells of 1/2, 1 or 2), against SMALL: exact ties of the walk's entry parameters
BOUNDARY_GRIDS = (((0, 0, 0), 1.0, (5, 5, 3)), ((0, 0, 0), 0.5, (10, 10, 6)), ((-1, -1, -1), 2.0, (3, 3, 2)), ((0, 0, 0), 1.0, (5, 5, 64)))
BOUNDARY_RAYS = (
    ((1, -1, 0.5), (0, 1, 0.25)), ((-1, 2, 0), (1, 0, 0.5)), ((2, 6, 3), (0, -1, -0.5)),          # in the planes x = 1, y = 2, x = 2
    ((1, 2, -1), (0, 0, 1)), ((1, 2, 4), (0, 0, -1)), ((0, 0, -1), (0, 0, 1)), ((2, 2, -3), (0, 0, 2)),          # along the edges x = 1, y = 2; x = y = 0; x = y = 2
    ((-1, 1, 1), (1, 0, 0)), ((6, 1, 2), (-1, 0, 0)), ((-1, 1, 1), (1, 0, 0.25)),                # in the planes z = 1 and z = 2 of the faces themselves (det = 0), and leaving z = 1
    ((-1, -1, 0), (1, 1, 0.5)), ((3, 3, 2), (-1, -1, -0.5)),                                      # through the edges x = y = k, meeting z = 1 at the corner (1, 1, 1)
    ((-1, -1, -1), (1, 1, 1)), ((5, 5, 5), (-1, -1, -1)), ((3, -1, -1), (-1, 1, 1)), ((-2, 4, 0), (1, -1, 0.5)),          # through the corners (k, k, k) and across
    ((0, 4, 0), (0, 0, 1)), ((4, 0, 3), (0, 0, -1)), ((0, 0, 1), (1, 1, 0)), ((0, 2, 1), (1, 0, 0.25)),          # from ON the box's faces, edges and corner
    ((1, 1, 1), (0, 0, 1)), ((1, 1, 1), (0, 0, -1)), ((2, 2, 2), (-1, -1, -1)), ((1, 1, 1.5), (1, 1, 0)),          # from a corner ON a face (t = 0 is a hit); between the sheets along a diagonal
    ((0.5, 0.5, -1), (0.5, 0.5, 1)), ((4.5, 4.5, 3), (-1, -1, -0.5)), ((-0.125, 1, 0), (0.125, 0, 1)), ((5.125, 1, 0.5), (-1, 0, 0.125)),          # from the margin's rim
)
