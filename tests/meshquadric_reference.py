"""Quadric error placement as include/perf_hip_meshquadric.h states it, in vectorised numpy, float64 and int64 on the fp32 values it is
given: the yardstick of tests/test_cpu_meshquadric_reference.py and tests/test_gpu_meshquadric.py, written from the statement line by
line, not from the kernels.  numpy's elementwise float64 operations round once each and contract nothing, and the rule uses only
+ - * / and rint, so every bit is reproducible.  Also the inputs the two test files share."""
import numpy as np

from tests import meshsimp_reference as simp

SCALE = 2.0 ** 40
SKIP = 2.0 ** 60
REGULARISER = 2.0 ** -10
TERMS = 9
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # xx, xy, xz, yy, yz, zz


def _grid64(lo, h, n):
    return np.asarray(lo, dtype=np.float32).astype(np.float64), float(np.float32(h)), np.asarray(n, dtype=np.int64)


def fractions(x, lo, h, n):
    """The cell rule on FINITE float64 coordinates [..., 3] -> (i int64, f float64)."""
    lo64, h64, n64 = _grid64(lo, h, n)
    t = (x - lo64) / h64
    t = np.minimum(np.maximum(t, 0.0), n64.astype(np.float64))
    i = np.minimum(np.floor(t).astype(np.int64), n64 - 1)
    return i, t - i.astype(np.float64)


def face_terms(vertices, faces, lo, h, n):
    """Steps 1 to 3 for faces whose indices are all inside: -> (normal [F, 3], scaled products [F, 6], fits bool [F], q int64 [F, 3, 9]
    per corner; rows of q of faces that do not fit are meaningless)."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    _, h64, _ = _grid64(lo, h, n)
    with np.errstate(all='ignore'):
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e1, e2 = (b - a) / h64, (c - a) / h64
        nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        scaled = np.stack([(nrm[:, i] * nrm[:, j]) * SCALE for i, j in PAIRS], axis=1)
        fits = (np.abs(scaled) < SKIP).all(axis=1)           # (False for a NaN and for an infinity)
        q = np.zeros((len(f), 3, TERMS), dtype=np.int64)
        ok = np.nonzero(fits)[0]
        qa = np.rint(scaled[ok]).astype(np.int64)            # (rint: ties to even)
        for k in range(3):
            _, frac = fractions(v[f[ok, k]], lo, h, n)          # (finite: a face that fits has a finite normal, so finite corners)
            r = frac - 0.5
            d = (nrm[ok, 0] * r[:, 0] + nrm[ok, 1] * r[:, 1]) + nrm[ok, 2] * r[:, 2]
            qb = np.rint((nrm[ok] * d[:, None]) * SCALE).astype(np.int64)
            q[ok, k, :6] = qa
            q[ok, k, 6:] = qb
    return nrm, scaled, fits, q


def sums(vertices, faces, lo, h, n, vertex_cluster, n_clusters):
    """Stage A -> (acc int64 [C, 9], bad_face, skipped_face)."""
    V = len(np.asarray(vertices).reshape(-1, 3))
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vc = np.asarray(vertex_cluster, dtype=np.int64)
    C = int(n_clusters)
    acc = np.zeros((C, TERMS), dtype=np.int64)
    inside = ((f >= 0) & (f < V)).all(axis=1)
    bad = int(np.nonzero(~inside)[0].min()) if (~inside).any() else -1
    idx = np.nonzero(inside)[0]
    cl = vc[f[idx]].reshape(-1, 3)
    has = ((cl >= 0) & (cl < C)).all(axis=1)
    idx, cl = idx[has], cl[has]
    _, _, fits, q = face_terms(vertices, f[idx], lo, h, n)
    skipped = int(idx[~fits].min()) if (~fits).any() else -1
    with np.errstate(over='ignore'):
        for k in range(3):
            np.add.at(acc, cl[fits, k], q[fits, k])          # (int64: wraps as the device's atomics do)
    return acc, bad, skipped


def place(vertices, lo, h, n, anchor, representative, acc):
    """Stage B -> (cluster vertices float32 [C, 3], info): info['solved'] bool [C] (False: the anchor's row), info['x'] float64 [C, 3] the
    solution BEFORE the clamp, info['m'] the anchor in the cell's centred coordinates, info['clamped'] the number of clamped components,
    info['M'], info['g'] the regularised system, info['lam']."""
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    anchor = np.asarray(anchor, dtype=np.float32).reshape(-1, 3)
    rep = np.asarray(representative, dtype=np.int64)
    acc = np.asarray(acc, dtype=np.int64).reshape(-1, TERMS)
    lo64, h64, _ = _grid64(lo, h, n)
    C, V = len(acc), len(v32)
    out = anchor.copy()
    with np.errstate(all='ignore'):
        t = acc.astype(np.float64) * 2.0 ** -40
        tr = (t[:, 0] + t[:, 3]) + t[:, 5]
        ok = (tr > 0.0) & (rep >= 0) & (rep < V)
        member = v32[np.where(ok, rep, 0)].astype(np.float64) if V else np.zeros((C, 3))
        ok &= np.isfinite(member).all(axis=1)
        i, _ = fractions(np.where(np.isfinite(member), member, 0.0), lo, h, n)
        centre = i.astype(np.float64) + 0.5
        m = (anchor.astype(np.float64) - lo64) / h64 - centre
        lam = tr * REGULARISER
        Mxx, Myy, Mzz, Mxy, Mxz, Myz = t[:, 0] + lam, t[:, 3] + lam, t[:, 5] + lam, t[:, 1], t[:, 2], t[:, 4]
        g = t[:, 6:] + lam[:, None] * m
        c00 = Myy * Mzz - Myz * Myz
        c01 = Mxz * Myz - Mxy * Mzz
        c02 = Mxy * Myz - Mxz * Myy
        c11 = Mxx * Mzz - Mxz * Mxz
        c12 = Mxy * Mxz - Mxx * Myz
        c22 = Mxx * Myy - Mxy * Mxy
        det = (Mxx * c00 + Mxy * c01) + Mxz * c02
        ok &= (det > 0.0) & np.isfinite(det)
        x = np.stack([((c00 * g[:, 0] + c01 * g[:, 1]) + c02 * g[:, 2]) / det, ((c01 * g[:, 0] + c11 * g[:, 1]) + c12 * g[:, 2]) / det,
                      ((c02 * g[:, 0] + c12 * g[:, 1]) + c22 * g[:, 2]) / det], axis=1)
        ok &= np.isfinite(x).all(axis=1)
        xc = np.minimum(np.maximum(x, -0.5), 0.5)
        p = lo64 + (centre + xc) * h64
    out[ok] = p[ok].astype(np.float32)
    M = np.stack([np.stack([Mxx, Mxy, Mxz], 1), np.stack([Mxy, Myy, Myz], 1), np.stack([Mxz, Myz, Mzz], 1)], 1)
    return out, {'solved': ok, 'x': x, 'm': m, 'clamped': int((xc != x)[ok].sum()), 'M': M, 'g': g, 'lam': lam, 'centre': centre}


def labelled(vertices, lo, h, n):
    """The clustering the placement sits on, by tests/meshsimp_reference.py -> (vertex_cluster int32 [V], C, anchor float32 [C, 3],
    representative int32 [C]); a vertex that is not finite gets -1 and the others cluster as if it were not there (ids rank the
    clusters' smallest members, so dropping a vertex that joins nothing leaves the order)."""
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    finite = np.isfinite(v32).all(axis=1)
    index = np.nonzero(finite)[0]
    vc = np.full(len(v32), -1, dtype=np.int32)
    if len(index) == 0:
        return vc, 0, np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    sub, C, placed, rep, _ = simp.cluster(v32[index], lo, h, n, 'mean')
    vc[index] = sub
    return vc, C, placed, index[rep].astype(np.int32)


def placement(vertices, faces, lo, h, n):
    """labelled -> sums -> place: (cluster vertices float32 [C, 3], acc, bad, skipped, info, the labelling)."""
    lab = labelled(vertices, lo, h, n)
    acc, bad, skipped = sums(vertices, faces, lo, h, n, lab[0], lab[1])
    out, info = place(vertices, lo, h, n, lab[2], lab[3], acc)
    return out, acc, bad, skipped, info, lab


def simplify(vertices, faces, lo, h, n, dedupe='oriented'):
    """simplify_mesh(placement='quadric') -> (vertices float32 [V', 3], faces int32 [F', 3], kept_vertex_index int32 [V']): the 'mean'
    simplification of tests/meshsimp_reference.py with the surviving clusters' quadric vertices."""
    out, _, _, _, _, (vc, C, _, rep) = placement(vertices, faces, lo, h, n)
    r, keep = simp.cluster_faces(faces, vc, dedupe)
    kept = r[keep.astype(bool)].astype(np.int64)
    used = np.zeros(C, dtype=bool)
    used[kept.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return out[used], new[kept].astype(np.int32).reshape(-1, 3), rep[used]


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------------
def patch(origin, du, dv, nu, nv):
    """A parallelogram of nu x nv quads, two triangles each: (vertices float64 [(nu + 1)(nv + 1), 3], faces int64 [2 nu nv, 3])."""
    origin, du, dv = (np.asarray(a, dtype=np.float64) for a in (origin, du, dv))
    u, w = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing='ij')
    vertices = origin + u.reshape(-1, 1) * du + w.reshape(-1, 1) * dv
    at = lambda a, b: a * (nv + 1) + b
    a, b = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a, b = a.reshape(-1), b.reshape(-1)
    faces = np.concatenate([np.stack([at(a, b), at(a + 1, b), at(a + 1, b + 1)], 1), np.stack([at(a, b), at(a + 1, b + 1), at(a, b + 1)], 1)])
    return vertices, faces


def join(parts):
    vertices, faces, base = [], [], 0
    for v, f in parts:
        vertices.append(v); faces.append(f + base); base += len(v)
    return np.concatenate(vertices).astype(np.float32), np.concatenate(faces).astype(np.int32)


BOX_HALF = 13.0 / 32.0          # the planes at +-13/32: at fractions 0.25 and 0.75 of their cells of the grid below
BOX_GRID = (np.array([-0.5, -0.5, -0.5], np.float32), np.float32(0.125), [8, 8, 8])
BOX_STEP = 1.0 / 64.0


def box_mesh():
    """A finely tessellated axis-aligned box, all coordinates dyadic (every product and every sum of the rule is exact on it): six
    patches of 52 x 52 quads at a spacing of h / 8 -> (vertices float32 [16854, 3], faces int32 [32448, 3])."""
    s, e, k = BOX_HALF, BOX_STEP, int(round(2 * BOX_HALF / BOX_STEP))
    parts = []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (-1.0, 1.0):
            origin = np.full(3, -s); origin[axis] = side * s
            du, dv = np.zeros(3), np.zeros(3)
            du[u], dv[w] = e, e
            parts.append(patch(origin, du, dv, k, k) if side > 0 else patch(origin, dv, du, k, k))
    return join(parts)


def box_corners():
    return np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) * BOX_HALF
