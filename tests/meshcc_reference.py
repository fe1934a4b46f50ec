"""The connected components of a triangle mesh as include/perf_hip_meshcc.h states them, in plain numpy: a sequential union-find with
ids by smallest vertex index, the per-component counts and signed volumes, the selection and the order-keeping compaction.  The yardstick
of tests/test_cpu_meshcc_reference.py (which pins it against scipy) and tests/test_gpu_meshcc.py, written from the statement, not from the
kernels (no atomics, no scan, no workspace).  Also the cases both files use."""
import functools
import math

import numpy as np

from tests import mesh_reference as R


def components(faces, n_vertices):
    """faces: int [F, 3], every index in [0, V) -> (vertex_component int32 [V], C)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = int(n_vertices)
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < V)
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)                # the smaller index stays the root: a root is its tree's smallest vertex

    for a, b, c in faces.tolist():
        union(a, b)
        union(b, c)
    roots = np.array([find(v) for v in range(V)], dtype=np.int64)
    smallest = np.unique(roots)                          # ascending: the rank of a component's smallest vertex is its id
    return np.searchsorted(smallest, roots).astype(np.int32), int(len(smallest))


def face_terms(vertices, faces, dtype=np.float64):
    """a . (b x c) / 6 per face, formed in `dtype` from the fp32 vertices."""
    v = np.asarray(vertices, dtype=np.float32).astype(dtype)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2])
            + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])) / dtype(6)


def stats(faces, vertex_component, n_components, vertices=None):
    """-> (faces int64 [C], vertices int32 [C], signed_volume float64 [C] or None).  The volumes: math.fsum over per-face terms formed
    in numpy.longdouble."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vc = np.asarray(vertex_component, dtype=np.int64)
    C = int(n_components)
    of_face = vc[faces[:, 0]] if len(faces) else np.zeros(0, dtype=np.int64)
    per_faces = np.bincount(of_face, minlength=C).astype(np.int64)
    per_vertices = np.bincount(vc, minlength=C).astype(np.int32)
    volume = None
    if vertices is not None:
        terms = face_terms(vertices, faces, np.longdouble)
        volume = np.array([math.fsum(float(t) for t in terms[of_face == c]) for c in range(C)], dtype=np.float64)
    return per_faces, per_vertices, volume


def select(per_faces, signed_volume=None, min_faces=0, keep_largest=None, orientation=None):
    """bool [C] by the statement's three conditions."""
    per_faces = np.asarray(per_faces, dtype=np.int64)
    C = len(per_faces)
    keep = per_faces >= min_faces
    if keep_largest is not None:
        order = sorted(range(C), key=lambda c: (-int(per_faces[c]), c))           # more faces first, then lower id
        rank = np.empty(C, dtype=np.int64)
        rank[order] = np.arange(C)
        keep &= rank < keep_largest
    if orientation == 'inward':
        keep &= np.asarray(signed_volume) < 0
    elif orientation == 'outward':
        keep &= np.asarray(signed_volume) > 0
    else:
        assert orientation is None
    return keep


def filter_mesh(vertices, faces, vertex_component, keep):
    """-> (vertices [V', 3], faces int32 [F', 3] re-indexed, kept_vertex_index int32 [V']): relative order kept."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vc = np.asarray(vertex_component, dtype=np.int64)
    keep = np.asarray(keep, dtype=bool)
    kept_vertex = keep[vc] if len(vc) else np.zeros(0, dtype=bool)
    index = np.nonzero(kept_vertex)[0].astype(np.int32)
    new = np.full(len(vc), -1, dtype=np.int64)
    new[index] = np.arange(len(index))
    kept_face = kept_vertex[faces[:, 0]] if len(faces) else np.zeros(0, dtype=bool)
    out = new[faces[kept_face]].astype(np.int32).reshape(-1, 3)
    assert out.min(initial=0) >= 0                       # all of a face's vertices are kept or none are
    return np.asarray(vertices)[index], out, index


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def fan(V):
    """V - 2 triangles around vertex 0."""
    i = np.arange(1, V - 1)
    return np.stack([np.zeros_like(i), i, i + 1], axis=1).astype(np.int32)


def strip(V):
    i = np.arange(V - 2)
    return np.stack([i, i + 1, i + 2], axis=1).astype(np.int32)


def quad_strip(n_quads):
    """Quad q = vertices 2q .. 2q + 3, two triangles each: a path of length ~ V / 2."""
    q = 2 * np.arange(n_quads)
    return np.stack([q, q + 1, q + 2, q + 1, q + 3, q + 2], axis=1).reshape(-1, 3).astype(np.int32), 2 * n_quads + 2


EDGE_SIZES = (63, 64, 65, 255, 256, 257, 65537)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (faces int32 [F, 3], V)."""
    rng = np.random.default_rng(20240607)
    out = {
        'empty': (np.zeros((0, 3), np.int32), 0),
        'five_loose_vertices': (np.zeros((0, 3), np.int32), 5),
        'one_triangle': (np.array([[0, 1, 2]], np.int32), 3),
        'two_triangles_one_shared_vertex': (np.array([[0, 1, 2], [2, 3, 4]], np.int32), 5),
        'two_triangles_disjoint': (np.array([[5, 1, 3], [2, 0, 4]], np.int32), 7),
        'repeated_index': (np.array([[0, 0, 1], [2, 3, 2], [4, 4, 4], [5, 6, 7]], np.int32), 9),
    }
    for V in EDGE_SIZES:
        out[f'fan_{V}'] = (fan(V), V)
        out[f'strip_{V}'] = (strip(V), V)
    f, V = quad_strip(4097)
    out['quad_strip_ascending'] = (f, V)
    out['quad_strip_descending'] = ((V - 1 - f).astype(np.int32), V)
    out['quad_strip_permuted'] = (rng.permutation(V).astype(np.int32)[f], V)
    V = 10001                                            # one hub vertex in 5,000 faces
    i = np.arange(5000)
    ring = np.delete(np.arange(V), V // 2)
    out['hub'] = (np.stack([np.full(5000, V // 2), ring[2 * i], ring[2 * i + 1]], axis=1).astype(np.int32), V)
    out['disjoint_triangles'] = (rng.permutation(9000).astype(np.int32).reshape(3000, 3), 9000)
    for name, F in (('random_quarter', 5000), ('random_half', 10000), ('random_full', 20000)):
        out[name] = (rng.integers(0, 20000, size=(F, 3)).astype(np.int32), 20000)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(vertex_component, C, faces per component, vertices per component) of a case, computed once."""
    faces, V = cases()[name]
    vc, C = components(faces, V)
    per_faces, per_vertices, _ = stats(faces, vc, C)
    for a in (vc, per_faces, per_vertices):
        a.setflags(write=False)
    return vc, C, per_faces, per_vertices


# the end-to-end field: five balls and a speck on a lattice of 24 x 20 x 28 cells, thresholded at 0
SHAPE = (24, 20, 28)
BALLS = (((6, 6, 6), 4.3), ((17, 6, 7), 3.6), ((7, 14, 20), 4.9), ((17, 13, 21), 3.2), ((12, 10, 13), 2.4))
SPECK = ((20.4, 3.3, 24.6), 0.8)
BALLS_FACES = (732, 828, 252, 444, 444, 28)              # per component id, as the float64 restatement finds them (pinned without a GPU)
BALLS_VERTICES = (368, 416, 128, 224, 224, 16)


def balls_field(without=None, speck=True, shape=SHAPE):
    """fp32 corner values: the maximum of the balls (but number `without`) and, speck, the speck."""
    parts = [R.ball(shape, c, r) for n, (c, r) in enumerate(BALLS) if n != without]
    if speck:
        parts.append(R.ball(shape, *SPECK))
    return np.maximum.reduce(parts)


# the hollow sphere: 20^3 cells in the box [-1, 1]^3, a shell of radius 6 and half thickness 1.6 around (10.2, 10.2, 10.2), thresholded at 0
SPHERE_LO, SPHERE_HI = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]


def hollow_sphere():
    g = np.meshgrid(*[np.arange(21, dtype=np.float64)] * 3, indexing='ij')
    r = np.sqrt(sum((x - 10.2) ** 2 for x in g))
    return (1.6 - np.abs(r - 6.0)).astype(np.float32)


def volume_tolerance(n_faces, largest_coordinate):
    """The bound of |device volume - exact| for a component of n faces inside |x| <= M.  One term a . (b x c) / 6 is at most M^3 and is
    formed with at most 6 u M^3 of rounding error (u = 2^-53: nine products, five sums, one division, first order); n terms added in
    ANY order lose at most (n - 1) u times the sum of their magnitudes <= n M^3.  Together n (n + 8) u M^3, with room for second order."""
    return n_faces * (n_faces + 8) * 2.0 ** -53 * float(largest_coordinate) ** 3
