"""Vertex clustering as include/perf_hip_meshsimp.h states it, in vectorised numpy, float64 and int64 on the fp32 vertices it is given: the
yardstick of tests/test_cpu_meshsimp_reference.py and tests/test_gpu_meshsimp.py, written from the statement, not from the kernels (it
works on whole arrays: no table, no probing, no scan and no workspace).  Also the stated hash functions, so a test can build keys that
collide, and the inputs the two test files share."""
import math

import numpy as np

MUL = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
EDGE_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537]


def grid_of(cell, box):
    """(lo float32 [3], h float32, n [3]) as the wrapper forms them: n = max(1, ceil((hi - lo) / h)) per axis in double."""
    h = np.float32(cell)
    lo = np.asarray(box[0], dtype=np.float32)
    n = [max(1, math.ceil((float(b) - float(a)) / float(h))) for a, b in zip(lo, box[1])]
    return lo, h, n


def cells(vertices, lo, h, n):
    """The cell rule -> (cell int64 [V, 3], q int64 [V, 3], key int64 [V]); every vertex must be finite."""
    x = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    assert np.isfinite(x).all()
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
    h = float(np.float32(h))
    nd = np.asarray(n, dtype=np.float64)
    t = (x - lo) / h
    t = np.minimum(np.maximum(t, 0.0), nd)
    i = np.minimum(np.floor(t).astype(np.int64), np.asarray(n, dtype=np.int64) - 1)
    f = t - i.astype(np.float64)
    q = np.rint(f * 4294967296.0).astype(np.int64)          # (rint: ties to even)
    key = i[:, 0] << 42 | i[:, 1] << 21 | i[:, 2]
    return i, q, key


def cluster(vertices, lo, h, n, placement='mean'):
    """-> (vertex_cluster int32 [V], C, cluster vertices float32 [C, 3], representative int32 [C], ties: the number of clusters in which
    two members are at the smallest d2)."""
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    V = len(v32)
    i, q, key = cells(v32, lo, h, n)
    order = np.argsort(key, kind='stable')                   # members of a key in ascending index
    sorted_keys = key[order]
    first = np.ones(V, dtype=bool)
    first[1:] = sorted_keys[1:] != sorted_keys[:-1]
    smallest_sorted = order[first]                           # the smallest member of each key, in key order
    group = np.cumsum(first) - 1                             # the key's position, per sorted vertex
    rank = np.empty(len(smallest_sorted), dtype=np.int64)
    rank[np.argsort(smallest_sorted, kind='stable')] = np.arange(len(smallest_sorted))          # ids: the ranks of the smallest members
    vc = np.empty(V, dtype=np.int64)
    vc[order] = rank[group]
    C = len(smallest_sorted)
    S = np.zeros((C, 3), dtype=np.int64)
    np.add.at(S, vc, q)
    count = np.bincount(vc, minlength=C).astype(np.int64)
    cell = np.zeros((C, 3), dtype=np.int64)
    cell[vc] = i
    lo64 = np.asarray(lo, dtype=np.float32).astype(np.float64)
    h64 = float(np.float32(h))
    m = S.astype(np.float64) / (count.astype(np.float64) * 4294967296.0)[:, None]
    p = lo64 + (cell.astype(np.float64) + m) * h64
    d = v32.astype(np.float64) - p[vc]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    best = np.full(C, np.inf)
    np.minimum.at(best, vc, d2)
    at_best = d2 == best[vc]
    rep = np.full(C, V, dtype=np.int64)
    np.minimum.at(rep, vc[at_best], np.nonzero(at_best)[0])
    ties = int((np.bincount(vc[at_best], minlength=C) > 1).sum())
    placed = p.astype(np.float32) if placement == 'mean' else v32[rep]
    return vc.astype(np.int32), C, placed, rep.astype(np.int32), ties


def canonical(triples, dedupe):
    """The canonical triples int64 [F, 3] of remapped faces: the smallest id rotated to the front; ascending for 'unoriented'."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    if dedupe == 'unoriented':
        return np.sort(t, axis=1)
    shift = np.argmin(t, axis=1)                             # (three different ids: one smallest)
    return np.stack([t[np.arange(len(t)), (shift + k) % 3] for k in range(3)], axis=1)


def cluster_faces(faces, vertex_cluster, dedupe='oriented'):
    """-> (remapped int32 [F, 3], keep uint8 [F])."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vc = np.asarray(vertex_cluster, dtype=np.int64)
    assert len(f) == 0 or (f.min() >= 0 and f.max() < len(vc))
    r = vc[f] if len(f) else f
    keep = (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])
    if dedupe is not None and keep.any():
        idx = np.nonzero(keep)[0]
        _, first = np.unique(canonical(r[idx], dedupe), axis=0, return_index=True)          # (the first occurrence: the smallest face index)
        keep[:] = False
        keep[idx[first]] = True
    return r.astype(np.int32), keep.astype(np.uint8)


def simplify(vertices, faces, lo, h, n, placement='mean', dedupe='oriented'):
    """-> (vertices float32 [V', 3], faces int32 [F', 3], kept_vertex_index int32 [V'])."""
    vc, C, placed, rep, _ = cluster(vertices, lo, h, n, placement)
    r, keep = cluster_faces(faces, vc, dedupe)
    kept = r[keep.astype(bool)].astype(np.int64)
    used = np.zeros(C, dtype=bool)
    used[kept.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return placed[used], new[kept].astype(np.int32).reshape(-1, 3), rep[used]


# ---- the stated hash functions -------------------------------------------------------------------------------------------------------------
def table_slots(n):
    t = 256
    while t < 2 * n:
        t *= 2
    return t


def cell_hash(key, bits):
    return ((int(key) * MUL) & MASK64) >> (64 - bits)


def face_hash(a, b, c, bits):
    return ((((((int(a) << 32 | int(b)) * MUL) & MASK64) >> (64 - bits)) + int(c)) & ((1 << bits) - 1))


def colliding_cells(count, bits, slot=5):
    """`count` different keys below 2^63 whose walks all start at `slot` of a table of 2^bits slots: key * MUL = slot << (64 - bits) | j
    is solved for key with the inverse of MUL modulo 2^64."""
    inverse = pow(MUL, -1, 1 << 64)
    keys, j = [], 0
    while len(keys) < count:
        key = ((slot << (64 - bits) | j) * inverse) & MASK64
        j += 1
        if key < 1 << 63:
            assert cell_hash(key, bits) == slot
            keys.append(key)
    return keys


def vertices_of_keys(keys):
    """The centres of the cells with these keys in the grid lo = 0, h = 1, n = 2^21: fp32 holds i + 0.5 exactly for i < 2^21."""
    k = np.asarray(keys, dtype=np.uint64).astype(np.int64)
    cell = np.stack([k >> 42, (k >> 21) & 0x1fffff, k & 0x1fffff], axis=1)
    return (cell.astype(np.float64) + 0.5).astype(np.float32)


def colliding_triples(count, bits, n_ids, dedupe, slot=9):
    """`count` different canonical triples (0, b, c) over ids below n_ids (>= 2^bits) whose walks all start at `slot`: c is solved from
    the hash of (0, b)."""
    out, b = [], 1
    while len(out) < count:
        assert b < n_ids
        c = (slot - face_hash(0, b, 0, bits)) % (1 << bits)
        if c not in (0, b) and (dedupe != 'unoriented' or c > b):
            assert face_hash(0, b, c, bits) == slot
            out.append((0, b, c))
        b += 1
    return np.asarray(out, dtype=np.int32)


# ---- shared inputs -------------------------------------------------------------------------------------------------------------------------
def fan(V):
    """Triangles (0, i, i + 1): V - 2 faces around vertex 0."""
    i = np.arange(1, max(V - 1, 1), dtype=np.int32)
    return np.stack([np.zeros_like(i), i, i + 1], axis=1) if V >= 3 else np.zeros((0, 3), dtype=np.int32)


def strip(V):
    """Triangles (i, i + 1, i + 2) with alternating winding."""
    i = np.arange(0, max(V - 2, 0), dtype=np.int32)
    f = np.stack([i, i + 1, i + 2], axis=1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    return f


def random_vertices(V, seed, lo=(-1.0, -1.25, -0.5), hi=(1.0, 0.75, 1.0)):
    rng = np.random.default_rng(seed)
    return (np.asarray(lo) + rng.random((V, 3)) * (np.asarray(hi) - np.asarray(lo))).astype(np.float32)


def ball_mesh(res=32, radius_cells=None):
    """The surface-nets mesh of a ball of radius 0.8 in the box [-1, 1]^3 on a lattice of res^3 cells (tests/mesh_reference.py) ->
    (vertices float32 [V, 3], faces int32 [F, 3])."""
    from tests import mesh_reference as M
    r = 0.4 * res if radius_cells is None else radius_cells
    field = M.ball((res,) * 3, (res / 2 + 0.25, res / 2 - 0.125, res / 2 + 0.0625), r)
    vertices, faces = M.surface_nets(field, 0.0, [-1.0] * 3, [1.0] * 3)
    return vertices.astype(np.float32), faces.astype(np.int32)
