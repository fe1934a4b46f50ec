"""Naive surface nets as include/perf_hip_mesh.h states them, in vectorised numpy and float64 on the fp32 field it is given: the
yardstick of tests/test_cpu_mesh_reference.py and tests/test_gpu_mesh.py, written from the statement, not from the kernel (it works
on whole arrays, has no chunks, no scan and no workspace).  Also the mesh properties the tests assert."""
import numpy as np

# the 12 edges of a cell: pairs a < b of corners (number 4 dx + 2 dy + dz) that differ in one offset, in lexicographic order of (a, b)
EDGES = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count('1') == 1]
assert EDGES == [(0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7)]


def _offset(c):
    return (c >> 2) & 1, (c >> 1) & 1, c & 1


def surface_nets(field, thr, lo, hi):
    """field: float32 [nx+1, ny+1, nz+1]; thr, lo [3], hi [3]: rounded to float32 first, as the C ABI takes them.
    -> (vertices float64 [V, 3], faces int64 [F, 3])."""
    field = np.asarray(field)
    assert field.dtype == np.float32 and field.ndim == 3
    n = np.array(field.shape) - 1
    nx, ny, nz = (int(v) for v in n)
    thr = float(np.float32(thr))
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
    hi = np.asarray(hi, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        inside = field >= np.float32(thr)                      # (a NaN compares false: outside)
    n_in = np.zeros((nx, ny, nz), dtype=np.int32)
    for c in range(8):
        dx, dy, dz = _offset(c)
        n_in += inside[dx:dx + nx, dy:dy + ny, dz:dz + nz]
    active = (n_in > 0) & (n_in < 8)
    rank = np.where(active, (np.cumsum(active.reshape(-1)) - 1).reshape(active.shape), -1)           # linear cell order
    ai, aj, ak = np.nonzero(active)
    cell = np.stack([ai, aj, ak], axis=1).astype(np.float64)
    val = [field[ai + _offset(c)[0], aj + _offset(c)[1], ak + _offset(c)[2]].astype(np.float64) for c in range(8)]
    ins = [inside[ai + _offset(c)[0], aj + _offset(c)[1], ak + _offset(c)[2]] for c in range(8)]
    total = np.zeros((3, len(ai)))
    crossings = np.zeros(len(ai))
    for a, b in EDGES:
        cross = (ins[a] != ins[b]).astype(np.float64)
        with np.errstate(invalid='ignore', divide='ignore'):
            t = (thr - val[a]) / (val[b] - val[a])
        t = np.clip(np.where(np.isnan(t), 0.5, t), 0.0, 1.0)
        axis = {4: 0, 2: 1, 1: 2}[b - a]
        for k in range(3):                                     # the crossing point: corner a's offset, t along the edge's axis
            if k == axis:
                total[k] += cross * t
            elif _offset(a)[k]:
                total[k] += cross
        crossings += cross
    p = cell + (total / crossings).T if len(ai) else cell
    vertices = lo + p * (hi - lo) / n.astype(np.float64)

    keys, quads = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        start, stop = [0, 0, 0], [0, 0, 0]
        start[a], stop[a] = 0, n[a]                            # p[a] < n[a]
        start[b], stop[b] = 1, n[b]                            # 1 <= p[b] <= n[b] - 1
        start[c], stop[c] = 1, n[c]
        if stop[b] <= start[b] or stop[c] <= start[c]:
            continue
        here = inside[start[0]:stop[0], start[1]:stop[1], start[2]:stop[2]]
        e = [0, 0, 0]; e[a] = 1
        there = inside[start[0] + e[0]:stop[0] + e[0], start[1] + e[1]:stop[1] + e[1], start[2] + e[2]:stop[2] + e[2]]
        idx = np.nonzero(here != there)
        pt = np.stack([idx[0] + start[0], idx[1] + start[1], idx[2] + start[2]], axis=1)
        eb = np.zeros(3, dtype=np.int64); eb[b] = 1
        ec = np.zeros(3, dtype=np.int64); ec[c] = 1
        r = lambda q: rank[q[:, 0], q[:, 1], q[:, 2]]
        quad = np.stack([r(pt - eb - ec), r(pt - ec), r(pt), r(pt - eb)], axis=1)
        assert quad.min(initial=0) >= 0                        # (an edge whose ends differ makes its four cells active)
        outside = ~inside[pt[:, 0], pt[:, 1], pt[:, 2]]
        quad[outside] = quad[outside][:, ::-1]
        keys.append(((pt[:, 0] * (ny + 1) + pt[:, 1]) * (nz + 1) + pt[:, 2]) * 3 + a)
        quads.append(quad)
    if not quads or sum(len(q) for q in quads) == 0:
        return vertices, np.zeros((0, 3), dtype=np.int64)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    quads = quads[np.argsort(keys, kind='stable')]
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    return vertices, faces.astype(np.int64)


def ball(shape, centre, radius):
    """fp32 corner values of a solid ball on a lattice of `shape` cells, in lattice units: radius - |x - centre| (>= 0 inside)."""
    g = np.meshgrid(*[np.arange(s + 1, dtype=np.float64) for s in shape], indexing='ij')
    return (radius - np.sqrt(sum((x - c) ** 2 for x, c in zip(g, centre)))).astype(np.float32)


def is_closed_oriented_manifold(faces):
    """Every directed edge occurs once and its reverse once."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = e[:, 0] * (int(f.max()) + 1) + e[:, 1]
    back = e[:, 1] * (int(f.max()) + 1) + e[:, 0]
    return len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(back))


def has_repeated_index(faces):
    f = np.asarray(faces)
    return bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any())


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, i]] for i in range(3))
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)
