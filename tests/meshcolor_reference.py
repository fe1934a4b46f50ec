"""The colouring of a mesh from the registered panoramas and the vertex normals from faces as include/perf_hip_meshcolor.h states them, in
numpy float64: the normal sums operation for operation as the header writes them (numpy does not contract), the colour sample as the
look-up of tests/meshvis_reference.py applied per channel, the weights and the blend in the header's order.  The yardstick of
tests/test_cpu_meshcolor_reference.py and tests/test_gpu_meshcolor.py, written from the statement, not from the kernels.  Also the inputs
both files use.

The blend takes the VISIBLE BITS AS AN INPUT: the GPU tests pass it the device's own, so the blend is compared where it is continuous and
the depth decision needs no guard band."""
import functools
import math

import numpy as np

from tests import meshvis_reference as V

U = V.U                       # the unit roundoff of fp32


# ---- stage A ----------------------------------------------------------------------------------------------------------------------------
def scale_log2(box):
    """s = 40 - ceil(log2(D^2)), D^2 the squared diagonal of box = (lo, hi); 0 for a box of no extent."""
    d2 = sum((float(b) - float(a)) ** 2 for a, b in zip(*box))
    if not math.isfinite(d2) or d2 <= 0.0:
        return 0
    return max(-200, min(200, 40 - math.ceil(math.log2(d2))))


def bad_face(faces, n_vertices):
    """The smallest index of a face with an index outside [0, V), or -1."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = np.nonzero(((f < 0) | (f >= n_vertices)).any(axis=1))[0]
    return int(bad[0]) if len(bad) else -1


def normal_sums(vertices, faces, s):
    """int64 [V, 3]: q_c = rint(n_c * 2^s) of every face added at its three vertices; a face whose scaled normal is not finite or reaches
    2^62, and a face with an index outside [0, V), contributes nothing.  Sums wrap as int64 does."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    acc = np.zeros((len(v), 3), dtype=np.int64)
    f = f[((f >= 0) & (f < len(v))).all(axis=1)]
    if not len(f):
        return acc
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        e1, e2 = v[b] - v[a], v[c] - v[a]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        scaled = np.stack([nx, ny, nz], axis=1) * 2.0 ** int(s)
        ok = (np.abs(scaled) < 2.0 ** 62).all(axis=1)          # (a NaN fails)
    q = np.rint(scaled[ok]).astype(np.int64)
    with np.errstate(over='ignore'):
        for corner in range(3):
            np.add.at(acc, f[ok, corner], q)
    return acc


def normals(acc):
    """float64 [V, 3]: A / sqrt((Ax Ax + Ay Ay) + Az Az), exactly 0 where the length is 0 (to be rounded to fp32 once)."""
    a = np.asarray(acc, dtype=np.int64).astype(np.float64).reshape(-1, 3)
    length = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(length[:, None] == 0, 0.0, a / length[:, None])


# ---- stage B ----------------------------------------------------------------------------------------------------------------------------
def sample(vertices, view, color_map):
    """float64 [V, 3]: the look-up of tests/meshvis_reference.py over each channel of color_map [H, W, 3]."""
    cmap = np.asarray(color_map, dtype=np.float32)
    return np.stack([V.lookup(vertices, {'pose': view['pose'], 'distance_map': cmap[..., c]})['proj'] for c in range(3)], axis=1)


def view_weights(vertices, vertex_normals, view, facing, power):
    """(passes bool [V], w float64 [V]) of one view, the depth test apart: dist > 0 and finite; with facing s > 0 and
    w = cos^power / dist^2, else w = 1 / dist^2; w > 0."""
    p = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    dist = V.lookup(vertices, view)['dist']
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ok = (dist > 0) & np.isfinite(dist)
        d2 = dist * dist
        if facing:
            n = np.asarray(vertex_normals, dtype=np.float32).astype(np.float64).reshape(-1, 3)
            g = np.asarray(view['pose'], dtype=np.float32).astype(np.float64)[:3, 3] - p
            s = (n[:, 0] * g[:, 0] + n[:, 1] * g[:, 1]) + n[:, 2] * g[:, 2]
            ok &= s > 0
            cos = s / (np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) * np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]))
            cp = cos
            for _ in range(int(power) - 1):
                cp = cp * cos
            w = cp / d2
        else:
            w = 1.0 / d2
        ok &= w > 0
    return ok, np.where(ok, w, 0.0)


def blend(vertices, vertex_normals, views, color_maps, visible_bits, facing=True, power=2, select='blend'):
    """-> dict: colors float64 [V, 3] (NaN where no view passed: the caller's fallback), weight float64 [V], used uint64 [V], best_view
    int8 [V], and per view w [K, V] (0 where the view did not pass) and samples [K, V, 3]."""
    n = len(np.asarray(vertices).reshape(-1, 3))
    k_views = len(views)
    visible = np.asarray(visible_bits).astype(np.uint64)
    used = np.zeros(n, dtype=np.uint64)
    w_all, c_all = np.zeros((k_views, n)), np.zeros((k_views, n, 3))
    num, den = np.zeros((n, 3)), np.zeros(n)
    best_w, best_k, best_c = np.zeros(n), np.full(n, -1, dtype=np.int8), np.full((n, 3), np.nan)
    for k, (view, cmap) in enumerate(zip(views, color_maps)):
        ok, w = view_weights(vertices, vertex_normals, view, facing, power)
        ok &= ((visible >> np.uint64(k)) & np.uint64(1)).astype(bool)
        w = np.where(ok, w, 0.0)
        c = np.where(ok[:, None], sample(vertices, view, cmap), 0.0)
        used |= ok.astype(np.uint64) << np.uint64(k)
        w_all[k], c_all[k] = w, c
        num, den = num + w[:, None] * c, den + w
        better = ok & ((best_k < 0) | (w > best_w))
        best_w, best_k, best_c = np.where(better, w, best_w), np.where(better, np.int8(k), best_k), np.where(better[:, None], c, best_c)
    some = used != 0
    with np.errstate(invalid='ignore', divide='ignore'):
        if select == 'best':
            colors, weight, best_view = best_c, best_w, best_k
        else:
            colors, weight, best_view = np.where(some[:, None], num / den[:, None], np.nan), den, np.full(n, -1, dtype=np.int8)
    return {'colors': colors, 'weight': np.where(some, weight, 0.0), 'used': used, 'best_view': best_view, 'w': w_all, 'samples': c_all}


def sample_bound(vertices, view, color_map):
    """float64 [V]: the bound of a colour sample's error, the largest of the three channels' V.guard with the channel as the view's map."""
    cmap = np.asarray(color_map, dtype=np.float32)
    return np.max([V.guard({'pose': view['pose'], 'distance_map': cmap[..., c]}, vertices) for c in range(3)], axis=0)


def color_bound(vertices, views, color_maps, used):
    """float64 [V]: |device - reference| per colour component is at most the largest sample bound among the used views, + 2^-18 for the
    weights (w_k carries the fp32 dist's 16 u relative error twice: a convex combination with weights perturbed by eps moves by at most
    2 eps times the colour range <= 1) + 2^-24 for the final rounding.  0 where no view is used."""
    used = np.asarray(used).astype(np.uint64)
    out = np.zeros(len(used))
    for k, (view, cmap) in enumerate(zip(views, color_maps)):
        on = ((used >> np.uint64(k)) & np.uint64(1)).astype(bool)
        if on.any():
            out = np.where(on, np.maximum(out, sample_bound(vertices, view, cmap)), out)
    return np.where(used != 0, out + 2.0 ** -18 + 2.0 ** -24, 0.0)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_color_maps(n_views, seed=0):
    """Smooth colour maps in [0.1, 0.9] of the sizes of V.make_views(n_views, seed), a different one per view and channel."""
    maps = []
    for k, view in enumerate(V.make_views(n_views, seed)):
        h, w = view['distance_map'].shape
        y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing='ij')
        m = np.stack([0.5 + 0.4 * np.sin(2.0 * x + 0.7 * k + c) * np.cos(2.5 * y - c) for c in range(3)], axis=2).astype(np.float32)
        m.setflags(write=False)
        maps.append(m)
    return tuple(maps)


@functools.lru_cache(maxsize=None)
def random_vertices(n, seed=0):
    """n vertices uniform in [-0.6, 0.6]^3, fp32."""
    v = np.random.default_rng(3000 + seed).uniform(-0.6, 0.6, size=(n, 3)).astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def random_normals(n, seed=0):
    """n unit vectors (to fp32 rounding), uniform on the sphere."""
    g = np.random.default_rng(4000 + seed).normal(size=(n, 3))
    g = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    g.setflags(write=False)
    return g


def fan(n_vertices, seed=0):
    """A fan around vertex 0 over n_vertices random vertices: faces (0, i, i + 1)."""
    v = np.random.default_rng(5000 + seed + n_vertices).uniform(-1, 1, size=(n_vertices, 3)).astype(np.float32)
    i = np.arange(1, max(n_vertices - 1, 1), dtype=np.int32)
    f = np.stack([np.zeros_like(i), i, i + 1], axis=1) if n_vertices >= 3 else np.zeros((0, 3), dtype=np.int32)
    return v, f.astype(np.int32)


def strip(n_vertices, seed=0):
    """A triangle strip over n_vertices random vertices: faces (i, i + 1, i + 2), every other one flipped."""
    v = np.random.default_rng(6000 + seed + n_vertices).uniform(-1, 1, size=(n_vertices, 3)).astype(np.float32)
    i = np.arange(0, max(n_vertices - 2, 0), dtype=np.int32)
    f = np.stack([i, np.where(i % 2 == 0, i + 1, i + 2), np.where(i % 2 == 0, i + 2, i + 1)], axis=1)
    return v, f.astype(np.int32)
