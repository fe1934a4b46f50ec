"""The cull of the faces no registered panorama saw as include/perf_hip_meshvis.h states it, in numpy float64: the vertex tests in the
exact real-number semantics of the reference's formulas (direction_to_img_coord, grid_sample with align_corners=False and border padding),
the face rule operation for operation as the header writes it, the compaction as plain index arithmetic.  The yardstick of
tests/test_cpu_meshvis_reference.py and tests/test_gpu_meshvis.py, written from the statement, not from the kernels.  Also the inputs both
files use.

A view is a dict {'pose': float32 [4, 4], 'distance_map': float32 [H, W]} (the map already masked: 0 where nothing was stored)."""
import functools

import numpy as np

from tests import mesh_reference as R
from tests import meshcc_reference as CC

U = 2.0 ** -24                # the unit roundoff of fp32


# ---- stage 1 ----------------------------------------------------------------------------------------------------------------------------
def lookup(vertices, view):
    """-> dict of float64 [V]: dist, proj, and what guard() needs (z, rho: the unit direction's height and distance from the polar axis,
    alpha).  Everything in float64 from the fp32 values."""
    p = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    pose = np.asarray(view['pose'], dtype=np.float32).astype(np.float64)
    m = np.asarray(view['distance_map'], dtype=np.float32).astype(np.float64)
    h, w = m.shape
    with np.errstate(invalid='ignore', divide='ignore'):
        local = (p - pose[:3, 3]) @ pose[:3, :3]                # R^T (p - t), row by row
        dist = np.sqrt((local ** 2).sum(axis=1))
        d = local / dist[:, None]
        d = d / np.sqrt((d ** 2).sum(axis=1))[:, None]
        beta, alpha = np.arcsin(np.clip(d[:, 2], -1, 1)), np.arctan2(d[:, 1], d[:, 0])
        row, col = -beta / np.pi + 0.5, -(alpha / (2 * np.pi)) + 0.5
        gx, gy = col * 2 - 1, row * 2 - 1
        ix = np.clip(((gx + 1) * w - 1) / 2, 0, w - 1)
        iy = np.clip(((gy + 1) * h - 1) / 2, 0, h - 1)
        bad = np.isnan(ix) | np.isnan(iy)
        ix, iy = np.where(bad, 0.0, ix), np.where(bad, 0.0, iy)
        x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
        wx1, wy1 = ix - x0, iy - y0
        at = lambda yy, xx: np.where((yy < h) & (xx < w), m[np.minimum(yy, h - 1), np.minimum(xx, w - 1)], 0.0)
        proj = at(y0, x0) * (1 - wx1) * (1 - wy1) + at(y0, x0 + 1) * wx1 * (1 - wy1) + at(y0 + 1, x0) * (1 - wx1) * wy1 + at(y0 + 1, x0 + 1) * wx1 * wy1
        proj = np.where(bad, np.nan, proj)
    return {'dist': dist, 'proj': proj, 'z': np.abs(d[:, 2]), 'rho': np.hypot(d[:, 0], d[:, 1]), 'alpha': alpha}


def margins(vertices, view):
    """dist - proj, float64 [V]: view k sees a vertex iff its margin < tol, and has it in free space iff its margin < -free_tol."""
    r = lookup(vertices, view)
    return r['dist'] - r['proj']


def guard(view, vertices):
    """float64 [V]: a bound of |the fp32 chain's (dist - (proj + eps)) - the exact margin - eps| for each vertex, so that the device's
    decision and the restatement's can differ only where |margin - eps| <= guard.  Derived from the chain of pano_reproject_kernel with
    u = 2^-24, first order, doubled at the end for the second:
      dist.  q = p - t: u |q_i| per component.  l_a = sum_b rt_ab q_b: three products and two sums, each (1 + u), on top of q's own:
        |dl_a| <= 4 u sum_b |rt_ab| |q_b| <= 4 sqrt(3) u |q|, so |dl| <= 12 u |q|.  dist = sqrt(l . l): 2.5 u relative for the squares,
        the sums and the root: |d dist| <= 16 u dist.
      direction.  d = l / dist, normalised once more: each component, of size <= 1, moves by at most (12 + 2.5 + 1) u from l and dist
        and the division, and by 4 u + 1 u from the second norm and division: dd = 24 u absolute with room.
      beta = asinf(d_z).  asin is steepest at the ends and convex on [0, 1], so moving z = |d_z| by dd moves it by at most
        asin(min(z + dd, 1)) - asin(z), computed here, which is sqrt(2 dd) at a pole and dd / sqrt(1 - z^2) away from it; asinf itself is
        within 4 ulp of a value below 2: 8 u.
      alpha = atan2f(d_y, d_x).  Moving (d_x, d_y), at rho from the origin, by at most sqrt(2) dd turns it by at most
        asin(sqrt(2) dd / rho) -- any angle at all (2 pi) when rho <= sqrt(2) dd, at a pole; atan2f is within 6 ulp of a value below 4: 24 u.
      pixel coordinates.  row = -beta / pi + 0.5 and col likewise are at most 1, as are the steps to gx, gy and (g + 1); each of the five
        roundings and the fp32 value of pi costs at most 2 u there, before the scale by H or W: d iy <= H (d beta / pi + 10 u),
        d ix <= W (d alpha / (2 pi) + 10 u).  The clamp does not stretch them.
      proj.  The bilinear interpolant's slope along x is a convex combination of differences of horizontally adjacent pixels, along y of
        vertically adjacent ones: |d proj| <= Gx d ix + Gy d iy with Gx, Gy the map's largest such differences.  Across the +-pi seam
        (pi - |alpha| <= d alpha) the clamped column jumps from 0 to W - 1: J = the largest |m[y, 0] - m[y, W - 1]| is added there.
        The four weights, four products and three sums of the accumulation and the sum with eps: 16 u max|m| (|eps| <= max|m| is
        assumed: the tests' tolerances are at most 1/8, their maps reach 0.44 and more).
    Infinite where the vertex sits on a view's centre."""
    r = lookup(vertices, view)
    m = np.asarray(view['distance_map'], dtype=np.float32).astype(np.float64)
    h, w = m.shape
    gx = np.abs(np.diff(m, axis=1)).max() if w > 1 else 0.0
    gy = np.abs(np.diff(m, axis=0)).max() if h > 1 else 0.0
    jump = np.abs(m[:, 0] - m[:, -1]).max()
    top = np.abs(m).max()
    dd = 24 * U
    with np.errstate(invalid='ignore'):
        d_beta = np.arcsin(np.minimum(r['z'] + dd, 1.0)) - np.arcsin(np.minimum(r['z'], 1.0)) + 8 * U
        turn = np.sqrt(2.0) * dd / np.maximum(r['rho'], 1e-300)
        d_alpha = np.where(turn < 1.0, np.arcsin(np.minimum(turn, 1.0)), 2 * np.pi) + 24 * U
        d_iy = h * (d_beta / np.pi + 10 * U)
        d_ix = w * (d_alpha / (2 * np.pi) + 10 * U)
        seam = (np.pi - np.abs(r['alpha'])) <= d_alpha
        g = 16 * U * r['dist'] + gx * d_ix + gy * d_iy + np.where(seam, jump, 0.0) + 16 * U * top
    return np.where(np.isfinite(g), 2 * g, np.inf)


def vertex_bits(vertices, views, tol, free_tol):
    """-> (visible uint64 [V], free uint64 [V]) by the float64 margins.  tol and free_tol are rounded to fp32 first, as the C ABI takes them."""
    tol, free_tol = float(np.float32(tol)), float(np.float32(free_tol))
    n = len(np.asarray(vertices).reshape(-1, 3))
    visible, free = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for k, view in enumerate(views):
        mg = margins(vertices, view)
        with np.errstate(invalid='ignore'):
            visible |= (mg < tol).astype(np.uint64) << np.uint64(k)
            free |= (mg < -free_tol).astype(np.uint64) << np.uint64(k)
    return visible, free


def outside_guard(vertices, views, tol, free_tol):
    """bool [V]: no view has the vertex within its guard of either threshold."""
    tol, free_tol = float(np.float32(tol)), float(np.float32(free_tol))
    ok = np.ones(len(vertices), dtype=bool)
    for view in views:
        mg, g = margins(vertices, view), guard(view, vertices)
        with np.errstate(invalid='ignore'):
            ok &= (np.abs(mg - tol) > g) & (np.abs(mg + free_tol) > g)
    return ok


# ---- stage 2 ----------------------------------------------------------------------------------------------------------------------------
def _popcount(x):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    return np.unpackbits(x.view(np.uint8)).reshape(len(x), 64).sum(axis=1).astype(np.int64)


def face_keep(faces, vertices, visible, free, centres, facing=True, min_views=1, carve=False):
    """uint8 [F], the header's sequence operation for operation in float64 (numpy does not contract).  Every index in [0, V)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(centres, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    k_views = len(t)
    low = np.uint64((1 << k_views) - 1)
    vis, fre = np.asarray(visible).astype(np.uint64), np.asarray(free).astype(np.uint64)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    bits = vis[a] & vis[b] & vis[c] & low
    if facing:
        e1, e2 = v[b] - v[a], v[c] - v[a]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        for k in range(k_views):
            g = t[k] - v[a]
            with np.errstate(invalid='ignore', over='ignore'):
                s = (nx * g[:, 0] + ny * g[:, 1]) + nz * g[:, 2]
                facing_k = s > 0
            bits &= ~np.where(facing_k, np.uint64(0), np.uint64(1) << np.uint64(k))
    keep = _popcount(bits) >= min_views
    if carve:
        keep &= ((fre[a] | fre[b] | fre[c]) & low) == 0
    return keep.astype(np.uint8)


# ---- stage 3 ----------------------------------------------------------------------------------------------------------------------------
def filter_faces(vertices, faces, keep):
    """-> (vertices [V', 3], faces int32 [F', 3] re-indexed, kept_vertex_index int32 [V']): a vertex is kept iff a kept face names it;
    relative order kept.  A sequential pass, as the statement reads."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keep = np.asarray(keep).astype(bool)
    n = len(vertices)
    named = np.zeros(n, dtype=bool)
    for f in faces[keep]:
        named[f] = True
    index = np.array([i for i in range(n) if named[i]], dtype=np.int32)
    new = np.full(n, -1, dtype=np.int64)
    for rank, i in enumerate(index):
        new[i] = rank
    return np.asarray(vertices)[index], new[faces[keep]].astype(np.int32).reshape(-1, 3), index


def cull(vertices, faces, views, tol=1 / 256, free_tol=None, facing=True, min_views=1, carve=False):
    """The three stages -> (vertices, faces, kept_vertex_index, face_keep)."""
    free_tol = tol if free_tol is None else free_tol
    visible, free = vertex_bits(vertices, views, tol, free_tol)
    centres = np.stack([np.asarray(v['pose'], dtype=np.float32)[:3, 3] for v in views])
    keep = face_keep(faces, vertices, visible, free, centres, facing, min_views, carve)
    return filter_faces(vertices, faces, keep) + (keep,)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
MAP_SIZES = ((16, 32), (33, 64), (7, 5))
TOL, FREE_TOL = 1 / 256, 1 / 64


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def make_views(n_views, seed=0):
    """n_views views: rotated, off-centre poses; map sizes 16 x 32, 33 x 64 and 7 x 5 in turn; smooth maps between 0.35 and 1.25 with
    zeroed (invalid) patches in every third view and a different column either side of the seam."""
    rng = np.random.default_rng(1000 + seed)
    views = []
    for k in range(n_views):
        h, w = MAP_SIZES[k % 3]
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = _rotation(rng).astype(np.float32)
        pose[:3, 3] = rng.uniform(-0.3, 0.3, 3).astype(np.float32)
        y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing='ij')
        m = 0.8 + 0.3 * np.sin(2.0 * x + k) * np.cos(3.0 * y) + 0.15 * x
        if k % 3 == 1:
            m[h // 4:h // 2, w // 3:w // 2] = 0.0
        m = m.astype(np.float32)
        for a in (pose, m):
            a.setflags(write=False)
        views.append({'pose': pose, 'distance_map': m})
    return tuple(views)


@functools.lru_cache(maxsize=None)
def guard_free_vertices(n_views, n, seed=0, tol=TOL, free_tol=FREE_TOL):
    """n random vertices in [-1.5, 1.5]^3 none of which lies within the guard of a threshold of any of make_views(n_views, seed): drawn with
    a fifth to spare, those inside a guard band rejected; at least 90 % of the draw must remain."""
    views = make_views(n_views, seed)
    rng = np.random.default_rng(2000 + 17 * seed + n_views)
    draw = rng.uniform(-1.5, 1.5, size=(n + n // 5 + 8, 3)).astype(np.float32)
    ok = outside_guard(draw, views, tol, free_tol)
    assert ok.sum() >= 0.9 * len(draw), (n_views, n, int(ok.sum()), len(draw))
    kept = draw[ok][:n]
    assert len(kept) == n
    kept.setflags(write=False)
    return kept


def special_vertices(views):
    """The degenerate vertices: at every view's centre, at its poles, on its +-pi seam, NaN, +-inf, 10^6 away."""
    out = [[np.nan, 0, 0], [0, np.nan, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [np.inf, np.inf, -np.inf], [1e6, -1e6, 1e6], [-1e6, 0, 0], [0, 0, 0]]
    for view in views[:8]:
        pose = np.asarray(view['pose'], dtype=np.float64)
        r, t = pose[:3, :3], pose[:3, 3]
        out.append(t)
        for local in ([0, 0, 0.5], [0, 0, -0.7], [-0.5, 0.0, 0.1], [-0.5, 1e-9, 0.0], [-0.5, -1e-9, 0.0], [0.5, 0, 0]):
            out.append(r @ np.array(local) + t)
    return np.array(out, dtype=np.float32)


# the hollow sphere of tests/meshcc_reference.py and the same shell with a tunnel of radius 1.7 cells carved through it along +x: ONE
# component with a positive signed volume, the trained room's situation
CENTRE = (0.02, 0.02, 0.02)              # lattice (10.2, 10.2, 10.2) in the box [-1, 1]^3 of 20^3 cells


def tunnel_field(cells=20):
    """cells: 20, or more to pad the lattice (the same field on more cells: the box grows with it, 0.1 per cell)."""
    g = np.meshgrid(*[np.arange(cells + 1, dtype=np.float64)] * 3, indexing='ij')
    shell = 1.6 - np.abs(np.sqrt(sum((x - 10.2) ** 2 for x in g)) - 6.0)
    rho = np.sqrt((g[1] - 10.2) ** 2 + (g[2] - 10.2) ** 2)
    return np.where(g[0] > 10.2, np.minimum(shell, rho - 1.7), shell).astype(np.float32)


def constant_view(centre=CENTRE, value=0.6, size=(16, 32)):
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = centre
    return {'pose': pose, 'distance_map': np.full(size, value, dtype=np.float32)}


@functools.lru_cache(maxsize=None)
def reference_mesh(which):
    """(vertices float32 [V, 3], faces int32 [F, 3]) of 'hollow_sphere' or 'tunnel' by the float64 surface nets, rounded to fp32."""
    field = CC.hollow_sphere() if which == 'hollow_sphere' else tunnel_field()
    vertices, faces = R.surface_nets(field, 0.0, CC.SPHERE_LO, CC.SPHERE_HI)
    vertices, faces = vertices.astype(np.float32), faces.astype(np.int32)
    vertices.setflags(write=False)
    faces.setflags(write=False)
    return vertices, faces
