"""The texture atlas of include/perf_hip_meshtex.h in numpy float64 and int64, written from the header's statement, not from the kernels:
the layout, the owner of a texel, the corner UVs, the texels' points and normals rounded to fp32 once, the coverage codes, the flag of a
face with an index outside [0, V), the interpolated fallback; and a bilinear sampler of an atlas image.  Every floating-point operation is
one numpy float64 operation, so each rounds once and nothing is contracted, as the header demands of the device.  Texel (column i, row j)
is element j S + i of every per-texel array."""
import numpy as np

SHAPES = ((64, 4, 512), (64, 5, 287), (64, 7, 161), (128, 8, 511), (64, 16, 31))          # (S, T, F): full, and odd face counts


def capacity(size, tile):
    return 2 * (size // tile) ** 2


def corners(n_faces, size, tile):
    """int64 [F, 3, 2]: the (column, row) of the corner texels a, b, c of every face."""
    f = np.arange(n_faces, dtype=np.int64)
    t, h, n, m = f >> 1, f & 1, size // tile, tile - 3
    x0, y0 = (t % n) * tile, (t // n) * tile
    out = np.empty((n_faces, 3, 2), dtype=np.int64)
    for k, (di, dj) in enumerate(((0, 0), (m, 0), (0, m))):
        out[:, k, 0] = np.where(h == 0, x0 + di, x0 + tile - 1 - di)
        out[:, k, 1] = np.where(h == 0, y0 + dj, y0 + tile - 1 - dj)
    return out


def uv(n_faces, size, tile):
    """fp32 [F, 3, 2]: (i + 0.5) / S in fp32 -- the sum is exact, the quotient rounds once."""
    c = corners(n_faces, size, tile)
    return (c.astype(np.float32) + np.float32(0.5)) / np.float32(size)


def owner(size, tile, n_faces):
    """Per texel, by the layout alone -> (face int64 [S, S] or -1, li, lj int64 [S, S], code uint8 [S, S]), indexed [row, column]."""
    row, col = np.meshgrid(np.arange(size, dtype=np.int64), np.arange(size, dtype=np.int64), indexing='ij')
    n = size // tile
    tx, ty = col // tile, row // tile
    i, j = col - tx * tile, row - ty * tile
    h = (i + j >= tile).astype(np.int64)
    face = 2 * (ty * n + tx) + h
    none = (tx >= n) | (ty >= n) | (face >= n_faces)
    li, lj = np.where(h == 1, tile - 1 - i, i), np.where(h == 1, tile - 1 - j, j)
    code = np.where(li + lj <= tile - 3, 1, 2).astype(np.uint8)
    return np.where(none, -1, face), np.where(none, 0, li), np.where(none, 0, lj), np.where(none, 0, code).astype(np.uint8)


def bad_face(faces, n_vertices):
    """The smallest index of a face with an index outside [0, V), or -1."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = np.nonzero(((f < 0) | (f >= n_vertices)).any(axis=1))[0]
    return int(bad[0]) if len(bad) else -1


def _rows(values, faces, face, k):
    """float64 [S, S, 3]: row faces[face, k] of values (fp32 [V, 3]) per texel; face must be valid where it is read."""
    return np.asarray(values, dtype=np.float32).astype(np.float64).reshape(-1, 3)[faces[face, k]]


def texels(vertices, faces, size, tile, normals=None, fallback=None):
    """The materialised route -> dict of flat per-texel arrays: points fp32 [S S, 3], point_normals fp32 [S S, 3], face_of int32 [S S],
    coverage uint8 [S S], fallback fp32 [S S, 3] (the interpolated per-vertex rows, when given), alpha / beta / gamma float64 [S S], and
    bad_face.  A texel of no face (a face with an index outside [0, V) included) holds point 0, normal 0, face_of -1, coverage 0."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    assert len(f) <= capacity(size, tile)
    face, li, lj, code = owner(size, tile, len(f))
    valid_face = ((f >= 0) & (f < len(v))).all(axis=1)
    live = face >= 0
    live[live] = valid_face[face[live]]
    face, code = np.where(live, face, -1), np.where(live, code, 0).astype(np.uint8)
    fs = np.where(valid_face[:, None], f, 0) if len(v) else np.zeros_like(f)          # (never read where the face is not live)
    safe = np.where(live, face, 0)
    m = float(tile - 3)
    beta, gamma = li.astype(np.float64) / m, lj.astype(np.float64) / m
    alpha = (1.0 - beta) - gamma
    out = {'face_of': face.astype(np.int32).reshape(-1), 'coverage': code.reshape(-1), 'alpha': alpha.reshape(-1), 'beta': beta.reshape(-1),
           'gamma': gamma.reshape(-1), 'bad_face': bad_face(f, len(v))}
    zero = np.zeros((size, size, 3), dtype=np.float32)
    if not live.any():
        out.update(points=zero.reshape(-1, 3), point_normals=zero.reshape(-1, 3).copy())
        if fallback is not None:
            out['fallback'] = zero.reshape(-1, 3).copy()
        return out
    with np.errstate(all='ignore'):
        a, b, c = (_rows(v, fs, safe, k) for k in range(3))
        B, G, A = beta[..., None], gamma[..., None], alpha[..., None]
        p = ((a + B * (b - a)) + G * (c - a)).astype(np.float32)
        if normals is None:
            e1, e2 = b - a, c - a
            nx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
            ny = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
            nz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
            length = np.sqrt((nx * nx + ny * ny) + nz * nz)
            nrm = np.stack([nx / length, ny / length, nz / length], axis=-1).astype(np.float32)
            nrm[length == 0.0] = 0.0
        else:
            na, nb, nc = (_rows(normals, fs, safe, k) for k in range(3))
            nrm = ((A * na + B * nb) + G * nc).astype(np.float32)
        out['points'] = np.where(live[..., None], p, zero).reshape(-1, 3)
        out['point_normals'] = np.where(live[..., None], nrm, zero).reshape(-1, 3)
        if fallback is not None:
            ca, cb, cc = (_rows(fallback, fs, safe, k) for k in range(3))
            out['fallback'] = np.where(live[..., None], ((A * ca + B * cb) + G * cc).astype(np.float32), zero).reshape(-1, 3)
    return out


def texel_position(n_faces, size, tile, face_ids, bary):
    """float64 [N, 2]: the (x, y) of points of faces in texel units, the centre of texel (i, j) at (i, j): the corners weighted by bary
    [N, 3] = (alpha, beta, gamma)."""
    c = corners(n_faces, size, tile).astype(np.float64)[np.asarray(face_ids, dtype=np.int64)]
    return (np.asarray(bary, dtype=np.float64)[:, :, None] * c).sum(axis=1)


def taps(xy, size):
    """The four bilinear taps of positions xy [N, 2] -> (columns int64 [N, 4], rows int64 [N, 4], weights float64 [N, 4]), NOT clamped: a
    tap outside the image shows as an index outside [0, S)."""
    x, y = xy[:, 0], xy[:, 1]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    cols = np.stack([x0, x0 + 1, x0, x0 + 1], axis=1).astype(np.int64)
    rows = np.stack([y0, y0, y0 + 1, y0 + 1], axis=1).astype(np.int64)
    weights = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], axis=1)
    return cols, rows, weights


def sample(image, xy):
    """Bilinear sampling of image [S, S, C] at xy, float64; taps clamped to the image."""
    size = image.shape[0]
    cols, rows, weights = taps(xy, size)
    values = np.asarray(image, dtype=np.float64)[np.clip(rows, 0, size - 1), np.clip(cols, 0, size - 1)]
    return (values * weights[..., None]).sum(axis=1)


def face_points(n_faces, per_face, seed=0):
    """(face_ids int64 [N], bary float64 [N, 3]): per_face random interior points and the 7 edge / corner points (three corners, three edge
    midpoints, the centroid's neighbour on the hypotenuse) of every face."""
    rng = np.random.default_rng(7000 + seed)
    r = rng.uniform(size=(n_faces, per_face, 2))
    flip = r.sum(axis=2) > 1
    r[flip] = 1 - r[flip]
    inner = np.concatenate([1 - r.sum(axis=2, keepdims=True), r], axis=2)
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5], [0, 0.25, 0.75]], dtype=np.float64)
    bary = np.concatenate([inner, np.broadcast_to(fixed, (n_faces, 7, 3))], axis=1)
    ids = np.repeat(np.arange(n_faces, dtype=np.int64), per_face + 7)
    return ids, bary.reshape(-1, 3)


def random_mesh(n_vertices, n_faces, seed=0):
    """fp32 [V, 3] uniform in [-0.6, 0.6]^3 and int32 [F, 3] random faces of three different vertices."""
    rng = np.random.default_rng(8000 + seed + n_faces)
    v = rng.uniform(-0.6, 0.6, size=(n_vertices, 3)).astype(np.float32)
    f = np.stack([rng.permutation(n_vertices)[:3] for _ in range(n_faces)]).astype(np.int32) if n_faces else np.zeros((0, 3), np.int32)
    return v, f


def parse_obj(path):
    """(v float64 [V, 3], vt float64 [N, 2], faces int64 [F, 3, 2] of 0-based (vertex, vt) pairs, mtllib, usemtl) of a Wavefront OBJ."""
    v, vt, faces, mtllib, usemtl = [], [], [], None, None
    for line in open(path):
        parts = line.split()
        if not parts:
            continue
        if parts[0] == 'v':
            v.append([float(x) for x in parts[1:4]])
        elif parts[0] == 'vt':
            vt.append([float(x) for x in parts[1:3]])
        elif parts[0] == 'f':
            faces.append([[int(x) - 1 for x in p.split('/')[:2]] for p in parts[1:4]])
        elif parts[0] == 'mtllib':
            mtllib = parts[1]
        elif parts[0] == 'usemtl':
            usemtl = parts[1]
    return (np.array(v, dtype=np.float64).reshape(-1, 3), np.array(vt, dtype=np.float64).reshape(-1, 2), np.array(faces, dtype=np.int64).reshape(-1, 3, 2),
            mtllib, usemtl)


def read_image(path):
    """uint8 [H, W, 3] of a PNG (through PIL) or a binary PPM."""
    if path.endswith('.ppm'):
        data = open(path, 'rb').read()
        magic, dims, top, rest = data.split(b'\n', 3)
        assert magic == b'P6' and top == b'255'
        w, h = (int(x) for x in dims.split())
        return np.frombuffer(rest, dtype=np.uint8).reshape(h, w, 3)
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))
