"""The numpy restatement of include/perf_hip_meshtex.h (tests/meshtex_reference.py) checked on its own, without a GPU: every texel of a used
tile has one owner; bilinear sampling at any point of a face touches only texels that face owns, inside the image; a function linear in the
barycentrics is reproduced within a derived bound; the two sides of a shared edge sample the same 3-D points; and write_obj's file reads
back (vt / f counts, the row flip, the clipping).

The bounds, with u = 2^-53 and values of magnitude at most C.  A texel's barycentrics are extrapolated to at most (m + 2) / m <= 3 (T = 4), so
|alpha| + |beta| + |gamma| <= 5.  A texel's value (alpha Ca + beta Cb) + gamma Cc carries the three weights' roundings (1, 1 and 2 u) and
five operations': at most 8 u * 5 C = 40 u C.  A sample's position is a sum of three products of magnitude <= S: 4 u S texels off, times the
slope of the function per texel, <= 2 C / m <= 2 C: 8 u S C.  The four weights and the weighted sum: another 40 u C; the expected value itself:
5 u C.  Together (8 S + 85) u C -- 1.2e-13 at S = 128, C = 1.  A tap whose weight is at most 8 S u is not told from a tap of weight zero
(the position is only known to 4 u S), so ownership is asked of the taps above that.  A texel's point is a double rounded to fp32 once:
the two sides of an edge form values that agree to double rounding, so their fp32 roundings differ by at most one ulp: 2^-23 max|v|."""
import numpy as np
import pytest

from tests import meshtex_reference as T

U = 2.0 ** -53


@pytest.mark.parametrize('size,tile,n_faces', T.SHAPES)
def test_every_texel_of_a_used_tile_has_one_owner(size, tile, n_faces):
    face, li, lj, code = T.owner(size, tile, n_faces)
    n, m = size // tile, tile - 3
    assert n_faces <= T.capacity(size, tile)
    used_tiles = (n_faces + 1) // 2
    row, col = np.meshgrid(np.arange(size), np.arange(size), indexing='ij')
    tile_of = np.where((col // tile < n) & (row // tile < n), (row // tile) * n + col // tile, -1)
    in_full = (tile_of >= 0) & (tile_of < n_faces // 2)
    assert (face[in_full] >> 1 == tile_of[in_full]).all() and (code[in_full] != 0).all()          # one owner, of the texel's own tile
    assert (face[(tile_of < 0) | (tile_of >= used_tiles)] == -1).all()
    if n_faces % 2:          # the last tile holds half 0 alone
        last = tile_of == used_tiles - 1
        assert set(np.unique(face[last])) == {-1, n_faces - 1}
    # the halves' sizes: half 0 owns li + lj <= m + 2, half 1 owns li + lj <= m + 1; every face has the same texel budget
    for f in (0, 1, n_faces - 1):
        mine = face == f
        top = m + 2 if f % 2 == 0 else m + 1
        assert (li[mine] + lj[mine]).max() == top and mine.sum() == (top + 1) * (top + 2) // 2, f
        assert ((code[mine] == 1) == (li[mine] + lj[mine] <= m)).all() and (code[mine] == 1).sum() == (m + 1) * (m + 2) // 2
    counts = np.bincount(face[face >= 0], minlength=n_faces)
    assert (counts[0::2] == counts[0]).all() and (counts[1::2] == counts[1]).all() and counts[0] + counts[1] == tile * tile
    # the corners are inside texels of their own face, on texel centres
    c = T.corners(n_faces, size, tile)
    assert (face[c[..., 1], c[..., 0]] == np.arange(n_faces)[:, None]).all() and (code[c[..., 1], c[..., 0]] == 1).all()
    uv = T.uv(n_faces, size, tile)
    assert uv.dtype == np.float32 and (uv.astype(np.float64) * size - 0.5 == c).all()          # (S a power of two: exact)


@pytest.mark.parametrize('size,tile,n_faces', T.SHAPES)
def test_bilinear_taps_stay_inside_the_face_and_a_linear_function_is_reproduced(size, tile, n_faces):
    face, _, _, _ = T.owner(size, tile, n_faces)
    ids, bary = T.face_points(n_faces, 200, seed=size + tile)
    xy = T.texel_position(n_faces, size, tile, ids, bary)
    cols, rows, weights = T.taps(xy, size)
    counted = weights > 8 * size * U
    assert (np.abs(weights.sum(axis=1) - 1) < 8 * U).all() and counted.any(axis=1).all()
    assert (cols[counted] >= 0).all() and (cols[counted] < size).all() and (rows[counted] >= 0).all() and (rows[counted] < size).all()
    owners = face[np.clip(rows, 0, size - 1), np.clip(cols, 0, size - 1)]
    assert (owners[counted] == np.broadcast_to(ids[:, None], owners.shape)[counted]).all()
    # a function linear in the barycentrics: per-vertex rows interpolated into the texels, sampled back
    vertices, faces = T.random_mesh(max(8, n_faces // 2), n_faces, seed=tile)
    colours = np.random.default_rng(tile).uniform(-1, 1, size=(len(vertices), 3)).astype(np.float32)
    ref = T.texels(vertices, faces, size, tile, fallback=colours)
    a, b, g = ref['alpha'], ref['beta'], ref['gamma']
    f = np.where(ref['face_of'] >= 0, ref['face_of'], 0)
    c64 = colours.astype(np.float64)
    image = ((a[:, None] * c64[faces[f, 0]] + b[:, None] * c64[faces[f, 1]]) + g[:, None] * c64[faces[f, 2]]).reshape(size, size, 3)          # (not rounded to fp32)
    got = T.sample(image, xy)
    want = (bary[:, 0:1] * c64[faces[ids, 0]] + bary[:, 1:2] * c64[faces[ids, 1]]) + bary[:, 2:3] * c64[faces[ids, 2]]
    bound = (8 * size + 85) * U * 1.0
    assert np.abs(got - want).max() <= bound, (np.abs(got - want).max(), bound)
    # the stored fallback is that image rounded to fp32 once
    covered = ref['coverage'] != 0
    assert (ref['fallback'][covered] == image.reshape(-1, 3).astype(np.float32)[covered]).all() and (ref['fallback'][~covered] == 0).all()


@pytest.mark.parametrize('size,tile', [(64, 4), (64, 5), (64, 7), (128, 8), (64, 16)])
def test_the_two_sides_of_a_shared_edge_sample_the_same_points(size, tile):
    vertices = np.random.default_rng(tile).uniform(-1, 1, size=(4, 3)).astype(np.float32)
    faces = np.array([[0, 1, 2], [1, 0, 3], [3, 2, 1], [2, 3, 0]], dtype=np.int32)          # face 0's ab, bc and ac against a leg, a hypotenuse and a leg
    ref = T.texels(vertices, faces, size, tile)
    face, li, lj, _ = (x.reshape(-1) for x in T.owner(size, tile, len(faces)))
    m = tile - 3
    points = ref['points'].astype(np.float64)

    def edge(f, which):          # the m + 1 samples of an edge of face f, ordered along it
        on = {'ab': (lj == 0) & (li <= m), 'ac': (li == 0) & (lj <= m), 'bc': li + lj == m}[which] & (face == f)
        order = np.argsort((lj if which == 'ac' else li)[on])
        assert on.sum() == m + 1
        return points[on][order]

    bound = 2.0 ** -23 * float(np.abs(vertices).max())
    for mine, other, reverse in ((edge(0, 'ab'), edge(1, 'ab'), True),          # a0 -> b0 = b1 <- a1
                                 (edge(0, 'bc'), edge(2, 'bc'), True),          # by li: c0 -> b0; face 2 = (3, 2, 1): c2 = 1 = b0 -> b2 = 2 = c0
                                 (edge(0, 'ac'), edge(3, 'ac'), True)):         # a0 -> c0; face 3 = (2, 3, 0): a3 = 2 = c0 -> c3 = 0 = a0
        other = other[::-1] if reverse else other
        assert np.abs(mine - other).max() <= bound, (np.abs(mine - other).max(), bound)
    # and the edges' ends are the vertices themselves
    assert (edge(0, 'ab')[0] == vertices[0]).all() and (edge(0, 'ac')[0] == vertices[0]).all()
    assert np.abs(edge(0, 'ab')[-1] - vertices[1]).max() <= bound and np.abs(edge(0, 'ac')[-1] - vertices[2]).max() <= bound


def test_texels_of_no_face_and_the_flag():
    vertices, faces = T.random_mesh(6, 5, seed=1)
    faces = faces.copy()
    faces[3, 1] = 6          # outside [0, V)
    faces[1, 0] = -1
    ref = T.texels(vertices, faces, 64, 8)
    assert ref['bad_face'] == 1
    for f in (1, 3):
        assert not (ref['face_of'] == f).any()
    none = ref['face_of'] < 0
    assert (ref['coverage'][none] == 0).all() and (ref['points'][none] == 0).all() and (ref['point_normals'][none] == 0).all()
    assert (ref['coverage'][~none] != 0).all() and sorted(np.unique(ref['face_of'][~none])) == [0, 2, 4]
    # flat normals are unit, the same all over a face; a zero-area face has normal 0
    n = ref['point_normals'][ref['face_of'] == 0]
    assert (n == n[0]).all() and abs(np.linalg.norm(n[0].astype(np.float64)) - 1) < 2.0 ** -23
    flat = T.texels(vertices, np.array([[0, 1, 1]], np.int32), 64, 8)
    assert (flat['point_normals'] == 0).all() and (flat['coverage'] != 0).sum() == 64 - 8 * 7 // 2


def test_atlas_layout_chooses_and_refuses():
    from perf_amd import _lib
    from perf_amd.mesh import atlas_layout
    assert atlas_layout(512, size=64) == (64, 4) and atlas_layout(511, size=128) == (128, 8) and atlas_layout(31, size=64) == (64, 16)
    assert atlas_layout(0, size=64) == (64, 64) and atlas_layout(2, size=100) == (100, 100) and atlas_layout(3, size=100) == (100, 50)
    assert atlas_layout(512, tile=4) == (64, 4) and atlas_layout(513, tile=4) == (128, 4) and atlas_layout(8191, tile=4) == (256, 4)
    assert atlas_layout(61446) == (2048, 8) and atlas_layout(0) == (64, 8) and atlas_layout(287, size=64, tile=5) == (64, 5)
    for s, t, f in T.SHAPES:          # the shapes of the tests are what the layout gives for their size
        assert atlas_layout(f, size=s) == (s, t) and T.capacity(s, t) >= f
    for kw in ({'n_faces': 513, 'size': 64}, {'n_faces': 513, 'size': 64, 'tile': 4}, {'n_faces': 1, 'size': 63}, {'n_faces': 1, 'size': 16385},
               {'n_faces': 1, 'tile': 3}, {'n_faces': 1, 'size': 64, 'tile': 65}, {'n_faces': -1, 'size': 64}, {'n_faces': 2 * 4096 ** 2 + 1, 'tile': 4}):
        with pytest.raises(_lib.PerfError):
            atlas_layout(**kw)


def test_write_obj_round_trip(tmp_path):
    import torch
    from perf_amd.mesh import Atlas, Mesh, atlas_image_u8, write_obj
    size, tile = 64, 8
    vertices, faces = T.random_mesh(9, 13, seed=2)
    image = np.random.default_rng(5).uniform(-0.5, 1.5, size=(size, size, 3)).astype(np.float32)          # beyond [0, 1]: clipped
    image[0, 0], image[size - 1, 0], image[0, size - 1] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    atlas = Atlas(size, tile, torch.from_numpy(T.uv(len(faces), size, tile)), torch.from_numpy(image), torch.zeros(size, size, dtype=torch.uint8),
                  torch.zeros(size, size), torch.zeros(size, size, dtype=torch.int64))
    path = str(tmp_path / 'tiny.obj')
    image_path = write_obj(path, Mesh(torch.from_numpy(vertices), torch.from_numpy(faces)), atlas)
    v, vt, f, mtllib, usemtl = T.parse_obj(path)
    assert len(v) == len(vertices) and len(vt) == 3 * len(faces) and len(f) == len(faces) and mtllib == 'tiny.mtl' and usemtl == 'atlas'
    assert (v.astype(np.float32) == vertices).all() and (f[..., 0] == faces).all()
    assert (f[..., 1] == np.arange(3 * len(faces)).reshape(-1, 3)).all()          # three vt per face, in corner order
    assert (vt.astype(np.float32) == T.uv(len(faces), size, tile).reshape(-1, 2)).all()
    mtl = open(str(tmp_path / 'tiny.mtl')).read()
    assert 'newmtl atlas' in mtl and 'map_Kd ' + image_path.rsplit('/', 1)[-1] in mtl
    pixels = T.read_image(image_path)
    want = np.rint(np.clip(image.astype(np.float64), 0, 1) * 255).astype(np.uint8)[::-1]          # row S - 1 first: OBJ's v points up
    assert pixels.shape == (size, size, 3) and (pixels == want).all() and (pixels == atlas_image_u8(atlas)).all()
    assert tuple(pixels[size - 1, 0]) == (255, 0, 0) and tuple(pixels[0, 0]) == (0, 255, 0) and tuple(pixels[size - 1, size - 1]) == (0, 0, 255)
    assert pixels.min() == 0 and pixels.max() == 255
    # a texel's colour is found where its uv points: v = (j + 0.5) / S from the bottom of the file's image
    u, w = vt[0]
    assert tuple(pixels[size - 1 - int(w * size), int(u * size)]) == tuple(want[::-1][int(w * size), int(u * size)])
