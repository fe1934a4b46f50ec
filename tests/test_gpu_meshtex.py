"""The texture atlas (include/perf_hip_meshtex.h, perf_amd/mesh.py) on the GPU.  The corner UVs, the texels' points and normals, face_of, the
coverage and the flag are compared TO THE BIT with the float64 restatement tests/meshtex_reference.py, every texel, no exclusions.  The
fused bake is compared to the bit with the composed route it fuses -- atlas_points, then panorama_colors (the blend kernel) on those points
and normals -- on every covered texel; uncovered texels hold fill, 0, 0.

"To the bit" for floats means: a NaN where the reference has a NaN, the same 32 bits everywhere else.  IEEE 754 leaves the sign and the
payload of a NaN an operation produces to the implementation (the host's invalid operations give a negative quiet NaN, the device's a
positive one), so which NaN it is states nothing about the rule.

The bound of the sampling test, for per-vertex colours of magnitude at most C = 1: a texel holds (alpha Ca + beta Cb) + gamma Cc rounded to
fp32 once, of magnitude at most (|alpha| + |beta| + |gamma|) C <= 5 C with the gutter's extrapolation (T = 4), so it is off by at most
5 * 2^-24; bilinear weights are a convex combination, which keeps that; the float64 sampling and the float64 expectation add the
(8 S + 85) 2^-53 of tests/test_cpu_meshtex_reference.py.  Two faces that share an edge are both within the bound of the same value there."""
import numpy as np
import pytest
import torch

from tests import meshcolor_reference as R
from tests import meshtex_reference as T
from tests import meshvis_reference as V

pytestmark = pytest.mark.gpu

SHAPES = T.SHAPES + ((256, 4, 8191),)
FILL = (0.25, 0.5, 0.75)
TOL = 1 / 256


def _mesh(vertices, faces, colors=None, normals=None):
    from perf_amd.mesh import Mesh
    dev = lambda a, t: None if a is None else torch.from_numpy(np.array(a, dtype=t, order='C')).cuda().reshape(-1, 3).contiguous()
    return Mesh(dev(vertices, np.float32), dev(faces, np.int32), dev(colors, np.float32), dev(normals, np.float32))


def _device_views(n_views):
    views, maps = V.make_views(n_views), R.make_color_maps(n_views)
    return [{'pose': torch.from_numpy(np.array(v['pose'])), 'distance_map': torch.from_numpy(np.array(v['distance_map'])).cuda(),
             'color_map': torch.from_numpy(np.array(m)).cuda()} for v, m in zip(views, maps)]


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype != np.float32:
        return bool((got == want).all())
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


def _check_points(vertices, faces, size, tile, normals=None):
    from perf_amd import ops
    mesh = _mesh(vertices, faces, normals=normals)
    ref = T.texels(vertices, faces, size, tile, normals=normals)
    points, point_normals, face_of, coverage, flag = ops.meshtex_points(mesh.vertices, mesh.faces, size, tile, mesh.normals)
    assert int(flag.item()) == ref['bad_face']
    assert _same_bits(face_of.cpu().numpy(), ref['face_of']) and _same_bits(coverage.cpu().numpy(), ref['coverage'])
    assert _same_bits(points.cpu().numpy(), ref['points'])
    assert _same_bits(point_normals.cpu().numpy(), ref['point_normals'])
    assert _same_bits(ops.meshtex_uv(len(faces), size, tile).cpu().numpy(), T.uv(len(faces), size, tile))
    return ref


@pytest.mark.parametrize('normals', ['flat', 'vertex'])
@pytest.mark.parametrize('size,tile,n_faces', SHAPES)
def test_points_equal_the_restatement_to_the_bit(size, tile, n_faces, normals):
    vertices, faces = T.random_mesh(max(8, n_faces // 2), n_faces, seed=size)
    ref = _check_points(vertices, faces, size, tile, R.random_normals(len(vertices), seed=tile) if normals == 'vertex' else None)
    assert ref['bad_face'] == -1 and (ref['coverage'] == 1).sum() == n_faces * (tile - 2) * (tile - 1) // 2
    assert (ref['face_of'] >= 0).sum() == (n_faces + 1) // 2 * (tile * (tile + 1) // 2) + n_faces // 2 * (tile * (tile - 1) // 2)


EDGE = {'zero_area_face': (np.array([[0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1], [0.3, 0.2, 0.1]], np.float32), np.array([[0, 1, 2], [3, 3, 0], [1, 1, 1], [0, 1, 3]], np.int32)),
        'nan_and_infinite_vertices': (np.array([[0, 0, 0], [0.5, 0.1, 0], [0.1, 0.7, 0.2], [np.nan, 0, 0], [0, -np.inf, 0], [0.3, 0.3, 0.9]], np.float32),
                                      np.array([[0, 1, 2], [0, 1, 3], [4, 1, 2], [2, 1, 5], [3, 4, 5]], np.int32)),
        'index_outside': (R.random_vertices(6), np.array([[0, 1, 2], [2, 6, 1], [3, 4, 5], [-1, 0, 1], [5, 4, 3]], np.int32)),
        'no_faces': (R.random_vertices(5), np.zeros((0, 3), np.int32)),
        'no_vertices': (np.zeros((0, 3), np.float32), np.array([[0, 0, 0]], np.int32))}


@pytest.mark.parametrize('normals', ['flat', 'vertex'])
@pytest.mark.parametrize('name', sorted(EDGE))
def test_points_of_degenerate_meshes(name, normals):
    vertices, faces = EDGE[name]
    for size, tile in ((64, 8), (65, 9)):
        ref = _check_points(vertices, faces, size, tile, R.random_normals(len(vertices), seed=3) if normals == 'vertex' else None)
        assert ref['bad_face'] == {'index_outside': 1, 'no_vertices': 0}.get(name, -1)
    if name == 'index_outside':
        from perf_amd import _lib
        from perf_amd.mesh import atlas_points, bake_panorama_texture
        for call in (lambda: atlas_points(_mesh(vertices, faces), 64, 8), lambda: bake_panorama_texture(_mesh(vertices, faces), _device_views(1), size=64)):
            with pytest.raises(_lib.PerfError, match=r'face 1 = \[2, 6, 1\] has an index outside \[0, 6\)'):
                call()


def _composed(mesh, size, tile, views, normals, fallback_rows, **kw):
    """The route the bake fuses: the materialised points and normals through the blend kernel."""
    from perf_amd.mesh import atlas_points, panorama_colors
    points, point_normals, face_of, coverage = atlas_points(mesh, size, tile, normals=normals)
    return panorama_colors(points, views, point_normals, fallback=fallback_rows, fill=FILL, **kw), coverage


@pytest.mark.parametrize('with_fallback', [False, True])
@pytest.mark.parametrize('facing', [True, False])
@pytest.mark.parametrize('select', ['blend', 'best'])
@pytest.mark.parametrize('n_views', [1, 3, 64])
def test_the_fused_bake_is_the_composed_route_to_the_bit(n_views, select, facing, with_fallback):
    from perf_amd.mesh import bake_panorama_texture
    size, tile, n_faces = 128, 8, 511
    vertices, faces = T.random_mesh(200, n_faces, seed=n_views)
    vertices = vertices * np.float32(1.5)          # in and out of the views' stored distances: some texels pass, some do not
    colors = np.random.default_rng(n_views).uniform(0, 1, size=(len(vertices), 3)).astype(np.float32) if with_fallback else None
    vertex_normals = R.random_normals(len(vertices), seed=1)
    views = _device_views(n_views)
    for normals in ('flat', 'mesh'):
        mesh = _mesh(vertices, faces, colors, vertex_normals)
        ref = T.texels(vertices, faces, size, tile, fallback=colors)
        rows = torch.from_numpy(ref['fallback']).cuda() if with_fallback else None
        kw = dict(tol=TOL, facing=facing, power=3, select=select)
        want, coverage = _composed(mesh, size, tile, views, normals, rows, **kw)
        atlas = bake_panorama_texture(mesh, views, size=size, tile=tile, normals=normals, fill=FILL, **kw)
        assert (atlas.size, atlas.tile) == (size, tile) and _same_bits(atlas.coverage.cpu().numpy().reshape(-1), ref['coverage'])
        covered = (coverage != 0).cpu().numpy()
        assert covered.sum() == (ref['coverage'] != 0).sum() > 0
        image, weight, used = atlas.image.cpu().numpy().reshape(-1, 3), atlas.weight.cpu().numpy().reshape(-1), atlas.used.cpu().numpy().reshape(-1)
        assert _same_bits(image[covered], want.colors.cpu().numpy()[covered])
        assert _same_bits(weight[covered], want.weight.cpu().numpy()[covered]) and _same_bits(used[covered], want.used.cpu().numpy()[covered])
        assert (image[~covered] == np.array(FILL, np.float32)).all() and (weight[~covered] == 0).all() and (used[~covered] == 0).all()
        # the comparison is of texels the views colour and of texels they do not: both kinds are there
        passed = used[covered] != 0
        assert passed.mean() > 0.05 and (~passed).sum() > 100, passed.mean()
        if with_fallback:          # where no view passed, the texel holds the interpolated rows
            assert _same_bits(image[covered][~passed], ref['fallback'][covered][~passed])
        assert _same_bits(atlas.uv.cpu().numpy(), T.uv(n_faces, size, tile))


@pytest.mark.parametrize('size,tile,n_faces', SHAPES)
def test_the_fused_bake_on_every_shape_and_from_run_to_run(size, tile, n_faces):
    from perf_amd.mesh import bake_panorama_texture
    vertices, faces = T.random_mesh(max(8, n_faces // 2), n_faces, seed=size)
    mesh, views = _mesh(vertices * np.float32(1.5), faces), _device_views(3)
    want, coverage = _composed(mesh, size, tile, views, 'flat', None, tol=TOL)
    first = bake_panorama_texture(mesh, views, size=size, tile=tile, fill=FILL, tol=TOL)
    again = bake_panorama_texture(mesh, views, size=size, tile=tile, fill=FILL, tol=TOL)
    for a, b in ((first.image, again.image), (first.weight, again.weight)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(first.used, again.used) and torch.equal(first.coverage, again.coverage) and torch.equal(first.uv, again.uv)
    covered = (coverage != 0).cpu().numpy()
    assert _same_bits(first.coverage.cpu().numpy().reshape(-1), coverage.cpu().numpy())
    assert _same_bits(first.image.cpu().numpy().reshape(-1, 3)[covered], want.colors.cpu().numpy()[covered])
    assert _same_bits(first.weight.cpu().numpy().reshape(-1)[covered], want.weight.cpu().numpy()[covered])
    assert _same_bits(first.used.cpu().numpy().reshape(-1)[covered], want.used.cpu().numpy()[covered])
    assert (first.image.cpu().numpy().reshape(-1, 3)[~covered] == np.array(FILL, np.float32)).all()
    assert (first.used.cpu().numpy().reshape(-1)[covered] != 0).mean() > 0.05


@pytest.mark.parametrize('size,tile', [(64, 4), (64, 5), (64, 7), (128, 8), (64, 16)])
def test_sampling_the_fallback_reproduces_the_vertex_colours(size, tile):
    from perf_amd.mesh import bake_panorama_texture, sample_atlas
    vertices = np.random.default_rng(tile).uniform(-1, 1, size=(4, 3)).astype(np.float32)
    faces = np.array([[0, 1, 2], [1, 0, 3], [3, 2, 1], [2, 3, 0]], dtype=np.int32)          # face 0 shares each of its edges
    colors = np.random.default_rng(size).uniform(0, 1, size=(4, 3)).astype(np.float32)
    atlas = bake_panorama_texture(_mesh(vertices, faces, colors), [], size=size, tile=tile, fill=FILL)          # no views: every covered texel takes the fallback
    assert (atlas.used == 0).all() and (atlas.weight == 0).all()
    ref = T.texels(vertices, faces, size, tile, fallback=colors)
    covered = ref['coverage'] != 0
    assert _same_bits(atlas.image.cpu().numpy().reshape(-1, 3)[covered], ref['fallback'][covered]) and _same_bits(atlas.coverage.cpu().numpy().reshape(-1), ref['coverage'])
    ids, bary = T.face_points(len(faces), 200, seed=tile)
    got = sample_atlas(atlas, torch.from_numpy(ids).cuda(), torch.from_numpy(bary).cuda()).cpu().numpy()
    c64 = colors.astype(np.float64)
    want = (bary[:, 0:1] * c64[faces[ids, 0]] + bary[:, 1:2] * c64[faces[ids, 1]]) + bary[:, 2:3] * c64[faces[ids, 2]]
    bound = 5 * 2.0 ** -24 + (8 * size + 85) * 2.0 ** -53
    assert np.abs(got - want).max() <= bound, (np.abs(got - want).max(), bound)
    # the torch sampler is the numpy one up to float64 rounding (another order of the same sums over texels of magnitude <= 5)
    assert np.abs(got - T.sample(atlas.image.cpu().numpy(), T.texel_position(len(faces), size, tile, ids, bary))).max() <= 5 * (8 * size + 85) * 2.0 ** -53
    # across a shared edge: the same 3-D points as points of the two faces
    s = np.linspace(0, 1, 33)[:, None]
    for (f0, w0), (f1, w1) in ((((0, (1 - s, s, 0 * s))), (1, (s, 1 - s, 0 * s))),          # v0 -> v1: face 0's ab, face 1 = (1, 0, 3)
                               ((0, (0 * s, 1 - s, s)), (2, (0 * s, s, 1 - s))),            # v1 -> v2: face 0's bc, face 2 = (3, 2, 1)
                               ((0, (1 - s, 0 * s, s)), (3, (s, 0 * s, 1 - s)))):           # v0 -> v2: face 0's ac, face 3 = (2, 3, 0)
        sides = []
        for f, w in ((f0, w0), (f1, w1)):
            b = np.concatenate(w, axis=1)
            sides.append(sample_atlas(atlas, torch.full((len(s),), f).cuda(), torch.from_numpy(b).cuda()).cpu().numpy())
            p = b @ vertices[faces[f]].astype(np.float64)
            sides.append(p)
        assert np.abs(sides[1] - sides[3]).max() < 1e-12          # (the same points)
        assert np.abs(sides[0] - sides[2]).max() <= 2 * bound, (np.abs(sides[0] - sides[2]).max(), bound)


@pytest.fixture(scope='module')
def scene():
    from perf_amd.scene import NeRFScene
    torch.manual_seed(0)
    sc = NeRFScene(dtype='fp16')
    sc.set_eval()
    return sc


def test_the_field_texture_is_the_field_at_the_covered_points(scene):
    from perf_amd.mesh import atlas_points, bake_field_texture, vertex_colors
    vertices, faces = T.random_mesh(40, 161, seed=5)
    mesh = _mesh(vertices, faces)
    atlas = bake_field_texture(scene, mesh, size=64, fill=FILL)
    assert (atlas.size, atlas.tile) == (64, 7)
    points, _, _, coverage = atlas_points(mesh, 64, 7)
    covered = coverage != 0
    image = atlas.image.reshape(-1, 3)
    assert torch.equal(image[covered], vertex_colors(scene, points[covered].contiguous())) and torch.equal(atlas.coverage.reshape(-1), coverage)
    assert (image[~covered] == torch.tensor(FILL, device='cuda')).all() and int(covered.sum()) == 81 * 28 + 80 * 21
    assert (atlas.used == 0).all() and torch.equal(atlas.weight.reshape(-1), covered.float())
    assert torch.equal(scene.bake_mesh_texture(mesh, None, size=64, fill=FILL).image, atlas.image)


def test_the_extraction_tools_path_writes_an_obj_that_reads_back(scene, tmp_path):
    from perf_amd.mesh import atlas_image_u8, write_obj
    vertices, faces = T.random_mesh(12, 31, seed=9)
    colors = np.random.default_rng(9).uniform(0, 1, size=(12, 3)).astype(np.float32)
    mesh = _mesh(vertices, faces, colors)
    atlas = scene.bake_mesh_texture(mesh, _device_views(3), size=64, tile=None, tol=TOL, select='blend', power=2)          # as tools/extract_mesh.py --texture 64 calls it
    assert (atlas.size, atlas.tile) == (64, 16)
    path = str(tmp_path / 'room.obj')
    image_path = write_obj(path, mesh, atlas)
    v, vt, f, mtllib, usemtl = T.parse_obj(path)
    assert (v.astype(np.float32) == vertices).all() and (f[..., 0] == faces).all() and (f[..., 1] == np.arange(93).reshape(31, 3)).all()
    assert (vt.astype(np.float32) == T.uv(31, 64, 16).reshape(-1, 2)).all() and mtllib == 'room.mtl' and usemtl == 'atlas'
    pixels = T.read_image(image_path)
    assert pixels.shape == (64, 64, 3) and (pixels == atlas_image_u8(atlas)).all()
    assert (pixels[::-1] == np.rint(np.clip(atlas.image.cpu().numpy().astype(np.float64), 0, 1) * 255).astype(np.uint8)).all()
