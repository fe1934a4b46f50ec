"""The cull of the faces no registered panorama saw (include/perf_hip_meshvis.h, perf_amd/mesh.py) on the GPU.  Everything is compared
EXACTLY: the vertex bits against the existing reprojection kernel (ops.pano_reproject, mode 0) on every input, the degenerate ones
included, and against the float64 restatement tests/meshvis_reference.py on the inputs none of whose (vertex, view) pairs lies inside the
restatement's guard (tests/test_cpu_meshvis_reference.py asserts that); the face rule and the compaction against the restatement; end to
end against clean_mesh on the hollow sphere and against the restatement on the shell with a tunnel, which clean_mesh cannot split."""
import numpy as np
import pytest
import torch

from tests import meshcc_reference as CC
from tests import meshvis_reference as V

pytestmark = pytest.mark.gpu


def _device_views(views):
    return [{'pose': torch.from_numpy(np.array(v['pose'])), 'distance_map': torch.from_numpy(np.array(v['distance_map'])).cuda()} for v in views]


def _words(t):
    return t.cpu().numpy().view(np.uint64)


# ---- 1. the bits against the existing kernel -----------------------------------------------------------------------------------------------
def _vertices_with_specials(n, views, seed):
    p = np.random.default_rng(seed).uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
    special = V.special_vertices(views)[:n]
    p[:len(special)] = special
    return p


@pytest.mark.parametrize('n_views', [1, 2, 3, 33, 64])
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 255, 256, 257, 65537])
def test_bits_equal_the_reprojection_kernel(n, n_views):
    from perf_amd import ops
    from perf_amd.mesh import vertex_visibility
    views = V.make_views(n_views)
    dev = _device_views(views)
    vertices = torch.from_numpy(_vertices_with_specials(n, views, 11 * n + n_views)).cuda()
    for tol, free_tol in ((V.TOL, V.FREE_TOL), (0.0, 0.0)):
        vis = vertex_visibility(vertices, dev, tol=tol, free_tol=free_tol)
        assert vis.n_views == n_views and vis.visible.dtype == vis.free.dtype == torch.int64 and tuple(vis.visible.shape) == tuple(vis.free.shape) == (n,)
        for got, eps in ((vis.visible, tol), (vis.free, -free_tol)):
            want = torch.zeros(n, dtype=torch.int64, device='cuda')
            for k, view in enumerate(dev):
                mask = torch.zeros(n, device='cuda')
                ops.pano_reproject(vertices, view['pose'], view['distance_map'], mask, 0, eps)
                want |= (mask > 0.5).long() << k
            assert torch.equal(got, want), (n, n_views, eps)            # (bits at or above K are zero: want has none)
    if n >= 256:
        assert vis.visible.ne(0).any() and vis.visible.eq(0).any()


def test_free_tol_defaults_to_tol_and_a_pool_is_accepted():
    from perf_amd.mesh import vertex_visibility

    class Pool:
        pass
    views = V.make_views(3)
    pool = Pool()
    pool.sup_infos = [{'pose': torch.from_numpy(np.array(v['pose'])).cuda(), 'distance_map': torch.from_numpy(np.array(v['distance_map'])).cuda()[..., None] * 2.0,
                       'mask': torch.full(v['distance_map'].shape + (1,), 0.5, device='cuda') > 0} for v in views]            # [H, W, 1] maps with a mask
    pool.sup_infos[1]['mask'] = torch.from_numpy(np.asarray(views[1]['distance_map']) > 0).cuda()[..., None]
    doubled = [{'pose': v['pose'], 'distance_map': np.asarray(v['distance_map']) * np.float32(2.0)} for v in views]
    vertices = torch.from_numpy(np.array(V.guard_free_vertices(3, 4099))).cuda()
    a = vertex_visibility(vertices, pool, tol=1 / 64)
    b = vertex_visibility(vertices, _device_views(doubled), tol=1 / 64, free_tol=1 / 64)
    assert torch.equal(a.visible, b.visible) and torch.equal(a.free, b.free)


# ---- 2. the bits against the float64 restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_views,n', [(1, 4099), (3, 4099), (64, 4099)])
def test_bits_equal_the_float64_restatement_on_the_guard_free_inputs(n_views, n):
    from perf_amd.mesh import vertex_visibility
    views = V.make_views(n_views)
    vertices = V.guard_free_vertices(n_views, n)
    want_visible, want_free = V.vertex_bits(vertices, views, V.TOL, V.FREE_TOL)
    vis = vertex_visibility(torch.from_numpy(np.array(vertices)).cuda(), _device_views(views), tol=V.TOL, free_tol=V.FREE_TOL)
    assert np.array_equal(_words(vis.visible), want_visible) and np.array_equal(_words(vis.free), want_free)


# ---- 3. the face rule ------------------------------------------------------------------------------------------------------------------------
def _face_cases():
    rng = np.random.default_rng(31)
    out = {}
    for n in CC.EDGE_SIZES:
        out[f'fan_{n}'] = (CC.fan(n), n, 3)
        out[f'strip_{n}'] = (CC.strip(n), n, 3)
    out['repeated_index'] = (np.array([[0, 0, 1], [2, 3, 2], [4, 4, 4], [5, 6, 7], [7, 6, 5]], np.int32), 9, 3)
    out['shuffled_triangles'] = (rng.integers(0, 2000, size=(3000, 3)).astype(np.int32), 2000, 64)
    return out


FACE_CASES = _face_cases()


@pytest.mark.parametrize('name', sorted(FACE_CASES))
def test_visible_faces_equal_the_restatement(name):
    from perf_amd.mesh import Mesh, vertex_visibility, visible_faces
    faces, n, n_views = FACE_CASES[name]
    views = V.make_views(n_views)
    dev = _device_views(views)
    vertices = np.random.default_rng(n).uniform(-0.8, 0.8, size=(n, 3)).astype(np.float32)
    vertices[0] = (0.05, 0.02, -0.03)                        # (the fans' hub: near every view, so that it does not decide every face)
    mesh = Mesh(torch.from_numpy(vertices).cuda(), torch.from_numpy(faces).cuda())
    vis = vertex_visibility(mesh.vertices, dev, tol=1 / 16, free_tol=1 / 4)          # (a wide band: many vertices are visible and not free)
    visible, free = _words(vis.visible), _words(vis.free)            # the device's own bits
    centres = np.stack([np.asarray(v['pose'])[:3, 3] for v in views])
    kept = set()
    for facing in (True, False):
        for carve in (True, False):
            for min_views in (1, 2, n_views):
                got = visible_faces(mesh, vis, dev, facing=facing, min_views=min_views, carve=carve)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (len(faces),)
                want = V.face_keep(faces, vertices, visible, free, centres, facing, min_views, carve)
                assert np.array_equal(got.cpu().numpy(), want), (name, facing, carve, min_views)
                kept.add(int(want.sum()))
    assert len(kept) > 1 or len(faces) < 61                  # (the combinations do not all say the same)


@pytest.mark.parametrize('bad', ['V', -1])
def test_a_face_index_outside_the_vertices_is_refused(bad):
    from perf_amd._lib import PerfError
    from perf_amd.mesh import Mesh, cull_unseen, vertex_visibility, visible_faces
    n = 300
    faces = CC.strip(n).copy()
    faces[7, 1] = faces[150, 2] = n if bad == 'V' else -1
    dev = _device_views(V.make_views(2))
    mesh = Mesh(torch.from_numpy(np.random.default_rng(2).uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32)).cuda(), torch.from_numpy(faces).cuda())
    vis = vertex_visibility(mesh.vertices, dev)
    message = r'face 7 = \[7, ' + str(n if bad == 'V' else -1) + r', 9\] has an index outside \[0, 300\)'
    with pytest.raises(PerfError, match='visible_faces: ' + message):
        visible_faces(mesh, vis, dev)
    with pytest.raises(PerfError, match='cull_unseen: ' + message):
        cull_unseen(mesh, dev)
    good = Mesh(mesh.vertices, torch.from_numpy(CC.strip(n)).cuda())          # and the device is as it was: the next call works
    assert tuple(visible_faces(good, vis, dev).shape) == (n - 2,)


# ---- 4. the compaction -----------------------------------------------------------------------------------------------------------------------
def _masks(n_faces, rng):
    one = np.zeros(n_faces, dtype=bool)
    one[n_faces // 2:n_faces // 2 + 1] = True
    return {'none': np.zeros(n_faces, dtype=bool), 'all': np.ones(n_faces, dtype=bool), 'every_other': np.arange(n_faces) % 2 == 0, 'one': one,
            'random_half': rng.random(n_faces) < 0.5}


def _same(a, b):
    assert a.vertices.dtype == b.vertices.dtype == torch.float32 and a.faces.dtype == b.faces.dtype == torch.int32
    assert a.vertices.shape == b.vertices.shape and torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))          # to the bit
    assert torch.equal(a.faces, b.faces)


@pytest.mark.parametrize('n_faces', [0, 1, 255, 256, 257, 65537])
def test_filter_faces_equals_the_restatement(n_faces):
    from perf_amd.mesh import Mesh, filter_faces
    rng = np.random.default_rng(100 + n_faces)
    n = n_faces // 2 + 3
    faces = rng.integers(0, n, size=(n_faces, 3)).astype(np.int32)
    vertices = rng.normal(size=(n, 3)).astype(np.float32)
    colors, normals = torch.rand(n, 3, device='cuda'), torch.randn(n, 3, device='cuda')
    mesh = Mesh(torch.from_numpy(vertices).cuda(), torch.from_numpy(faces).cuda(), colors, normals)
    order = rng.permutation(n_faces)
    shuffled = Mesh(mesh.vertices, torch.from_numpy(faces[order]).cuda(), colors, normals)
    for name, keep in _masks(n_faces, rng).items():
        want_vertices, want_faces, want_index = V.filter_faces(vertices, faces, keep)
        dev_keep = torch.from_numpy(keep).cuda()
        got, index = filter_faces(mesh, dev_keep if name != 'every_other' else dev_keep.to(torch.uint8) * 3)          # bool, or any nonzero uint8
        assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), want_index), name
        assert np.array_equal(got.vertices.cpu().numpy(), want_vertices) and np.array_equal(got.faces.cpu().numpy(), want_faces.reshape(-1, 3)), name
        assert got.faces.dtype == torch.int32 and tuple(got.faces.shape) == (int(keep.sum()), 3) and tuple(got.vertices.shape) == (len(want_index), 3)
        assert torch.equal(got.colors, colors[index.long()]) and torch.equal(got.normals, normals[index.long()])
        again, index_again = filter_faces(mesh, dev_keep)                # two runs give the same bits
        _same(got, again)
        assert torch.equal(index, index_again)
        other, other_index = filter_faces(shuffled, torch.from_numpy(keep[order]).cuda())          # shuffled faces: the same vertices, the faces permuted with them
        assert torch.equal(other_index, index) and torch.equal(other.vertices, got.vertices)
        assert np.array_equal(other.faces.cpu().numpy(), V.filter_faces(vertices, faces[order], keep[order])[1].reshape(-1, 3))


def test_capacities_below_the_counted_totals_are_refused():
    from perf_amd import ops
    from perf_amd._lib import PerfError
    rng = np.random.default_rng(9)
    faces = torch.from_numpy(rng.integers(0, 500, size=(1000, 3)).astype(np.int32)).cuda()
    vertices = torch.from_numpy(rng.normal(size=(500, 3)).astype(np.float32)).cuda()
    keep = np.arange(1000) % 4 == 0
    _, want_faces, want_index = V.filter_faces(vertices.cpu().numpy(), faces.cpu().numpy(), keep)
    nv, nf = len(want_index), len(want_faces)
    dev_keep = torch.from_numpy(keep).cuda()
    counts, ws = ops.meshvis_filter_count(faces, 500, dev_keep)
    assert counts.tolist() == [nv, nf] and nf == 250
    with pytest.raises(PerfError, match=f'room for {nv - 1} vertices, {nv} were counted'):
        ops.meshvis_filter_write(faces, 500, dev_keep, ws, nv - 1, nf, vertices)
    with pytest.raises(PerfError, match=f'room for {nf - 1} faces, {nf} were counted'):
        ops.meshvis_filter_write(faces, 500, dev_keep, ws, nv, nf - 1, vertices)
    out_vertices, out_faces, index = ops.meshvis_filter_write(faces, 500, dev_keep, ws, nv, nf, vertices)
    assert int(out_faces.max()) == nv - 1 and int(out_faces.min()) == 0 and torch.equal(out_vertices, vertices[index.long()])
    assert np.array_equal(out_faces.cpu().numpy(), want_faces)


def test_a_kept_face_with_an_index_outside_the_vertices_is_dropped():
    from perf_amd.mesh import Mesh, filter_faces
    faces = CC.strip(300).copy()
    faces[7, 1], faces[150, 2] = 300, -1
    mesh = Mesh(torch.zeros(300, 3, device='cuda'), torch.from_numpy(faces).cuda())
    got, index = filter_faces(mesh, torch.ones(298, dtype=torch.bool, device='cuda'))
    assert tuple(got.faces.shape) == (296, 3) and torch.equal(index, torch.arange(300, dtype=torch.int32, device='cuda'))
    assert np.array_equal(got.faces.cpu().numpy(), np.delete(CC.strip(300), [7, 150], axis=0))


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------------
_MESHES = {}


def _mesh_of(which):
    """The device's surface-nets mesh of the hollow sphere / the shell with a tunnel, made once."""
    if which not in _MESHES:
        from perf_amd.mesh import surface_nets
        field = CC.hollow_sphere() if which == 'hollow_sphere' else V.tunnel_field()
        _MESHES[which] = surface_nets(torch.from_numpy(field).cuda(), 0.0, CC.SPHERE_LO, CC.SPHERE_HI)
    return _MESHES[which]


def _equals_the_restatement(mesh, got, views, **kw):
    vertices, faces = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    tol = kw.get('tol', 1 / 256)
    assert V.outside_guard(vertices, views, tol, kw.get('free_tol') or tol).all()            # no vertex of the mesh is near a decision
    want_vertices, want_faces, _, _ = V.cull(vertices, faces, list(views), **kw)
    assert np.array_equal(got.vertices.cpu().numpy(), want_vertices) and np.array_equal(got.faces.cpu().numpy(), want_faces.reshape(-1, 3))
    return len(want_faces), len(want_vertices)


def test_on_the_hollow_sphere_the_cull_is_the_inward_component():
    from perf_amd.mesh import clean_mesh, cull_unseen
    mesh = _mesh_of('hollow_sphere')
    views = (V.constant_view(),)
    got = cull_unseen(mesh, _device_views(views))
    _same(got, clean_mesh(mesh, orientation='inward'))
    assert _equals_the_restatement(mesh, got, views) == (768, 386)


def test_the_tunnel_field_is_one_component_and_the_cull_splits_it():
    from perf_amd.mesh import clean_mesh, connected_components, cull_unseen
    mesh = _mesh_of('tunnel')
    comps = connected_components(mesh)
    assert comps.faces.tolist() == [3000] and float(comps.signed_volume[0]) > 1.4
    assert clean_mesh(mesh, orientation='inward').faces.shape[0] == 0
    views = (V.constant_view(),)
    got = cull_unseen(mesh, _device_views(views))
    assert _equals_the_restatement(mesh, got, views) == (774, 394)
    assert connected_components(got).faces.tolist() == [774]


@pytest.mark.parametrize('centre', [(0.02, 0.02, 0.02), (0.25, -0.1, 0.15)])
def test_facing_alone_selects_the_inner_skin(centre):
    from perf_amd.mesh import clean_mesh, cull_unseen
    mesh = _mesh_of('hollow_sphere')
    views = (V.constant_view(centre, 0.9 if centre[0] < 0.1 else 2.0),)            # every vertex passes the depth test
    got = cull_unseen(mesh, _device_views(views))
    _same(got, clean_mesh(mesh, orientation='inward'))
    assert _equals_the_restatement(mesh, got, views)[0] == 768
    everything = cull_unseen(mesh, _device_views(views), facing=False)
    _same(everything, mesh)


def test_carve_drops_what_lies_in_a_second_views_free_space():
    from perf_amd.mesh import cull_unseen
    mesh = _mesh_of('hollow_sphere')
    # the first view stored the inner skin itself (0.44 away); the second stands outside the sphere, sees the near cap of the outer skin from
    # the front, and its map (1.1) stops short of the far side: the near caps of both skins float in its free space
    views = (V.constant_view(V.CENTRE, 0.44), V.constant_view((1.4, 0.02, 0.02), 1.1, (7, 5)))
    dev = _device_views(views)
    kw = {'tol': 1 / 16, 'free_tol': 1 / 8}
    plain = cull_unseen(mesh, dev, **kw)
    n_plain, _ = _equals_the_restatement(mesh, plain, views, **kw)
    assert n_plain > 768                                     # (the inner skin by the first view and the outer skin's near cap by the second)
    carved = cull_unseen(mesh, dev, carve=True, **kw)
    n_carved, _ = _equals_the_restatement(mesh, carved, views, carve=True, **kw)
    assert 0 < n_carved < n_plain
    both = cull_unseen(mesh, dev, min_views=2, facing=False, **kw)
    assert 0 < _equals_the_restatement(mesh, both, views, min_views=2, facing=False, **kw)[0] < n_plain


def test_the_brick_path_culls_to_the_same_components():
    from perf_amd.mesh import connected_components, cull_unseen, surface_nets, surface_nets_bricks
    field = V.tunnel_field(24)                               # the tunnel's lattice padded to a multiple of 8; the box grows with it
    lo, hi = CC.SPHERE_LO, [1.4, 1.4, 1.4]
    dense = surface_nets(torch.from_numpy(field).cuda(), 0.0, lo, hi)
    values = np.ascontiguousarray(field[:24, :24, :24].reshape(3, 8, 3, 8, 3, 8).transpose(0, 2, 4, 1, 3, 5)).reshape(27, 8, 8, 8)
    ids = torch.arange(27, dtype=torch.int32, device='cuda')
    sparse, _ = surface_nets_bricks(torch.from_numpy(values).cuda(), ids, ids.view(3, 3, 3).clone(), (24, 24, 24), 0.0, -1.0, lo, hi)
    assert sparse.faces.shape[0] == dense.faces.shape[0] == 3000
    dev = _device_views((V.constant_view(),))
    pairs = lambda mesh: sorted(zip(*(t.tolist() for t in connected_components(mesh)[1:3])))
    a, b = cull_unseen(dense, dev), cull_unseen(sparse, dev)
    assert pairs(a) == pairs(b) == [(774, 394)]
    assert torch.equal(torch.sort(a.vertices.view(torch.int32), dim=0).values, torch.sort(b.vertices.view(torch.int32), dim=0).values)          # the same vertices, to the bit
