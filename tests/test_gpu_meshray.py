"""Rays against a mesh on the device (include/perf_hip_meshray.h, perf_amd/mesh.py) against the float64 restatement of
tests/meshray_reference.py: the cell lists as sets per cell, the closest hit TO THE BIT (the rule is + - * / in double with contraction
off, and the restatement performs the same operations in the same order), its independence of the grid, the segment occlusion, and the
end-to-end identities on the cull's fixtures: the occlusion-aware cull of the hollow sphere is its inward component whatever the winding."""
import numpy as np
import pytest
import torch

from tests import meshcc_reference as CC
from tests import meshray_reference as M
from tests import meshvis_reference as V

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cached inputs are read-only)


def _mesh(vertices, faces):
    from perf_amd.mesh import Mesh
    return Mesh(_dev(np.asarray(vertices, dtype=np.float32).reshape(-1, 3)), _dev(np.asarray(faces, dtype=np.int32).reshape(-1, 3)))


def _bits(t):
    """The words of a result: float32 compared as int32, so that a NaN, the sign of a zero and the last bit all count."""
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_hits(got, want):
    for name, g, w in zip(('t', 'face', 'u', 'v'), got, want):
        g, w = _bits(g), _bits(w)
        differ = np.nonzero(g != w)[0]
        assert not len(differ), (name, len(differ), differ[:5], g[differ[:5]], w[differ[:5]])


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------------------
def _device_lists(vertices, faces, origin, cell, dims):
    """The device's cell lists as {cell: sorted list}, the flag, and the reference count, by the count -> scan -> write protocol."""
    from perf_amd import ops
    mesh = _mesh(vertices, faces)
    counts, flag = ops.meshray_grid_count(mesh.vertices, mesh.faces, origin, cell, dims)
    per_cell = counts.cpu().numpy().copy()
    offsets, total = ops.exclusive_scan_i32(counts)
    r = int(total.item())
    assert r == int(per_cell.sum())
    refs = ops.meshray_grid_write(mesh.vertices, mesh.faces, origin, cell, dims, counts, offsets, r)
    assert not counts.any()                                  # consumed
    refs, offsets = refs.cpu().numpy(), offsets.cpu().numpy()
    lists = {c: sorted(refs[offsets[c]:offsets[c] + n].tolist()) for c, n in enumerate(per_cell) if n}
    return lists, int(flag.item()), r


def _grid_cases():
    rng = np.random.default_rng(3)
    tri_v, tri_f = M.TRIANGLE
    loose = lambda n, lo, hi, size: ((rng.uniform(lo, hi, size=(n, 1, 3)) + rng.uniform(-size, size, size=(n, 3, 3))).reshape(-1, 3).astype(np.float32),
                                      np.arange(3 * n, dtype=np.int32).reshape(-1, 3))
    column = loose(200, (0.1, 0.1, 0.0), (0.9, 0.9, 64.0), 1.5)
    cube = loose(300, -1.0, 1.0, 0.3)
    return {
        'no_faces': (tri_v, np.zeros((0, 3), np.int32), (0, 0, 0), 1.0, (2, 2, 2)),
        'one_face_one_cell': (tri_v, tri_f, (-1, -1, 0), 8.0, (1, 1, 1)),
        'one_face_spanning_5x3x2': (tri_v, tri_f, (0, 0, 0), 1.0, (5, 3, 2)),              # z = 1 is the boundary plane of the two layers: listed in both
        'one_face_below_a_boundary_plane': (tri_v, tri_f, (0, 0, 0.25), 1.0, (5, 3, 2)),    # the margin (1/8) does not reach the upper layer
        'one_face_outside_the_box': (tri_v, tri_f, (8, 8, 8), 1.0, (2, 2, 2)),
        'faces_that_can_never_be_hit': (*M.SMALL, (-0.5, -0.5, 0), 0.75, (7, 7, 3)),
        'a_column_of_64_cells': (*column, (0, 0, 0), 1.0, (1, 1, 64)),
        'a_cube_of_17_cells': (*cube, (-1, -1, -1), 2.0 / 17.0, (17, 17, 17)),
    }


@pytest.mark.parametrize('name', list(_grid_cases()))
def test_cell_lists_equal_the_restatement(name):
    vertices, faces, origin, cell, dims = _grid_cases()[name]
    want, bad = M.cell_lists(vertices, faces, origin, cell, dims)
    got, flag, r = _device_lists(vertices, faces, origin, cell, dims)
    assert flag == bad and r == sum(len(s) for s in want.values())
    assert got == {c: sorted(s) for c, s in want.items()}                               # (a sorted list: no face twice in a cell)
    if name == 'faces_that_can_never_be_hit':
        assert flag == 0 and not any({0, 1} & set(s) for s in got.values())
    if name == 'one_face_spanning_5x3x2':
        assert len(got) == 30
    if name in ('no_faces', 'one_face_outside_the_box'):
        assert got == {} and r == 0


def test_a_capacity_below_the_counted_references_is_refused():
    from perf_amd import _lib, ops
    vertices, faces = M.TRIANGLE
    mesh = _mesh(vertices, faces)
    box = ((0, 0, 0), 1.0, (5, 3, 2))
    counts, _ = ops.meshray_grid_count(mesh.vertices, mesh.faces, *box)
    offsets, total = ops.exclusive_scan_i32(counts)
    assert int(total.item()) == 30
    refs = torch.empty(29, dtype=torch.int32, device='cuda')
    lib = _lib.load()
    import ctypes
    rc = lib.perf_meshray_grid_write(mesh.vertices.data_ptr(), 3, mesh.faces.data_ptr(), 1, (ctypes.c_float * 3)(0, 0, 0), 1.0, (ctypes.c_int32 * 3)(5, 3, 2),
                                     counts.data_ptr(), offsets.data_ptr(), 30, refs.data_ptr(), 29, None)
    assert rc == -1 and b'room for 29 references, 30 were counted' in lib.perf_last_error()
    assert int(counts.sum().item()) == 30                    # refused before the launch: nothing was consumed


# ---- 2. the cast -----------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _fixture(which):
    """(Mesh on the device, its vertices and faces on the host, the rays on the host) of the two large inputs, made once."""
    if which not in _CACHE:
        if which == 'hollow_sphere':
            (vertices, faces), rays = V.reference_mesh('hollow_sphere'), M.sphere_rays()
        else:
            (vertices, faces), rays = M.random_triangles(), M.triangle_rays()
        _CACHE[which] = (_mesh(vertices, faces), vertices, faces, rays)
    return _CACHE[which]


def _special_rays():
    """The hand cases' rays (t_min 0, t_max inf) and the degenerate ones, against M.SMALL (the triangle z = 1 is its face 4, the coincident
    pair z = 2 its faces 2 and 3)."""
    rays = [(o, d) for (o, d, t_min, t_max), _ in M.HAND_RAYS if t_min == 0.0 and t_max == np.inf]
    inf, nan = np.inf, np.nan
    rays += [((1, -1, 0.5), (0, 1, 0.25)),                   # in the plane x = 1, a cell boundary of every dyadic cell edge: hits (1, 1, 1) at t = 2
             ((-1, 2, 0), (1, 0, 0.5)),                      # in the plane y = 2
             ((1, 1, 5), (0, 0, -1)), ((1, 1, 1.5), (0, 0, 1)), ((1, 1, 1.5), (0, 0, -1)),          # from above; from between the two sheets, either way
             ((100, 100, 100), (-1, -1, -1)), ((100, 100, 100), (1, 0, 0)), ((-50, 1, 1.5), (1, 0, 0)),          # from far outside: towards, missing the box, between the sheets
             ((1, 1, 0), (0, 0, 0)), ((nan, 1, 0), (0, 0, 1)), ((1, 1, 0), (0, nan, 1)), ((inf, 1, 0), (-1, 0, 0)), ((1, 1, 0), (0, 0, inf)), ((1, 1, 0), (-inf, inf, 1)),
             ((1, 1, 0), (0, 0, 3e38)), ((1, 1, 0), (0, 0, 1e-38)), ((1, 1, -3e38), (0, 0, 1)), ((0.5, 0.25, 0), (1e-30, 0, 1))]
    o, d = (np.array([r[k] for r in rays], dtype=np.float32) for k in (0, 1))
    return o, d


@pytest.mark.parametrize('cell', [None, 1.0, 0.25, 64.0])
def test_special_rays_equal_the_restatement_to_the_bit(cell):
    from perf_amd.mesh import build_ray_grid, cast_rays
    vertices, faces = M.SMALL
    mesh = _mesh(vertices, faces)
    grid = build_ray_grid(mesh, cell)
    assert grid.bad_face == 0
    o, d = _special_rays()
    for t_min, t_max in ((0.0, np.inf), (1.0, 2.0), (0.5, 1.0), (1.25, 8.0), (0.0, 0.75), (-np.inf, np.inf), (2.0, 1.0)):
        want = M.cast(vertices, faces, o, d, t_min, t_max)
        _same_hits(cast_rays(mesh, grid, _dev(o), _dev(d), t_min, t_max), want)
        flag = cast_rays(mesh, grid, _dev(o), _dev(d), t_min, t_max, any_hit=True)
        assert flag.dtype == torch.uint8 and np.array_equal(flag.cpu().numpy(), (want[1] >= 0).astype(np.uint8))
    triangle = _mesh(*M.TRIANGLE)                           # the hand-computed answers themselves
    grid = build_ray_grid(triangle, cell)
    for (ro, rd, t_min, t_max), want in M.HAND_RAYS:
        got = cast_rays(triangle, grid, _dev(np.array([ro], np.float32)), _dev(np.array([rd], np.float32)), t_min, t_max)
        assert (float(got.t[0]), int(got.face[0]), float(got.u[0]), float(got.v[0])) == tuple(want), (ro, rd)


def _hand_grid(mesh, origin, cell, dims):
    """A RayGrid over a box given by hand, by the protocol itself: count -> scan -> ONE host read -> write."""
    from perf_amd import ops
    from perf_amd.mesh import RayGrid
    counts, flag = ops.meshray_grid_count(mesh.vertices, mesh.faces, origin, cell, dims)
    offsets, total = ops.exclusive_scan_i32(counts)
    r, bad = (int(v) for v in torch.cat([total, flag]).tolist())
    refs = ops.meshray_grid_write(mesh.vertices, mesh.faces, origin, cell, dims, counts, offsets, r)
    return RayGrid(tuple(float(v) for v in origin), float(cell), tuple(dims), offsets, refs, int(mesh.vertices.shape[0]), int(mesh.faces.shape[0]), bad)


@pytest.mark.parametrize('box', M.BOUNDARY_GRIDS, ids=lambda b: 'x'.join(str(n) for n in b[2]))
def test_rays_in_cell_boundary_planes_along_edges_and_through_corners(box):
    """build_ray_grid puts the box's corner at min - cell / 8, so no dyadic plane is a cell boundary there.  Here the corner and the cell are
    dyadic: the rays' planes x = 1, y = 2, z = 1 ARE cell boundaries, the diagonal rays pass through cell edges and corners, and the walk's
    entry parameters tie exactly.  Every finite vertex of M.SMALL lies inside each box, so the walked result is brute force's."""
    from perf_amd.mesh import cast_rays
    origin, cell, dims = box
    vertices, faces = M.SMALL
    finite = vertices[np.isfinite(vertices).all(axis=1)].astype(np.float64)
    assert (finite >= np.array(origin)).all() and (finite < np.array(origin) + cell * np.array(dims)).all()
    for k in range(3):                                       # planes the rays run in are cell boundaries of this grid (both but with cells of 2: x = y = z = 1)
        assert ((1.0 - origin[k]) / cell) % 1 == 0 and (cell == 2.0 or ((2.0 - origin[k]) / cell) % 1 == 0)
    mesh = _mesh(vertices, faces)
    grid = _hand_grid(mesh, origin, cell, dims)
    assert grid.bad_face == 0
    so, sd = _special_rays()
    o = np.concatenate([np.array([r[0] for r in M.BOUNDARY_RAYS], dtype=np.float32), so])
    d = np.concatenate([np.array([r[1] for r in M.BOUNDARY_RAYS], dtype=np.float32), sd])
    for t_min, t_max in ((0.0, np.inf), (-np.inf, np.inf), (1.0, 3.0), (0.0, 2.0)):
        want = M.cast(vertices, faces, o, d, t_min, t_max)
        _same_hits(cast_rays(mesh, grid, _dev(o), _dev(d), t_min, t_max), want)
        assert np.array_equal(cast_rays(mesh, grid, _dev(o), _dev(d), t_min, t_max, any_hit=True).cpu().numpy(), (want[1] >= 0).astype(np.uint8))
    want = M.cast(vertices, faces, o, d)
    assert int((want[1][:len(M.BOUNDARY_RAYS)] >= 0).sum()) == 24          # the boundary rays do meet the faces (the four that do not lie in the faces' planes)


@pytest.mark.parametrize('n', [0, 65537])
def test_ray_counts(n):
    from perf_amd.mesh import build_ray_grid, cast_rays
    vertices, faces = M.SMALL
    mesh = _mesh(vertices, faces)
    grid = build_ray_grid(mesh, 1.0)
    rng = np.random.default_rng(n)
    o = rng.uniform(-1, 5, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    so, sd = _special_rays()
    o[:min(n, len(so))], d[:min(n, len(sd))] = so[:n], sd[:n]
    got = cast_rays(mesh, grid, _dev(o), _dev(d))
    assert [tuple(t.shape) for t in got] == [(n,)] * 4 and [t.dtype for t in got] == [torch.float32, torch.int32, torch.float32, torch.float32]
    _same_hits(got, M.cast(vertices, faces, o, d))
    assert tuple(cast_rays(mesh, grid, _dev(o), _dev(d), any_hit=True).shape) == (n,)


@pytest.mark.parametrize('which', ['hollow_sphere', 'triangles'])
def test_random_rays_equal_the_restatement_and_do_not_depend_on_the_grid(which):
    from perf_amd.mesh import build_ray_grid, cast_rays
    mesh, vertices, faces, (o, d) = _fixture(which)
    want = M.expected_cast(which)
    assert 0.3 < (want[1] >= 0).mean() < 0.99                # the input exercises hits and misses
    default = build_ray_grid(mesh)
    longest = float((vertices.max(axis=0) - vertices.min(axis=0)).max())
    grids = [default, build_ray_grid(mesh, 2 * default.cell), build_ray_grid(mesh, 7.3 * default.cell), build_ray_grid(mesh, 4 * longest)]
    assert grids[3].dims == (1, 1, 1) and int(grids[3].refs.numel()) == len(faces)          # brute force on the device
    assert max(default.dims) > 8 and len({g.dims for g in grids}) == 4
    ro, rd = _dev(o), _dev(d)
    first = cast_rays(mesh, default, ro, rd)
    _same_hits(first, want)
    for grid in grids:
        _same_hits(cast_rays(mesh, grid, ro, rd), first)     # (the default again: two runs are bit-identical)
        assert np.array_equal(cast_rays(mesh, grid, ro, rd, any_hit=True).cpu().numpy(), (want[1] >= 0).astype(np.uint8))


# ---- 3. the occlusion ------------------------------------------------------------------------------------------------------------------------
def _views_of(centres):
    out = []
    for c in centres:
        view = V.constant_view(tuple(float(x) for x in c), 2.0, (4, 8))
        out.append({'pose': _dev(view['pose']), 'distance_map': _dev(view['distance_map'])})
    return out


@pytest.mark.parametrize('n_views,density', [(1, 0.7), (3, 0.5), (64, 1 / 16)])
def test_occluded_bits_equal_the_restatement(n_views, density):
    from perf_amd.mesh import Visibility, build_ray_grid, vertex_occlusion
    mesh, vertices, faces, _ = _fixture('hollow_sphere')
    rng = np.random.default_rng(100 + n_views)
    centres = rng.uniform(-1.2, 1.2, size=(n_views, 3)).astype(np.float32)
    centres[0] = M.VIEW
    mask = np.zeros(len(vertices), dtype=np.uint64)
    for k in range(64):                                      # bits at and above K are set too: they must come back 0
        mask |= (rng.random(len(vertices)) < density).astype(np.uint64) << np.uint64(k)
    mask = mask.view(np.int64)
    want = M.occluded(vertices, faces, centres, mask)
    visibility = Visibility(_dev(mask), torch.zeros(len(vertices), dtype=torch.int64, device='cuda'), n_views)
    views = _views_of(centres)
    for cell in (None, 0.5):
        got = vertex_occlusion(mesh, build_ray_grid(mesh, cell), views, visibility).cpu().numpy()
        assert np.array_equal(got, want)
    low = np.uint64((1 << n_views) - 1) if n_views < 64 else ~np.uint64(0)
    assert not (got.view(np.uint64) & ~(mask.view(np.uint64) & low)).any() and want.any()


def test_incident_faces_are_not_tested_and_empty_inputs_work():
    from perf_amd.mesh import Visibility, build_ray_grid, vertex_occlusion
    ring = [(np.cos(a), np.sin(a), 0.0) for a in np.arange(8) * np.pi / 4]
    vertices = np.array([(0, 0, 1)] + ring, dtype=np.float32)          # a cone: a fan of 8 faces around its apex, vertex 0
    faces = np.array([(0, 1 + i, 1 + (i + 1) % 8) for i in range(8)], dtype=np.int32)
    mesh = _mesh(vertices, faces)
    grid = build_ray_grid(mesh)
    centres = np.array([(0, 0, 3), (0.3, -0.2, 2.5), (0, 0, -3), (-3, 0.1, 0.2)], dtype=np.float32)          # two on the apex's side, one below, one beside
    ones = np.full(9, -1, dtype=np.int64)
    zero = torch.zeros(9, dtype=torch.int64, device='cuda')
    got = vertex_occlusion(mesh, grid, _views_of(centres), Visibility(_dev(ones), zero, 4)).cpu().numpy()
    want = M.occluded(vertices, faces, centres, ones)
    assert np.array_equal(got, want)
    assert not (got & 3).any() and got[0] == 0 and (got & 8).any()          # nothing from the apex's side; the apex: every face names it; the cone hides its far side
    # K = 0, and V = 0
    assert not vertex_occlusion(mesh, grid, [], Visibility(_dev(ones), zero, 0)).any()
    empty = _mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    none = torch.zeros(0, dtype=torch.int64, device='cuda')
    grid = build_ray_grid(empty)
    assert grid.dims == (1, 1, 1) and grid.refs.numel() == 0
    assert tuple(vertex_occlusion(empty, grid, _views_of(centres), Visibility(none, none, 4)).shape) == (0,)
    from perf_amd.mesh import cast_rays
    got = cast_rays(empty, grid, _dev(np.zeros((2, 3), np.float32)), _dev(np.ones((2, 3), np.float32)))
    assert got.face.tolist() == [-1, -1] and torch.isinf(got.t).all()


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------------
def _surface(which):
    """The device's surface-nets mesh of the hollow sphere / the shell with a tunnel / the ball, made once."""
    key = 'surface_' + which
    if key not in _CACHE:
        from perf_amd.mesh import surface_nets
        field = {'hollow_sphere': CC.hollow_sphere, 'tunnel': V.tunnel_field, 'ball': M.ball_field}[which]()
        _CACHE[key] = surface_nets(_dev(field), 0.0, CC.SPHERE_LO, CC.SPHERE_HI)
    return _CACHE[key]


def _same_mesh(a, b):
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.faces, b.faces)


def test_on_the_hollow_sphere_the_occlusion_cull_is_the_inward_component_whatever_the_winding():
    from perf_amd.mesh import Mesh, clean_mesh, cull_occluded, cull_unseen
    mesh = _surface('hollow_sphere')
    views = _views_of([M.VIEW])                              # the map (2.0) passes every vertex
    _same_mesh(cull_unseen(mesh, views, facing=False), mesh)
    inward = clean_mesh(mesh, orientation='inward')
    assert (inward.faces.shape[0], inward.vertices.shape[0]) == (768, 386)
    _same_mesh(cull_occluded(mesh, views, facing=False), inward)
    _same_mesh(cull_occluded(mesh, views), inward)
    _same_mesh(cull_occluded(mesh, views, facing=False, cell=0.37), inward)
    # the winding reversed: the facing heuristic keeps the wrong skin (or nothing), the segment test the same 768 faces
    flipped = Mesh(mesh.vertices, mesh.faces[:, [0, 2, 1]].contiguous())
    assert cull_unseen(flipped, views).faces.shape[0] in (2196, 0)
    got = cull_occluded(flipped, views, facing=False)
    assert torch.equal(got.vertices.view(torch.int32), inward.vertices.view(torch.int32)) and torch.equal(got.faces, inward.faces[:, [0, 2, 1]])


def test_on_the_tunnel_field_the_occlusion_cull_keeps_the_restatements_faces():
    from perf_amd.mesh import cull_occluded
    mesh = _surface('tunnel')
    vertices, faces = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    occluded = M.occluded(vertices, faces, [M.VIEW], np.ones(len(vertices), dtype=np.int64)) != 0
    keep = ~occluded[faces.astype(np.int64)].any(axis=1)
    assert int(keep.sum()) == 802
    want_vertices, want_faces, _ = V.filter_faces(vertices, faces, keep)
    got = cull_occluded(mesh, _views_of([M.VIEW]), facing=False)
    assert np.array_equal(got.vertices.cpu().numpy().view(np.int32), want_vertices.view(np.int32)) and np.array_equal(got.faces.cpu().numpy(), want_faces.reshape(-1, 3))


def test_mesh_distance_from_the_centre_of_a_ball():
    from perf_amd.mesh import build_ray_grid, cast_rays, mesh_distance
    mesh = _surface('ball')
    vertices, faces = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    o, d = M.ball_rays()
    want = M.cast(vertices, faces, o, d)
    assert (want[1] >= 0).all()                              # the seed: no ray of the restatement slips through an edge
    grid = build_ray_grid(mesh)
    got = mesh_distance(mesh, grid, _dev(o), _dev(d))
    assert np.array_equal(_bits(got), _bits(want[0]))
    _same_hits(cast_rays(mesh, grid, _dev(o), _dev(d)), want)
    distance = got.cpu().numpy().astype(np.float64) * np.linalg.norm(d.astype(np.float64), axis=1)
    assert np.abs(distance - M.BALL_RADIUS).max() <= M.BALL_SPACING          # within one lattice spacing of the radius


def test_render_mesh_distance_has_the_shape_of_the_rendered_distance():
    from perf_amd.scene import NeRFScene, Rays
    mesh = _surface('ball')
    o, d = M.ball_rays(64)
    rays = Rays(_dev(o).view(8, 8, 3), _dev(d).view(8, 8, 3))
    got = NeRFScene.render_mesh_distance(None, mesh, rays)
    assert tuple(got.shape) == (8, 8, 1) and (got - M.BALL_RADIUS).abs().max() <= M.BALL_SPACING
    away = Rays(_dev(o + 5).view(8, 8, 3), _dev(np.abs(d)).view(8, 8, 3))
    assert (NeRFScene.render_mesh_distance(None, mesh, away) == 5.0).all()          # a miss holds what the eval tail leaves for an empty ray
