"""The connected components of a triangle mesh (include/perf_hip_meshcc.h, perf_amd/mesh.py) on the GPU.  The yardstick is the numpy
restatement tests/meshcc_reference.py (pinned against scipy by tests/test_cpu_meshcc_reference.py): labels, counts, selections and
compacted meshes are compared EXACTLY; only the signed volumes have a tolerance, derived in meshcc_reference.volume_tolerance from the
kernel's own arithmetic.  End to end the cleaning is checked as an identity: dropping a component of a surface-nets mesh IS meshing the
field without the thing that made it, vertices to the bit."""
import math

import numpy as np
import pytest
import torch

from tests import meshcc_reference as CC

pytestmark = pytest.mark.gpu

LO, HI = [-1.0, -1.25, -0.5], [1.0, 0.75, 1.0]           # (the box of tests/test_gpu_mesh.py: the three axes scale differently)


def _components(faces, V, vertices=None):
    from perf_amd.mesh import connected_components
    v = None if vertices is None else torch.from_numpy(np.ascontiguousarray(vertices, dtype=np.float32)).cuda()
    comps = connected_components(torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).cuda(), n_vertices=V, vertices=v)
    assert comps.vertex_component.dtype == torch.int32 and comps.faces.dtype == torch.int64 and comps.vertices.dtype == torch.int32
    assert tuple(comps.vertex_component.shape) == (V,) and comps.faces.shape == comps.vertices.shape
    assert (comps.signed_volume is None) == (vertices is None)
    return comps


def _check_case(name):
    faces, V = CC.cases()[name]
    vc, C, per_faces, per_vertices = CC.expected(name)
    comps = _components(faces, V)
    assert comps.faces.numel() == C
    assert np.array_equal(comps.vertex_component.cpu().numpy(), vc)
    assert np.array_equal(comps.faces.cpu().numpy(), per_faces) and np.array_equal(comps.vertices.cpu().numpy(), per_vertices)
    return comps


@pytest.mark.parametrize('name', ['empty', 'five_loose_vertices', 'one_triangle', 'two_triangles_one_shared_vertex', 'two_triangles_disjoint', 'repeated_index'])
def test_degenerate(name):
    _check_case(name)


@pytest.mark.parametrize('V', CC.EDGE_SIZES)
@pytest.mark.parametrize('kind', ['fan', 'strip'])
def test_wave_and_workgroup_edges(kind, V):
    _check_case(f'{kind}_{V}')


@pytest.mark.parametrize('order', ['ascending', 'descending', 'permuted'])
def test_diameter(order):
    """A path of ~ V / 2 hops: what a propagation with too few rounds or a retry from a stale read gets wrong."""
    _check_case('quad_strip_' + order)


@pytest.mark.parametrize('name', ['hub', 'disjoint_triangles'])
def test_contention(name):
    _check_case(name)


@pytest.mark.parametrize('name', ['random_quarter', 'random_half', 'random_full'])
def test_random_graphs(name):
    _check_case(name)


@pytest.mark.parametrize('name', ['random_half', 'quad_strip_permuted', 'disjoint_triangles', 'hub'])
def test_the_order_of_the_faces_does_not_matter(name):
    faces, V = CC.cases()[name]
    vc, C, per_faces, per_vertices = CC.expected(name)
    shuffled = faces[np.random.default_rng(5).permutation(len(faces))]
    comps = _components(shuffled, V)
    assert np.array_equal(comps.vertex_component.cpu().numpy(), vc)
    assert np.array_equal(comps.faces.cpu().numpy(), per_faces) and np.array_equal(comps.vertices.cpu().numpy(), per_vertices)


# ---- end to end: surface nets of synthetic fields ---------------------------------------------------------------------------------------
def _mesh_of(field, lo=LO, hi=HI):
    from perf_amd.mesh import surface_nets
    return surface_nets(torch.from_numpy(field).cuda(), 0.0, lo, hi)


_BALLS = {}


def _balls():
    """The mesh of the five balls and the speck and its components, made once."""
    if not _BALLS:
        from perf_amd.mesh import connected_components
        mesh = _mesh_of(CC.balls_field())
        _BALLS['mesh'], _BALLS['components'] = mesh, connected_components(mesh)
    return _BALLS['mesh'], _BALLS['components']


def _same(a, b):
    assert a.vertices.dtype == b.vertices.dtype == torch.float32 and a.faces.dtype == b.faces.dtype == torch.int32
    assert a.vertices.shape == b.vertices.shape and torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))          # to the bit
    assert torch.equal(a.faces, b.faces)


def test_the_balls_have_the_stated_components():
    mesh, comps = _balls()
    assert tuple(mesh.vertices.shape) == (1376, 3) and tuple(mesh.faces.shape) == (2728, 3)
    assert tuple(comps.faces.tolist()) == CC.BALLS_FACES and tuple(comps.vertices.tolist()) == CC.BALLS_VERTICES
    vc, C = CC.components(mesh.faces.cpu().numpy(), 1376)
    assert C == 6 and np.array_equal(comps.vertex_component.cpu().numpy(), vc)
    assert (comps.signed_volume > 0).all()


def test_dropping_the_speck_is_meshing_the_field_without_it():
    from perf_amd.mesh import clean_mesh
    mesh, _ = _balls()
    _same(clean_mesh(mesh, min_faces=100), _mesh_of(CC.balls_field(speck=False)))


@pytest.mark.parametrize('ball', range(5))
def test_dropping_a_ball_is_meshing_the_field_without_it(ball):
    from perf_amd.mesh import filter_mesh
    mesh, comps = _balls()
    vc = comps.vertex_component.long()
    lattice = (mesh.vertices.double().cpu() - torch.tensor(LO, dtype=torch.float64)) / (torch.tensor(HI, dtype=torch.float64) - torch.tensor(LO, dtype=torch.float64)) \
        * torch.tensor(CC.SHAPE, dtype=torch.float64)
    centres = torch.stack([lattice[vc.cpu() == c].mean(dim=0) for c in range(6)])
    component = int((centres - torch.tensor(CC.BALLS[ball][0], dtype=torch.float64)).norm(dim=1).argmin())          # the ball's component
    assert float((centres[component] - torch.tensor(CC.BALLS[ball][0], dtype=torch.float64)).norm()) < 0.5
    keep = torch.ones(6, dtype=torch.bool, device='cuda')
    keep[component] = False
    cleaned, index = filter_mesh(mesh, comps, keep)
    _same(cleaned, _mesh_of(CC.balls_field(without=ball)))
    assert index.dtype == torch.int32 and torch.equal(index.long(), torch.nonzero(vc != component).flatten())


def test_keep_largest_breaks_the_tie_by_the_lower_id():
    from perf_amd.mesh import clean_mesh, select_components
    mesh, comps = _balls()
    assert torch.nonzero(select_components(comps, keep_largest=3)).flatten().tolist() == [0, 1, 3]          # 3 and 4 tie at 444 faces
    for kw in ({'keep_largest': 1}, {'keep_largest': 4}, {'keep_largest': 0}, {'keep_largest': 9}, {'min_faces': 444}, {'min_faces': 445, 'keep_largest': 3},
               {'orientation': 'outward'}, {'orientation': 'inward'}, {'min_faces': 29, 'orientation': 'outward', 'keep_largest': 5}):
        want = CC.select(comps.faces.cpu().numpy(), comps.signed_volume.cpu().numpy(), **kw)
        assert select_components(comps, **kw).cpu().numpy().tolist() == want.tolist(), kw
    assert clean_mesh(mesh, keep_largest=3).faces.shape[0] == 732 + 828 + 444
    empty = clean_mesh(mesh, orientation='inward')
    assert tuple(empty.vertices.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 3)


def test_cleaning_is_bit_identical_from_run_to_run():
    from perf_amd.mesh import clean_mesh, connected_components, filter_mesh, select_components
    faces, V = CC.cases()['random_half']
    vertices = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (V, 3)).astype(np.float32)).cuda()
    from perf_amd.mesh import Mesh
    mesh = Mesh(vertices, torch.from_numpy(faces).cuda())
    runs = []
    for _ in range(2):
        comps = connected_components(mesh)
        cleaned, index = filter_mesh(mesh, comps, select_components(comps, min_faces=2, keep_largest=40))
        again = clean_mesh(mesh, min_faces=2, keep_largest=40)
        _same(cleaned, again)
        runs.append((cleaned, index))
    _same(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    vc, C, per_faces, _ = CC.expected('random_half')
    v, f, idx = CC.filter_mesh(vertices.cpu().numpy(), faces, vc, CC.select(per_faces, min_faces=2, keep_largest=40))
    assert np.array_equal(runs[0][0].vertices.cpu().numpy(), v) and np.array_equal(runs[0][0].faces.cpu().numpy(), f) and np.array_equal(runs[0][1].cpu().numpy(), idx)


def test_orientation_picks_a_skin_of_the_hollow_sphere():
    from perf_amd.mesh import clean_mesh, connected_components
    mesh = _mesh_of(CC.hollow_sphere(), CC.SPHERE_LO, CC.SPHERE_HI)
    comps = connected_components(mesh)
    assert sorted(comps.faces.tolist()) == [768, 2196]
    inner, outer = clean_mesh(mesh, orientation='inward'), clean_mesh(mesh, orientation='outward')
    assert inner.faces.shape[0] == 768 and outer.faces.shape[0] == 2196
    assert connected_components(inner).faces.tolist() == [768] and connected_components(outer).faces.tolist() == [2196]
    assert inner.vertices.shape[0] + outer.vertices.shape[0] == mesh.vertices.shape[0]


@pytest.mark.parametrize('which', ['balls', 'hollow_sphere'])
def test_signed_volumes(which):
    """|device - reference| <= n (n + 8) u M^3 per component of n faces inside |x| <= M, u = 2^-53 (meshcc_reference.volume_tolerance:
    6 u M^3 for forming one term a . (b x c) / 6 <= M^3 in double, (n - 1) u n M^3 for adding n of them in any order).  The reference:
    math.fsum over per-face terms formed in numpy.longdouble.  M = 1.25 for the balls' box, 1 for the sphere's."""
    from perf_amd.mesh import connected_components
    mesh = _balls()[0] if which == 'balls' else _mesh_of(CC.hollow_sphere(), CC.SPHERE_LO, CC.SPHERE_HI)
    M = 1.25 if which == 'balls' else 1.0
    assert float(mesh.vertices.abs().max()) <= M
    comps = connected_components(mesh)
    per_faces, _, want = CC.stats(mesh.faces.cpu().numpy(), comps.vertex_component.cpu().numpy(), comps.faces.numel(), mesh.vertices.cpu().numpy())
    got = comps.signed_volume.cpu().numpy()
    assert got.dtype == np.float64
    for c in range(len(want)):
        err, tol = abs(got[c] - want[c]), CC.volume_tolerance(int(per_faces[c]), M)
        print(f'{which} component {c}: {int(per_faces[c])} faces, volume {want[c]:+.6f}, error {err:.3e}, tolerance {tol:.3e}')
        assert err <= tol, (c, got[c], want[c], tol)
    if which == 'hollow_sphere':
        assert abs(got[np.argmax(per_faces)] - 1.80) < 0.01 and abs(got[np.argmin(per_faces)] + 0.34) < 0.01


def test_colors_and_normals_are_carried():
    from perf_amd.mesh import Mesh, clean_mesh, filter_mesh, select_components
    mesh, comps = _balls()
    g = torch.Generator(device='cuda').manual_seed(1)
    colors = torch.rand(1376, 3, device='cuda', generator=g)
    normals = torch.nn.functional.normalize(torch.randn(1376, 3, device='cuda', generator=g), dim=1)
    full = Mesh(mesh.vertices, mesh.faces, colors, normals)
    keep = select_components(comps, min_faces=300)
    cleaned, index = filter_mesh(full, comps, keep)
    assert torch.equal(cleaned.colors, colors[index.long()]) and torch.equal(cleaned.normals, normals[index.long()])
    assert torch.equal(cleaned.vertices, mesh.vertices[index.long()])
    again = clean_mesh(full, min_faces=300)
    assert torch.equal(again.colors, cleaned.colors) and torch.equal(again.normals, cleaned.normals)
    only_colors = clean_mesh(Mesh(mesh.vertices, mesh.faces, colors, None), min_faces=300)
    assert only_colors.normals is None and torch.equal(only_colors.colors, cleaned.colors)


def test_the_brick_path_cleans_to_the_same_components():
    from perf_amd.mesh import clean_mesh, connected_components, surface_nets_bricks
    shape = (24, 24, 32)                                     # the balls' lattice padded to a multiple of 8
    field = CC.balls_field(shape=shape)
    dense = clean_mesh(_mesh_of(field), min_faces=100)
    bricks = tuple(s // 8 for s in shape)
    m = bricks[0] * bricks[1] * bricks[2]
    values = np.ascontiguousarray(field[:24, :24, :32].reshape(bricks[0], 8, bricks[1], 8, bricks[2], 8).transpose(0, 2, 4, 1, 3, 5)).reshape(m, 8, 8, 8)
    ids = torch.arange(m, dtype=torch.int32, device='cuda')
    sparse, _ = surface_nets_bricks(torch.from_numpy(values).cuda(), ids, ids.view(bricks).clone(), shape, 0.0, -1.0, LO, HI)
    assert sparse.faces.shape[0] == 2728
    pairs = lambda mesh: sorted(zip(*(t.tolist() for t in connected_components(mesh)[1:3])))
    cleaned = clean_mesh(sparse, min_faces=100)
    assert pairs(cleaned) == pairs(dense) == sorted(zip(CC.BALLS_FACES[:5], CC.BALLS_VERTICES[:5]))
    assert len(pairs(sparse)) == 6


def test_capacities_below_the_counted_totals_are_refused():
    from perf_amd import ops
    from perf_amd._lib import PerfError
    mesh, comps = _balls()
    keep = comps.faces >= 100
    counts, ws = ops.meshcc_filter_count(mesh.faces, comps.vertex_component, keep)
    assert counts.tolist() == [1376 - 16, 2728 - 28]
    with pytest.raises(PerfError, match='room for 1359 vertices, 1360 were counted'):
        ops.meshcc_filter_write(mesh.faces, comps.vertex_component, keep, ws, 1359, 2700, mesh.vertices)
    with pytest.raises(PerfError, match='room for 2699 faces, 2700 were counted'):
        ops.meshcc_filter_write(mesh.faces, comps.vertex_component, keep, ws, 1360, 2699, mesh.vertices)
    vertices, faces, index = ops.meshcc_filter_write(mesh.faces, comps.vertex_component, keep, ws, 1360, 2700, mesh.vertices)
    assert int(faces.max()) == 1359 and int(faces.min()) == 0 and torch.equal(vertices, mesh.vertices[index.long()])


@pytest.mark.parametrize('bad', ['V', -1])
def test_a_face_index_outside_the_vertices_is_refused(bad):
    from perf_amd._lib import PerfError
    from perf_amd.mesh import connected_components
    V = 300
    faces = CC.strip(V).copy()
    faces[7, 1] = faces[150, 2] = V if bad == 'V' else -1
    with pytest.raises(PerfError, match=r'face 7 = \[7, ' + str(V if bad == 'V' else -1) + r', 9\] has an index outside \[0, 300\)'):
        connected_components(torch.from_numpy(faces).cuda(), n_vertices=V)
    faces = CC.strip(V)                                      # and the device is as it was: the next call labels
    assert connected_components(torch.from_numpy(faces).cuda(), n_vertices=V).faces.tolist() == [V - 2]
