"""The simplification by vertex clustering (include/perf_hip_meshsimp.h, perf_amd/mesh.py) on the GPU.  The yardstick is the numpy
restatement tests/meshsimp_reference.py (pinned against an independent formulation by tests/test_cpu_meshsimp_reference.py): cluster
ids, positions, representatives, remapped faces, keep masks and compacted meshes are compared EXACTLY, floats to the bit.  The probe
chains are built from the hash functions the header states."""
import numpy as np
import pytest
import torch

from tests import meshsimp_reference as R

pytestmark = pytest.mark.gpu

LO, HI = (-1.0, -1.25, -0.5), (1.0, 0.75, 1.0)
BOX = (LO, HI)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _check_clusters(vertices, cell, box, placement='mean'):
    """cluster_vertices against the restatement -> (Clusters, vertex_cluster of the restatement)."""
    from perf_amd.mesh import cluster_vertices
    lo, h, n = R.grid_of(cell, box)
    vc, C, placed, rep, _ = R.cluster(vertices, lo, h, n, placement)
    got = cluster_vertices(_dev(vertices, np.float32).view(-1, 3), cell, box, placement)
    assert got.vertex_cluster.dtype == torch.int32 and got.representative.dtype == torch.int32 and got.vertices.dtype == torch.float32
    assert got.n_clusters == C and tuple(got.vertices.shape) == (C, 3) and tuple(got.representative.shape) == (C,)
    assert np.array_equal(got.vertex_cluster.cpu().numpy(), vc)
    assert np.array_equal(got.representative.cpu().numpy(), rep)
    assert np.array_equal(_bits(got.vertices), placed.view(np.int32))
    return got, vc


def _check_faces(faces, clusters, vc, dedupe):
    from perf_amd.mesh import cluster_faces
    r, keep = R.cluster_faces(faces, vc, dedupe)
    got_r, got_keep = cluster_faces(_dev(faces, np.int32).view(-1, 3), clusters, dedupe)
    assert got_r.dtype == torch.int32 and got_keep.dtype == torch.uint8
    assert np.array_equal(got_r.cpu().numpy(), r) and np.array_equal(got_keep.cpu().numpy(), keep)
    return keep


def _check_simplify(vertices, faces, cell, box=BOX, placement='mean', dedupe='oriented'):
    from perf_amd.mesh import Mesh, simplify_mesh
    lo, h, n = R.grid_of(cell, box)
    v, f, k = R.simplify(vertices, faces, lo, h, n, placement, dedupe)
    mesh, index = simplify_mesh(Mesh(_dev(vertices, np.float32).view(-1, 3), _dev(faces, np.int32).view(-1, 3)), cell, box, placement, dedupe)
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32 and index.dtype == torch.int32
    assert tuple(mesh.vertices.shape) == v.shape and tuple(mesh.faces.shape) == f.shape
    assert np.array_equal(_bits(mesh.vertices), v.view(np.int32)) and np.array_equal(mesh.faces.cpu().numpy(), f) and np.array_equal(index.cpu().numpy(), k)
    return mesh, index


# ---- scan and group edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', R.EDGE_SIZES)
def test_scan_and_group_edges_of_the_vertices(V):
    """V at the edges of a wave, a workgroup and a level of the scan; a cell that leaves a few members per cluster."""
    vertices = R.random_vertices(V, 100 + V)
    clusters, vc = _check_clusters(vertices, 0.07 if V > 1000 else 0.4, BOX)
    if V >= 3:
        _check_faces(R.strip(V), clusters, vc, 'oriented')


@pytest.mark.parametrize('F', R.EDGE_SIZES)
def test_scan_and_group_edges_of_the_faces(F):
    """F at the same edges: random triangles over 300 vertices in about 150 cells."""
    vertices = R.random_vertices(300, 7)
    faces = np.random.default_rng(200 + F).integers(0, 300, size=(F, 3)).astype(np.int32)
    for dedupe in ('oriented', 'unoriented', None):
        _check_simplify(vertices, faces, 0.35, dedupe=dedupe)


# ---- probe chains -----------------------------------------------------------------------------------------------------------------------------
GRID21 = ((0.0, 0.0, 0.0), (float(1 << 21),) * 3)


def test_a_probe_chain_of_4097_cells_from_one_slot():
    """4,097 vertices in different cells whose walks all start at one slot of the 16,384: the last to arrive passes 4,096 others."""
    keys = R.colliding_cells(4097, 14)
    vertices = R.vertices_of_keys(keys)
    assert R.table_slots(4097) == 1 << 14 and R.grid_of(1.0, GRID21)[2] == [1 << 21] * 3
    clusters, vc = _check_clusters(vertices, 1.0, GRID21)
    assert clusters.n_clusters == 4097 and np.array_equal(vc, np.arange(4097))
    twice = np.concatenate([vertices, vertices[::-1]])          # and every cell a second time, the chain walked to its own slot again
    clusters, vc = _check_clusters(twice, 1.0, GRID21)
    assert clusters.n_clusters == 4097


@pytest.mark.parametrize('V', [128, 4096, 65536])
def test_a_table_filled_to_its_stated_minimum(V):
    """2 V is a power of two: the table has exactly 2 V slots, and every vertex has a cell of its own."""
    assert R.table_slots(V) == max(2 * V, 256)
    rng = np.random.default_rng(V)
    keys = rng.permutation(np.unique(rng.integers(0, 1 << 30, size=2 * V)))[:V].astype(np.int64)
    assert len(keys) == V
    keys = (keys & 0x3ff) << 42 | ((keys >> 10) & 0x3ff) << 21 | (keys >> 20)
    clusters, vc = _check_clusters(R.vertices_of_keys(keys), 1.0, GRID21)
    assert clusters.n_clusters == V


@pytest.mark.parametrize('dedupe', ['oriented', 'unoriented'])
def test_a_probe_chain_of_4097_face_triples_from_one_slot(dedupe):
    """16,384 vertices in cells of their own (cluster id = index), 4,097 different triples whose walks start at one slot, each twice."""
    V = 1 << 14
    vertices = R.vertices_of_keys(np.arange(V, dtype=np.int64) * 3 + 1)
    triples = R.colliding_triples(4097, 14, V, dedupe)
    once = np.concatenate([triples, triples[:2047]])          # 6,144 faces: a table of 2^14 slots, the slot the triples were built for
    assert R.table_slots(len(once)) == 1 << 14
    again = once[:, [1, 2, 0]] if dedupe == 'oriented' else once[:, [0, 2, 1]]
    again[:4097] = once[:4097][::-1][:, [2, 0, 1]]
    clusters, vc = _check_clusters(vertices, 1.0, GRID21)
    assert np.array_equal(vc, np.arange(V))
    keep = _check_faces(once, clusters, vc, dedupe)
    assert keep.sum() == 4097
    _check_simplify(vertices, again, 1.0, GRID21, dedupe=dedupe)


@pytest.mark.parametrize('F', [128, 4096])
def test_a_face_table_filled_to_its_stated_minimum(F):
    V = 3 * F
    vertices = R.vertices_of_keys(np.arange(V, dtype=np.int64) * 5 + 2)
    faces = np.random.default_rng(F).permutation(V).astype(np.int32).reshape(F, 3)          # F different triples
    mesh, _ = _check_simplify(vertices, faces, 1.0, GRID21)
    assert R.table_slots(F) == max(2 * F, 256) and mesh.faces.shape[0] == F


# ---- one hot address --------------------------------------------------------------------------------------------------------------------------
def test_all_vertices_in_one_cell():
    """65,537 vertices in ONE cell: one contended slot, three contended sums, one contended minimum."""
    vertices = R.random_vertices(65537, 3, (0.1, 0.1, 0.1), (0.9, 0.9, 0.9))
    lo, h, n = R.grid_of(1.0, ((0, 0, 0), (1, 1, 1)))
    assert n == [1, 1, 1] and R.cluster(vertices, lo, h, n)[4] == 0          # (no tie for the representative)
    for placement in ('mean', 'member'):
        clusters, vc = _check_clusters(vertices, 1.0, ((0, 0, 0), (1, 1, 1)), placement)
        assert clusters.n_clusters == 1
    _check_simplify(vertices, R.strip(65537), 1.0, ((0, 0, 0), (1, 1, 1)))


def test_257_cells_of_255_members_each():
    rng = np.random.default_rng(4)
    cell_of = np.repeat(np.arange(257), 255)
    vertices = (np.stack([cell_of % 7, (cell_of // 7) % 7, cell_of // 49], axis=1) + 0.05 + 0.9 * rng.random((257 * 255, 3))).astype(np.float32)
    box = ((0, 0, 0), (7, 7, 7))
    lo, h, n = R.grid_of(1.0, box)
    assert R.cluster(vertices, lo, h, n)[4] == 0
    clusters, _ = _check_clusters(vertices, 1.0, box)
    assert clusters.n_clusters == 257
    shuffled = vertices[rng.permutation(len(vertices))]          # and with no run of one cell along a wave
    assert R.cluster(shuffled, lo, h, n)[4] == 0
    _check_clusters(shuffled, 1.0, box, 'member')


# ---- geometry edges ---------------------------------------------------------------------------------------------------------------------------
def test_vertices_on_cell_faces_at_the_borders_and_outside():
    g = np.arange(0, 5, dtype=np.float64) * 0.25          # exactly on the cell faces of lo = 0, h = 0.25, n = 4: at lo, at hi (t = n, f = 1)
    on_faces = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    outside = np.array([[-3, 0.3, 0.3], [5, 0.3, 0.3], [0.3, -1e30, 1e30], [1.0000001, 0.9999999, -1e-30], [3e38, -3e38, 0.5]])
    inside = R.random_vertices(200, 9, (0, 0, 0), (1, 1, 1))
    vertices = np.concatenate([on_faces, outside, inside]).astype(np.float32)
    box = ((0, 0, 0), (1, 1, 1))
    for placement in ('mean', 'member'):
        clusters, _ = _check_clusters(vertices, 0.25, box, placement)
    assert clusters.n_clusters == 64
    _check_simplify(vertices, np.random.default_rng(1).integers(0, len(vertices), size=(500, 3)), 0.25, box)


@pytest.mark.parametrize('cell', [0.3, 0.1, 1 / 3, 0.0123])
def test_a_cell_edge_that_is_no_power_of_two(cell):
    vertices = R.random_vertices(3000, 21)
    _check_clusters(vertices, cell, BOX)
    _check_simplify(vertices, np.random.default_rng(2).integers(0, 3000, size=(6000, 3)), cell, placement='member')


def test_a_grid_of_1_by_1_by_2_to_the_21():
    rng = np.random.default_rng(5)
    z = np.concatenate([rng.integers(0, 1 << 21, size=2000), [0, (1 << 21) - 1, (1 << 21) - 1]])
    vertices = np.stack([rng.random(len(z)), rng.random(len(z)), z + np.float32(0.5)], axis=1).astype(np.float32)
    box = ((0, 0, 0), (1.0, 1.0, float(1 << 21)))
    assert R.grid_of(1.0, box)[2] == [1, 1, 1 << 21]
    _check_clusters(vertices, 1.0, box)
    from perf_amd._lib import PerfError
    from perf_amd.mesh import cluster_vertices
    with pytest.raises(PerfError, match='more than 2\\^21'):
        cluster_vertices(_dev(vertices, np.float32), 1.0, ((0, 0, 0), (1.0, 1.0, float(1 << 21) + 1)))


def test_coordinates_of_a_million():
    vertices = (1e6 + 40 * np.random.default_rng(6).random((4000, 3))).astype(np.float32)
    box = ((1e6 - 1, 1e6 - 1, 1e6 - 1), (1e6 + 41, 1e6 + 41, 1e6 + 41))
    _check_clusters(vertices, 2.5, box)
    _check_simplify(vertices, R.strip(4000), 2.5, box, 'member')


def test_the_box_of_the_vertices_themselves():
    """box=None: the bounds come from the device (exactly: minima and maxima), the grid from them."""
    from perf_amd import ops
    vertices = R.random_vertices(70001, 8)
    vertices[17] = [-7.5, 0.0, 3.25]
    bounds = ops.meshsimp_bounds(_dev(vertices, np.float32)).cpu().numpy()
    assert np.array_equal(bounds[:3], vertices.min(axis=0)) and np.array_equal(bounds[3:], vertices.max(axis=0))
    box = (vertices.min(axis=0).tolist(), vertices.max(axis=0).tolist())
    got, _ = _check_clusters(vertices, 0.11, box)
    from perf_amd.mesh import cluster_vertices
    own = cluster_vertices(_dev(vertices, np.float32), 0.11)
    assert torch.equal(own.vertex_cluster, got.vertex_cluster) and torch.equal(own.vertices, got.vertices) and torch.equal(own.representative, got.representative)
    assert ops.meshsimp_bounds(torch.zeros(0, 3, device='cuda')).tolist() == [float('inf')] * 3 + [-float('inf')] * 3


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [float('nan'), float('inf'), -float('inf')])
def test_a_vertex_that_is_not_finite_is_refused(bad):
    from perf_amd._lib import PerfError
    from perf_amd.mesh import Mesh, cluster_vertices, simplify_mesh
    vertices = R.random_vertices(300, 1)
    vertices[150, 0] = vertices[41, 2] = bad
    dev = _dev(vertices, np.float32)
    for call in (lambda: cluster_vertices(dev, 0.3, BOX), lambda: cluster_vertices(dev, 0.3), lambda: simplify_mesh(Mesh(dev, _dev(R.strip(300), np.int32)), 0.3, BOX)):
        with pytest.raises(PerfError, match=r'vertex 41 = \[.*\] has a coordinate that is not finite'):
            call()
    _check_clusters(R.random_vertices(300, 1), 0.3, BOX)          # and the device is as it was: the next call clusters


@pytest.mark.parametrize('bad', ['V', -1])
def test_a_face_index_outside_the_vertices_is_refused(bad):
    from perf_amd._lib import PerfError
    from perf_amd.mesh import Mesh, cluster_faces, cluster_vertices, simplify_mesh
    V = 300
    vertices = _dev(R.random_vertices(V, 2), np.float32)
    faces = np.stack([np.arange(V - 2), np.arange(V - 2) + 1, np.arange(V - 2) + 2], axis=1).astype(np.int32)
    faces[7, 1] = faces[150, 2] = V if bad == 'V' else -1
    match = r'face 7 = \[7, ' + str(V if bad == 'V' else -1) + r', 9\] has an index outside \[0, 300\)'
    with pytest.raises(PerfError, match=match):
        simplify_mesh(Mesh(vertices, _dev(faces, np.int32)), 0.3, BOX)
    with pytest.raises(PerfError, match=match):
        cluster_faces(_dev(faces, np.int32), cluster_vertices(vertices, 0.3, BOX))
    _check_simplify(R.random_vertices(V, 2), R.strip(V), 0.3)


# ---- faces ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['ascending', 'descending', 'permuted'])
@pytest.mark.parametrize('kind', ['fan', 'strip'])
def test_fans_and_strips(kind, order):
    V = 1000
    vertices = R.random_vertices(V, 31)
    perm = {'ascending': np.arange(V), 'descending': np.arange(V)[::-1], 'permuted': np.random.default_rng(3).permutation(V)}[order]
    faces = perm[getattr(R, kind)(V)].astype(np.int32)          # the same shape over renamed vertices
    for dedupe in ('oriented', 'unoriented', None):
        _check_simplify(vertices, faces, 0.25, dedupe=dedupe)


def test_repeated_indices():
    vertices = R.random_vertices(400, 32)
    faces = R.strip(400).copy()
    faces[5] = [9, 9, 9]; faces[6] = [3, 8, 3]; faces[7] = [4, 4, 200]; faces[8] = [300, 2, 2]
    for dedupe in ('oriented', 'unoriented', None):
        _check_simplify(vertices, faces, 0.05, dedupe=dedupe)


@pytest.mark.parametrize('dedupe', ['oriented', 'unoriented', None])
def test_3000_shuffled_triangles_over_500_vertices_in_about_60_cells(dedupe):
    vertices = R.random_vertices(500, 33)
    lo, h, n = R.grid_of(0.5, BOX)
    vc, C, _, _, ties = R.cluster(vertices, lo, h, n)
    assert 48 <= C <= 64 and ties == 0
    faces = np.random.default_rng(34).integers(0, 500, size=(3000, 3)).astype(np.int32)
    r, keep = R.cluster_faces(faces, vc, dedupe)
    assert 0 < keep.sum() < 3000 and (dedupe is None or keep.sum() < R.cluster_faces(faces, vc, None)[1].sum())          # degenerates and duplicates
    clusters, _ = _check_clusters(vertices, 0.5, BOX)
    _check_faces(faces, clusters, vc, dedupe)
    for placement in ('mean', 'member'):
        _check_simplify(vertices, faces, 0.5, placement=placement, dedupe=dedupe)


_BALL = {}


def _ball():
    if not _BALL:
        _BALL['mesh'] = R.ball_mesh(32)
    return _BALL['mesh']


def test_two_coincident_sheets_of_opposite_winding():
    vertices, faces = _ball()
    both = np.concatenate([faces, faces[:, [0, 2, 1]]])
    box = ([-1.0] * 3, [1.0] * 3)
    one, _ = _check_simplify(vertices, faces, 0.125, box)
    oriented, _ = _check_simplify(vertices, both, 0.125, box, dedupe='oriented')
    unoriented, _ = _check_simplify(vertices, both, 0.125, box, dedupe='unoriented')
    assert oriented.faces.shape[0] == 2 * one.faces.shape[0] and 0 < unoriented.faces.shape[0] <= one.faces.shape[0]
    assert torch.equal(unoriented.vertices, one.vertices)


# ---- independence -----------------------------------------------------------------------------------------------------------------------------
def test_the_order_of_the_faces_changes_only_the_order_of_the_faces():
    vertices, faces = _ball()
    box = ([-1.0] * 3, [1.0] * 3)
    mesh, index = _check_simplify(vertices, faces, 0.125, box)
    shuffled, shuffled_index = _check_simplify(vertices, faces[np.random.default_rng(5).permutation(len(faces))], 0.125, box)
    assert torch.equal(shuffled.vertices, mesh.vertices) and torch.equal(shuffled_index, index)
    rows = lambda m: sorted(tuple(min(r[s:] + r[:s] for s in range(3))) for r in m.faces.tolist())
    assert rows(shuffled) == rows(mesh) and not torch.equal(shuffled.faces, mesh.faces)


@pytest.mark.parametrize('placement', ['mean', 'member'])
def test_two_runs_are_bit_identical(placement):
    from perf_amd.mesh import Mesh, simplify_mesh
    vertices, faces = _ball()
    mesh = Mesh(_dev(vertices, np.float32), _dev(faces, np.int32))
    a, ia = simplify_mesh(mesh, 0.125, placement=placement)
    b, ib = simplify_mesh(mesh, 0.125, placement=placement)
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.faces, b.faces) and torch.equal(ia, ib)
    if placement == 'member':
        assert torch.equal(a.vertices.view(torch.int32), mesh.vertices[ia.long()].view(torch.int32))
        mean, im = simplify_mesh(mesh, 0.125)
        assert torch.equal(im, ia) and torch.equal(mean.faces, a.faces) and not torch.equal(mean.vertices, a.vertices)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def _ball_field(res=64):
    from tests import mesh_reference as M
    return M.ball((res,) * 3, (res / 2 + 0.25, res / 2 - 0.125, res / 2 + 0.0625), 0.4 * res)


def test_the_extracted_ball_simplifies_to_the_restatement_and_carries_its_attributes():
    from perf_amd.mesh import Mesh, simplify_mesh, surface_nets
    extracted = surface_nets(torch.from_numpy(_ball_field()).cuda(), 0.0, LO, HI)
    V = extracted.vertices.shape[0]
    g = torch.Generator(device='cuda').manual_seed(1)
    colors = torch.rand(V, 3, device='cuda', generator=g)
    normals = torch.nn.functional.normalize(torch.randn(V, 3, device='cuda', generator=g), dim=1)
    cell = 2 * 2.0 / 64
    lo, h, n = R.grid_of(cell, BOX)
    v, f, k = R.simplify(extracted.vertices.cpu().numpy(), extracted.faces.cpu().numpy(), lo, h, n)
    mesh, index = simplify_mesh(Mesh(extracted.vertices, extracted.faces, colors, normals), cell, BOX)
    assert 0 < len(f) < extracted.faces.shape[0] and 0 < len(v) < V
    assert np.array_equal(_bits(mesh.vertices), v.view(np.int32)) and np.array_equal(mesh.faces.cpu().numpy(), f) and np.array_equal(index.cpu().numpy(), k)
    assert torch.equal(mesh.colors, colors[index.long()]) and torch.equal(mesh.normals, normals[index.long()])
    only_colors, _ = simplify_mesh(Mesh(extracted.vertices, extracted.faces, colors, None), cell, BOX, placement='member')
    assert only_colors.normals is None and torch.equal(only_colors.colors, mesh.colors) and torch.equal(only_colors.vertices, extracted.vertices[index.long()])


def test_the_brick_path_simplifies_to_the_same_mesh():
    """The brick mesher makes the same vertices in another order and the same faces in another order: the same cells, the same means (the
    sums are exact in any order), the same set of faces over them."""
    from perf_amd.mesh import simplify_mesh, surface_nets, surface_nets_bricks
    res = 64
    field = _ball_field(res)
    dense = surface_nets(torch.from_numpy(field).cuda(), 0.0, LO, HI)
    b = res // 8
    values = np.ascontiguousarray(field[:res, :res, :res].reshape(b, 8, b, 8, b, 8).transpose(0, 2, 4, 1, 3, 5)).reshape(b ** 3, 8, 8, 8)
    ids = torch.arange(b ** 3, dtype=torch.int32, device='cuda')
    sparse, _ = surface_nets_bricks(torch.from_numpy(values).cuda(), ids, ids.view(b, b, b).clone(), (res,) * 3, 0.0, -1.0, LO, HI)
    assert sparse.faces.shape == dense.faces.shape and sparse.vertices.shape == dense.vertices.shape
    cell = 2 * 2.0 / 64
    a, _ = simplify_mesh(dense, cell, BOX)
    c, _ = simplify_mesh(sparse, cell, BOX)
    rows = lambda m: sorted(tuple(tuple(_bits(m.vertices)[i].tolist()) for i in r[s:] + r[:s]) for r in m.faces.tolist() for s in range(3))
    assert a.faces.shape == c.faces.shape and sorted(map(tuple, _bits(a.vertices).tolist())) == sorted(map(tuple, _bits(c.vertices).tolist()))
    assert rows(a) == rows(c)
