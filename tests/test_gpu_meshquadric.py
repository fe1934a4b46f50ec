"""The quadric error placement (include/perf_hip_meshquadric.h, perf_amd/mesh.py) on the GPU.  The yardstick is the numpy restatement
tests/meshquadric_reference.py (pinned against an independent formulation by tests/test_cpu_meshquadric_reference.py): the int64 sums,
the two flags and the placed vertices are compared EXACTLY, floats to the bit.  The labelling, the anchor and the representatives the
kernels read are the restatement's own, so a case fails for this unit's reasons only."""
import numpy as np
import pytest
import torch

from tests import meshquadric_reference as Q
from tests.test_cpu_meshquadric_reference import _local_mesh, _random_mesh, ties_mesh

pytestmark = pytest.mark.gpu

UNIT = (np.zeros(3, np.float32), np.float32(0.125), [8, 8, 8])
ONE = (np.zeros(3, np.float32), np.float32(1.0), [1, 1, 1])


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _run(vertices, faces, grid, lab):
    """The two entry points on the restatement's labelling -> (acc, flags, vertices) as numpy."""
    from perf_amd import ops
    lo, h, n = grid
    vc, C, anchor, rep = lab
    v, f = _dev(vertices, np.float32).view(-1, 3), _dev(faces, np.int32).view(-1, 3)
    acc, flags = ops.meshquadric_sums(v, f, lo, h, n, _dev(vc, np.int32), C)
    out = ops.meshquadric_place(v, lo, h, n, _dev(anchor, np.float32).view(-1, 3), _dev(rep, np.int32), acc)
    assert acc.dtype == torch.int64 and tuple(acc.shape) == (C, 9) and out.dtype == torch.float32 and tuple(out.shape) == (C, 3)
    return acc.cpu().numpy(), flags.cpu().numpy(), out


def _check(vertices, faces, grid):
    """-> (the restatement's outputs, the device's vertices)."""
    want, acc, bad, skipped, info, lab = Q.placement(vertices, faces, *grid)
    got_acc, got_flags, got = _run(vertices, faces, grid, lab)
    assert got_flags.tolist() == [bad, skipped]
    assert np.array_equal(got_acc, acc)
    assert np.array_equal(_bits(got), want.view(np.int32))
    return (want, acc, bad, skipped, info, lab), got


# ---- the edges of a wave and a workgroup ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [0, 1, 63, 64, 65, 255, 256, 257, 1025, 65537])
def test_face_counts_at_the_edges_of_a_wave_and_a_workgroup(F):
    vertices, faces = _local_mesh(max(64, F // 3), max(F, 1), 10 + F)
    (_, acc, bad, skipped, info, _), _ = _check(vertices, faces[:F], UNIT)
    assert (bad, skipped) == (-1, -1) and (F == 0 or acc.any()) and (F < 63 or info['solved'].any())


def test_every_face_in_one_cell():
    """4,097 faces whose 27 x 4,097 terms all land on one 72-byte row."""
    vertices, faces = _random_mesh(500, 4097, 3)
    (_, acc, _, _, info, (vc, C, _, _)), _ = _check(vertices, faces, ONE)
    assert C == 1 and acc.all() and info['solved'].all()


def test_faces_that_cycle_through_three_clusters_lane_by_lane():
    """Face i lies wholly in cluster i % 3: no two neighbouring lanes share a row."""
    rng = np.random.default_rng(5)
    vertices = (rng.random((300, 3)) * 0.125 + np.repeat(np.array([[0, 0, 0], [0.5, 0.25, 0.125], [0.75, 0.75, 0.75]]), 100, axis=0)).astype(np.float32)
    i = np.arange(2000)
    faces = np.stack([rng.integers(0, 100, 2000), rng.integers(0, 100, 2000), rng.integers(0, 100, 2000)], axis=1) + 100 * (i % 3)[:, None]
    (_, acc, _, _, _, (vc, C, _, _)), _ = _check(vertices, faces, UNIT)
    assert C == 3 and acc.all()


def test_corners_in_one_two_and_three_clusters():
    vertices = np.array([[0.01, 0.02, 0.03], [0.10, 0.03, 0.01], [0.03, 0.11, 0.05],           # cell (0, 0, 0)
                         [0.14, 0.02, 0.03], [0.20, 0.10, 0.04],                                 # cell (1, 0, 0)
                         [0.05, 0.30, 0.11]], dtype=np.float32)                                  # cell (0, 2, 0)
    faces = np.array([[0, 1, 2], [0, 1, 3], [3, 0, 4], [0, 3, 5], [5, 4, 2], [2, 1, 0]], dtype=np.int32)
    (_, acc, _, _, info, (vc, C, _, _)), _ = _check(vertices, faces, UNIT)
    assert C == 3 and sorted(len(set(vc[f])) for f in faces) == [1, 1, 2, 2, 3, 3] and info['solved'].all()


def test_faces_without_area_and_with_a_repeated_index():
    vertices, faces = _local_mesh(200, 300, 7)
    vertices[10], vertices[11], vertices[12] = (0.25, 0.25, 0.25), (0.5, 0.5, 0.5), (0.375, 0.375, 0.375)          # collinear, dyadic
    faces[::4] = faces[::4][:, [0, 0, 2]]
    faces[1::16] = faces[1::16][:, [1, 1, 1]]
    faces[2] = (10, 11, 12)
    (_, _, bad, skipped, _, _), _ = _check(vertices, faces, UNIT)
    assert (bad, skipped) == (-1, -1)
    only = np.array([[10, 11, 12], [3, 3, 4], [5, 5, 5]], dtype=np.int32)
    (want, acc, _, _, info, (_, _, anchor, _)), _ = _check(vertices, only, UNIT)
    assert not acc.any() and np.array_equal(want.view(np.int32), anchor.view(np.int32))


def test_a_face_index_outside_the_vertices_is_not_followed():
    vertices, faces = _local_mesh(300, 1000, 8)
    faces[700, 1], faces[41, 2], faces[500, 0] = 300, -1, 1 << 30
    (_, _, bad, _, _, _), _ = _check(vertices, faces, UNIT)
    assert bad == 41


def test_a_vertex_that_is_not_finite_has_no_cluster_and_its_faces_count_nothing():
    vertices, faces = _local_mesh(300, 1000, 9)
    vertices[17, 1], vertices[100, 0], vertices[201] = np.nan, np.inf, (-np.inf, np.nan, 0.0)
    (_, _, bad, skipped, _, (vc, _, _, _)), _ = _check(vertices, faces, UNIT)
    assert (bad, skipped) == (-1, -1) and (vc[[17, 100, 201]] == -1).all() and np.isin(faces, [17, 100, 201]).any()


def test_the_skip_rule_just_below_at_and_far_above_it():
    """A face of 32 x (32 - 2^-10) cells is summed, one of 32 x 32 cells sits on 2^60 and is skipped, as is one that spans 2^12 cells."""
    h = np.float32(1 / 64)
    vertices = np.array([[0, 0, 0], [32 / 64, 0, 0], [0, 32 / 64, 0], [0, (32 - 2.0 ** -10) / 64, 0], [64, 0, 0], [0, 64, 0.25], [0.3, 0.2, 0.1]], dtype=np.float32)
    grid = (np.zeros(3, np.float32), h, [4096, 4096, 32])
    for faces, flag in (([[0, 1, 3]], -1), ([[0, 1, 3], [0, 1, 2]], 1), ([[0, 4, 5], [0, 1, 3], [0, 1, 2]], 0), ([[6, 1, 3], [6, 4, 5]], 1)):
        (_, acc, _, skipped, _, _), _ = _check(vertices, np.array(faces, dtype=np.int32), grid)
        assert skipped == flag and acc.any()
    _, scaled, fits, _ = Q.face_terms(vertices, np.array([[0, 1, 3], [0, 1, 2]], dtype=np.int32), *grid)
    assert fits.tolist() == [True, False] and 2.0 ** 59 < scaled[0, 5] < scaled[1, 5] == 2.0 ** 60


def test_ties_of_both_signs_round_to_even():
    vertices, faces = ties_mesh()
    _, scaled, _, _ = Q.face_terms(vertices, faces, *ONE)
    half = np.abs(scaled - np.trunc(scaled)) == 0.5
    assert (half & (scaled > 0)).any() and (half & (scaled < 0)).any()
    _check(vertices, faces, ONE)
    _check(vertices, faces, (np.zeros(3, np.float32), np.float32(0.5), [2, 2, 2]))          # (the same faces four times as heavy: no ties)


def test_vertices_on_cell_boundaries_and_outside_the_box():
    rng = np.random.default_rng(11)
    on = rng.integers(0, 9, (200, 3)) / 8.0                                  # on the cells' corners, the far border included
    out = rng.random((200, 3)) * 3.0 - 1.0                                   # up to a box width outside: clamped into the border cells
    vertices = np.concatenate([on, out, rng.random((200, 3))]).astype(np.float32)
    _, faces = _random_mesh(600, 3000, 12)
    (_, acc, _, _, info, _), _ = _check(vertices, faces, UNIT)
    assert acc.any() and info['solved'].any()


@pytest.mark.parametrize('grid', [ONE, (np.array([-1.0, 2.0, 0.0], np.float32), np.float32(2.0 ** -21), [1, 1, 1 << 21])], ids=['one cell', '1 x 1 x 2^21'])
def test_a_one_cell_grid_and_a_column_of_2_21_cells(grid):
    rng = np.random.default_rng(13)
    lo, h, n = grid
    vertices = (lo.astype(np.float64) + rng.random((400, 3)) * float(h)).astype(np.float32)
    if n[2] > 1:          # fifty groups along the column, each a few cells long; the two ends on the borders
        vertices[:, 2] = np.sort(np.floor(rng.random(400) * 50) / 50 + rng.random(400) * 4 * float(h))
        vertices[:8, 2], vertices[-8:, 2] = 0.0, 1.0
    base = rng.integers(0, 397, 1500)
    faces = np.stack([base, base + 1, base + 2], axis=1)                     # neighbours along the column: most faces stay in their group
    (_, acc, _, _, info, (_, C, _, _)), _ = _check(vertices, faces, grid)
    assert acc.any() and (C == 1 or C > 50)


def test_clusters_with_no_face_keep_the_anchor():
    vertices, faces = _local_mesh(400, 600, 14)
    faces = faces[(faces < 200).all(axis=1)]                                 # the second half of the sheet has no face
    (want, acc, _, _, info, (vc, C, anchor, _)), got = _check(vertices, faces, UNIT)
    bare = ~acc.any(axis=1)
    assert bare.sum() > 5 and (~info['solved'][bare]).all() and np.array_equal(_bits(got)[bare], anchor.view(np.int32)[bare])


def test_two_planes_that_meet_outside_the_cell_are_clamped():
    """Two sheets of slopes 0.2 and 0.4 in x (cell units) that meet near x = -1, a cell outside: the vertex stops at the cell's wall."""
    a = Q.patch((0.03125, 0.0625, 0.3), (0.0625, 0, 0.0125), (0, 0.0625, 0), 7, 14)
    b = Q.patch((0.53125, 0.0625, 0.7125), (0.0625, 0, 0.025), (0, 0.0625, 0), 7, 14)
    vertices, faces = Q.join([a, b])
    (want, _, _, _, info, (_, C, _, _)), _ = _check(vertices, faces, ONE)
    assert C == 1 and info['solved'].all() and info['clamped'] >= 1 and info['x'][0, 0] < -0.5 and want[0, 0] == 0.0


def test_the_tessellated_box():
    vertices, faces = Q.box_mesh()
    (want, _, _, _, info, _), _ = _check(vertices, faces, Q.BOX_GRID)
    assert info['solved'].all() and info['clamped'] == 0


# ---- order and repetition ---------------------------------------------------------------------------------------------------------------------
def test_bit_identical_under_a_permutation_of_the_faces_and_from_run_to_run():
    vertices, faces = _local_mesh(3000, 20000, 15)
    lab = Q.labelled(vertices, *UNIT)
    acc, flags, out = _run(vertices, faces, UNIT, lab)
    again = _run(vertices, faces, UNIT, lab)
    shuffled = _run(vertices, faces[np.random.default_rng(16).permutation(len(faces))], UNIT, lab)
    for other in (again, shuffled):
        assert np.array_equal(other[0], acc) and np.array_equal(_bits(other[2]), _bits(out))
    assert np.array_equal(acc, Q.sums(vertices, faces, *UNIT, lab[0], lab[1])[0])


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dedupe', ['oriented', 'unoriented', None])
def test_simplify_mesh_quadric_is_the_mean_simplification_with_the_quadric_vertices(dedupe):
    from perf_amd.mesh import Mesh, simplify_mesh
    vertices, faces = Q.box_mesh()
    lo, h, n = Q.BOX_GRID
    box = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    rng = np.random.default_rng(17)
    colors, normals = _dev(rng.random((len(vertices), 3)), np.float32), _dev(rng.normal(size=(len(vertices), 3)), np.float32)
    mesh = Mesh(_dev(vertices, np.float32), _dev(faces, np.int32), colors, normals)
    got, index = simplify_mesh(mesh, 0.125, box, 'quadric', dedupe)
    mean, mean_index = simplify_mesh(mesh, 0.125, box, 'mean', dedupe)
    v, f, k = Q.simplify(vertices, faces, lo, h, n, dedupe)
    assert np.array_equal(_bits(got.vertices), v.view(np.int32)) and np.array_equal(got.faces.cpu().numpy(), f) and np.array_equal(index.cpu().numpy(), k)
    assert torch.equal(got.faces, mean.faces) and torch.equal(index, mean_index) and index.dtype == torch.int32
    assert torch.equal(got.colors, mean.colors) and torch.equal(got.normals, mean.normals) and torch.equal(got.colors, colors[index.long()])
    assert not torch.equal(got.vertices, mean.vertices)
    # The corners of the box are vertices of the simplified mesh within the bound the CPU test derives, lambda / (sigma_min + lambda)
    # |m - x*|: three equal orthogonal planes give sigma_min = tr / 3, and mean and corner share a quarter-cell octant, so the bound
    # is below 3 * 2^-10 * sqrt(3) / 4 < 0.002 cells.  The mean's vertices miss the corners by more than ten times that.
    for corner in Q.box_corners():
        miss = lambda m: float((m.vertices.double() - torch.tensor(corner, device='cuda')).norm(dim=1).min())
        assert miss(got) < 0.002 * 0.125 and miss(mean) > 10 * 0.002 * 0.125


def test_quadric_placement_on_clusters_made_apart():
    from perf_amd.mesh import Mesh, cluster_vertices, quadric_placement
    vertices, faces = _local_mesh(2000, 6000, 18)
    box = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    mesh = Mesh(_dev(vertices, np.float32), _dev(faces, np.int32))
    want, _, _, skipped, _, _ = Q.placement(vertices, faces, *UNIT)
    for placement in ('mean', 'member'):
        clusters = cluster_vertices(mesh.vertices, 0.125, box, placement)
        placed = quadric_placement(mesh, clusters, 0.125, box)
        assert np.array_equal(_bits(placed.vertices), want.view(np.int32))
        assert placed.skipped.dtype == torch.int64 and tuple(placed.skipped.shape) == (1,) and int(placed.skipped) == skipped == -1
