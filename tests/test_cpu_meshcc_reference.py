"""tests/meshcc_reference.py -- the numpy restatement of include/perf_hip_meshcc.h that the GPU tests compare against -- pinned without a
GPU: on every case the GPU tests use it agrees with scipy.sparse.csgraph.connected_components after re-ranking scipy's labels by smallest
vertex; its counts, selection and compaction are checked on meshes small enough to do by hand; and the two synthetic fields of the GPU
tests have the components the GPU tests expect of them."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import mesh_reference as R
from tests import meshcc_reference as CC


def _scipy_labels(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(V, V))
    C, labels = connected_components(graph, directed=False)
    if V == 0:
        return np.zeros(0, dtype=np.int32), 0
    first = np.full(C, V, dtype=np.int64)
    np.minimum.at(first, labels, np.arange(V))               # the smallest vertex of each of scipy's components
    rank = np.empty(C, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(C)
    return rank[labels].astype(np.int32), int(C)


@pytest.mark.parametrize('name', sorted(CC.cases()))
def test_agrees_with_scipy(name):
    faces, V = CC.cases()[name]
    vc, C, per_faces, per_vertices = CC.expected(name)
    labels, count = _scipy_labels(faces, V)
    assert C == count and np.array_equal(vc, labels)
    assert vc.dtype == np.int32 and per_faces.dtype == np.int64 and per_vertices.dtype == np.int32
    assert per_faces.sum() == len(faces) and per_vertices.sum() == V and (per_vertices >= 1).all()
    if V:                                                    # ids by smallest vertex: the first vertex of component c comes after that of c - 1
        first = np.array([np.nonzero(vc == c)[0][0] for c in range(min(C, 50))])
        assert (np.diff(first) > 0).all() and vc[0] == 0


def test_cases_are_what_their_names_say():
    x = CC.expected
    assert x('empty')[1] == 0 and x('five_loose_vertices')[1] == 5 and list(x('five_loose_vertices')[2]) == [0] * 5
    assert x('one_triangle')[1] == 1 and x('two_triangles_one_shared_vertex')[1] == 1
    assert list(x('two_triangles_disjoint')[0]) == [0, 1, 0, 1, 0, 1, 2] and list(x('two_triangles_disjoint')[2]) == [1, 1, 0]
    assert list(x('repeated_index')[0]) == [0, 0, 1, 1, 2, 3, 3, 3, 4] and list(x('repeated_index')[2]) == [1, 1, 1, 1, 0]
    for V in CC.EDGE_SIZES:
        assert x(f'fan_{V}')[1] == 1 and x(f'strip_{V}')[1] == 1 and x(f'fan_{V}')[2][0] == V - 2
    for order in ('ascending', 'descending', 'permuted'):
        assert x('quad_strip_' + order)[1] == 1 and x('quad_strip_' + order)[2][0] == 2 * 4097
    assert sorted(x('hub')[2])[-1] == 5000 and x('hub')[1] == 1
    assert x('disjoint_triangles')[1] == 3000 and set(x('disjoint_triangles')[3]) == {3}
    sizes = [int(x(n)[3].max()) for n in ('random_quarter', 'random_half', 'random_full')]
    assert sizes[0] < sizes[1] < sizes[2] < 20000            # a giant component that grows with F, beside many small ones:
    for n in ('random_quarter', 'random_half', 'random_full'):
        assert x(n)[1] > 500 and len(set(x(n)[3])) >= 3      # sizes from 1 (a vertex in no face) to the giant one


def test_selection_and_compaction_by_hand():
    faces = np.array([[4, 5, 6], [0, 1, 2], [6, 5, 7], [1, 2, 0], [8, 9, 10], [2, 1, 0]], dtype=np.int32)
    vc, C = CC.components(faces, 12)
    assert list(vc) == [0, 0, 0, 1, 2, 2, 2, 2, 3, 3, 3, 4] and C == 5
    per_faces, per_vertices, _ = CC.stats(faces, vc, C)
    assert list(per_faces) == [3, 0, 2, 1, 0] and list(per_vertices) == [3, 1, 4, 3, 1]
    assert list(CC.select(per_faces, min_faces=1)) == [True, False, True, True, False]
    assert list(CC.select(per_faces, keep_largest=2)) == [True, False, True, False, False]
    assert list(CC.select(per_faces, keep_largest=4)) == [True, True, True, True, False]          # the tie at 0 faces: the lower id
    assert list(CC.select(per_faces, [1.0, 0.0, -1.0, 2.0, 0.0], orientation='inward')) == [False, False, True, False, False]
    assert list(CC.select(per_faces, [1.0, 0.0, -1.0, 2.0, 0.0], min_faces=2, orientation='outward')) == [True, False, False, False, False]
    vertices = np.arange(36, dtype=np.float32).reshape(12, 3)
    v, f, index = CC.filter_mesh(vertices, faces, vc, np.array([False, True, True, False, False]))
    assert list(index) == [3, 4, 5, 6, 7] and np.array_equal(v, vertices[index])
    assert f.tolist() == [[1, 2, 3], [3, 2, 4]]


def test_signed_volume_of_a_tetrahedron():
    vertices = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32) + np.float32(0.25)
    outward = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)
    _, _, volume = CC.stats(outward, np.zeros(4, np.int32), 1, vertices)
    assert abs(volume[0] - 1.0 / 6.0) < 1e-15
    _, _, volume = CC.stats(outward[:, ::-1], np.zeros(4, np.int32), 1, vertices)
    assert abs(volume[0] + 1.0 / 6.0) < 1e-15


def test_the_balls_field_has_the_stated_components():
    vertices, faces = R.surface_nets(CC.balls_field(), 0.0, [0, 0, 0], CC.SHAPE)
    assert len(vertices) == 1376 and len(faces) == 2728
    vc, C = CC.components(faces, len(vertices))
    per_faces, per_vertices, volume = CC.stats(faces, vc, C, vertices.astype(np.float32))
    assert C == 6 and tuple(per_faces) == CC.BALLS_FACES and tuple(per_vertices) == CC.BALLS_VERTICES
    assert (volume > 0).all()                                # closed, normals from high density to low: outward
    for c in range(C):
        assert R.is_closed_oriented_manifold(CC.filter_mesh(vertices, faces, vc, np.arange(C) == c)[1])
    assert list(np.nonzero(CC.select(per_faces, keep_largest=3))[0]) == [0, 1, 3]          # 3 and 4 tie at 444 faces
    # compaction keeps order and surface nets ranks cells linearly: dropping the speck is meshing the field without it
    v, f, _ = CC.filter_mesh(vertices, faces, vc, CC.select(per_faces, min_faces=100))
    v2, f2 = R.surface_nets(CC.balls_field(speck=False), 0.0, [0, 0, 0], CC.SHAPE)
    assert np.array_equal(v, v2) and np.array_equal(f, f2)


def test_the_hollow_sphere_has_two_skins():
    vertices, faces = R.surface_nets(CC.hollow_sphere(), 0.0, CC.SPHERE_LO, CC.SPHERE_HI)
    vc, C = CC.components(faces, len(vertices))
    per_faces, _, volume = CC.stats(faces, vc, C, vertices.astype(np.float32))
    assert C == 2 and sorted(per_faces) == [768, 2196]
    outer, inner = int(np.argmax(per_faces)), int(np.argmin(per_faces))
    assert abs(volume[outer] - 1.80) < 0.01 and abs(volume[inner] + 0.34) < 0.01
    assert list(CC.select(per_faces, volume, orientation='inward')) == [c == inner for c in range(2)]
    assert list(CC.select(per_faces, volume, orientation='outward')) == [c == outer for c in range(2)]
