"""The float64 restatement of include/perf_hip_meshray.h (tests/meshray_reference.py) pinned without a GPU: on rays against one dyadic
triangle whose answers are computed by hand (every operation is exact there), and on the cull's fixtures, where the segment test against
the mesh itself separates the two skins of the hollow sphere and opens the shell with a tunnel."""
import numpy as np
import pytest

from tests import meshcc_reference as CC
from tests import meshray_reference as M
from tests import meshvis_reference as V


@pytest.mark.parametrize('case', range(len(M.HAND_RAYS)))
def test_hand_computed_rays(case):
    (o, d, t_min, t_max), want = M.HAND_RAYS[case]
    vertices, faces = M.TRIANGLE
    t, face, u, v = (a[0] for a in M.cast(vertices, faces, [o], [d], t_min, t_max))
    assert (float(t), int(face), float(u), float(v)) == tuple(want), (o, d)
    assert int(M.any_hit(vertices, faces, [o], [d], t_min, t_max)[0]) == (want[1] >= 0)


def test_the_inclusive_bounds_are_decided_exactly():
    vertices, faces = M.TRIANGLE
    step = 2.0 ** -20                       # the smallest step fp32 resolves at these coordinates and beyond the rule's rounding there
    for o, inside in (((2, 0, 0), True), ((2, -step, 0), False), ((2 + step, 2, 0), False), ((2 - step, 2, 0), True), ((-step, 1, 0), False), ((0, 1, 0), True)):
        assert (M.cast(vertices, faces, [o], [(0, 0, 1)])[1][0] >= 0) == inside, o


def test_the_closest_hit_is_the_lexicographic_minimum_of_t_and_face():
    # two coincident triangles and a nearer one listed last; a face with a NaN vertex and one with an index outside [0, V) are never hit
    vertices = np.array([[0, 0, 2], [4, 0, 2], [0, 4, 2], [0, 0, 1], [4, 0, 1], [0, 4, 1], [np.nan, 0, 0.5]], dtype=np.float32)
    faces = np.array([[0, 1, 6], [0, 1, 9], [2, 1, 0], [0, 1, 2], [3, 4, 5]], dtype=np.int32)
    o, d = [(1, 1, 0)], [(0, 0, 1)]
    assert [a[0] for a in M.cast(vertices, faces, o, d)[:2]] == [1.0, 4]
    assert [a[0] for a in M.cast(vertices, faces, o, d, 1.5, 8.0)[:2]] == [2.0, 2]              # equal t: the smaller face index
    assert M.valid_faces(vertices, faces).tolist() == [False, False, True, True, True]
    assert M.cell_lists(vertices, faces, (0, 0, 0), 8.0, (1, 1, 1)) == ({0: {2, 3, 4}}, 0)


def test_the_segment_test_is_strict_and_skips_the_incident_faces():
    vertices = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1], [1, 1, 0], [1, 1, 1], [1, 1, 3]], dtype=np.float32)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    ones = np.ones(len(vertices), dtype=np.int64)
    # from below the triangle: a centre beyond it is hidden (t = 1/2), one on it is not (t = 1, strict), one before it is not (t = 2)
    for centre, hidden in (((1, 1, 2), True), ((1, 1, 1), False), ((1, 1, 0.5), False)):
        bits = M.occluded(vertices, faces, [centre], ones)
        assert bits[3] == int(hidden), centre
    # vertex 4 lies ON the triangle: t = 0 is no hit; vertices 0 .. 2 are the triangle's own: it is not tested for them
    bits = M.occluded(vertices, faces, [(1, 1, -1), (1, 1, 2)], 3 * ones)
    assert bits.tolist() == [0, 0, 0, 2, 0, 1]
    assert M.occluded(vertices, faces, [(1, 1, -1), (1, 1, 2)], np.array([0, 0, 0, 1, 0, 2])).tolist() == [0] * 6          # a subset of the mask


def test_the_cell_lists_follow_the_margin():
    vertices, faces = M.TRIANGLE                             # x, y in [0, 4], z = 1; cell 1, margin 1/8
    lists, bad = M.cell_lists(vertices, faces, (0, 0, 0), 1.0, (5, 3, 2))
    assert bad == -1 and set(lists) == {(i * 3 + j) * 2 + k for i in range(5) for j in range(3) for k in range(2)}          # z = 1 lies in the boundary plane: both sides
    lists, _ = M.cell_lists(vertices, faces, (0, 0, 0.25), 1.0, (5, 3, 2))
    assert {c % 2 for c in lists} == {0}                     # z - 0.25 = 0.75: the margin reaches 0.875 and no further
    assert M.cell_lists(vertices, faces, (8, 8, 8), 1.0, (2, 2, 2)) == ({}, -1)          # wholly outside the box


def test_the_occlusion_separates_the_skins_of_the_hollow_sphere():
    vertices, faces = V.reference_mesh('hollow_sphere')
    assert (len(vertices), len(faces)) == (1486, 2964)
    occluded, keep = M.skin_occlusion('hollow_sphere', M.VIEW)
    assert int(occluded.sum()) == 1100 and int(keep.sum()) == 768
    # the unoccluded faces are the inward component: the inner skin
    vc, n = CC.components(faces, len(vertices))
    _, _, volume = CC.stats(faces, vc, n, vertices)
    inner = int(np.argmin(volume))
    assert volume[inner] < 0 and np.array_equal(keep, vc[faces[:, 0]] == inner)
    assert int((vc == inner).sum()) == 386 and not occluded[vc == inner].any() and occluded[vc != inner].all()


def test_the_rule_is_not_watertight_along_shared_edges():
    # from the centre of the box one segment in 1,100 runs through an edge of the inner skin and is outside both of its faces; from the
    # centre of the shell (which fp32 does not hold exactly) four do
    assert int(M.skin_occlusion('hollow_sphere', (0.0, 0.0, 0.0))[0].sum()) == 1099
    assert int(M.skin_occlusion('hollow_sphere', V.CENTRE)[0].sum()) == 1096
    assert int(M.skin_occlusion('hollow_sphere', (0.0, 0.0, 0.0))[1].sum()) == 768          # (the leaked vertex's faces have occluded vertices still)


def test_the_occlusion_opens_the_shell_with_a_tunnel():
    vertices, faces = V.reference_mesh('tunnel')
    assert len(faces) == 3000
    occluded, keep = M.skin_occlusion('tunnel', M.VIEW)
    assert int(keep.sum()) == 802 and int(occluded.sum()) == 1093
