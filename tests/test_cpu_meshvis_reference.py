"""tests/meshvis_reference.py -- the float64 restatement of include/perf_hip_meshvis.h that the GPU tests compare against -- pinned without a
GPU: its vertex test agrees with the torch formulation of the reprojection tests (perf_amd/visibility.py) outside the guard; it finds the
stated faces of the hollow sphere and of the shell with a tunnel; its compaction is a direct np.unique compaction; and NO (vertex, view)
pair of the GPU tests' guard-free inputs lies inside the guard, so the exact comparison of tests/test_gpu_meshvis.py leaves out nothing."""
import numpy as np
import pytest
import torch

from tests import mesh_reference as R
from tests import meshcc_reference as CC
from tests import meshvis_reference as V

GUARD_FREE = ((1, 4099), (3, 4099), (64, 4099))          # (K, V) of the GPU tests' guard-free inputs


def _torch_margin(vertices, view):
    from perf_amd.visibility import _lookup_distance
    m = torch.from_numpy(np.asarray(view['distance_map'], dtype=np.float64))[..., None]
    info = {'pose': torch.from_numpy(np.asarray(view['pose'], dtype=np.float64)), 'distance_map': m, 'mask': torch.ones_like(m)}
    dist, proj = _lookup_distance(torch.from_numpy(np.asarray(vertices, dtype=np.float64))[None], info)
    return (dist - proj)[0, :, 0].numpy()


@pytest.mark.parametrize('n_views', [3, 64])
def test_stage_1_agrees_with_the_torch_formulation_outside_the_guard(n_views):
    views = V.make_views(n_views)
    vertices = np.random.default_rng(7).uniform(-1.5, 1.5, size=(3000, 3)).astype(np.float32)
    decided = 0
    for view in views:
        want, got, g = _torch_margin(vertices, view), V.margins(vertices, view), V.guard(view, vertices)
        for eps in (V.TOL, -V.FREE_TOL, 0.0):
            outside = np.abs(got - eps) > g
            assert np.array_equal((got < eps)[outside], (want < eps)[outside])
            decided += int(outside.sum())
        assert np.abs(got - want)[np.isfinite(g) & (g < 1e-3)].max() < 1e-9          # (float64 against float64: the same real-number formulas)
    assert decided >= 0.97 * 3 * 3000 * n_views


def test_the_guard_is_small_away_from_the_poles_and_infinite_at_a_centre():
    view = V.make_views(3)[1]                                # 33 x 64 with a zeroed patch
    pose = np.asarray(view['pose'], dtype=np.float64)
    equator = (pose[:3, :3] @ np.array([0.6, 0.3, 0.05]) + pose[:3, 3])[None]
    pole = (pose[:3, :3] @ np.array([0.0, 0.0, 0.6]) + pose[:3, 3])[None]
    assert V.guard(view, equator)[0] < 1e-3                  # (about a hundredth of a pixel's worth of the zeroed patch's edge)
    assert V.guard(view, pole)[0] > V.guard(view, equator)[0] * 10
    assert np.isinf(V.guard(view, pose[:3, 3][None].astype(np.float32))[0])


@pytest.mark.parametrize('n_views,n', GUARD_FREE)
def test_no_pair_of_the_gpu_inputs_lies_inside_the_guard(n_views, n):
    views = V.make_views(n_views)
    vertices = V.guard_free_vertices(n_views, n)             # (asserts that at least 90 % of its draw remained)
    assert vertices.shape == (n, 3) and vertices.dtype == np.float32
    for view in views:
        mg, g = V.margins(vertices, view), V.guard(view, vertices)
        assert np.isfinite(g).all() and (np.abs(mg - V.TOL) > g).all() and (np.abs(mg + V.FREE_TOL) > g).all()
    visible, free = V.vertex_bits(vertices, views, V.TOL, V.FREE_TOL)
    for bits in (visible, free):                             # both outcomes occur, and no bit at or above K is set
        assert bits.any() and (n_views == 64 or not (bits >> np.uint64(n_views)).any())
        assert (V._popcount(bits) < n_views).any()
    assert not (free & ~visible).any()                       # free implies visible: -free_tol < tol


def test_hollow_sphere():
    vertices, faces = V.reference_mesh('hollow_sphere')
    view = V.constant_view()
    new_vertices, new_faces, index, keep = V.cull(vertices, faces, [view])
    assert (len(new_faces), len(new_vertices)) == (768, 386)
    # exactly the inner skin: the component with the negative signed volume
    vc, C = CC.components(faces, len(vertices))
    per_faces, _, volume = CC.stats(faces, vc, C, vertices)
    assert C == 2 and sorted(per_faces.tolist()) == [768, 2196]
    inner = CC.filter_mesh(vertices, faces, vc, volume < 0)
    assert np.array_equal(inner[0], new_vertices) and np.array_equal(inner[1], new_faces) and np.array_equal(inner[2], index)
    assert np.abs(V.margins(vertices, view) - V.TOL).min() > 0.045


def test_tunnel_field_is_one_component_the_cull_splits():
    vertices, faces = V.reference_mesh('tunnel')
    vc, C = CC.components(faces, len(vertices))
    assert C == 1 and len(faces) == 3000 and abs(R.signed_volume(vertices, faces) - 1.43) < 0.01
    assert not CC.select(np.array([3000]), np.array([R.signed_volume(vertices, faces)]), orientation='inward').any()          # what clean_mesh keeps: nothing
    view = V.constant_view()
    new_vertices, new_faces, index, keep = V.cull(vertices, faces, [view])
    assert (len(new_faces), len(new_vertices)) == (774, 394)
    assert np.abs(V.margins(vertices, view) - V.TOL).min() > 0.045          # no vertex near the decision
    assert CC.components(new_faces, len(new_vertices))[1] == 1
    # the smallest facing determinant among the depth-visible faces
    visible, free = V.vertex_bits(vertices, [view], V.TOL, V.TOL)
    seen = (visible[faces] != 0).all(axis=1)
    v = vertices.astype(np.float64)
    a, b, c = (v[faces[seen][:, i]] for i in range(3))
    s = np.einsum('ij,ij->i', np.cross(b - a, c - a), np.asarray(V.CENTRE, dtype=np.float32).astype(np.float64) - a)
    assert np.abs(s).min() > 6e-5


@pytest.mark.parametrize('centre', [(0.02, 0.02, 0.02), (0.25, -0.1, 0.15)])
def test_facing_alone_selects_the_inner_skin(centre):
    vertices, faces = V.reference_mesh('hollow_sphere')
    view = V.constant_view(centre, 2.0)                      # every vertex passes the depth test
    visible, free = V.vertex_bits(vertices, [view], V.TOL, V.TOL)
    assert (visible == 1).all()
    keep = V.face_keep(faces, vertices, visible, free, [centre], facing=True)
    vc, C = CC.components(faces, len(vertices))
    _, _, volume = CC.stats(faces, vc, C, vertices)
    assert keep.sum() == 768 and np.array_equal(keep.astype(bool), (volume < 0)[vc[faces[:, 0]]])
    assert V.face_keep(faces, vertices, visible, free, [centre], facing=False).all()


def test_face_rule_counts_views_and_carves():
    vertices = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 1], [1, 1, 2], [0, 1, 3]], dtype=np.int32)
    centres = np.array([[0.2, 0.2, 1.0], [0.2, 0.2, -1.0], [0.2, 0.2, 2.0]], dtype=np.float32)
    visible = np.array([0b111, 0b111, 0b111, 0b101], dtype=np.uint64)
    free = np.array([0, 0b010, 0, 0], dtype=np.uint64)
    assert V.face_keep(faces, vertices, visible, free, centres, facing=False).tolist() == [1, 1, 1, 1]
    assert V.face_keep(faces, vertices, visible, free, centres, facing=False, min_views=3).tolist() == [1, 1, 1, 0]
    assert V.face_keep(faces, vertices, visible, free, centres, facing=True).tolist() == [1, 1, 0, 0]          # the degenerate face faces nobody, the last one looks away
    assert V.face_keep(faces, vertices, visible, free, centres, facing=True, min_views=2).tolist() == [1, 0, 0, 0]
    assert V.face_keep(faces, vertices, visible, free, centres, facing=False, carve=True).tolist() == [0, 0, 0, 0]
    assert V.face_keep(faces, vertices, visible, free, centres[:1], facing=False, carve=True).tolist() == [1, 1, 1, 1]          # bits at or above K do not count


@pytest.mark.parametrize('n_faces', [0, 1, 257, 3000])
def test_stage_3_is_a_unique_based_compaction(n_faces):
    rng = np.random.default_rng(n_faces)
    n_vertices = 2 * n_faces + 5
    faces = rng.integers(0, n_vertices, size=(n_faces, 3)).astype(np.int32)
    vertices = rng.normal(size=(n_vertices, 3)).astype(np.float32)
    for keep in (np.zeros(n_faces, bool), np.ones(n_faces, bool), np.arange(n_faces) % 2 == 0, rng.random(n_faces) < 0.5):
        new_vertices, new_faces, index = V.filter_faces(vertices, faces, keep)
        want_index, inverse = np.unique(faces[keep], return_inverse=True)
        assert np.array_equal(index, want_index) and np.array_equal(new_faces, inverse.reshape(-1, 3)) and np.array_equal(new_vertices, vertices[want_index])
        assert index.dtype == np.int32 and new_faces.dtype == np.int32
