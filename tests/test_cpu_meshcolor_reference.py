"""The numpy restatement of include/perf_hip_meshcolor.h (tests/meshcolor_reference.py) checked on its own, without a GPU: the two caps
that keep the GPU test from passing on vertices nobody saw or on bounds that allow anything, the normal sums' independence of the faces'
order, the orientation of the normals, and the blend's identities.

Measured here on V.make_views(K) with R.make_color_maps(K), R.random_vertices(4096) and R.random_normals(4096), facing with power 2, the
visible bits by the float64 margins at tol 1/256: a view passes for 35.6 % of the vertices at K = 1, 63.2 % at K = 3, 79.1 % at K = 25
and 82.0 % at K = 64; the colour bound's median over the coloured vertices is 1.1e-5 .. 1.6e-5 and it is above 1/255 for none of them
(the caps asserted are >= 30 % at K = 1, >= 60 % at K >= 3, and at most 1 % of the bounds above 1/255)."""
import numpy as np
import pytest

from tests import meshcolor_reference as R
from tests import meshvis_reference as V

N = 4096


@pytest.mark.parametrize('n_views', [1, 3, 25, 64])
def test_the_caps_of_the_gpu_test_hold_on_the_reference(n_views):
    views, maps, vertices = V.make_views(n_views), R.make_color_maps(n_views), R.random_vertices(N)
    visible, _ = V.vertex_bits(vertices, views, V.TOL, V.TOL)
    out = R.blend(vertices, R.random_normals(N), views, maps, visible, facing=True, power=2)
    coloured = out['used'] != 0
    bound = R.color_bound(vertices, views, maps, out['used'])
    print(n_views, 'coloured share', coloured.mean(), 'bound median', np.median(bound[coloured]), 'share above 1/255', (bound[coloured] > 1 / 255).mean())
    assert coloured.mean() >= (0.30 if n_views == 1 else 0.60)
    assert (bound[coloured] > 1 / 255).mean() <= 0.01
    assert np.isfinite(out['colors'][coloured]).all() and (out['colors'][coloured] >= 0.1 - 1e-6).all() and (out['colors'][coloured] <= 0.9 + 1e-6).all()
    assert np.isnan(out['colors'][~coloured]).all() and (out['weight'][~coloured] == 0).all() and (out['weight'][coloured] > 0).all()


def test_normal_sums_do_not_depend_on_the_order_of_the_faces():
    vertices, faces = V.reference_mesh('hollow_sphere')
    s = R.scale_log2(((-1, -1, -1), (1, 1, 1)))
    assert s == 40 - 4          # D^2 = 12
    acc = R.normal_sums(vertices, faces, s)
    assert np.abs(acc).max() < 2 ** 40 * 64 and np.abs(acc).max() > 2 ** 20
    shuffled = faces[np.random.default_rng(1).permutation(len(faces))]
    assert np.array_equal(R.normal_sums(vertices, shuffled, s), acc)
    rolled = np.roll(faces, 1, axis=1)          # (the same faces from another corner: the same normals up to rounding, not to the bit)
    assert np.abs(R.normal_sums(vertices, rolled, s) - acc).max() <= 64
    # faces that contribute nothing: an index outside [0, V), a NaN vertex, a scaled normal of 2^62 and more
    extra = np.concatenate([faces, [[0, 1, len(vertices)], [-1, 0, 1]]]).astype(np.int32)
    assert np.array_equal(R.normal_sums(vertices, extra, s), acc) and R.bad_face(extra, len(vertices)) == len(faces) and R.bad_face(faces, len(vertices)) == -1
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    one = np.array([[0, 1, 2]], dtype=np.int32)
    assert np.array_equal(R.normal_sums(tri, one, 61), np.tile([0, 0, 2 ** 61], (3, 1))) and not R.normal_sums(tri, one, 62).any()
    assert not R.normal_sums(np.array([[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]], dtype=np.float32), one, 0).any()
    assert not R.normal_sums(np.array([[0, 0, 0], [np.inf, 0, 0], [0, 1, 0]], dtype=np.float32), one, 0).any()


def test_inner_skin_normals_point_at_the_centre():
    vertices, faces = V.reference_mesh('hollow_sphere')
    n = R.normals(R.normal_sums(vertices, faces, 36))
    to_centre = np.asarray(V.CENTRE) - vertices.astype(np.float64)
    radius = np.linalg.norm(to_centre, axis=1)
    cos = (n * to_centre).sum(axis=1) / radius
    inner = radius < 0.6          # the skins sit at 0.44 and 0.76
    assert inner.sum() > 100 and (~inner).sum() > 100
    assert (np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-12).all()
    assert (cos[inner] > 0.9).all() and (cos[~inner] < -0.9).all()
    # a vertex no face names, and one whose faces cancel, have the normal 0 exactly
    lone = np.concatenate([vertices, [[0.5, 0.5, 0.5]]]).astype(np.float32)
    assert not R.normals(R.normal_sums(lone, faces, 36))[-1].any()
    both = np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int32)
    assert not R.normals(R.normal_sums(vertices[:3], both, 36)).any()


@pytest.mark.parametrize('copies', [2, 3, 4])
def test_identical_views_blend_to_the_single_sample(copies):
    view, cmap = V.make_views(1)[0], R.make_color_maps(1)[0]
    vertices = R.random_vertices(N)
    visible, _ = V.vertex_bits(vertices, [view], V.TOL, V.TOL)
    single = R.sample(vertices, view, cmap)
    all_bits = visible * np.uint64((1 << copies) - 1)
    out = R.blend(vertices, None, [view] * copies, [cmap] * copies, all_bits, facing=False)
    seen = visible != 0
    assert seen.mean() > 0.3 and np.array_equal(out['used'], all_bits)
    assert np.abs(out['colors'][seen] - single[seen]).max() <= 4 * 2.0 ** -53


def test_a_permutation_of_the_views_maps_best_view_through_it():
    k = 7
    views, maps, vertices, vertex_normals = V.make_views(k), R.make_color_maps(k), R.random_vertices(N), R.random_normals(N)
    visible, _ = V.vertex_bits(vertices, views, V.TOL, V.TOL)
    for facing in (False, True):
        out = R.blend(vertices, vertex_normals, views, maps, visible, facing=facing, power=2, select='best')
        perm = np.random.default_rng(5).permutation(k)          # the new view i is the old view perm[i]
        moved = np.zeros_like(visible)
        for i in range(k):
            moved |= ((visible >> np.uint64(perm[i])) & np.uint64(1)) << np.uint64(i)
        other = R.blend(vertices, vertex_normals, [views[i] for i in perm], [maps[i] for i in perm], moved, facing=facing, power=2, select='best')
        some = out['best_view'] >= 0
        assert some.mean() > (0.3 if facing else 0.6) and np.array_equal(other['best_view'] >= 0, some)
        assert np.array_equal(perm[other['best_view'][some]], out['best_view'][some])
        assert np.array_equal(other['colors'][some], out['colors'][some]) and np.array_equal(other['weight'], out['weight'])
        # the best view has the largest weight, and the smaller index among equals
        assert np.array_equal(out['w'].max(axis=0)[some], out['weight'][some]) and np.array_equal(out['w'].argmax(axis=0)[some], out['best_view'][some])
    blended = R.blend(vertices, vertex_normals, views, maps, visible, facing=True, power=2)
    assert (blended['best_view'] == -1).all() and np.array_equal(blended['used'] & ~visible, np.zeros_like(visible))


def test_power_sharpens_the_weights_towards_the_facing_view():
    views, maps, vertices, vertex_normals = V.make_views(3), R.make_color_maps(3), R.random_vertices(N), R.random_normals(N)
    visible, _ = V.vertex_bits(vertices, views, V.TOL, V.TOL)
    w1 = R.blend(vertices, vertex_normals, views, maps, visible, facing=True, power=1)['w']
    w8 = R.blend(vertices, vertex_normals, views, maps, visible, facing=True, power=8)['w']
    on = w1 > 0
    assert np.array_equal(on, w8 > 0) and (w8[on] <= w1[on] * (1 + 1e-12)).all() and (w8[on] < w1[on]).mean() > 0.99
