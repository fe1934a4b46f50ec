"""The numpy restatement of surface nets (tests/mesh_reference.py), which the GPU tests compare the kernels against, checked on its own:
a solid ball gives a closed, consistently oriented manifold of the counted size whose volume is the ball's up to the algorithm's
corner-cutting; empty and full fields give nothing."""
import numpy as np
import pytest

from tests import mesh_reference as R

BALLS = [((24, 26, 28), (12.3, 13.6, 14.4), 9.7), ((16, 18, 20), (8.3, 9.6, 10.4), 6.2)]


def test_ball_is_a_closed_oriented_manifold_of_the_balls_volume():
    shape, centre, radius = BALLS[0]
    vertices, faces = R.surface_nets(R.ball(shape, centre, radius), 0.0, [0, 0, 0], shape)        # (world units = lattice units)
    assert vertices.shape == (1770, 3) and faces.shape == (3536, 3)
    assert faces.min() == 0 and faces.max() == 1769
    assert R.is_closed_oriented_manifold(faces) and not R.has_repeated_index(faces)
    ratio = R.signed_volume(vertices, faces) / (4.0 / 3.0 * np.pi * radius ** 3)
    print(f'signed volume / ball volume: {ratio:.4f}')
    assert abs(ratio - 1.0) <= 0.03              # positive: the normals point out of the ball, from high values to low
    assert np.linalg.norm(vertices - np.array(centre), axis=1).max() <= radius + 1e-5          # chords of a convex body: never outside
    assert np.linalg.norm(vertices - np.array(centre), axis=1).min() >= radius - 3 ** 0.5       # and within a cell's diagonal of it


def test_smaller_ball_and_a_box_that_is_not_the_lattice():
    shape, centre, radius = BALLS[1]
    field = R.ball(shape, centre, radius)
    unit, _ = R.surface_nets(field, 0.0, [0, 0, 0], shape)
    lo, hi = np.array([-1.0, 0.5, 2.0]), np.array([3.0, 1.5, 2.5])
    vertices, faces = R.surface_nets(field, 0.0, lo, hi)
    assert np.abs(vertices - (lo + unit * (hi - lo) / np.array(shape))).max() < 1e-12
    assert R.is_closed_oriented_manifold(faces) and not R.has_repeated_index(faces)
    ratio = R.signed_volume(unit, faces) / (4.0 / 3.0 * np.pi * radius ** 3)
    assert 0.95 <= ratio <= 1.0, ratio


def test_a_ball_that_runs_into_the_border_is_closed_when_the_border_is_outside():
    shape = (12, 12, 12)
    field = R.ball(shape, (2.2, 6.1, 9.9), 4.3)
    field[0], field[-1], field[:, 0], field[:, -1], field[:, :, 0], field[:, :, -1] = -1, -1, -1, -1, -1, -1
    vertices, faces = R.surface_nets(field, 0.0, [0, 0, 0], shape)
    assert len(faces) > 0 and R.is_closed_oriented_manifold(faces) and R.signed_volume(vertices, faces) > 0


@pytest.mark.parametrize('value,thr', [(0.0, 0.5), (1.0, 0.5), (0.5, 0.5)])        # empty, full, and equal to thr everywhere: inside, so full
def test_empty_and_full_fields_give_nothing(value, thr):
    vertices, faces = R.surface_nets(np.full((6, 8, 4), value, dtype=np.float32), thr, [0, 0, 0], [1, 1, 1])
    assert vertices.shape == (0, 3) and faces.shape == (0, 3)


def test_special_values_and_the_smallest_lattice():
    field = np.zeros((2, 2, 2), dtype=np.float32)
    field[0, 0, 0] = 1.0
    vertices, faces = R.surface_nets(field, 0.25, [0, 0, 0], [1, 1, 1])
    assert np.allclose(vertices, [[0.25, 0.25, 0.25]]) and faces.shape == (0, 3)         # three crossings at t = 3/4 from the corner: mean of (3/4,0,0) ...
    field[0, 0, 0] = np.inf; field[1, 1, 1] = np.nan
    vertices, _ = R.surface_nets(field, 0.25, [0, 0, 0], [1, 1, 1])
    assert np.allclose(vertices, [[1 / 6, 1 / 6, 1 / 6]])                                 # an infinite end: t is NaN -> 1/2; the NaN corner is outside
