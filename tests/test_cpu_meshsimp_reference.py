"""tests/meshsimp_reference.py, the yardstick of the GPU tests of the vertex clustering, pinned without a GPU against an independent
formulation -- np.unique on the keys, Python-int sums added with np.add.at, a set of canonical triples, loops over clusters -- and against
the properties a clustered mesh must have."""
import numpy as np
import pytest

from tests import meshsimp_reference as R

LO, HI = (-1.0, -1.25, -0.5), (1.0, 0.75, 1.0)


def _independent(vertices, faces, lo, h, n, placement, dedupe):
    """Clusters by np.unique, sums as Python ints, faces through a set: loops where the restatement has array operations."""
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    V = len(v32)
    cell, q, key = R.cells(v32, lo, h, n)
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)          # first: the smallest member of each key
    ids = np.argsort(np.argsort(first))                       # the rank of each key's smallest member
    vc = ids[inverse] if V else np.zeros(0, dtype=np.int64)
    C = len(uniq)
    S = np.zeros((C, 3), dtype=object)
    np.add.at(S, vc, q.astype(object))
    count = np.zeros(C, dtype=object)
    np.add.at(count, vc, 1)
    lo64, h64 = np.asarray(lo, dtype=np.float32).astype(np.float64), float(np.float32(h))
    placed, rep = np.zeros((C, 3), dtype=np.float32), np.zeros(C, dtype=np.int32)
    for c in range(C):
        members = np.nonzero(vc == c)[0]
        i = cell[members[0]]
        p = np.array([lo64[a] + (float(i[a]) + float(int(S[c, a])) / (float(int(count[c])) * 4294967296.0)) * h64 for a in range(3)])
        best = None
        for v in members:
            d = v32[v].astype(np.float64) - p
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if best is None or d2 < best[0]:
                best = (d2, v)
        rep[c] = best[1]
        placed[c] = p.astype(np.float32) if placement == 'mean' else v32[best[1]]
    seen, kept = set(), []
    for f in np.asarray(faces, dtype=np.int64).reshape(-1, 3):
        t = tuple(int(vc[x]) for x in f)
        if len(set(t)) < 3:
            continue
        if dedupe is not None:
            k = tuple(sorted(t)) if dedupe == 'unoriented' else min(t[s:] + t[:s] for s in range(3))
            if k in seen:
                continue
            seen.add(k)
        kept.append(t)
    kept = np.asarray(kept, dtype=np.int64).reshape(-1, 3)
    used = sorted(set(kept.reshape(-1).tolist()))
    new = {c: k for k, c in enumerate(used)}
    out_faces = np.asarray([[new[c] for c in t] for t in kept], dtype=np.int32).reshape(-1, 3)
    return placed[used].reshape(-1, 3), out_faces, rep[used]


def _agree(vertices, faces, cell, box=(LO, HI)):
    lo, h, n = R.grid_of(cell, box)
    for placement in ('mean', 'member'):
        for dedupe in ('oriented', 'unoriented', None):
            got = R.simplify(vertices, faces, lo, h, n, placement, dedupe)
            want = _independent(vertices, faces, lo, h, n, placement, dedupe)
            assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
            assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (placement, dedupe)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (placement, dedupe)
    return R.simplify(vertices, faces, lo, h, n)


def test_empty_meshes():
    v, f, k = _agree(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0.25)
    assert v.shape == (0, 3) and f.shape == (0, 3) and k.shape == (0,)
    v, f, k = _agree(R.random_vertices(5, 0), np.zeros((0, 3), np.int32), 0.25)
    assert v.shape == (0, 3) and f.shape == (0, 3) and k.shape == (0,)


def test_one_triangle_in_one_cell_leaves_nothing():
    vertices = np.array([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [0.1, 0.2, 0.1]], np.float32)
    v, f, k = _agree(vertices, np.array([[0, 1, 2]], np.int32), 0.5, ((0, 0, 0), (1, 1, 1)))
    assert len(v) == 0 and len(f) == 0 and len(k) == 0


def test_one_triangle_over_three_cells_stays():
    vertices = np.array([[0.1, 0.1, 0.1], [0.7, 0.1, 0.1], [0.1, 0.7, 0.1]], np.float32)
    v, f, k = _agree(vertices, np.array([[2, 0, 1]], np.int32), 0.5, ((0, 0, 0), (1, 1, 1)))
    assert np.array_equal(v, vertices) and f.tolist() == [[2, 0, 1]] and k.tolist() == [0, 1, 2]


@pytest.mark.parametrize('kind', ['fan', 'strip'])
@pytest.mark.parametrize('V', [3, 64, 257])
def test_fans_and_strips(kind, V):
    vertices = R.random_vertices(V, V)
    _agree(vertices, getattr(R, kind)(V), 0.3)
    _agree(vertices, getattr(R, kind)(V)[::-1], 0.6)


def test_the_cell_rule_at_the_edges():
    lo, h, n = np.float32([0, 0, 0]), np.float32(0.25), [4, 4, 4]
    x = np.array([[0, 0.25, 1.0], [-3, 5, 0.999999], [np.nextafter(np.float32(0.25), np.float32(0)), 0.5, 0.75]], np.float32)
    cell, q, key = R.cells(x, lo, h, n)
    assert cell.tolist() == [[0, 1, 3], [0, 3, 3], [0, 2, 3]]
    assert q[0].tolist() == [0, 0, 1 << 32] and q[1, 0] == 0 and q[1, 1] == 1 << 32          # at lo, on a cell face, at hi (t = n, f = 1); clamped from outside
    assert 0 < q[2, 0] < 1 << 32 and q[2, 1] == 0 and q[2, 2] == 0
    assert key[0] == 0 << 42 | 1 << 21 | 3


def test_the_stated_hashes_collide_where_they_are_built_to():
    keys = R.colliding_cells(300, 10)
    assert len(set(keys)) == 300 and all(R.cell_hash(k, 10) == 5 for k in keys)
    _, _, back = R.cells(R.vertices_of_keys(keys), [0, 0, 0], 1.0, [1 << 21] * 3)
    assert back.tolist() == keys
    for dedupe in ('oriented', 'unoriented'):
        t = R.colliding_triples(300, 10, 4096, dedupe)
        assert len({tuple(r) for r in t.tolist()}) == 300 and all(R.face_hash(*r, 10) == 9 for r in t.tolist())
        assert np.array_equal(R.canonical(t, dedupe), t)
    assert [R.table_slots(n) for n in (0, 1, 128, 129, 4096, 4097, 65536)] == [256, 256, 256, 512, 8192, 16384, 131072]


_BALL = {}


def _ball():
    if not _BALL:
        _BALL['mesh'] = R.ball_mesh(32)
    return _BALL['mesh']


def test_the_ball_clustered_at_twice_the_lattice_spacing():
    vertices, faces = _ball()
    cell = 2 * 2.0 / 32
    box = ([-1.0] * 3, [1.0] * 3)
    lo, h, n = R.grid_of(cell, box)
    assert n == [16, 16, 16]
    centre = -1.0 + 2.0 * np.array([16.25, 15.875, 16.0625]) / 32
    off = lambda v: np.abs(np.linalg.norm(v.astype(np.float64) - centre, axis=1) - 0.8)
    v, f, k = _agree(vertices, faces, cell, box)
    assert 0 < len(f) < len(faces) and 0 < len(v) < len(vertices)
    # every 'mean' vertex lies inside the cell of its members (closed: a mean may round onto a face)
    cells_in, _, _ = R.cells(vertices[k], lo, h, n)
    low = lo.astype(np.float64) + cells_in * float(h)
    assert (v >= low.astype(np.float32)).all() and (v <= (low + float(h)).astype(np.float32)).all()
    # a mean lies in the hull of members that share a cell
    assert off(v).max() <= off(vertices).max() + np.sqrt(3.0) * cell
    # every vertex carries a representative of its own cluster (the lattice makes ties here, and means them: the smaller index wins in
    # both formulations)
    vc, C, _, rep, ties = R.cluster(vertices, lo, h, n)
    assert ties > 0 and np.array_equal(vc[rep], np.arange(C)) and set(k.tolist()) <= set(rep.tolist())
    # 'member': every output vertex is an input vertex, to the bit
    vm, fm, km = R.simplify(vertices, faces, lo, h, n, 'member')
    assert np.array_equal(vm.view(np.int32), vertices[km].view(np.int32)) and np.array_equal(fm, f) and np.array_equal(km, k)


def test_unoriented_keeps_one_of_two_coincident_sheets():
    vertices, faces = _ball()
    both = np.concatenate([faces, faces[:, [0, 2, 1]]])          # the same sheet again with the opposite winding
    lo, h, n = R.grid_of(2 * 2.0 / 32, ([-1.0] * 3, [1.0] * 3))
    one = R.simplify(vertices, faces, lo, h, n, dedupe='oriented')
    oriented = R.simplify(vertices, both, lo, h, n, dedupe='oriented')
    unoriented = R.simplify(vertices, both, lo, h, n, dedupe='unoriented')
    assert len(oriented[1]) == 2 * len(one[1]) and np.array_equal(oriented[1][:len(one[1])], one[1])
    assert len(unoriented[1]) <= len(one[1]) and np.array_equal(unoriented[0], one[0])
    sets = lambda f: {tuple(sorted(r)) for r in f.tolist()}
    assert sets(unoriented[1]) == sets(one[1]) and len(sets(unoriented[1])) == len(unoriented[1])


def test_generated_draws_have_no_representative_tie():
    """The condition of the GPU inputs: no two members of a cluster at equal d2 (at least 90 % of each draw remains: all of it here)."""
    for V, seed, cell in ((65537, 11, 0.05), (3000, 12, 0.4)):
        lo, h, n = R.grid_of(cell, (LO, HI))
        assert R.cluster(R.random_vertices(V, seed), lo, h, n)[4] == 0
