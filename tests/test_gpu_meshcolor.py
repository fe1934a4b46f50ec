"""The colouring from the registered panoramas and the vertex normals from faces (include/perf_hip_meshcolor.h, perf_amd/mesh.py) on the
GPU, against the float64 restatement tests/meshcolor_reference.py.  The normal sums are compared to the bit; the unit normals to one fp32
ulp (double sqrt and division followed by one rounding can differ only at a rounding tie).  The blend is given the DEVICE'S OWN visible
bits (vertex_visibility), so it is compared where it is continuous: colours within the derived bound of R.color_bound (the largest
V.guard of the used views' channels + 2^-18 + 2^-24), weights within 2^-17 relative, the used bits exactly.  tests/
test_cpu_meshcolor_reference.py asserts on the same inputs that enough vertices are coloured and that the bound is small."""
import numpy as np
import pytest
import torch

from tests import meshcolor_reference as R
from tests import meshvis_reference as V

pytestmark = pytest.mark.gpu

BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def _device_views(views, maps):
    return [{'pose': torch.from_numpy(np.array(v['pose'])), 'distance_map': torch.from_numpy(np.array(v['distance_map'])).cuda(),
             'color_map': torch.from_numpy(np.array(m)).cuda()} for v, m in zip(views, maps)]


def _words(t):
    return t.cpu().numpy().view(np.uint64)


def _mesh(vertices, faces):
    from perf_amd.mesh import Mesh
    return Mesh(torch.from_numpy(np.array(vertices, dtype=np.float32, order='C')).cuda().reshape(-1, 3).contiguous(),
                torch.from_numpy(np.array(faces, dtype=np.int32, order='C')).cuda().reshape(-1, 3).contiguous())


# ---- stage A: the normals -----------------------------------------------------------------------------------------------------------------
def _normal_cases():
    out = {'empty': (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
           'no_faces': (R.random_vertices(5), np.zeros((0, 3), np.int32)),
           'one_triangle': (np.array([[0, 0, 0], [0.5, 0.1, 0], [0.1, 0.7, 0.2]], np.float32), np.array([[0, 1, 2]], np.int32)),
           'degenerate_triangle': (np.array([[0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1], [0.3, 0.2, 0.1]], np.float32), np.array([[0, 1, 2], [3, 3, 0], [1, 1, 1]], np.int32)),
           'nan_and_infinite_vertices': (np.array([[0, 0, 0], [0.5, 0.1, 0], [0.1, 0.7, 0.2], [np.nan, 0, 0], [0, -np.inf, 0], [0.3, 0.3, 0.9]], np.float32),
                                         np.array([[0, 1, 2], [0, 1, 3], [4, 1, 2], [2, 1, 5], [3, 4, 5]], np.int32)),
           'unnamed_vertex': (R.random_vertices(7), np.array([[0, 1, 2], [2, 1, 4], [6, 5, 4]], np.int32)),
           'cancelling_faces': (R.random_vertices(4), np.array([[0, 1, 2], [0, 2, 1], [3, 1, 2]], np.int32)),
           'hub_5000': R.fan(5002),
           'hollow_sphere': V.reference_mesh('hollow_sphere'), 'tunnel': V.reference_mesh('tunnel')}
    for n in (63, 64, 65, 255, 256, 257, 65537):
        out[f'fan_{n}'] = R.fan(n)
        out[f'strip_{n}'] = R.strip(n)
    return out


NORMAL_CASES = _normal_cases()


@pytest.mark.parametrize('name', sorted(NORMAL_CASES))
def test_normal_sums_equal_the_restatement_to_the_bit(name):
    from perf_amd import ops
    from perf_amd.mesh import face_normals
    vertices, faces = NORMAL_CASES[name]
    mesh = _mesh(vertices, faces)
    s = R.scale_log2(BOX)
    want = R.normal_sums(vertices, faces, s)
    acc, flag = ops.meshcolor_normal_sums(mesh.vertices, mesh.faces, s)
    again, _ = ops.meshcolor_normal_sums(mesh.vertices, mesh.faces, s)
    shuffled = mesh.faces[torch.from_numpy(np.random.default_rng(3).permutation(len(faces))).cuda()].contiguous() if len(faces) else mesh.faces
    moved, _ = ops.meshcolor_normal_sums(mesh.vertices, shuffled, s)
    assert int(flag.item()) == -1 and acc.dtype == torch.int64 and tuple(acc.shape) == (len(vertices), 3)
    assert np.array_equal(acc.cpu().numpy(), want)
    assert torch.equal(acc, again) and torch.equal(acc, moved)          # from run to run, and under a shuffle of the faces
    if name == 'hub_5000':
        assert (mesh.faces == 0).any(dim=1).sum().item() == 5000
    if name in ('degenerate_triangle', 'no_faces'):
        assert not want.any()
    if name == 'cancelling_faces':
        assert not want[0].any() and want[1:].all()
    if name == 'nan_and_infinite_vertices':
        assert not want[3:5].any() and want[5].any() and np.array_equal(want, R.normal_sums(vertices, faces[[0, 3]], s))
    # the unit normals: one fp32 ulp, and exactly 0 where the restatement's are
    want_n = R.normals(want)
    got = ops.meshcolor_normals(acc).cpu().numpy()
    nearest = want_n.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want_n.shape and np.isfinite(got).all()
    assert (np.abs(got.astype(np.float64) - nearest) <= np.spacing(np.abs(nearest))).all()
    zero = ~want_n.any(axis=1)
    assert not got[zero].any() and np.array_equal(got.any(axis=1), ~zero)
    assert np.array_equal(face_normals(mesh, BOX).cpu().numpy(), got)
    if name in ('unnamed_vertex', 'no_faces', 'cancelling_faces'):
        assert zero.any()
    if name in ('hollow_sphere', 'one_triangle'):          # box None: the vertices' own bounds set the scale; the normals agree to rounding
        own = face_normals(mesh).cpu().numpy()
        assert np.abs(own - got).max() < 1e-5


@pytest.mark.parametrize('bad_index', [-1, 'V'])
def test_a_face_index_outside_the_vertices_is_named_and_not_followed(bad_index):
    from perf_amd import _lib, ops
    from perf_amd.mesh import face_normals
    vertices, faces = V.reference_mesh('hollow_sphere')
    bad = np.array(faces)
    first, second = 1234, 2500
    bad[first, 1] = len(vertices) if bad_index == 'V' else -1
    bad[second, 2] = len(vertices) if bad_index == 'V' else -1
    mesh = _mesh(vertices, bad)
    acc, flag = ops.meshcolor_normal_sums(mesh.vertices, mesh.faces, 36)
    assert int(flag.item()) == first
    assert np.array_equal(acc.cpu().numpy(), R.normal_sums(vertices, np.delete(bad, [first, second], axis=0), 36))
    with pytest.raises(_lib.PerfError, match=f'face_normals: face {first} = .* has an index outside'):
        face_normals(mesh, BOX)


# ---- stage B: the blend -------------------------------------------------------------------------------------------------------------------
def _blend_vertices(n, views):
    """n vertices of R.random_vertices, the first ones replaced by the degenerate ones (NaN, infinite, centres, poles, seam)."""
    p = np.array(R.random_vertices(max(n, 1), seed=n)[:n])
    special = V.special_vertices(views)[:max(n // 2, min(n, 1))] if views else np.zeros((0, 3), np.float32)
    p[:len(special)] = special[:n]
    return p


def _blend_normals(n):
    """unit normals, with a zero, a NaN and an infinite row among them."""
    g = np.array(R.random_normals(max(n, 1), seed=n)[:n])
    for row, value in ((3, 0.0), (5, np.nan), (6, np.inf)):
        if n > 40 + row:
            g[40 + row] = value
    return g


def _check_blend(n_views, n, facing, power, select, with_fallback):
    from perf_amd.mesh import panorama_colors, vertex_visibility
    views, maps = V.make_views(n_views), R.make_color_maps(n_views)
    dev = _device_views(views, maps)
    p, normals = _blend_vertices(n, views), _blend_normals(n)
    vertices = torch.from_numpy(p).cuda().reshape(-1, 3)
    fallback = torch.from_numpy(np.random.default_rng(n).uniform(0, 1, size=(n, 3)).astype(np.float32)).cuda().reshape(-1, 3) if with_fallback else None
    fill = (0.125, 0.25, 0.75)
    kw = dict(normals=torch.from_numpy(normals).cuda().reshape(-1, 3) if facing else None, tol=V.TOL, facing=facing, power=power, select=select, fallback=fallback, fill=fill)
    out = panorama_colors(vertices, dev, **kw)
    again = panorama_colors(vertices, dev, **kw)
    assert out.colors.dtype == out.weight.dtype == torch.float32 and out.used.dtype == torch.int64 and out.best_view.dtype == torch.int8
    assert tuple(out.colors.shape) == (n, 3) and tuple(out.weight.shape) == tuple(out.used.shape) == tuple(out.best_view.shape) == (n,)
    for a, b in zip(out, again):          # bit-identical from run to run
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    visible = _words(vertex_visibility(vertices, dev, tol=V.TOL).visible)
    colors, weight, used, best = out.colors.cpu().numpy(), out.weight.cpu().numpy(), _words(out.used), out.best_view.cpu().numpy()
    want = R.blend(p, normals, views, maps, visible, facing=facing, power=power, select=select)
    # the used bits
    assert not (used & ~visible).any()
    assert np.array_equal(used, want['used'])
    if not facing:
        at_centre = np.zeros(n, dtype=np.uint64)
        for k, view in enumerate(views):
            at_centre |= (V.lookup(p, view)['dist'] == 0).astype(np.uint64) << np.uint64(k)
        assert np.array_equal(used, visible & ~at_centre)
    some = used != 0
    # every output is finite, whatever the vertex
    assert np.isfinite(colors).all() and np.isfinite(weight).all()
    # the fallback rows and the fill, to the bit
    assert (weight[~some] == 0).all() and (weight[some] > 0).all()
    rest = fallback.cpu().numpy()[~some] if with_fallback else np.tile(np.array(fill, dtype=np.float32), ((~some).sum(), 1))
    assert np.array_equal(colors[~some], rest)
    if n_views == 0:
        assert not some.any()
    # the weights and the colours
    if select == 'blend':
        assert (best == -1).all()
        assert (np.abs(weight[some] - want['weight'][some]) <= 2.0 ** -17 * want['weight'][some]).all()
        bound = R.color_bound(p, views, maps, used)
        ok = some & np.isfinite(bound)
        assert (np.abs(colors[ok] - want['colors'][ok]) <= bound[ok, None]).all(), (np.abs(colors[ok] - want['colors'][ok]) / bound[ok, None]).max()
    else:
        assert np.array_equal(best >= 0, some) and (best[~some] == -1).all() and (best < max(n_views, 1)).all()
        idx = np.nonzero(some)[0]
        if not len(idx):
            return 0.0
        w_of_best = want['w'][best[idx].astype(np.int64), idx]          # the restatement's weight of the device's choice
        assert (w_of_best >= (1 - 2.0 ** -17) * want['w'].max(axis=0)[idx]).all()
        assert (np.abs(weight[idx] - w_of_best) <= 2.0 ** -17 * w_of_best).all()
        assert ((used[idx] >> best[idx].astype(np.uint64)) & np.uint64(1)).all()
        for k in np.unique(best[idx]):
            rows = idx[best[idx] == k]
            b = R.sample_bound(p[rows], views[k], maps[k])          # (no final rounding: the colour is the fp32 sample itself)
            fin = np.isfinite(b)
            assert (np.abs(colors[rows][fin] - want['samples'][k][rows][fin]) <= b[fin, None]).all()
    return some.mean() if n else 0.0


@pytest.mark.parametrize('n_views,n', [(0, 1), (0, 257), (1, 0), (1, 255), (2, 256), (3, 1), (3, 65537), (25, 4096), (63, 257), (64, 4096)])
@pytest.mark.parametrize('facing', [False, True])
def test_blend_equals_the_restatement(n_views, n, facing):
    share = _check_blend(n_views, n, facing, 2, 'blend', with_fallback=(n_views + n) % 2 == 0)
    if n >= 4096:          # (the CPU test's caps, on the device's bits; facing passes about half of what the depth test does)
        assert share >= 0.6


@pytest.mark.parametrize('power', [1, 2, 8])
def test_powers_equal_the_restatement(power):
    assert _check_blend(3, 4096, True, power, 'blend', with_fallback=True) >= 0.6


@pytest.mark.parametrize('n_views,n,facing', [(0, 255, True), (1, 257, True), (3, 4096, False), (25, 4096, True), (64, 257, True), (64, 4096, False)])
def test_best_view_equals_the_restatement(n_views, n, facing):
    _check_blend(n_views, n, facing, 2, 'best', with_fallback=facing)


def test_refusals_of_the_python_surface():
    from perf_amd import _lib
    from perf_amd.mesh import color_from_panoramas, panorama_colors
    views, maps = V.make_views(2), R.make_color_maps(2)
    dev = _device_views(views, maps)
    vertices = torch.from_numpy(np.array(R.random_vertices(16))).cuda()
    vertex_normals = torch.from_numpy(np.array(R.random_normals(16))).cuda()
    mesh = _mesh(R.random_vertices(16), [[0, 1, 2]])
    no_map = [{k: v for k, v in d.items() if k != 'color_map'} for d in dev]
    cpu_map = [dict(d, color_map=d['color_map'].cpu()) for d in dev]
    other_size = [dict(d, color_map=d['color_map'][:-1].contiguous()) for d in dev]
    for call, reason in ((lambda: panorama_colors(vertices, no_map, vertex_normals), 'has no color_map'), (lambda: panorama_colors(vertices, cpu_map, vertex_normals), 'CUDA'),
                         (lambda: panorama_colors(vertices, other_size, vertex_normals), "of its distance map's size"), (lambda: panorama_colors(vertices, dev), 'facing'),
                         (lambda: panorama_colors(vertices, dev, vertex_normals, power=9), 'outside 1 .. 8'),
                         (lambda: panorama_colors(vertices, dev, vertex_normals, select='mean'), "'blend' or 'best'"),
                         (lambda: panorama_colors(vertices, dev, vertex_normals, tol=-1.0), 'negative or not finite'),
                         (lambda: panorama_colors(vertices, dev * 33, vertex_normals), 'more than 64'),
                         (lambda: color_from_panoramas(mesh, dev, normals='mesh'), "needs mesh.normals"), (lambda: color_from_panoramas(mesh, dev, normals='field'), "'faces' or 'mesh'")):
        with pytest.raises(_lib.PerfError, match=reason):
            call()


def test_a_pool_with_masks_is_accepted():
    from perf_amd.mesh import panorama_colors

    class Pool:
        pass
    views, maps = V.make_views(3), R.make_color_maps(3)
    pool = Pool()
    pool.sup_infos = [{'pose': torch.from_numpy(np.array(v['pose'])).cuda(), 'distance_map': torch.from_numpy(np.array(v['distance_map'])).cuda()[..., None] * 2.0,
                       'mask': torch.from_numpy(np.asarray(v['distance_map']) > 0).cuda()[..., None], 'color_map': torch.from_numpy(np.array(m)).cuda()}
                      for v, m in zip(views, maps)]            # [H, W, 1] maps with a mask, as SupInfoPool.sup_infos holds them
    doubled = [{'pose': v['pose'], 'distance_map': np.asarray(v['distance_map']) * np.float32(2.0)} for v in views]
    vertices = torch.from_numpy(np.array(R.random_vertices(4096))).cuda()
    vertex_normals = torch.from_numpy(np.array(R.random_normals(4096))).cuda()
    a = panorama_colors(vertices, pool, vertex_normals, tol=1 / 64)
    b = panorama_colors(vertices, _device_views(doubled, maps), vertex_normals, tol=1 / 64)
    assert a.used.ne(0).float().mean().item() > 0.6
    assert torch.equal(a.colors, b.colors) and torch.equal(a.weight, b.weight) and torch.equal(a.used, b.used) and torch.equal(a.best_view, b.best_view)


# ---- the colouring and the cull run one look-up ---------------------------------------------------------------------------------------------
def _lookup_views(k, tiny, rng):
    """k views with centres in [-0.5, 0.5]^3 and 8 x 16 maps of distances that split the vertices (view `tiny`: 1 x 1).  View 0 is not
    rotated, so a vertex straight above it has d_z = 1 and one on its seam d_y = 0 exactly; the others have random rotations."""
    poses, dmaps, cmaps = [], [], []
    for i in range(k):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        if i == 0:
            q = np.eye(3)
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3], pose[:3, 3] = q, rng.uniform(-0.5, 0.5, size=3)
        h, w = (1, 1) if i == tiny else (8, 16)
        poses.append(pose)
        dmaps.append(rng.uniform(0.2, 2.0, size=(h, w)).astype(np.float32))
        cmaps.append(rng.uniform(0.0, 1.0, size=(h, w, 3)).astype(np.float32))
    return poses, dmaps, cmaps


def _lookup_vertices(n, poses, rng):
    """For each of the first four views: straight above and below its centre (asinf(+-1)) and on its seam (atan2f at +-pi, and a hair to
    either side of it); then random vertices in the box [-1.5, 1.5]^3 around the centres."""
    special = []
    for pose in poses[:4]:
        rot, t = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
        for local in ((0, 0, 0.75), (0, 0, -0.75), (-0.6, 0.0, 0), (-0.6, 1e-6, 0), (-0.6, -1e-6, 0)):
            special.append(t + rot @ np.array(local))
    p = np.concatenate([np.array(special).reshape(-1, 3), rng.uniform(-1.5, 1.5, size=(n, 3))])[:n]
    return np.ascontiguousarray(p, dtype=np.float32)


@pytest.mark.parametrize('n_views,tiny', [(1, None), (1, 0), (64, 5)])
@pytest.mark.parametrize('n', [257, 1])
def test_used_bits_without_facing_are_the_culls_visible_bits(n, n_views, tiny):
    """One full workgroup and a one-thread tail (257) or one vertex; one view or all 64 (bit 63, the whole LDS descriptor array); a 1 x 1
    map (w - 1 = 0: both clamps coincide) among 8 x 16 ones.  No vertex lies at a centre: there dist == 0, which the colouring, unlike
    the cull, refuses by rule.  Everywhere else the two kernels run the same look-up, so the words are equal."""
    from perf_amd import ops
    rng = np.random.default_rng(1000 * n + 10 * n_views + (tiny or 0))
    poses, dmaps, cmaps = _lookup_views(n_views, tiny, rng)
    p = _lookup_vertices(n, poses, rng)
    centres = np.array([pose[:3, 3] for pose in poses])
    assert (p[:, None, :] != centres[None]).any(axis=2).all()
    vertices = torch.from_numpy(p).cuda()
    views, _, sizes, held = ops.meshvis_views(poses, [torch.from_numpy(m).cuda() for m in dmaps])
    pointers, held_colours = ops.meshcolor_maps([torch.from_numpy(m).cuda() for m in cmaps], sizes)
    tol = 1 / 64
    visible, _ = ops.meshvis_vertex_bits(vertices, views, sizes, tol, 0.0)
    _, _, used, _ = ops.meshcolor_blend(vertices, None, views, sizes, pointers, tol, facing=False)
    assert used.dtype == visible.dtype == torch.int64 and tuple(used.shape) == tuple(visible.shape) == (n,)
    assert torch.equal(used, visible)
    if n == 257:          # the comparison is not of empty words with empty words: bits are set and bits are clear
        words = _words(visible)
        low = np.uint64((1 << n_views) - 1) if n_views < 64 else ~np.uint64(0)
        assert words.any() and (~words & low).any()
        if n_views == 64:
            assert (words >> np.uint64(63)).any()


# ---- identities ---------------------------------------------------------------------------------------------------------------------------
def _tunnel(color=None):
    from perf_amd.mesh import cull_unseen
    view = V.constant_view()
    h, w = view['distance_map'].shape
    cmap = np.broadcast_to(np.array(color, dtype=np.float32), (h, w, 3)).copy() if color is not None else R.make_color_maps(1)[0]
    assert cmap.shape == (h, w, 3)
    dev = _device_views([view], [cmap])
    culled = cull_unseen(_mesh(*V.reference_mesh('tunnel')), dev, min_views=1, facing=False)
    assert 0 < len(culled.faces) < len(V.reference_mesh('tunnel')[1])
    return culled, dev, view, cmap


def test_a_culled_mesh_has_no_vertex_on_the_fallback():
    from perf_amd.mesh import color_from_panoramas, panorama_colors
    culled, dev, view, cmap = _tunnel()
    out = panorama_colors(culled.vertices, dev, facing=False, fill=(2.0, 2.0, 2.0))
    assert (out.used == 1).all() and (out.weight > 0).all() and (out.colors < 1.0).all()
    coloured = color_from_panoramas(culled, dev, facing=False, fill=(2.0, 2.0, 2.0))
    assert torch.equal(coloured.colors, out.colors) and coloured.normals is None and coloured.faces is culled.faces
    want = R.sample(culled.vertices.cpu().numpy(), view, cmap)          # one view: the blend is its sample
    bound = R.sample_bound(culled.vertices.cpu().numpy(), view, cmap) + 2.0 ** -18 + 2.0 ** -24
    assert (np.abs(out.colors.cpu().numpy() - want) <= bound[:, None]).all()


def test_a_constant_colour_map_colours_every_vertex_with_it():
    from perf_amd.mesh import color_from_panoramas
    constant = (0.25, 0.5, 0.75)
    culled, dev, _, _ = _tunnel(constant)
    for normals in ('faces', 'mesh'):
        mesh = culled._replace(normals=torch.nn.functional.normalize(torch.tensor(V.CENTRE, device='cuda') - culled.vertices, dim=1))
        for select in ('blend', 'best'):
            coloured = color_from_panoramas(mesh, dev, normals=normals, select=select, fill=(9.0, 9.0, 9.0), box=BOX)
            on = (coloured.colors != 9.0).all(dim=1)
            assert on.float().mean() > 0.9 and coloured.normals is mesh.normals          # (the inner skin faces the view at its centre)
            assert (coloured.colors[on] - torch.tensor(constant, device='cuda')).abs().max().item() <= 4 * 2.0 ** -24


def test_mesh_normals_against_face_normals_on_the_sphere():
    from perf_amd.mesh import color_from_panoramas, face_normals
    views, maps = V.make_views(3), R.make_color_maps(3)
    dev = _device_views(views, maps)
    mesh = _mesh(*V.reference_mesh('hollow_sphere'))
    by_faces = color_from_panoramas(mesh, dev, normals='faces', box=BOX, tol=1 / 8)
    with_normals = mesh._replace(normals=face_normals(mesh, BOX), colors=torch.full_like(mesh.vertices, 0.3))
    by_mesh = color_from_panoramas(with_normals, dev, normals='mesh', tol=1 / 8)
    assert (by_faces.colors != 0.5).any() and (by_faces.colors == 0.5).all(dim=1).any()
    assert torch.equal((by_faces.colors == 0.5).all(dim=1), (by_mesh.colors == 0.3).all(dim=1))          # fill there, mesh.colors (the fallback) here
    on = (by_faces.colors != 0.5).any(dim=1)
    assert torch.equal(by_faces.colors[on], by_mesh.colors[on])


def test_the_simplification_carries_the_colours_and_a_ply_round_trip_reads_them_back(tmp_path):
    from perf_amd.mesh import color_from_panoramas, simplify_mesh, write_ply
    views, maps = V.make_views(3), R.make_color_maps(3)
    dev = _device_views(views, maps)
    coloured = color_from_panoramas(_mesh(*V.reference_mesh('hollow_sphere')), dev, box=BOX, tol=1 / 8)
    small, index = simplify_mesh(coloured, 0.25, box=BOX)
    assert 0 < len(small.vertices) < len(coloured.vertices) and torch.equal(small.colors, coloured.colors[index.long()])
    path = tmp_path / 'coloured.ply'
    write_ply(str(path), small)
    raw = path.read_bytes()
    head, body = raw.split(b'end_header\n', 1)
    assert b'property uchar red' in head and b'property uchar green' in head and b'property uchar blue' in head and b'property float nx' not in head
    rows = np.frombuffer(body, dtype=[('xyz', '<f4', (3,)), ('rgb', 'u1', (3,))], count=len(small.vertices))
    assert np.array_equal(rows['xyz'], small.vertices.cpu().numpy())
    assert np.array_equal(rows['rgb'], np.rint(np.clip(small.colors.cpu().numpy(), 0.0, 1.0) * 255.0).astype(np.uint8))
    assert len(np.unique(rows['rgb'], axis=0)) > 16
