"""Grid backward, the owners' main loops (bwd_stream_masks and bwd_stream_codes in perf_amd/csrc/hashgrid_bwd.hip) on the shapes
tests/test_gpu_bwd_tile_masks.py does not reach.  The comparison is that file's: the default owners (tile masks / byte codes) against
the owners that stream positions (use_codes=False), which form every index with the 32-bit multiply, enqueue nothing and which
tests/test_gpu_exact_gradients.py holds to the integer oracle.  Fixed-point mode adds integers, so its tables must be equal to the bit;
fp32 mode adds floats in another order and must stay within 1e-4 x max|table|.

What the shapes are for:
 * the coded owners multiply with the 24-bit multiplier (only the low 24 bits of gy * P_y, gz * P_z -- dense levels: gy * res,
   gz * res^2 -- count on a level of at most 2^24 entries): cells beyond 2^24 and negative cells on y / z, with x inside the cube so
   that no level escapes to the generic owners, are where the low 24 bits of that product could part from the 32-bit one -- on a mask
   grid (T = 2^18) and on a byte-code grid (T = 2^21: 128 tiles per hashed level);
 * the four sample slots of an iteration enter a wave's queue one after the other at scalar-side positions: one slot full and three
   empty, for each slot, at the owners of one tile -- and the rest of the samples at the owners of another;
 * a live count below the capacity (the last iteration's lanes without a group of their own hit nothing);
 * the dense byte-code owners (levels 1..3 of the default grid) under both interpolations, uniform points and points whose x-corners
   part at chunk boundaries;
 * two runs equal to the bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRIME_Y, PRIME_Z = 2654435761, 805459861
TILE = 16384


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from perf_amd import ops as _ops
    return _ops


def _cfg(**kw):
    from perf_amd.grid import GridConfig
    kw.setdefault('n_levels', 16)
    kw.setdefault('log2_hashmap_size', 18)
    return GridConfig(**kw)


def _dfeat(cfg, n, g):
    dfeat = torch.randn(cfg.n_levels, n, 2, generator=g).cuda()
    amax = dfeat.abs().amax(dim=(1, 2)).contiguous()
    return dfeat, torch.cat([amax, torch.zeros(16 - amax.numel(), device='cuda')])


def _check(ops, cfg, x, dfeat, amax, tag, n_dev=None):
    """mask / code owners against position-streaming owners, both modes; returns the fixed-point table"""
    a_fix = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax, n_dev=n_dev)
    b_fix = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax, n_dev=n_dev, use_codes=False)
    a_f32 = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev)
    b_f32 = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev, use_codes=False)
    assert bool(torch.isfinite(a_fix).all()) and bool(torch.isfinite(a_f32).all()), tag
    assert bool(a_fix.any()), tag
    assert torch.equal(a_fix, b_fix), (tag, float((a_fix - b_fix).abs().max()))
    assert float((a_f32 - b_f32).abs().max()) <= 1e-4 * float(b_f32.abs().max()), tag
    return a_fix


def _far_rows(n, g):
    """uniform points; y of every 5th and z of every 7th row far outside the cube, on either side: grid cells of up to
    3e5 x scale ~ 1.2e9 (beyond 2^24, below 2^31) and their negatives, x stays inside"""
    x = torch.rand(n, 3, generator=g)
    far = torch.tensor([1e4, -1e4, 3e5, -3e5])
    iy, iz = torch.arange(0, n, 5), torch.arange(1, n, 7)
    x[iy, 1] = far[torch.arange(iy.numel()) % 4]
    x[iz, 2] = far[(torch.arange(iz.numel()) + 1) % 4]
    return x.contiguous()


@pytest.mark.parametrize('log2_t', [18, 21])
def test_cells_beyond_24_bits_and_negative_cells(ops, log2_t):
    cfg = _cfg(log2_hashmap_size=log2_t)
    tiles = (1 << log2_t) // TILE
    assert int(cfg.hashed[15]) == 1 and int(cfg.size[15]) == tiles * TILE and tiles == (16 if log2_t == 18 else 128)
    g = torch.Generator().manual_seed(200 + log2_t)
    n = 4099
    x = _far_rows(n, g)
    assert float((x[:, 1].abs() * float(cfg.scale[15])).max()) > float(1 << 24) and float(x[:, 0].min()) >= 0.0 and float(x[:, 0].max()) < 1.0
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x.cuda(), dfeat, amax, ('far', log2_t))


def _tiles_named(cfg, l, p):
    """the tiles of hashed level l that the four (y,z) combinations of point p name"""
    pos = np.float32(p) * np.float32(cfg.scale[l]) + np.float32(0.5)
    gy, gz = int(np.floor(pos[1])), int(np.floor(pos[2]))
    mask = int(cfg.size[l]) - 1
    return {((((gy + by) * PRIME_Y) ^ ((gz + bz) * PRIME_Z)) & mask) // TILE for by in (0, 1) for bz in (0, 1)}


@pytest.mark.parametrize('slot', [0, 1, 2, 3])
def test_one_slot_full_three_empty(ops, slot):
    cfg = _cfg()
    l = int(np.argmax(cfg.hashed))
    a = np.array([0.3711, 0.6127, 0.4409], np.float32)
    b = None
    for cand in np.random.RandomState(5).rand(64, 3).astype(np.float32):       # a second point that names other tiles at level l
        if not (_tiles_named(cfg, l, a) & _tiles_named(cfg, l, cand)):
            b = cand
            break
    assert b is not None
    n = 1024 * 4 + 3
    x = torch.from_numpy(b).repeat(n, 1)
    x[slot::4] = torch.from_numpy(a)            # exactly the samples 4k + slot name a's tiles
    g = torch.Generator().manual_seed(300 + slot)
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x.contiguous().cuda(), dfeat, amax, ('slot', slot))


@pytest.mark.parametrize('live', [5, 257])
def test_live_count_below_capacity(ops, live):
    cfg = _cfg()
    g = torch.Generator().manual_seed(400 + live)
    cap = 4096
    x = torch.rand(cap, 3, generator=g)
    x[live:] = float('nan')                     # rows past the live count must not be read into the sums
    x = x.cuda()
    dfeat, amax = _dfeat(cfg, cap, g)
    n_dev = torch.tensor([live], dtype=torch.int64, device='cuda')
    got = _check(ops, cfg, x, dfeat, amax, ('live', live), n_dev=n_dev)
    ref = ops.hashgrid_bwd(cfg, x[:live].contiguous(), dfeat[:, :live].contiguous(), level_absmax=amax, use_codes=False)
    assert torch.equal(got, ref)


@pytest.mark.parametrize('points', ['uniform', 'x_at_chunk_ends'])
@pytest.mark.parametrize('interpolation', ['Linear', 'Smoothstep'])
def test_dense_code_owners_both_interpolations(ops, interpolation, points):
    cfg = _cfg(interpolation=interpolation)
    dense_multi_tile = [l for l in range(cfg.n_levels) if not int(cfg.hashed[l]) and int(cfg.size[l]) > TILE]
    assert dense_multi_tile, 'the default grid has dense levels of several tiles (byte-code owners)'
    g = torch.Generator().manual_seed(500)
    n = 4099
    x = torch.rand(n, 3, generator=g)
    if points == 'x_at_chunk_ends':
        x[:, 0] = 0.999                         # the last cell along x: the two x-corners of a combination part at a chunk boundary
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x.cuda(), dfeat, amax, (interpolation, points))


def test_two_runs_are_equal_to_the_bit(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(600)
    n = 4099
    x = _far_rows(n, g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    first = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax)
    second = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax)
    assert torch.equal(first, second)
