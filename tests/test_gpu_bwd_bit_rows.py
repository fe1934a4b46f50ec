"""Grid backward, hashed levels of at most 16 tiles: the pre-pass leaves one bit row per tile (store_bit_rows in
perf_amd/csrc/hashgrid_bwd.hip: a 16 x 64 bit transposition of a wave's tile masks) and an owner walks its own row, a halfword per
lane and round (bwd_stream_bits).  The rows are not exported, so the check is what they produce: ops.hashgrid_bwd with a full
workspace against use_codes=False, the position-streaming owners, which use no pre-pass and which tests/test_gpu_exact_gradients.py
holds to the integer oracle.  Fixed-point tables must be equal to the bit; fp32 tables add floats in another order and stay within
1e-4 x max|table|, the bound of tests/test_gpu_tile_codes_prepass.py.

A wave's round is ROUND = 1,024 samples (kBitRoundSamples: 16 bits x 64 lanes), a workgroup's sixteen waves cover 16 x ROUND in one
round each, a pre-pass block is 256 samples, a lane of it holds 4, a DPP row of it 64.  Calls of fewer than 256 rows of capacity have
no room for a block's pieces in their code slot and take the position-streaming owners on these levels; the live counts below a
2,048-row capacity reach the bit rows with 0, 1, 255, 257 and 1,025 live samples."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROUND = 16 * 64                 # kBitRoundSamples
WAVES = 16                      # kBwdThreads / 64


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


def _amax(dfeat):
    amax = torch.nan_to_num(dfeat, nan=0.0).abs().amax(dim=(1, 2)).contiguous() if dfeat.shape[1] else torch.zeros(dfeat.shape[0], device='cuda')
    return torch.cat([amax, torch.zeros(16 - amax.numel(), device='cuda')])


def _dfeat(cfg, n, g):
    dfeat = torch.randn(cfg.n_levels, n, 2, generator=g).cuda()
    return dfeat, _amax(dfeat)


def _check(ops, cfg, x, dfeat, amax, tag, n_dev=None):
    """bit-row / code owners against position-streaming owners, both modes; returns the fixed-point table"""
    a_fix = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax, n_dev=n_dev)
    b_fix = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax, n_dev=n_dev, use_codes=False)
    a_f32 = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev)
    b_f32 = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev, use_codes=False)
    assert bool(torch.isfinite(a_fix).all()) and bool(torch.isfinite(a_f32).all()), tag
    assert torch.equal(a_fix, b_fix), (tag, float((a_fix - b_fix).abs().max()))
    assert float((a_f32 - b_f32).abs().max()) <= 1e-4 * float(b_f32.abs().max()), tag
    return a_fix


def test_default_grid_has_twelve_bit_row_levels():
    cfg = _cfg()
    hashed = [l for l in range(16) if int(cfg.hashed[l])]
    assert hashed == list(range(4, 16)) and all(int(cfg.size[l]) == 1 << 18 for l in hashed)       # 16 tiles of 16,384 entries each


@pytest.mark.parametrize('n', [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, ROUND - 1, ROUND, ROUND + 1, 4099,
                               WAVES * ROUND + 1, 2 * WAVES * ROUND + 1])
def test_sample_counts(ops, n):
    """a lane's 4 samples, a DPP row's 64, a block's 256, a wave's round, and one and two rounds of every wave of the workgroup"""
    cfg = _cfg()
    g = torch.Generator().manual_seed(300 + n % 1000)
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, n)


def test_burst_of_one_point(ops):
    """every sample names the same tiles: a round holds 1,024 hits, more than the queue bound, and goes in by nibbles"""
    cfg = _cfg()
    g = torch.Generator().manual_seed(31)
    n = 4099
    x = torch.tensor([[0.3711, 0.6127, 0.4409]]).repeat(n, 1).contiguous().cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, 'one point')


def test_burst_of_one_ray(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(32)
    n = 4099
    d = torch.nn.functional.normalize(torch.randn(1, 3, generator=g), dim=-1)
    t = (torch.arange(n) + 0.5) / n
    x = (0.5 + 0.45 * t[:, None] * d).contiguous().cuda()         # one ray from the centre of the cube
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, 'one ray')


@pytest.mark.parametrize('live', [0, 1, 255, 257, 1025])
def test_live_count_below_capacity(ops, live):
    cfg = _cfg()
    g = torch.Generator().manual_seed(33)
    cap = 2048
    x = torch.rand(cap, 3, generator=g)
    dfeat = torch.randn(cfg.n_levels, cap, 2, generator=g)
    x[live:] = float('nan')                     # rows past the live count must not be read
    dfeat[:, live:] = float('nan')
    x, dfeat = x.cuda(), dfeat.cuda()
    amax = _amax(dfeat)
    n_dev = torch.tensor([live], dtype=torch.int64, device='cuda')
    got = _check(ops, cfg, x, dfeat, amax, live, n_dev=n_dev)
    if live == 0:
        assert not bool(got.any())
    else:                                       # the same table as a call that holds the live rows only
        ref = ops.hashgrid_bwd(cfg, x[:live].contiguous(), dfeat[:, :live].contiguous(), level_absmax=amax, use_codes=False)
        assert torch.equal(got, ref)


@pytest.mark.parametrize('gradient', ['zero', 'nonzero'])
def test_points_far_outside_the_cube(ops, gradient):
    """points whose x-corners leave the first 16,384 columns of a hashed level: without gradient nothing escapes and the bit rows are
    used, with gradient the level goes to the generic owners"""
    cfg = _cfg()
    g = torch.Generator().manual_seed(34)
    n = 4099
    x = torch.rand(n, 3, generator=g)
    far = torch.tensor([5, 258, 1023, 1024, 4095, 4098])
    x[far, 0] = 40.0
    x[far[::2], 1] = -3.0
    assert any(40.0 * float(cfg.scale[l]) + 0.5 >= 16383 for l in range(16) if int(cfg.hashed[l]))
    dfeat = torch.randn(cfg.n_levels, n, 2, generator=g)
    if gradient == 'zero':
        dfeat[:, far] = 0.0
    dfeat = dfeat.cuda()
    _check(ops, cfg, x.cuda(), dfeat, _amax(dfeat), gradient)


def test_rows_with_zero_gradient(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(35)
    n = 4099
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat = torch.randn(cfg.n_levels, n, 2, generator=g)
    dfeat[:, ::3] = 0.0
    dfeat[5, :] = 0.0                            # and a whole level
    dfeat = dfeat.cuda()
    _check(ops, cfg, x, dfeat, _amax(dfeat), 'zero rows')


@pytest.mark.parametrize('kind', ['uniform', 'point'])
@pytest.mark.parametrize('log2_t, tiles', [(14, 1), (15, 2), (16, 4), (17, 8), (19, 32)])
def test_other_tile_counts(ops, log2_t, tiles, kind):
    """2, 4 and 8 tiles: rows above the tile count stay unwritten and unread; 32 tiles keep the byte codes, one tile is not coded"""
    cfg = _cfg(log2_hashmap_size=log2_t)
    assert int(cfg.size[15]) == tiles * 16384 and int(cfg.hashed[15]) == 1
    g = torch.Generator().manual_seed(36)
    n = 4099
    x = (torch.rand(n, 3, generator=g) if kind == 'uniform' else torch.tensor([[0.3711, 0.6127, 0.4409]]).repeat(n, 1).contiguous()).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, (log2_t, kind))


@pytest.mark.parametrize('interpolation', ['Linear', 'Smoothstep'])
def test_both_interpolations(ops, interpolation):
    cfg = _cfg(interpolation=interpolation)
    g = torch.Generator().manual_seed(37)
    n = 4099
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, interpolation)


def test_unaligned_positions(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(38)
    n = 4099
    buf = torch.rand(3 * n + 8, generator=g).cuda()
    x = buf[1:1 + 3 * n].view(n, 3)             # starts one float into the buffer
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    dfeat, amax = _dfeat(cfg, n, g)
    got = _check(ops, cfg, x, dfeat, amax, 'unaligned')
    assert torch.equal(got, ops.hashgrid_bwd(cfg, x.clone(), dfeat, level_absmax=amax))


def test_accumulate_onto_a_table(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(39)
    n = 4099
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    base = torch.randn(cfg.n_params, generator=g).cuda()
    outs = []
    for fixed in (True, False):
        for use_codes in (True, False):
            outs.append(ops.hashgrid_bwd(cfg, x, dfeat, out=base.clone(), accumulate=True, level_absmax=amax if fixed else None,
                                         use_codes=use_codes))
    a_fix, b_fix, a_f32, b_f32 = outs
    assert not torch.equal(a_fix, base)
    assert torch.equal(a_fix, b_fix), float((a_fix - b_fix).abs().max())
    assert float((a_f32 - b_f32).abs().max()) <= 1e-4 * float(b_f32.abs().max())


def test_raw_fields_with_given_shifts(ops):
    """the data-parallel form: units given by the caller, the table receives the int32 field pairs"""
    cfg = _cfg()
    g = torch.Generator().manual_seed(40)
    n = 4099
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, _ = _dfeat(cfg, n, g)
    shifts = torch.zeros(24, dtype=torch.int32)
    shifts[:16] = 16                            # |dfeat| < 8 and a few samples per entry: fields far below 2^29
    shifts = shifts.cuda()
    a = ops.hashgrid_bwd(cfg, x, dfeat, shifts=shifts, raw_fields=True).view(torch.int32)
    b = ops.hashgrid_bwd(cfg, x, dfeat, shifts=shifts, raw_fields=True, use_codes=False).view(torch.int32)
    assert bool(a.any()) and int(a.abs().max()) < 1 << 29
    assert torch.equal(a, b)


def test_two_runs_are_equal_to_the_bit(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(41)
    n = WAVES * ROUND + 1
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    first = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax)
    second = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax)
    assert torch.equal(first, second)
