"""Grid backward, the tile-code pre-pass (tile_codes4_kernel in perf_amd/csrc/hashgrid_bwd.hip): a workgroup per escape word of 256
samples, four samples per lane, the coded levels split over the workgroup's four waves.

The codes are not exported, so the check is what they produce: ops.hashgrid_bwd with a full workspace (pre-pass + code-streaming
owners) against use_codes=False, the position-streaming owners that use no pre-pass, as tests/test_gpu_bwd_tile_masks.py::_check
compares them: fixed-point tables equal to the bit, fp32 tables within 1e-4 x max|table|.

The sample counts sit around 65,536 (the live count at which the pre-pass used to change its shape; the sizes stay now that it has
one): the count itself, a last lane with 1 and 3 samples, a last word with 255 and 1 samples, a live count below the capacity with NaN
rows behind it, positions that are not 16-byte aligned (the scalar-load path), points far outside the cube with and without gradient
(escape and no escape), hashed levels of 32 tiles (byte codes) and of one tile (only dense levels coded), both interpolations."""
import pytest
import torch

pytestmark = pytest.mark.gpu


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
    return dfeat, _amax(cfg, dfeat)


def _amax(cfg, dfeat):
    amax = torch.nan_to_num(dfeat, nan=0.0).abs().amax(dim=(1, 2)).contiguous()
    return torch.cat([amax, torch.zeros(16 - amax.numel(), device='cuda')])


def _check(ops, cfg, x, dfeat, amax, tag, n_dev=None):
    """pre-pass + code owners against position-streaming owners, both modes; returns the two fixed-point tables' common value"""
    a_fix = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax, n_dev=n_dev)
    b_fix = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax, n_dev=n_dev, use_codes=False)
    a_f32 = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev)
    b_f32 = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev, use_codes=False)
    assert bool(torch.isfinite(a_fix).all()) and bool(torch.isfinite(a_f32).all()), tag
    assert torch.equal(a_fix, b_fix), (tag, float((a_fix - b_fix).abs().max()))
    assert float((a_f32 - b_f32).abs().max()) <= 1e-4 * float(b_f32.abs().max()), tag
    return a_fix


@pytest.mark.parametrize('n', [65536, 65537, 65539, 65791, 65793, 131073])
def test_threshold_sizes(ops, n):
    cfg = _cfg()
    g = torch.Generator().manual_seed(200 + n % 1000)
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, n)


@pytest.mark.parametrize('live', [65535, 65536, 65540])
def test_live_count_below_capacity(ops, live):
    cfg = _cfg()
    g = torch.Generator().manual_seed(21)
    cap = 131072
    x = torch.rand(cap, 3, generator=g)
    dfeat = torch.randn(cfg.n_levels, cap, 2, generator=g)
    x[live:] = float('nan')                     # rows past the live count must not be read
    dfeat[:, live:] = float('nan')
    x, dfeat = x.cuda(), dfeat.cuda()
    amax = _amax(cfg, dfeat)
    n_dev = torch.tensor([live], dtype=torch.int64, device='cuda')
    got = _check(ops, cfg, x, dfeat, amax, live, n_dev=n_dev)
    ref = ops.hashgrid_bwd(cfg, x[:live].contiguous(), dfeat[:, :live].contiguous(), level_absmax=amax, use_codes=False)
    assert torch.equal(got, ref)                # the same table as a call that holds the live rows only


def test_unaligned_positions(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(22)
    n = 65540
    buf = torch.rand(3 * n + 8, generator=g).cuda()
    x = buf[1:1 + 3 * n].view(n, 3)             # starts one float into the buffer
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    dfeat, amax = _dfeat(cfg, n, g)
    got = _check(ops, cfg, x, dfeat, amax, 'unaligned')
    aligned = x.clone()
    assert aligned.data_ptr() % 16 == 0
    assert torch.equal(got, ops.hashgrid_bwd(cfg, aligned, dfeat, level_absmax=amax))


@pytest.mark.parametrize('gradient', ['nonzero', 'zero'])
def test_points_outside_the_cube(ops, gradient):
    """a few points whose x-corners leave the first 16,384 columns of a hashed level: with gradient the level escapes to the generic
    owners, without it the codes are harmless and nothing escapes"""
    cfg = _cfg()
    g = torch.Generator().manual_seed(23)
    n = 65536
    x = torch.rand(n, 3, generator=g)
    far = torch.tensor([5, 258, 4099, 32771, 65533, 65535])       # in the first, a middle and the last word, and in one lane's tail
    x[far, 0] = 40.0
    x[far[::2], 1] = -3.0
    hashed = [l for l in range(cfg.n_levels) if int(cfg.hashed[l])]
    assert any(40.0 * float(cfg.scale[l]) + 0.5 >= 16383 for l in hashed)
    dfeat = torch.randn(cfg.n_levels, n, 2, generator=g)
    if gradient == 'zero':
        dfeat[:, far] = 0.0
    dfeat = dfeat.cuda()
    _check(ops, cfg, x.cuda(), dfeat, _amax(cfg, dfeat), gradient)


@pytest.mark.parametrize('log2_t', [19, 14])
def test_other_level_kinds(ops, log2_t):
    """hashed levels of 32 tiles (byte codes) and of one tile (not coded: the list holds the dense levels only)"""
    cfg = _cfg(log2_hashmap_size=log2_t)
    assert int(cfg.size[15]) == 1 << log2_t and int(cfg.hashed[15]) == 1
    g = torch.Generator().manual_seed(24)
    n = 65540
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, log2_t)


@pytest.mark.parametrize('interpolation', ['Linear', 'Smoothstep'])
def test_both_interpolations(ops, interpolation):
    cfg = _cfg(interpolation=interpolation)
    g = torch.Generator().manual_seed(25)
    n = 65540
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, interpolation)


def test_two_runs_are_equal_to_the_bit(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(26)
    n = 65793
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    first = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax)
    second = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax)
    assert torch.equal(first, second)
