"""Grid backward, hashed levels of at most 16 tiles: the owners that stream a 16-bit tile mask per sample (bwd_stream_masks in
perf_amd/csrc/hashgrid_bwd.hip, the default with a full workspace) against the owners that stream positions (use_codes=False), which
the mask path does not touch and which tests/test_gpu_exact_gradients.py holds to the integer oracle.

Fixed-point mode adds integers, so its tables must be equal to the bit; fp32 mode adds floats in another order and must stay within
1e-4 x max|table| (the bound of test_hashgrid_bwd_coded_owners_equal_streaming_owners).  The shapes are the smallest at which the
loop takes each of its paths: a ragged tail of fewer than 4 / 256 / 1,024 samples, one workgroup iteration and several, samples that
all hit one tile (re-queue path, burst drains, the queue bound), a live count below the capacity,
positions that send a level back to the generic owners, and tile counts on either side of the mask / byte-code threshold."""
import numpy as np
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
    amax = dfeat.abs().amax(dim=(1, 2)).contiguous() if n else torch.zeros(cfg.n_levels, device='cuda')
    return dfeat, torch.cat([amax, torch.zeros(16 - amax.numel(), device='cuda')])


def _check(ops, cfg, x, dfeat, amax, tag, n_dev=None, **kw):
    """mask / code owners against position-streaming owners, both modes; returns the fixed-point table"""
    a_fix = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax, n_dev=n_dev, **kw)
    b_fix = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax, n_dev=n_dev, use_codes=False, **kw)
    a_f32 = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev, **kw)
    b_f32 = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev, use_codes=False, **kw)
    assert bool(torch.isfinite(a_fix).all()) and bool(torch.isfinite(a_f32).all()), tag
    assert torch.equal(a_fix, b_fix), (tag, float((a_fix - b_fix).abs().max()))
    assert float((a_f32 - b_f32).abs().max()) <= 1e-4 * float(b_f32.abs().max()), tag
    return a_fix


def _first_hashed(cfg):
    return int(np.argmax(cfg.hashed))


def _one_cell(cfg, kind, n, g):
    """'point': n copies of one interior point; 'cell': n points inside one cell of the first hashed level"""
    if kind == 'point':
        return torch.tensor([[0.3711, 0.6127, 0.4409]]).repeat(n, 1).contiguous()
    l = _first_hashed(cfg)
    cell = torch.tensor([11.0, 17.0, 23.0])
    u = 0.05 + 0.9 * torch.rand(n, 3, generator=g)
    return ((cell + u - 0.5) / float(cfg.scale[l])).contiguous()         # grid position = x * scale + 0.5


def test_default_grid_is_the_mask_case():
    cfg = _cfg()
    l = _first_hashed(cfg)
    assert l == 4 and all(int(cfg.size[k]) == 1 << 18 for k in range(l, 16))     # twelve hashed levels of 16 tiles


@pytest.mark.parametrize('n', [1, 3, 255, 1027, 4099])
def test_ragged_sizes(ops, n):
    cfg = _cfg()
    g = torch.Generator().manual_seed(100 + n)
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, n)


@pytest.mark.parametrize('kind', ['point', 'cell'])
def test_one_cell(ops, kind):
    cfg = _cfg()
    g = torch.Generator().manual_seed(7)
    n = 8192
    x = _one_cell(cfg, kind, n, g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, kind)


def test_one_ray_origin(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(8)
    d = torch.nn.functional.normalize(torch.randn(128, 3, generator=g), dim=-1)
    t = (torch.arange(64) + 0.5) / 64
    x = ((d[:, None, :] * t[None, :, None]).reshape(-1, 3) * 0.5 + 0.5).contiguous().cuda()
    dfeat, amax = _dfeat(cfg, x.shape[0], g)
    _check(ops, cfg, x, dfeat, amax, 'rays')


@pytest.mark.parametrize('live', [0, 1, 100, 4095])
def test_live_count_below_capacity(ops, live):
    cfg = _cfg()
    g = torch.Generator().manual_seed(9)
    cap = 4096
    x = torch.rand(cap, 3, generator=g)
    x[live:] = float('nan')                     # rows past the live count must not be read into the sums
    x = x.cuda()
    dfeat, amax = _dfeat(cfg, cap, g)
    n_dev = torch.tensor([live], dtype=torch.int64, device='cuda')
    got = _check(ops, cfg, x, dfeat, amax, live, n_dev=n_dev)
    if live == 0:
        assert not bool(got.any())
    else:       # the same table as a call that holds the live rows only
        ref = ops.hashgrid_bwd(cfg, x[:live].contiguous(), dfeat[:, :live].contiguous(), level_absmax=amax, use_codes=False)
        assert torch.equal(got, ref)


def test_outside_the_cube(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(10)
    n = 4099
    x = torch.rand(n, 3, generator=g)
    x[::7, 0] = -0.25
    x[5::11, 0] = 9.5
    x[3::13, 1] = -3.0
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x.cuda(), dfeat, amax, 'outside')


@pytest.mark.parametrize('kind', ['uniform', 'point'])
@pytest.mark.parametrize('log2_t', [14, 15, 19])
def test_other_tile_counts(ops, log2_t, kind):
    """1 and 2 tiles per hashed level (position-streaming owners, mask owners) and 32 (the byte codes that stay)"""
    cfg = _cfg(log2_hashmap_size=log2_t)
    assert int(cfg.size[15]) == 1 << log2_t and int(cfg.hashed[15]) == 1
    g = torch.Generator().manual_seed(11)
    n = 4099 if kind == 'uniform' else 8192
    x = (torch.rand(n, 3, generator=g) if kind == 'uniform' else _one_cell(cfg, 'point', n, g)).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, (log2_t, kind))


@pytest.mark.parametrize('live', [None, 3001])
def test_accumulate_onto_a_table(ops, live):
    cfg = _cfg()
    g = torch.Generator().manual_seed(12)
    n = 4099
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    base = torch.randn(cfg.n_params, generator=g).cuda()
    n_dev = None if live is None else torch.tensor([live], dtype=torch.int64, device='cuda')
    outs = []
    for fixed in (True, False):
        for use_codes in (True, False):
            outs.append(ops.hashgrid_bwd(cfg, x, dfeat, out=base.clone(), accumulate=True, level_absmax=amax if fixed else None,
                                         n_dev=n_dev, use_codes=use_codes))
    a_fix, b_fix, a_f32, b_f32 = outs
    assert not torch.equal(a_fix, base)
    assert torch.equal(a_fix, b_fix), float((a_fix - b_fix).abs().max())
    assert float((a_f32 - b_f32).abs().max()) <= 1e-4 * float(b_f32.abs().max())


@pytest.mark.parametrize('interpolation', ['Linear', 'Smoothstep'])
def test_both_interpolations(ops, interpolation):
    cfg = _cfg(interpolation=interpolation)
    g = torch.Generator().manual_seed(13)
    n = 4099
    x = torch.rand(n, 3, generator=g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    _check(ops, cfg, x, dfeat, amax, interpolation)


def test_two_runs_are_equal_to_the_bit(ops):
    cfg = _cfg()
    g = torch.Generator().manual_seed(14)
    n = 8192
    x = _one_cell(cfg, 'cell', n, g).cuda()
    dfeat, amax = _dfeat(cfg, n, g)
    first = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax)
    second = ops.hashgrid_bwd(cfg, x, dfeat, level_absmax=amax)
    assert torch.equal(first, second)
