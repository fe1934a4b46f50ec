"""The pair encode's level-at-a-time body and its plan of slots (perf_amd/csrc/hashgrid_pair.hip) on the grids where they can go wrong:
one pair encode equals two single encodes to the bit (torch.equal), for both dtypes, on grids whose slots are all single-level, all
dense with a padded part, a mix of single- and two-level slots in one part, dense levels without a hashed partner, and one level.

The slots of a grid are restated here from GridConfig.hashed by the rule pair_plan documents -- every hashed level alone, except the
finest ones, which sit beside the dense levels, one each, the finest hashed beside the coarsest dense; dense levels beyond the number
of hashed ones alone; eight slots to a part, a part of 3, 5, 6 or 7 padded with empty slots to a power of two -- and each case states
the slots it expects, so that a reader sees the structure is really hit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _parts(cfg):
    """pair_plan's rule on GridConfig.hashed: a list of parts, each a list of slots (level, level or None); None: an empty slot."""
    hashed = [l for l in range(cfg.n_levels) if cfg.hashed[l]]
    dense = [l for l in range(cfg.n_levels) if not cfg.hashed[l]]
    n_both = min(len(dense), len(hashed))
    slots = [(l, None) for l in hashed[:len(hashed) - n_both]]
    slots += [(d, hashed[len(hashed) - 1 - k] if k < n_both else None) for k, d in enumerate(dense)]
    parts = []
    for s0 in range(0, len(slots), 8):
        part = slots[s0:s0 + 8]
        width = 1
        while width < len(part):
            width *= 2
        parts.append(part + [None] * (width - len(part)))
    return parts


# name -> (n_levels, log2_hashmap_size, GridConfig.hashed, the parts expected)
GRIDS = {
    # every level hashed: single-level slots only, two parts of eight
    'all_hashed': (16, 10, [1] * 16, [[(l, None) for l in range(8)], [(l, None) for l in range(8, 16)]]),
    # dense levels only; the part of three is padded with one empty slot
    'dense_padded': (3, 18, [0, 0, 0], [[(0, None), (1, None), (2, None), None]]),
    # 2 dense, 14 hashed: part 0 holds eight single-level slots, part 1 four single-level and two two-level slots, padded to eight
    'mixed_part': (16, 14, [0, 0] + [1] * 14, [[(l, None) for l in range(2, 10)],
                                               [(10, None), (11, None), (12, None), (13, None), (0, 15), (1, 14), None, None]]),
    # 4 dense, 2 hashed: dense levels 2 and 3 have no hashed partner
    'dense_alone': (6, 18, [0, 0, 0, 0, 1, 1], [[(0, 5), (1, 4), (2, None), (3, None)]]),
    'one_level': (1, 18, [0], [[(0, None)]]),
}
_STATE = {}


def _grid(name, interpolation='Linear'):
    from perf_amd.grid import GridConfig
    n_levels, log2_t, hashed, parts = GRIDS[name]
    cfg = GridConfig(n_levels=n_levels, log2_hashmap_size=log2_t, interpolation=interpolation)
    assert [int(h) for h in cfg.hashed] == hashed, name
    assert _parts(cfg) == parts, name
    return cfg


def _tables(name, dtype):
    """two random 16-bit tables of the grid and their pair table, made once per (grid, dtype)"""
    from perf_amd import ops
    key = (name, dtype)
    if key not in _STATE:
        cfg = _grid(name)
        g = torch.Generator().manual_seed(101 + 2 * sorted(GRIDS).index(name) + (dtype == 'fp16'))
        ta = ops.cast_params(((torch.rand(cfg.n_params, generator=g) * 2 - 1) * 0.5).cuda(), dtype)
        tb = ops.cast_params(((torch.rand(cfg.n_params, generator=g) * 2 - 1) * 0.5).cuda(), dtype)
        pair = ops.pair_table(cfg, ta.device)
        ops.pair_fill(pair, 0, ta); ops.pair_fill(pair, 1, tb)
        _STATE[key] = (ta, tb, pair)
    return _STATE[key]


def _threshold_points():
    """Two waves on either side of the share threshold (56 heads) at every level, the coarsest included: wave 0 has 57 runs (56 points in
    cells of their own, then a run of 8: not shared), wave 1 has 56 (55 points, then a run of 9: shared).  The points sit in the middle of
    distinct cells of the coarsest level (scale 15: cell = floor(15 x + 0.5)), so they are in distinct cells of every finer level too."""
    cells = torch.tensor([[cx, cy, cz] for cz in (3, 9) for cy in range(2, 10) for cx in range(2, 10)], dtype=torch.float32)      # 128 cells
    p = cells / 15.0
    wave0 = torch.cat([p[:56], p[56:57].expand(8, 3)])
    wave1 = torch.cat([p[64:119], p[119:120].expand(9, 3)])
    return torch.cat([wave0, wave1])


def _point_sets():
    if 'points' not in _STATE:
        g = torch.Generator().manual_seed(7)
        sets = {}
        for n in (1, 63, 64, 65, 255, 256, 257, 4099):                 # around a wave and a chunk of 256; coordinates exactly 0.0 and 1.0
            x = torch.rand(n, 3, generator=g)
            x[0] = torch.tensor([0.0, 1.0, 0.5])
            if n > 2:
                x[n // 2] = torch.tensor([1.0, 1.0, 1.0]); x[n - 1] = torch.tensor([0.0, 0.0, 0.0])
            sets[f'uniform{n}'] = x
        d = torch.nn.functional.normalize(torch.randn(64, 3, generator=g), dim=-1)      # 64 rays x 64 lattice samples from one origin: runs share a gather
        t = (torch.arange(64)[None, :] + torch.rand(64, 1, generator=g)) * (0.99 / 64)
        sets['rays'] = (0.5 + 0.5 * d[:, None, :] * t[:, :, None]).reshape(-1, 3)
        sets['identical'] = torch.rand(1, 3, generator=g).expand(64, 3)                # one head
        sets['threshold'] = _threshold_points()
        _STATE['points'] = {k: v.contiguous().cuda() for k, v in sets.items()}
    return _STATE['points']


def test_threshold_points_straddle_the_share_threshold():
    """(what the `threshold` set claims, at the coarsest level: runs counted as the kernel counts them, lane against lane - 1)"""
    x = _threshold_points()
    cell = torch.floor(x * 15.0 + 0.5).to(torch.int64)
    for w, want in ((0, 57), (1, 56)):
        c = cell[64 * w:64 * w + 64]
        heads = 1 + int((c[1:] != c[:-1]).any(dim=1).sum())
        assert heads == want, (w, heads)


@pytest.mark.parametrize('name', sorted(GRIDS))
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_pair_encode_equals_two_single_encodes(dtype, name):
    from perf_amd import ops
    ta, tb, pair = _tables(name, dtype)
    for interpolation in ('Linear', 'Smoothstep'):
        cfg = _grid(name, interpolation)
        for pname, x in _point_sets().items():
            fa, fb = ops.hashgrid_fwd_pair(cfg, x, pair, dtype)
            assert torch.equal(fa, ops.hashgrid_fwd(cfg, x, ta)), (interpolation, pname)
            assert torch.equal(fb, ops.hashgrid_fwd(cfg, x, tb)), (interpolation, pname)
    # capacity 8192, 4099 live rows through n_dev: the rows past the count keep their fill
    x = torch.rand(8192, 3, generator=torch.Generator().manual_seed(8)).cuda()
    n_dev = torch.tensor([4099], dtype=torch.int64, device='cuda')
    fill = torch.full((cfg.n_levels, 8192, 2), 3.0, dtype=ta.dtype, device='cuda')
    fa, fb = ops.hashgrid_fwd_pair(cfg, x, pair, dtype, n_dev=n_dev, out=(fill.clone(), fill.clone()))
    for f, t in ((fa, ta), (fb, tb)):
        assert torch.equal(f[:, :4099], ops.hashgrid_fwd(cfg, x, t, n_dev=n_dev)[:, :4099])
        assert torch.equal(f[:, 4099:], fill[:, 4099:])


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_past_the_chunk_limit_of_a_launch(dtype):
    """n = 4096 x 256 + 300: two chunks more than a launch's 4096 per part, the second one partial -- the workgroups' chunk-stride loop
    runs a second time for them.  Two levels (both hashed at T = 10: two single-level slots) keep it small."""
    from perf_amd import ops
    from perf_amd.grid import GridConfig
    cfg = GridConfig(n_levels=2, log2_hashmap_size=10)
    assert [int(h) for h in cfg.hashed] == [1, 1] and _parts(cfg) == [[(0, None), (1, None)]]
    g = torch.Generator().manual_seed(9)
    ta = ops.cast_params(((torch.rand(cfg.n_params, generator=g) * 2 - 1) * 0.5).cuda(), dtype)
    tb = ops.cast_params(((torch.rand(cfg.n_params, generator=g) * 2 - 1) * 0.5).cuda(), dtype)
    pair = ops.pair_table(cfg, ta.device)
    ops.pair_fill(pair, 0, ta); ops.pair_fill(pair, 1, tb)
    if 'big' not in _STATE:
        _STATE['big'] = torch.rand(4096 * 256 + 300, 3, generator=torch.Generator().manual_seed(10)).cuda()
    x = _STATE['big']
    fa, fb = ops.hashgrid_fwd_pair(cfg, x, pair, dtype)
    assert torch.equal(fa, ops.hashgrid_fwd(cfg, x, ta))
    assert torch.equal(fb, ops.hashgrid_fwd(cfg, x, tb))
