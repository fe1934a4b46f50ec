"""The pair table (include/perf_hip_pair.h) on the GPU: one pair encode equals two single encodes to the bit, for both feature arrays;
perf_pair_fill writes one field's half and leaves the other; what the kernel is not built for is refused before a launch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

PERF_E_INVALID = -1          # include/perf_hip.h
_TABLES = {}


def _setup(dtype, log2_t):
    """(grid of either interpolation -> the same tables) two random 16-bit tables, their pair table; made once per (dtype, T)."""
    from perf_amd import ops
    from perf_amd.grid import GridConfig
    key = (dtype, log2_t)
    if key not in _TABLES:
        cfg = GridConfig(log2_hashmap_size=log2_t)
        g = torch.Generator().manual_seed(11 + log2_t)
        ta = ops.cast_params(((torch.rand(cfg.n_params, generator=g) * 2 - 1) * 0.5).cuda(), dtype)
        tb = ops.cast_params(((torch.rand(cfg.n_params, generator=g) * 2 - 1) * 0.5).cuda(), dtype)
        pair = ops.pair_table(cfg, ta.device)
        ops.pair_fill(pair, 0, ta); ops.pair_fill(pair, 1, tb)
        _TABLES[key] = (ta, tb, pair)
    return _TABLES[key]


def _point_sets():
    g = torch.Generator().manual_seed(5)
    sets = {}
    for n in (1, 255, 257, 4099):                                  # (a) uniform, with coordinates exactly 0.0 and 1.0
        x = torch.rand(n, 3, generator=g)
        x[0] = torch.tensor([0.0, 1.0, 0.5])
        if n > 2:
            x[n // 2] = torch.tensor([1.0, 1.0, 1.0]); x[n - 1] = torch.tensor([0.0, 0.0, 0.0])
        sets[f'uniform{n}'] = x
    d = torch.nn.functional.normalize(torch.randn(64, 3, generator=g), dim=-1)      # (b) 64 rays x 64 lattice samples from one origin
    t = (torch.arange(64)[None, :] + torch.rand(64, 1, generator=g)) * (0.99 / 64)
    sets['rays'] = (0.5 + 0.5 * d[:, None, :] * t[:, :, None]).reshape(-1, 3)
    sets['identical'] = torch.rand(1, 3, generator=g).expand(64, 3)                # (c)
    return {k: v.contiguous().cuda() for k, v in sets.items()}


@pytest.mark.parametrize('log2_t', [18, 14])
@pytest.mark.parametrize('interpolation', ['Linear', 'Smoothstep'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_pair_encode_equals_two_single_encodes(dtype, interpolation, log2_t):
    from perf_amd import ops
    from perf_amd.grid import GridConfig
    cfg = GridConfig(log2_hashmap_size=log2_t, interpolation=interpolation)
    ta, tb, pair = _setup(dtype, log2_t)
    for name, x in _point_sets().items():
        fa, fb = ops.hashgrid_fwd_pair(cfg, x, pair, dtype)
        assert torch.equal(fa, ops.hashgrid_fwd(cfg, x, ta)), name
        assert torch.equal(fb, ops.hashgrid_fwd(cfg, x, tb)), name
    # capacity 8192, 4099 live rows: the rows beyond the count are not touched
    x = torch.rand(8192, 3, generator=torch.Generator().manual_seed(6)).cuda()
    n_dev = torch.tensor([4099], dtype=torch.int64, device='cuda')
    fill = torch.full((16, 8192, 2), 3.0, dtype=ta.dtype, device='cuda')
    fa, fb = ops.hashgrid_fwd_pair(cfg, x, pair, dtype, n_dev=n_dev, out=(fill.clone(), fill.clone()))
    for f, t in ((fa, ta), (fb, tb)):
        assert torch.equal(f[:, :4099], ops.hashgrid_fwd(cfg, x, t, n_dev=n_dev)[:, :4099])
        assert torch.equal(f[:, 4099:], fill[:, 4099:])


@pytest.mark.parametrize('field', [0, 1])
def test_pair_fill_writes_one_field(field):
    from perf_amd import ops
    from perf_amd.grid import GridConfig
    cfg = GridConfig(log2_hashmap_size=10)
    g = torch.Generator().manual_seed(2)
    pair = torch.randint(-2 ** 31, 2 ** 31 - 1, (cfg.total, 2), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    before = pair.clone()
    # a table behind a network part of odd length: 4-byte, not 16-byte aligned
    w16 = torch.randn(4161 * 2 + cfg.n_params, generator=g).to(torch.bfloat16).cuda()
    table = w16[4161 * 2:]
    assert table.data_ptr() % 16 != 0
    ops.pair_fill(pair, field, table)
    assert torch.equal(pair[:, field].contiguous().view(torch.bfloat16), table)
    assert torch.equal(pair[:, 1 - field], before[:, 1 - field])


def test_refusals_happen_before_a_launch():
    from perf_amd import _lib
    from perf_amd.grid import GridConfig
    lib = _lib.load()
    fake = ctypes.c_void_p(64)       # never dereferenced

    def fwd(cfg, **kw):
        a = {'x': fake, 'pair': fake, 'fa': fake, 'fb': fake, 'dtype': 0}
        a.update(kw)
        d = cfg.desc()
        rc = lib.perf_hashgrid_fwd_pair(ctypes.byref(d), a['x'], a['pair'], a['fa'], a['fb'], 64, None, a['dtype'], None)
        return rc, (lib.perf_last_error() or b'').decode()

    rc, msg = fwd(GridConfig(layout='line_local', sb_shift=(3, 3, 2)))
    assert rc == PERF_E_INVALID and 'tcnn' in msg, msg
    rc, msg = fwd(GridConfig(n_levels=20))
    assert rc == PERF_E_INVALID and '20 levels' in msg, msg
    for kw in ({'x': None}, {'pair': None}, {'fa': None}, {'fb': None}):
        rc, msg = fwd(GridConfig(), **kw)
        assert rc == PERF_E_INVALID and 'NULL pointer' in msg, (kw, msg)
    rc, msg = fwd(GridConfig(), dtype=7)
    assert rc == PERF_E_INVALID and 'dtype' in msg, msg
    rc, msg = fwd(GridConfig(), pair=ctypes.c_void_p(68))
    assert rc == PERF_E_INVALID and '8-byte aligned' in msg, msg
    assert lib.perf_pair_fill(None, 0, fake, 64, None) == PERF_E_INVALID
    assert lib.perf_pair_fill(fake, 2, fake, 64, None) == PERF_E_INVALID
    torch.cuda.synchronize()
