"""The fixed-point table gradient TO THE BIT on the paths plan_tiles picks for grids other than the default one, and with a live
gradient outside the unit cube -- against oracle/perf_oracle.py:grid_fixed_fields, as tests/test_gpu_exact_gradients.py does for the
default grid inside the cube:

  * byte-code owners (hashed levels of 17..255 tiles), bitmap owners (tile_bitmap_kernel: hashed levels of 256..2048 tiles, dense
    levels from 32 tiles on), the replica counts of the dense levels of a grid that has bitmap levels (plan_tiles: large_grid);
  * the 64-bit fixed-point global-atomics scatter and its unfix (hashgrid_bwd_atomic_fixed_kernel, hashgrid_bwd_unfix_kernel): their
    own packing and unpacking of the two fields, their own maximum for the headroom loop;
  * hashed levels with res + 2 >= 16384, where the association of the weight product switches per sample at cell x = 16383;
  * the escape of a coded, bit-row or bitmap level to the generic owners when a sample outside the cube carries a gradient: uint32
    index wrap on hashed levels, the modulo on dense ones, cell x = -1 as uint32.

Which path a level takes is restated here from plan_tiles' thresholds (_plan) and every grid states the list it expects, so that a
reader sees the path is really hit; a batch states which of its levels escape (_escaped).  Every comparison is an equality, except the
fp32 mode's at the end, whose bound is derived in its docstring."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import perf_oracle as O  # noqa: E402
from tests.test_gpu_exact_gradients import (FP, FLAG_LEVEL, _amax24, _assert_same_fields, _assert_table, _check_raw, _dev_shifts,  # noqa: E402
                                            _dfeat, _ray_points, _shifts_for)

TILE = 16384                    # hashgrid_bwd.hip: kTileEntries
BITMAP_MAX_TILES = 2048         # kBitmapMaxTiles
BITMAP_MIN_DENSE_TILES = 32     # kBitmapMinDenseTiles
MASK_TILES = 16                 # kMaskTiles: hashed levels up to here keep bit rows, beyond byte codes
BIT_ROW_MIN_SAMPLES = 256       # kCodeSamplesPerBlock: below it a call's bit-row levels take the position-streaming owners
INTERPS = ['Linear', 'Smoothstep']


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from perf_amd import ops as _ops
    return _ops


def _plan(cfg, n, use_codes=True):
    """plan_tiles / plan_codes of a fixed-point call restated from GridConfig: per level (tiles, path, replicas).  use_codes=False is a
    workspace without room for the tile codes and the bitmaps.  Paths:
      'single'   one dense tile, position-streaming (run-merging) owners         'generic'  position-streaming owners, several tiles
      'dense'    dense level, code-streaming owners                              'bits'     hashed, <= 16 tiles, one bit row per tile
      'bytes'    hashed, 17..255 tiles, a byte per (y,z) combination             'bitmap'   owners that read tile_bitmap_kernel's rows
      'atomics'  the global-atomics scatter (fixed point: 64-bit words, then hashgrid_bwd_unfix_kernel)
    replicas: of the dense levels of a grid with bitmap levels (large_grid); None where this file does not restate them."""
    bitmap_tiles = BITMAP_MAX_TILES if use_codes else 0
    tiles, wide = [], []
    for l in range(cfg.n_levels):
        nt = -(-int(cfg.size[l]) // TILE)
        if not cfg.hashed[l]:
            nt = 1 << (nt - 1).bit_length()             # dense ownership is a bit field of the index
        tiles.append(nt)
        wide.append(int(cfg.res[l]) + 2 >= TILE)       # "(y,z) decides the tile" needs gx + 1 < 16384
    takes_bitmap = [tiles[l] <= bitmap_tiles and ((tiles[l] > 255 and not wide[l]) if cfg.hashed[l] else tiles[l] >= BITMAP_MIN_DENSE_TILES)
                    for l in range(cfg.n_levels)]
    large_grid = any(takes_bitmap)
    plan = []
    for l in range(cfg.n_levels):
        nt, hashed = tiles[l], bool(cfg.hashed[l])
        if takes_bitmap[l]:
            plan.append((nt, 'bitmap', 1))
        elif nt > (255 if hashed else 64):
            plan.append((nt, 'atomics', None))
        elif hashed:
            coded = use_codes and 2 <= nt and not wide[l] and not (nt <= MASK_TILES and n < BIT_ROW_MIN_SAMPLES)
            plan.append((nt, ('bits' if nt <= MASK_TILES else 'bytes') if coded else 'generic', 1))
        else:
            r = {1: 8, 2: 8, 4: 6, 8: 4}.get(nt, 2) if large_grid else None
            plan.append((nt, 'single' if nt == 1 else ('dense' if use_codes else 'generic'), r))
    return plan


# name -> (GridConfig arguments, the plan expected with room for codes and bitmaps, the plan expected without)
H16 = [(16, 'bits', 1)] * 12
G16 = [(16, 'generic', 1)] * 12
GRIDS = {
    'default': (dict(),
                [(1, 'single', None), (1, 'single', None), (4, 'dense', None), (8, 'dense', None)] + H16,
                [(1, 'single', None), (1, 'single', None), (4, 'generic', None), (8, 'generic', None)] + G16),
    # res 8192: byte codes; res 16384 and 32768: "(y,z) decides the tile" fails inside the cube, generic owners
    't19fine': (dict(n_levels=3, log2_hashmap_size=19, base_resolution=8192, per_level_scale=2.0),
                [(32, 'bytes', 1), (32, 'generic', 1), (32, 'generic', 1)],
                [(32, 'generic', 1)] * 3),
    't18fine': (dict(n_levels=4, log2_hashmap_size=18, base_resolution=4096, per_level_scale=2.0),
                [(16, 'bits', 1), (16, 'bits', 1), (16, 'generic', 1), (16, 'generic', 1)],
                [(16, 'generic', 1)] * 4),
    # dense 16 tiles coded with the large grid's 2 replicas, dense 128 tiles and three hashed levels of 256 tiles on bitmaps
    't22': (dict(n_levels=5, log2_hashmap_size=22, base_resolution=64, per_level_scale=2.0),
            [(16, 'dense', 2), (128, 'bitmap', 1), (256, 'bitmap', 1), (256, 'bitmap', 1), (256, 'bitmap', 1)],
            [(16, 'generic', None), (128, 'atomics', None), (256, 'atomics', None), (256, 'atomics', None), (256, 'atomics', None)]),
    't22b96': (dict(n_levels=3, log2_hashmap_size=22, base_resolution=96, per_level_scale=2.0),
               [(64, 'bitmap', 1), (256, 'bitmap', 1), (256, 'bitmap', 1)],
               [(64, 'generic', None), (256, 'atomics', None), (256, 'atomics', None)]),
    # dense levels only: 2, 8 and 16 tiles with the large grid's 8, 4 and 2 replicas, 64 tiles on bitmaps
    't20': (dict(n_levels=4, log2_hashmap_size=20, base_resolution=32, per_level_scale=1.3819),
            [(2, 'dense', 8), (8, 'dense', 4), (16, 'dense', 2), (64, 'bitmap', 1)],
            [(2, 'generic', None), (8, 'generic', None), (16, 'generic', None), (64, 'generic', None)]),
    # res 16384 and 32768 at 256 tiles: neither coded nor bitmap owners -- ALWAYS the global atomics
    't22fine': (dict(n_levels=4, log2_hashmap_size=22, base_resolution=4096, per_level_scale=2.0),
                [(256, 'bitmap', 1), (256, 'bitmap', 1), (256, 'atomics', None), (256, 'atomics', None)],
                [(256, 'atomics', None)] * 4),
    # the grid of tests/test_gpu_ops.py:test_hashgrid_bwd_large_levels: hashed levels of 512 tiles
    't23': (dict(n_levels=6, log2_hashmap_size=23, base_resolution=32, per_level_scale=2.0),
            [(2, 'dense', 8), (16, 'dense', 2), (128, 'bitmap', 1), (512, 'bitmap', 1), (512, 'bitmap', 1), (512, 'bitmap', 1)],
            [(2, 'generic', None), (16, 'generic', None), (128, 'atomics', None), (512, 'atomics', None), (512, 'atomics', None),
             (512, 'atomics', None)]),
}
BITMAP_GRIDS = ('t22', 't22b96', 't20', 't22fine', 't23')
N, N_LIVE = 5003, 3970                           # ragged against the 256 and 1,024 samples of a pre-pass block
BATCH_SEED = {'uniform': 1, 'rays': 2, 'outside': 3, 'tiny1': 4, 'tiny255': 5, 'live': 6}
# every batch of a grid with a different sign pattern; 'neg_pos' (the borrow between the packed fields) at least once per grid
BATCH_SIGNS = {'uniform': 'neg_pos', 'rays': 'mixed', 'outside': 'neg_pos', 'tiny1': 'neg_pos', 'tiny255': 'pos_neg', 'live': 'zero_level'}
_STATE = {}


def _grid(name, interp):
    from perf_amd.grid import GridConfig
    kw, with_codes, without = GRIDS[name]
    cfg = GridConfig(interpolation=interp, **kw)
    lv = O.grid_levels(cfg.n_levels, 2, cfg.log2_hashmap_size, cfg.base_resolution, cfg.per_level_scale)
    assert lv.total == cfg.total and np.array_equal(lv.size, cfg.size) and np.array_equal(lv.hashed, cfg.hashed.astype(bool))
    assert _plan(cfg, N) == with_codes, (name, _plan(cfg, N))
    assert _plan(cfg, N, use_codes=False) == without, (name, _plan(cfg, N, use_codes=False))
    assert cfg.total * 8 <= 221 << 20                                   # bytes of the table on the device
    return cfg, lv


def _cell_x(x, lv, l):
    """cell x of every sample as uint32 (grid_fixed_weights' own rule, from grid_pos)"""
    return np.floor(O.grid_pos(np.ascontiguousarray(x[:, 0], np.float32), lv.scale[l])).astype(np.int64) & 0xFFFFFFFF


def _escaped(cfg, lv, x, dfeat, n_live, n, use_codes=True):
    """the plan of a call on THIS batch: a bit-row, byte-code or hashed bitmap level whose pre-pass meets a live sample with a gradient
    and cell x >= 16383 (as uint32: left of the cube, or far to the right) goes back to the generic owners, whole"""
    xn = x[:n_live].numpy()
    out = []
    for l, (nt, path, r) in enumerate(_plan(cfg, n, use_codes)):
        if path in ('bits', 'bytes') or (path == 'bitmap' and cfg.hashed[l]):
            live = dfeat[l, :n_live].numpy().any(1)
            if (live & (_cell_x(xn, lv, l) >= O.PAIR_PATH_MAX_CELL_X)).any():
                path = 'generic'
        out.append(path)
    return out


def _batch(grid, batch, interp):
    """(x, n_live, weights of the live rows per level): made once per (grid, batch, interpolation) and left unchanged"""
    key = (grid, batch, interp)
    if key not in _STATE:
        cfg, lv = _grid(grid, interp)
        g = torch.Generator().manual_seed(BATCH_SEED[batch])
        n_live = None
        if batch == 'rays':
            x = _ray_points(40000, g)                   # bursts on a few tiles, runs in one cell
        elif batch in ('tiny1', 'tiny255'):
            x = torch.rand(int(batch[4:]), 3, generator=g)      # below one bit-row slot, below one pre-pass block
        else:
            x = torch.rand(N, 3, generator=g)
        if batch == 'outside':                          # all with their gradients kept
            x[::7, 0] = -0.25
            x[5::11, 0] = 9.5
            x[3::13, 1] = -3.0
            x[4::17, 2] = 1.75
        if batch == 'live':
            x[N_LIVE:] = float('nan')                   # rows past the live count must not be read
            n_live = N_LIVE
        n_live = x.shape[0] if n_live is None else n_live
        xn = x[:n_live].numpy()
        if batch not in ('tiny1', 'tiny255'):
            inside = ((xn >= 0) & (xn <= 1)).all(1)
            for l in range(lv.n_levels):
                if not lv.hashed[l]:
                    continue
                pair = _cell_x(xn, lv, l) < O.PAIR_PATH_MAX_CELL_X
                if int(lv.res[l]) == 32768:
                    # the association switches INSIDE the level, with no help from points outside the cube
                    assert (pair & inside).sum() >= inside.sum() // 4 and (~pair & inside).sum() >= inside.sum() // 4, (grid, batch, l)
                if batch == 'outside':                  # both associations on every hashed level
                    assert pair.sum() >= 0.05 * n_live and (~pair).sum() >= 0.05 * n_live, (grid, l, int(pair.sum()))
        weights = [O.grid_fixed_weights(xn, lv, l, interp) for l in range(lv.n_levels)]
        _STATE[key] = (x, n_live, weights)
    return _STATE[key]


def _gradient(grid, batch, interp, signs=None):
    cfg, lv = _grid(grid, interp)
    x, n_live, weights = _batch(grid, batch, interp)
    g = torch.Generator().manual_seed(100 + BATCH_SEED[batch] + len(grid))
    dfeat = _dfeat(cfg, x, g, BATCH_SIGNS[batch] if signs is None else signs, outside=True)
    n = x.shape[0]
    escaped = _escaped(cfg, lv, x, dfeat, n_live, n)
    planned = [p for _, p, _ in _plan(cfg, n)]
    if batch == 'outside':                              # every coded hashed level escapes; the dense ones wrap in place
        assert all(e == 'generic' for e, p, h in zip(escaped, planned, cfg.hashed) if h and p != 'atomics'), (grid, escaped)
        assert all(e == p for e, p, h in zip(escaped, planned, cfg.hashed) if not h)
    else:                                               # (a level with res + 2 >= 16384 is not coded in the first place)
        assert escaped == planned, (grid, batch, escaped)
    return cfg, lv, x, n_live, weights, dfeat


# ---- (a) given units, raw fields ---------------------------------------------------------------------------------------------------
RAW_GRIDS = ('t18fine', 't19fine', 't22', 't22b96', 't20', 't23')
RAW_CASES = [('default', 'outside')] + [(gr, b) for gr in RAW_GRIDS for b in ('uniform', 'rays', 'outside', 'tiny1', 'tiny255', 'live')]


@pytest.mark.parametrize('interp', INTERPS)
@pytest.mark.parametrize('grid,batch', RAW_CASES, ids=[f'{gr}-{b}' for gr, b in RAW_CASES])
def test_raw_fields_equal_the_integer_oracle(ops, grid, batch, interp):
    """three unit sets (fine, 10 bits coarser, unit = largest contribution), the overflow flag stays 0.  Grids with bitmap levels run
    with their bitmaps only: without them those levels are on the global atomics, which have no raw fields (refused: below)."""
    cfg, lv, x, n_live, weights, dfeat = _gradient(grid, batch, interp)
    codes = (True,) if grid in BITMAP_GRIDS else (True, False)
    _check_raw(ops, cfg, lv, x, dfeat, interp, n_live, f'{grid} / {batch}', codes=codes, weights=weights)


def test_raw_fields_are_refused_for_levels_on_the_global_atomics(ops):
    cfg, lv, x, n_live, weights, dfeat = _gradient('t22', 'uniform', 'Linear')
    assert 'atomics' in [p for _, p, _ in _plan(cfg, x.shape[0], use_codes=False)]
    with pytest.raises(Exception, match='raw fields / given units are not available for levels on the global-atomics scatter'):
        ops.hashgrid_bwd(cfg, x.cuda(), dfeat.cuda(), shifts=_dev_shifts([8] * cfg.n_levels), raw_fields=True, use_codes=False)
    cfg, lv, x, n_live, weights, dfeat = _gradient('t22fine', 'uniform', 'Linear')      # (with its bitmaps, too: res 16384 and 32768)
    with pytest.raises(Exception, match='raw fields / given units are not available for levels on the global-atomics scatter'):
        ops.hashgrid_bwd(cfg, x.cuda(), dfeat.cuda(), shifts=_dev_shifts([8] * cfg.n_levels), raw_fields=True)


# ---- (b) derived units, the float table, the closed loop ------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', INTERPS)
@pytest.mark.parametrize('batch', ['live', 'outside', 'rays'])
@pytest.mark.parametrize('grid', list(GRIDS))
def test_derived_units_and_the_headroom_loop(ops, grid, batch, interp):
    """without state (the static fan-in guess); with a fresh state; then the gradient x 8 with the state the first call left -- on the
    atomics levels that state comes from hashgrid_bwd_unfix_kernel's own maximum.  Grids with bitmap levels also without room for the
    bitmaps: their large levels on the 64-bit atomics scatter and its unfix, held to the oracle directly."""
    cfg, lv, x, n_live, weights, base = _gradient(grid, batch, interp, signs='neg_pos' if batch == 'live' else 'mixed')
    L, n = cfg.n_levels, x.shape[0]
    xc = x.cuda()
    n_dev = None if n_live == n else torch.tensor([n_live], dtype=torch.int64, device='cuda')
    flag = ops.overflow_flag(xc.device)

    def want(d, adj):
        amax = _amax24(d, L)
        shifts = [FP.fixed_point_shift(float(amax[l]), n_live, int(cfg.size[l]), None if adj is None else adj[l]) for l in range(L)]
        fields = O.grid_fixed_fields(x, d, lv, shifts, interp, n_live, weights=weights)
        fm = O.fixed_field_max(fields, lv)
        assert int(fm.max()) < FLAG_LEVEL, fm
        return amax.cuda(), shifts, fields, fm

    static = want(base, None)
    first = want(base, [0] * L)
    adj1 = [FP.headroom_feedback(0, int(first[3][l])) for l in range(L)]
    second = want(base * 8.0, adj1)                     # (a power of two: the same fp32 mantissas)
    adj2 = [FP.headroom_feedback(adj1[l], int(second[3][l])) for l in range(L)]
    for use_codes in ((True, False) if grid in BITMAP_GRIDS else (True,)):
        what = f'{grid} / {batch} / use_codes={use_codes}'
        flag.zero_()
        amax, shifts, fields, _ = static
        _assert_table(ops.hashgrid_bwd(cfg, xc, base.cuda(), level_absmax=amax, n_dev=n_dev, use_codes=use_codes), fields, lv, shifts, what + ', no state')
        hr = ops.headroom_state(xc.device)
        for call, (d, (amax, shifts, fields, fm), adj) in enumerate(((base, first, adj1), (base * 8.0, second, adj2))):
            got = ops.hashgrid_bwd(cfg, xc, d.cuda(), level_absmax=amax, n_dev=n_dev, use_codes=use_codes, hr_state=hr)
            _assert_table(got, fields, lv, shifts, what + f', call {call}')
            state = hr.cpu().tolist()
            assert state[:L] == adj, (what, call, state[:L], adj)
            assert not any(state[24:24 + L]) and state[48] == 0, (what, call, state[24:])        # maxima and ticket consumed
        assert int(flag.item()) == 0, what
    # (with the start bias the largest field of a sparse level lands on either side of the band's lower edge, 2^21: across the cases
    #  about half of the levels -- atomics levels among them -- leave the first call with an adjustment of -1, the others with 0)


# ---- (c) the data-parallel pieces on bitmap levels ------------------------------------------------------------------------------------
def test_two_raw_tables_added_and_unfixed_on_a_slice_of_bitmap_levels(ops):
    cfg, lv, x, n, weights, dfeat = _gradient('t22', 'rays', 'Linear', signs='neg_pos')
    cut = 11003
    shifts = _shifts_for(x, dfeat, lv, 'Linear', n, weights)
    want = O.grid_fixed_fields(x, dfeat, lv, shifts, weights=weights)
    sh = _dev_shifts(shifts)
    total = torch.zeros(cfg.n_params, dtype=torch.int32, device='cuda')
    for lo, hi in ((0, cut), (cut, n)):
        f = ops.hashgrid_bwd(cfg, x[lo:hi].contiguous().cuda(), dfeat[:, lo:hi].contiguous().cuda(), shifts=sh, raw_fields=True)
        total += f.view(torch.int32)                    # wrapping int32, as the reduce-scatter adds
    _assert_same_fields(total.view(-1, 2).cpu().numpy(), want, lv, 'sum of two raw tables')
    # a rank's slice: from inside the dense bitmap level to inside the second hashed bitmap level
    plan = _plan(cfg, n)
    assert plan[1][1] == 'bitmap' and not cfg.hashed[1] and plan[3][1] == 'bitmap' and cfg.hashed[2] and cfg.hashed[3]
    e_lo = int(cfg.offset[1]) + 1000001
    e_hi = int(cfg.offset[3]) + 2000003
    shard = total.view(-1, 2)[e_lo:e_hi].clone()
    field_max = torch.full((24,), -1, dtype=torch.int32, device='cuda')
    flag = ops.overflow_flag('cuda'); flag.zero_()
    ops.fixed_unfix(cfg, shard, e_lo, e_hi, sh, field_max=field_max, flag=flag)
    got = shard.view(torch.float32).cpu().numpy()
    assert np.array_equal(got, O.fixed_fields_to_float(want, lv, shifts)[e_lo:e_hi])
    fm = O.fixed_field_max(want, lv, e_lo, e_hi)
    assert field_max.cpu().tolist() == fm.tolist() + [0] * (24 - cfg.n_levels)
    assert fm[0] == 0 and fm[1:4].min() > 0 and fm[4] == 0 and int(flag.item()) == 0


# ---- (e) fp32 mode: one inequality -------------------------------------------------------------------------------------------------------
def _fp32_terms(lv, weights, dfeat, n_live, levels=None):
    """per entry and feature: the float64 sum T of w * g (w: the fp32 weight of grid_fixed_weights), the sum S of |w g|, and the
    number of contributions cnt -- a sample without gradient contributes nothing in the kernels and a zero here"""
    T = np.zeros((lv.total, 2), np.float64)
    S = np.zeros((lv.total, 2), np.float64)
    cnt = np.zeros(lv.total, np.int64)
    for l in (range(lv.n_levels) if levels is None else levels):
        idx, w = weights[l]
        lo, size = int(lv.offset[l]), int(lv.size[l])
        g = dfeat[l, :n_live].numpy().astype(np.float64)
        flat = idx[:n_live].astype(np.int64).reshape(-1)
        cnt[lo:lo + size] = np.bincount(flat, minlength=size)
        for k in range(2):
            p = (w[:n_live].astype(np.float64) * g[:, k, None]).reshape(-1)
            T[lo:lo + size, k] = np.bincount(flat, weights=p, minlength=size)
            S[lo:lo + size, k] = np.bincount(flat, weights=np.abs(p), minlength=size)
    return T, S, cnt


def _assert_fp32_bound(got, T, S, cnt, lv, levels, what):
    worst = {}
    for l in levels:
        lo, hi = int(lv.offset[l]), int(lv.offset[l]) + int(lv.size[l])
        err = np.abs(got[lo:hi].astype(np.float64) - T[lo:hi])
        bound = (cnt[lo:hi, None] + 3) * 2.0 ** -24 * S[lo:hi]
        assert not got[lo:hi][S[lo:hi] == 0].any(), (what, l)
        ratio = np.where(S[lo:hi] > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
        worst[l] = float(ratio.max())
    print(f'fp32 bound, {what}: largest |error| / bound per level ' + ' '.join(f'{l}:{r:.3f}' for l, r in worst.items()))
    assert max(worst.values()) <= 1.0, (what, worst)
    assert max(worst.values()) > 0.0                    # (the check has something to look at)
    return worst


FP32_CASES = [('t22', 'uniform'), ('t22', 'outside'), ('t22fine', 'uniform'), ('t22fine', 'outside'), ('default', 'outside')]


@pytest.mark.parametrize('interp', INTERPS)
@pytest.mark.parametrize('grid,batch', FP32_CASES, ids=[f'{gr}-{b}' for gr, b in FP32_CASES])
def test_fp32_mode_within_the_bound_of_a_sum_in_any_order(ops, grid, batch, interp):
    """Without level_absmax the kernels add fl32(w g) in fp32, in an order nobody fixes (LDS atomics, replica slabs, global atomics).
    Per entry, with T the float64 sum of the cnt products w g and u = 2^-24:

        |kernel - T| <= (cnt + 3) u sum |w g|

    -- the first-order bound of a sum of cnt terms in ANY order is (cnt - 1) u sum |terms|; one more u is the rounding of each product;
    two more cover the last bit of w, where the kernels' two associations of the three-factor product and the order of a replica's
    slab sum may differ from the oracle's statement.  The bound is derived, not measured: the largest ratio per level is printed.
    (On an MI355X: 0.29-0.40 on every level whose owners use the association the oracle names; 0.66-0.99 on hashed levels on the fp32
    global-atomics scatter, which forms (wx wy) wz for every sample -- an entry with ONE contribution then carries the product's
    rounding and the last bit of w against a bound of 4 u.  Two roundings per association allow up to 4 u between the two in theory;
    on these batches the last bit is what differs.)"""
    cfg, lv, x, n_live, weights, dfeat = _gradient(grid, batch, interp)
    T, S, cnt = _fp32_terms(lv, weights, dfeat, n_live)
    xc, dc = x.cuda(), dfeat.cuda()
    for use_codes in ((True, False) if grid in BITMAP_GRIDS else (True,)):
        got = ops.hashgrid_bwd(cfg, xc, dc, use_codes=use_codes).cpu().numpy().reshape(-1, 2)
        _assert_fp32_bound(got, T, S, cnt, lv, range(cfg.n_levels), f'{grid} / {batch} / {interp} / use_codes={use_codes}')


# ---- (d) accumulate=True on a zeroed table ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', INTERPS)
@pytest.mark.parametrize('grid', ['t22', 't22fine'])
def test_accumulate_on_a_zeroed_table_is_the_overwriting_call(ops, grid, interp):
    """Both calls are fixed-point calls -- for the levels on LDS owners.  perf_hashgrid_bwd sends ACCUMULATING atomics levels through
    the fp32 scatter (the 64-bit words need the level's slice to themselves): the res 16384 and 32768 levels of 't22fine' are then an
    fp32 result, held to the fp32 bound above instead of to equality."""
    cfg, lv, x, n_live, weights, dfeat = _gradient(grid, 'uniform', interp)
    L = cfg.n_levels
    amax = _amax24(dfeat, L)
    shifts = [FP.fixed_point_shift(float(amax[l]), n_live, int(cfg.size[l])) for l in range(L)]
    fields = O.grid_fixed_fields(x, dfeat, lv, shifts, interp, n_live, weights=weights)
    xc, dc = x.cuda(), dfeat.cuda()
    over = torch.zeros(cfg.n_params, device='cuda')
    ops.hashgrid_bwd(cfg, xc, dc, out=over, level_absmax=amax.cuda())
    _assert_table(over, fields, lv, shifts, f'{grid} overwrite')
    acc = torch.zeros(cfg.n_params, device='cuda')
    ops.hashgrid_bwd(cfg, xc, dc, out=acc, accumulate=True, level_absmax=amax.cuda())
    on_atomics = [l for l, (_, p, _) in enumerate(_plan(cfg, x.shape[0])) if p == 'atomics']
    assert on_atomics == ([2, 3] if grid == 't22fine' else [])
    a, o = acc.cpu().numpy().reshape(-1, 2), over.cpu().numpy().reshape(-1, 2)
    for l in range(L):
        lo, hi = int(lv.offset[l]), int(lv.offset[l]) + int(lv.size[l])
        if l not in on_atomics:
            assert np.array_equal(a[lo:hi], o[lo:hi]), (grid, l)
    if on_atomics:
        T, S, cnt = _fp32_terms(lv, weights, dfeat, n_live, on_atomics)
        _assert_fp32_bound(a, T, S, cnt, lv, on_atomics, f'{grid} / accumulate / {interp}')
