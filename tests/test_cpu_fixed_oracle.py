"""CPU tests (no GPU) of the integer oracle of the fixed-point table gradient (oracle/perf_oracle.py:grid_fixed_fields): against a
float64 sum of the same contributions, for rounding bias, for order and partition independence, and the overlap fold; its corner
indices and its association rule against a slow restatement in Python integers on levels with res + 2 >= 16384 and on positions
outside the unit cube.  The GPU tests (tests/test_gpu_exact_gradients.py, tests/test_gpu_exact_gradients_large.py) demand equality
with it to the bit, so it has to be right on its own."""
import math
from fractions import Fraction

import numpy as np
import torch

from oracle import perf_oracle as O

F32 = np.float32


def _case(lv, n, seed, scale=1e-3):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g).numpy()
    x[-1] = 1.0
    x[-2] = 0.0
    x[:16, 0] = (np.arange(16) + 0.5) / float(lv.scale[min(3, lv.n_levels - 1)])       # on cell faces of one level
    dfeat = (torch.randn(lv.n_levels, n, 2, generator=g) * scale).numpy()
    # units: the largest contribution of a level spans 2^16 of them, so that the fp32 rounding of w * g (2^-24 relative) stays below
    # 2^-8 units per contribution and the bound below is about the rint alone
    shifts = [16 - int(np.ceil(np.log2(np.abs(dfeat[l]).max()))) for l in range(lv.n_levels)]
    return x, dfeat, shifts


def _float64_sum(x, dfeat, lv, shifts, interp):
    """(sum of w * g * 2^shift in float64, number of contributions) per entry and feature, no rounding to units"""
    ref = np.zeros((lv.total, 2), np.float64)
    cnt = np.zeros(lv.total, np.int64)
    for l in range(lv.n_levels):
        idx, w = O.grid_fixed_weights(x, lv, l, interp)
        lo, size = int(lv.offset[l]), int(lv.size[l])
        for c in range(8):
            ok = idx[:, c] < size
            ic = idx[ok, c].astype(np.int64) + lo
            np.add.at(ref, ic, w[ok, c, None].astype(np.float64) * dfeat[l][ok].astype(np.float64) * 2.0 ** shifts[l])
            np.add.at(cnt, ic, 1)
    if lv.layout == 'line_overlap':
        O.fold_overlap_copies(ref, lv)
        c2 = cnt[:, None].copy()
        O.fold_overlap_copies(c2, lv)
        cnt = c2[:, 0]
    return ref, cnt


def test_integer_fields_against_a_float64_sum_and_without_rounding_bias():
    for interp in ('Linear', 'Smoothstep'):
        lv = O.grid_levels(n_levels=8, log2_hashmap_size=14)
        x, dfeat, shifts = _case(lv, 6001, seed=3)
        got = O.grid_fixed_fields(x, dfeat, lv, shifts, interp)
        assert got.dtype == np.int64 and got.shape == (lv.total, 2)
        ref, cnt = _float64_sum(x, dfeat, lv, shifts, interp)
        err = got.astype(np.float64) - ref
        # every contribution is off by at most half a unit (rint) plus the fp32 rounding of its product
        assert (np.abs(err) <= 0.5 * cnt[:, None] + 1).all()
        assert not got[cnt == 0].any()
        for l in range(lv.n_levels):
            lo, hi = int(lv.offset[l]), int(lv.offset[l]) + int(lv.size[l])
            e = err[lo:hi][cnt[lo:hi] > 0].reshape(-1)
            assert e.size > 500
            # round to nearest even has no bias: the signed mean over a level's entries within 3 standard errors of zero
            # (truncation would shift every contribution by half a unit towards zero / minus infinity)
            assert abs(e.mean()) <= 3.0 * e.std() / np.sqrt(e.size), (interp, l, e.mean(), e.std(), e.size)
            assert e.std() > 0.1                                          # ... and the check has something to look at


def test_a_contribution_is_rounded_to_nearest_even_not_truncated():
    lv = O.grid_levels(n_levels=1, log2_hashmap_size=14)
    s = float(lv.scale[0])
    x = np.array([[0.5 / s, 0.5 / s, 0.5 / s]], F32)                      # grid position (1, 1, 1) exactly: corner 0 has weight 1
    idx, w = O.grid_fixed_weights(x, lv, 0)
    assert w[0, 0] == 1.0 and not w[0, 1:].any()
    for g, want in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (0.75, 1), (-0.75, -1), (0.25, 0), (3.0, 3)):
        d = np.array([[[g, -g]]], F32)
        f = O.grid_fixed_fields(x, d, lv, [0])
        assert f[int(idx[0, 0])].tolist() == [want, -want], (g, f[int(idx[0, 0])])
        assert np.abs(f).sum() == 2 * abs(want)
        assert O.grid_fixed_fields(x, d, lv, [3])[int(idx[0, 0]), 0] == int(g * 8)       # exact in finer units


def test_integer_fields_do_not_depend_on_order_partition_or_live_capacity():
    lv = O.grid_levels()                                                   # the default L16 / T18 grid
    x, dfeat, shifts = _case(lv, 3001, seed=5)
    whole = O.grid_fixed_fields(x, dfeat, lv, shifts)
    perm = np.random.default_rng(1).permutation(x.shape[0])
    assert np.array_equal(O.grid_fixed_fields(x[perm], dfeat[:, perm], lv, shifts), whole)
    cut = 1234
    a = O.grid_fixed_fields(x[:cut], dfeat[:, :cut], lv, shifts)
    b = O.grid_fixed_fields(x[cut:], dfeat[:, cut:], lv, shifts)
    assert np.array_equal(a + b, whole)
    assert np.array_equal(O.grid_fixed_fields(x, dfeat, lv, shifts, n_live=cut), a)      # rows past the live count do not exist
    assert not O.grid_fixed_fields(x, dfeat, lv, shifts, n_live=0).any()
    # the hashed levels of this grid use the pair association, the dense ones the generic one: they differ in the last bit of w
    _, wd = O.grid_fixed_weights(x, lv, 0)
    _, wh = O.grid_fixed_weights(x, lv, 15)
    assert lv.hashed[15] and not lv.hashed[0]
    for w in (wd, wh):
        assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() < 1e-6
    # the negative-value convention of the level maxima: -(v + 1)
    t = np.zeros((lv.total, 2), np.int64)
    t[int(lv.offset[2]) + 5, 1] = -7
    t[int(lv.offset[3]), 0] = 9
    m = O.fixed_field_max(t, lv)
    assert m[2] == 6 and m[3] == 9 and m.sum() == 15
    assert O.fixed_field_max(t, lv, int(lv.offset[3]) + 1, lv.total)[3] == 0
    # int32 -> fp32 rounds to nearest even above 2^24
    t[0, 0] = (1 << 24) + 1
    t[1, 0] = -((1 << 24) + 3)
    fl = O.fixed_fields_to_float(t, lv, [4] * 16)
    assert fl[0, 0] == F32(2.0 ** 20) and fl[1, 0] == -F32((1 << 24) + 4) / 16


def test_the_two_associations_differ_and_each_is_what_it_says():
    lv = O.grid_levels()
    rng = np.random.default_rng(9)
    x = rng.random((4000, 3)).astype(F32)
    for l, hashed in ((1, False), (12, True)):
        assert bool(lv.hashed[l]) == hashed
        idx, w = O.grid_fixed_weights(x, lv, l)
        _, f = O.grid_corner_indices(x, lv, l)
        wx, wy, wz = F32(1) - f[:, 0], f[:, 1], F32(1) - f[:, 2]          # corner 2: (0, 1, 0)
        generic, pair = (wx * wy) * wz, wx * (wy * wz)
        assert (generic != pair).any()                                     # the association is visible in the last bit
        assert np.array_equal(w[:, 2], pair if hashed else generic)
    # a position left of the unit cube (cell x = -1 as uint32) takes the generic loop on a hashed level too
    xo = x.copy(); xo[:, 0] = -0.01
    _, w = O.grid_fixed_weights(xo, lv, 12)
    _, f = O.grid_corner_indices(xo, lv, 12)
    assert np.array_equal(w[:, 2], ((F32(1) - f[:, 0]) * f[:, 1]) * (F32(1) - f[:, 2]))


# ---- the input classes of tests/test_gpu_exact_gradients_large.py: res + 2 >= 16384, positions outside the unit cube -----------------
def _outside_batch(n, seed):
    """uniform points, a share of them outside the unit cube on every side (the 'outside' batch of the GPU tests)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g)
    x[::7, 0] = -0.25
    x[5::11, 0] = 9.5
    x[3::13, 1] = -3.0
    x[4::17, 2] = 1.75
    return x.numpy()


def _fl32(v: Fraction) -> Fraction:
    """a rational rounded to the nearest fp32 number, ties to even (normal and subnormal range), in integer arithmetic"""
    if v == 0:
        return v
    s, a = (-1 if v < 0 else 1), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    q = a / quantum
    k = q.numerator // q.denominator
    rest = q - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k % 2 == 1):
        k += 1
    return s * k * quantum


def _slow_corners(x, lv, level):
    """grid_corner_indices and the pair flag of grid_fixed_weights once more, one sample at a time: Python integers for the cell, the
    hash and the wrap, % for the dense modulo, math.floor, and the fma of the grid position as a rational rounded once"""
    M = 0xFFFFFFFF
    scale = Fraction(float(lv.scale[level]))
    res, size, hashed = int(lv.res[level]), int(lv.size[level]), bool(lv.hashed[level])
    idx, frac, pair, cells = [], [], [], []
    for p in x:
        pos = [_fl32(Fraction(float(F32(c))) * scale + Fraction(1, 2)) for c in p]
        cell = [math.floor(v) for v in pos]
        frac.append([float(v - c) for v, c in zip(pos, cell)])          # (exact: both are fp32 numbers of one binade or less)
        u = [c & M for c in cell]                                          # (uint32)(int32) of the kernels: two's complement
        row = []
        for c in range(8):
            cx, cy, cz = (u[0] + (c & 1)) & M, (u[1] + ((c >> 1) & 1)) & M, (u[2] + (c >> 2)) & M
            if hashed:
                h = cx ^ ((cy * 2654435761) & M) ^ ((cz * 805459861) & M)
            else:
                h = (cx + cy * res + cz * res * res) & M
            row.append(h % size)
        idx.append(row)
        pair.append(hashed and u[0] < 16383)
        cells.append(cell)
    return np.array(idx, np.int64), np.array(frac, np.float64), np.array(pair), cells


def _both_associations(f):
    one = (F32(1.0) - f).astype(F32)
    generic, paired = np.zeros((f.shape[0], 8), F32), np.zeros((f.shape[0], 8), F32)
    for c in range(8):
        wx, wy, wz = (f[:, 0] if c & 1 else one[:, 0]), (f[:, 1] if c & 2 else one[:, 1]), (f[:, 2] if c & 4 else one[:, 2])
        generic[:, c] = ((wx * wy).astype(F32) * wz).astype(F32)
        paired[:, c] = (wx * (wy * wz).astype(F32)).astype(F32)
    return generic, paired


# the three finest levels of the GPU tests' fine grids (res 8192, 16384, 32768; all hashed), and a coarse grid with two dense levels
FINE = dict(n_levels=3, log2_hashmap_size=14, base_resolution=8192, per_level_scale=2.0)
COARSE = dict(n_levels=3, log2_hashmap_size=14)


def test_corner_indices_and_the_association_rule_against_a_slow_integer_restatement():
    for kw, hashed in ((FINE, [True, True, True]), (COARSE, [False, False, True])):
        lv = O.grid_levels(**kw)
        assert lv.hashed.tolist() == hashed
        x = _outside_batch(300, seed=21)
        x[-1] = 1.0
        x[-2] = 0.0
        x[-3] = [16383.0 / 32767.0, 0.5, 0.5]                            # around the cell where the association switches
        x[-4] = [16382.4 / 32767.0, 0.5, 0.5]
        classes = set()
        for l in range(lv.n_levels):
            want_idx, want_frac, want_pair, cells = _slow_corners(x, lv, l)
            idx, f = O.grid_corner_indices(x, lv, l)
            assert np.array_equal(idx.astype(np.int64), want_idx), (kw, l)
            assert np.array_equal(f.astype(np.float64), want_frac), (kw, l)
            idx2, w = O.grid_fixed_weights(x, lv, l)
            assert np.array_equal(idx2, idx)
            generic, paired = _both_associations(f)
            assert np.array_equal(w, np.where(want_pair[:, None], paired, generic)), (kw, l)
            outside = ((x < 0) | (x > 1)).any(1)
            classes |= {(bool(lv.hashed[l]), bool(p), bool(o)) for p, o in zip(want_pair, outside)}
            if not lv.hashed[l]:                                           # the modulo of a dense level is taken, and not by every sample
                assert any(min(c) < 0 for c in cells) and any(max(c) > int(lv.res[l]) for c in cells) and not want_pair.any()
        if kw is FINE:      # hashed: both associations inside the cube (res 32768) and outside it (a pair: outside along y or z only)
            assert {(True, True, False), (True, False, False), (True, True, True), (True, False, True)} <= classes


def test_integer_fields_outside_the_cube_and_on_fine_levels_against_a_float64_sum():
    for kw in (FINE, COARSE):
        for interp in ('Linear', 'Smoothstep'):
            lv = O.grid_levels(**kw)
            x = _outside_batch(5003, seed=22)
            g = torch.Generator().manual_seed(23)
            dfeat = (torch.randn(lv.n_levels, 5003, 2, generator=g) * 1e-3).numpy()      # (gradients kept outside the cube)
            shifts = [16 - int(np.ceil(np.log2(np.abs(dfeat[l]).max()))) for l in range(lv.n_levels)]
            got = O.grid_fixed_fields(x, dfeat, lv, shifts, interp)
            ref, cnt = _float64_sum(x, dfeat, lv, shifts, interp)
            assert (np.abs(got - ref) <= 0.5 * cnt[:, None] + 1).all(), (kw, interp)
            assert not got[cnt == 0].any() and cnt.sum() == 8 * 5003 * lv.n_levels


def test_the_association_matters_on_either_side_of_cell_16383():
    """a kernel with the wrong association on one side of the switch must not pass the GPU tests' equality: on the res 32768 level
    enough samples of a 5,003-sample batch have a weight whose last bit depends on the association, on both sides"""
    lv = O.grid_levels(**FINE)
    assert int(lv.res[2]) == 32768
    x = torch.rand(5003, 3, generator=torch.Generator().manual_seed(1)).numpy()
    _, f = O.grid_corner_indices(x, lv, 2)
    _, w = O.grid_fixed_weights(x, lv, 2)
    generic, paired = _both_associations(f)
    differ = (generic != paired).any(1)
    pair = np.floor(O.grid_pos(x[:, 0], lv.scale[2])) < 16383
    # (few of 5,003: a grid position near 2^14 keeps 9 or 10 fraction bits, so most three-factor products are exact either way -- and
    #  fewer right of the switch, where positions are larger.  One differing sample on a side fails an equality; 16 is a margin.)
    assert differ.sum() >= 50 and (differ & pair).sum() >= 16 and (differ & ~pair).sum() >= 16, (int((differ & pair).sum()), int((differ & ~pair).sum()))
    assert np.array_equal(w, np.where(pair[:, None], paired, generic))
    # ... and the integers see it at fine units (the largest field near 2^26, as the GPU tests' fine set: a contribution of 2^k units
    # has an fp32 ulp of 2^(k - 23) units, so only the large ones carry the last bit of w into the integer): one association for
    # the whole level, either one, gives other fields
    idx = [O.grid_corner_indices(x, lv, l)[0] for l in range(3)]
    dfeat = torch.randn(3, 5003, 2, generator=torch.Generator().manual_seed(2)).numpy()
    for shift in (24,):
        right = O.grid_fixed_fields(x, dfeat, lv, [shift] * 3)
        for wrong in (generic, paired):
            ws = [O.grid_fixed_weights(x, lv, l) for l in range(2)] + [(idx[2], wrong)]
            other = O.grid_fixed_fields(x, dfeat, lv, [shift] * 3, weights=ws)
            lo = int(lv.offset[2])
            assert np.array_equal(other[:lo], right[:lo]) and (other[lo:] != right[lo:]).sum() >= 8, shift


def test_the_overlap_fold_gives_both_copies_the_vertex_sum():
    lv = O.grid_levels(n_levels=4, log2_hashmap_size=15, per_level_scale=2.0, layout='line_overlap', sb_shift=(2, 2, 1), local_min_res=16)
    assert lv.local.all()
    for interp in ('Linear', 'Smoothstep'):
        x, dfeat, shifts = _case(lv, 2001, seed=11)
        got = O.grid_fixed_fields(x, dfeat, lv, shifts, interp)
        runs = 1 << (lv.sb_shift[0] - 2)
        total_direct = np.zeros((lv.n_levels, 2), np.int64)
        for l in range(lv.n_levels):
            lo, n = int(lv.offset[l]), int(lv.size[l])
            v = got[lo:lo + n].reshape(n // (32 * runs), runs, 8, 4, 2)
            assert np.array_equal(v[:, :-1, :, 3], v[:, 1:, :, 0])        # the two copies hold the same integers
            idx, w = O.grid_fixed_weights(x, lv, l, interp)
            for c in range(8):
                ok = idx[:, c] < n
                for k in range(2):
                    total_direct[l, k] += int(np.rint((w[ok, c] * dfeat[l][ok, k]).astype(F32).astype(np.float64) * 2.0 ** shifts[l]).sum())
            once = v.copy()
            once[:, 1:, :, 0] = 0                                           # every shared vertex counted once
            assert np.array_equal(once.reshape(-1, 2).sum(0), total_direct[l])
        ref, cnt = _float64_sum(x, dfeat, lv, shifts, interp)
        assert (np.abs(got - ref) <= 0.5 * cnt[:, None] + 1).all()
        # the fold on integers is the fold on floats
        a = np.arange(lv.total * 2, dtype=np.int64).reshape(-1, 2)
        assert np.array_equal(O.fold_overlap_copies(a.copy(), lv), O.fold_overlap_copies(a.astype(np.float64), lv).astype(np.int64))
