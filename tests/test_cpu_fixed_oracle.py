"""CPU tests (no GPU) of the integer oracle of the fixed-point table gradient (oracle/perf_oracle.py:grid_fixed_fields): against a
float64 sum of the same contributions, for rounding bias, for order and partition independence, and the overlap fold.  The GPU tests
(tests/test_gpu_exact_gradients.py) demand equality with it to the bit, so it has to be right on its own."""
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
