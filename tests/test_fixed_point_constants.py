"""The constants of the fixed-point grid gradient, DERIVED instead of remembered (CPU; no GPU, no library call).

perf_amd/csrc/grid_fixed_point.hpp keeps the largest field of a level inside [2^21, 2^25) units, hashgrid_bwd.hip raises the overflow
flag at 2^29; each number was set after a failure on the GPU.  This file restates the closed loop in Python -- with
the constants PARSED from the sources, so the test follows them -- and checks the properties the numbers have to have together:

  1. integer fields are sums modulo 2^32: a partial sum (one replica, one rank, one arrival order) may wrap as long as the FINAL sum
     fits -- which is why the flag is only ever tested on final sums, and why 2^29 (not 2^31) is enough of a limit: the flag level
     plus the largest single contribution still fits an int32;
  2. the band is wider than the loop's granularity: from any starting headroom a stationary gradient is brought into the band and
     STAYS there (no oscillation: a correction never overshoots the other edge), upward in one call, downward one bit per call;
  3. the margin between the band and the flag: a level whose largest sum grows by less than 2^(29 - 25) = 16x from one call to the
     next is never flagged (the soak that motivated 16x saw 4x jumps flag 8 of 112,500 steps with a 4x margin);
  4. the resolution that is left: inside the band the largest contribution of a call is at least 2^(31 - 28) = 8 units, and with the
     static fan-in guess (no state) never less than 2^7 units.
"""
import math
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'perf_amd', 'csrc')


def _const(text, name):
    m = re.search(r'\b' + name + r'\s*=\s*(-?\d+)', text)
    assert m, name
    return int(m.group(1))


def _constants():
    hpp = open(os.path.join(CSRC, 'grid_fixed_point.hpp')).read()
    bwd = open(os.path.join(CSRC, 'hashgrid_bwd.hip')).read()
    flags = set(re.findall(r'field_max >= \(1 << (\d+)\)', bwd))
    assert len(flags) == 1, flags                      # every owner path and the replica reduction flag at the same level
    clamp = re.search(r'h = h < (\d+) \? \1 : \(h > (\d+) \? \2 : h\);\s*\} else \{\s*h = h < (\d+) \? \3 : \(h > (\d+) \? \4 : h\);', hpp)
    assert clamp, 'fixed_point_shift: the clamps of the headroom moved'
    floor = re.search(r'adj > (-\d+)\) adj -= 1', hpp)
    assert floor
    # the exponent rule: e from frexpf (am < 2^e), 0 for am <= 0, clamped from below; shift = 31 - h - e
    expo = re.search(r'int e = 0;\s*if \(am > 0\.f\) \(void\)frexpf\(am, &e\);[^\n]*\n\s*if \(e < (-\d+)\) e = \1;', hpp)
    assert expo, 'fixed_point_shift: the exponent rule moved'
    assert re.search(r'return 31 - h - e;', hpp), 'fixed_point_shift: the shift is no longer 31 - h - e'
    assert re.search(r'fan = \(8ull \* \(unsigned long long\)n_live \+ size - 1ull\) / size;', hpp), 'fixed_point_shift: the fan-in guess moved'
    return dict(top=_const(hpp, 'kHeadroomTopBit'), low=_const(hpp, 'kHeadroomLowBit'), bias=_const(hpp, 'kHeadroomStartBias'),
                flag=int(flags.pop()), h_min=int(clamp.group(1)), h_max=int(clamp.group(2)), h_min_static=int(clamp.group(3)),
                h_max_static=int(clamp.group(4)), adj_floor=int(floor.group(1)), max_replicas=_const(bwd, 'kMaxReplicas'),
                e_min=int(expo.group(1)))


C = _constants()


def headroom_feedback(adj, fm):
    """grid_fixed_point.hpp:headroom_feedback"""
    if fm >= (1 << C['top']):
        adj += fm.bit_length() - C['top'] + 1
    elif fm < (1 << C['low']) and adj > C['adj_floor']:
        adj -= 1
    return adj


def headroom_bits(fan, adj=None):
    """grid_fixed_point.hpp:fixed_point_shift, the headroom h (the unit of a level is 2^(e - 31 + h) for max |dfeat| < 2^e)."""
    h = (0 if fan <= 1 else (fan - 1).bit_length()) + 6
    if adj is None:
        return min(max(h, C['h_min_static']), C['h_max_static'])
    return min(max(h + adj + C['bias'], C['h_min']), C['h_max'])


def fixed_point_shift(am, n_live, size, adj=None):
    """grid_fixed_point.hpp:fixed_point_shift: one unit of a level is 2^-shift.  am = the level's max |dfeat| (fp32), n_live the live
    sample count, size the level's entries, adj the level's headroom state (None: no state, the static guess)."""
    am = float(np.float32(am))
    e = 0
    if am > 0.0:
        _, e = math.frexp(am)                        # am = m 2^e, 0.5 <= m < 1 (frexpf; a subnormal am gives e < -126)
    e = max(e, C['e_min'])
    fan = (8 * int(n_live) + int(size) - 1) // int(size)
    return 31 - headroom_bits(fan, adj) - e


def test_the_exponent_rule_of_the_unit():
    assert C['e_min'] == -80
    # the largest contribution |w g| <= am < 2^e spans less than 2^(31 - h) units: h bits of headroom below the int32 sign
    for am in (1.0, 0.75, 1.5, 3e-5, 2.0 ** -60, 123456.0, float(np.nextafter(np.float32(2.0), np.float32(0.0)))):
        for n, size in ((4099, 4096), (1 << 20, 1 << 18), (1, 1 << 18)):
            for adj in (None, 0, -5, 7):
                sh = fixed_point_shift(am, n, size, adj)
                fan = (8 * n + size - 1) // size
                h = headroom_bits(fan, adj)
                assert am * 2.0 ** sh < 2.0 ** (31 - h) <= 2.0 * am * 2.0 ** sh
    # an exact power of two sits at the BOTTOM of its binade (frexp: 1.0 = 0.5 * 2^1)
    assert fixed_point_shift(1.0, 1, 1 << 18) == fixed_point_shift(1.5, 1, 1 << 18) == fixed_point_shift(0.5, 1, 1 << 18) - 1
    # no gradient at all: e = 0; vanishing gradients: the clamp keeps 2^shift a finite fp32 (shift <= 31 - 4 + 80 < 128)
    assert fixed_point_shift(0.0, 1000, 4096) == 31 - headroom_bits(2)
    assert fixed_point_shift(1e-30, 1000, 4096) == fixed_point_shift(2.0 ** -90, 1000, 4096) == 31 - headroom_bits(2) + 80
    assert 31 - C['h_min'] - C['e_min'] < 128


def test_partial_sums_may_wrap_only_the_final_sum_has_to_fit():
    rng = np.random.default_rng(3)
    big = (1 << 31) - 1
    for _ in range(200):
        n = int(rng.integers(2, 4000))
        contrib = rng.integers(-(1 << 28), 1 << 28, size=n, dtype=np.int64)
        contrib -= contrib.sum() // n                                  # a final sum of modest size from partials that do not stay modest
        true = int(contrib.sum())
        assert abs(true) <= big
        for parts in (1, 2, C['max_replicas']):                        # replicas / ranks: any partition, any order inside a part
            order = rng.permutation(n)
            slabs = [np.int32(0)] * parts
            with np.errstate(over='ignore'):
                for k, i in enumerate(order):
                    slabs[k % parts] = np.int32(slabs[k % parts] + np.int32(contrib[i]))      # wraps like the LDS / global integer adds
                total = np.int32(0)
                for s in slabs:
                    total = np.int32(total + s)
            assert int(total) == true
    # the flag level leaves room for one more contribution of ANY size the unit allows (a contribution is < 2^(31 - h_min) units)
    assert (1 << C['flag']) + (1 << (31 - C['h_min'])) <= big + 1
    # ... and a sum that was NOT flagged is exact: below the flag level the int32 never wrapped in the final value
    assert (1 << C['flag']) < big


def test_the_loop_reaches_the_band_and_stays_there():
    top, low = 1 << C['top'], 1 << C['low']
    assert C['top'] - C['low'] >= 2                                      # wider than one downward step plus one bit of noise
    for fan in (1, 32, 1700, 50000):
        for true_log2 in range(-6, 30):                                   # the largest final sum of the level, in units of the largest contribution
            adj, history = 0, []
            for call in range(64):
                h = headroom_bits(fan, adj)
                fm = int(2.0 ** (true_log2 + 31 - h))                      # largest |field| in units of this call
                fm = min(fm, (1 << 31) - 1)
                history.append((h, fm))
                new = headroom_feedback(adj, fm)
                if new == adj:
                    break
                adj = new
            h, fm = history[-1]
            settled = low <= fm < top
            pinned = (h == C['h_min'] and fm < low) or (h == C['h_max'] and fm >= top) or (adj == C['adj_floor'] and fm < low)
            assert settled or pinned, (fan, true_log2, history[-3:])
            if settled:
                # stays: the same gradient again changes nothing, and the call that corrected upward did not overshoot the lower edge
                assert headroom_feedback(adj, fm) == adj
            ups = [i for i in range(1, len(history)) if history[i][0] > history[i - 1][0]]
            downs = [i for i in range(1, len(history)) if history[i][0] < history[i - 1][0]]
            assert not (ups and downs), (fan, true_log2, history)         # no oscillation: a stationary gradient moves the unit ONE way
            # upward: the excess bits at once -- ONE correction from a value that was measured (a saturated int32 says nothing about the excess)
            assert sum(1 for i in ups if history[i - 1][1] < (1 << 31) - 1) <= 1, history
            for i in ups:
                if history[i - 1][1] < (1 << 31) - 1 and history[i][0] < C['h_max']:       # (not clamped at the widest headroom)
                    assert (1 << (C['top'] - 2)) <= history[i][1] < (1 << (C['top'] - 1)), history     # ... and it lands two bits below the top


def test_a_sixteenfold_jump_between_two_calls_is_not_flagged():
    margin = C['flag'] - C['top']
    assert margin == 4                                                   # 16x: DESIGN.md 5.1 (the soak flagged 4x jumps with a 2-bit margin)
    top = 1 << C['top']
    for fm in (1 << C['low'], top - 1):
        for jump in (2, 4, 8, 15.99):
            assert fm * jump < (1 << C['flag'])
    assert (top - 1) * 16.01 >= (1 << C['flag'])                          # ... and that is exactly where it ends


def test_the_resolution_that_is_left():
    # closed loop: the largest contribution of a call spans at least 2^(31 - h_max) units
    assert 31 - C['h_max'] >= 3
    # static guess (no state): never coarser than 2^-7 of the largest contribution, 64x the average fan-in before a flag
    assert 31 - C['h_max_static'] >= 7
    for fan in (1, 2, 32, 1700):
        h = headroom_bits(fan)
        assert (1 << h) >= min(64 * fan, 1 << C['h_max_static']) or h == C['h_min_static']
    # a fresh state starts on the safe side of the static guess by kHeadroomStartBias bits
    assert headroom_bits(32, 0) - ((31).bit_length() + 6) == C['bias'] > 0
