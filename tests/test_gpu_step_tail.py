"""The optimizer step in every launch form (perf_adam_step, perf_adam_step_dev: adam_kernel / adam4_kernel of perf_amd/csrc/misc.hip)
against float64 Adam, the device-side schedule of perf_step_bookkeeping, and the 16-bit conversions of perf_cast_params on every
rounding edge.

Reference and bars: tests/adam_reference.py (float64 evaluation of the documented formula; per-element bars counted from the fp32
roundings of the kernel's expression).  Every array a kernel writes is a view into a larger buffer with sentinel values on both
sides, and every test asserts the sentinels untouched.  Each test prints the worst measured error / bar per output."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import adam_reference as AR  # noqa: E402

SENT = 7.25                  # sentinel of the fp32 buffers
SENT16 = 0x5A5A              # ... and of the 16-bit ones (a bit pattern)
PAD = 16
VECTOR, SCALAR = 4, 1        # floats in front of a view: 16-byte aligned (four elements per thread from n = 1024 on) / 4-byte (one per thread)
N = 4099
STEPS = (1, 2, 3, 10, 1000, 100000)
SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1027, 65539)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from perf_amd import ops as _ops
    return _ops


def _t16(name):
    return {None: None, 'bf16': torch.bfloat16, 'fp16': torch.float16}[name]


class _Dev:
    """A CPU state (p, m, v, g) on the device, every array a view `lead` floats into a sentinel-filled buffer; the working copy (if any)
    `w_lead` halves into one of its own."""

    def __init__(self, state, lead, w16=None, w_lead=8):
        self.n, self.lead, self.w_lead = state[0].numel(), lead, w_lead
        self.bufs = []
        for x in state:
            buf = torch.full((lead + self.n + PAD,), SENT, dtype=torch.float32)
            buf[lead:lead + self.n] = x
            self.bufs.append(buf.cuda())
        self.p, self.m, self.v, self.g = (b[lead:lead + self.n] for b in self.bufs)
        self.w = self.wbuf = None
        if w16 is not None:
            self.wbuf = torch.full((w_lead + self.n + PAD,), SENT16, dtype=torch.int16).view(_t16(w16)).cuda()
            self.w = self.wbuf[w_lead:w_lead + self.n]

    def takes_vector_kernel(self):
        """adam_launch's condition, from the pointers: all four fp32 arrays 16-byte and the working copy 8-byte aligned, n >= 1024."""
        a = [x.data_ptr() % 16 for x in (self.p, self.m, self.v, self.g)]
        assert a == [4 * (self.lead % 4)] * 4, a
        if self.w is not None:
            assert self.w.data_ptr() % 16 == 2 * self.w_lead % 16
        return a == [0, 0, 0, 0] and (self.w is None or self.w.data_ptr() % 8 == 0) and self.n >= 1024

    def assert_sentinels(self):
        for b in self.bufs:
            assert bool((b[:self.lead] == SENT).all()) and bool((b[self.lead + self.n:] == SENT).all())
        if self.wbuf is not None:
            wb = self.wbuf.view(torch.int16)
            assert bool((wb[:self.w_lead] == SENT16).all()) and bool((wb[self.w_lead + self.n:] == SENT16).all())

    def cpu(self):
        return tuple(x.cpu() for x in (self.p, self.m, self.v, self.g))

    def assert_working_copy(self):
        """the working copy is p' converted as torch converts it, bit for bit"""
        assert torch.equal(self.w.cpu().view(torch.int16), self.p.cpu().to(self.w.dtype).view(torch.int16))


@functools.lru_cache(maxsize=None)
def _state(family, n, seed=11):
    return AR.make_state(family, n, seed)


@functools.lru_cache(maxsize=None)
def _ref(family, n, t, hi):
    """-> (float64 (p', m', v'), {dev: bars}) of one step from _state(family, n); computed once, never modified."""
    b1, b2, eps, lr = AR.HYPERS[hi]
    st = _state(family, n)
    return AR.adam_step_f64(*st, t, lr, b1, b2, eps), {dev: AR.adam_bounds(*st, t, lr, b1, b2, eps, dev=dev) for dev in (False, True)}


def _scalar(value, dtype):
    return torch.tensor([value], dtype=dtype, device='cuda')


def _launch(ops, d, entry, t, hi, zero_grad=True, gate=None, clear_flag=None, lr=None):
    b1, b2, eps, lr0 = AR.HYPERS[hi]
    lr = lr0 if lr is None else lr
    if entry == 'host':
        ops.adam_step(d.p, d.m, d.v, d.g, t, lr, b1, b2, eps, w16=d.w, zero_grad=zero_grad)
    else:
        ops.adam_step_dev(d.p, d.m, d.v, d.g, _scalar(t, torch.int32), _scalar(lr, torch.float32), b1, b2, eps, w16=d.w, zero_grad=zero_grad,
                          gate=None if gate is None else _scalar(gate, torch.int64), clear_flag=clear_flag)


def _ratios(got, ref, tol, keep=None):
    """-> worst |got - ref| / tol per output (p, m, v); asserts every element within its bar.  keep: mask of the elements compared."""
    worst = []
    for name, x, r, bar in zip('pmv', got, ref, tol):
        x = x.double()
        if keep is not None:
            x, r, bar = x[keep], r[keep], bar[keep]
        assert bool(torch.isfinite(x).all()), name
        ratio = (x - r).abs() / bar
        worst.append(float(ratio.max()))
        bad = int((ratio > 1).sum())
        assert bad == 0, f"{name}': {bad} of {x.numel()} elements outside their bar, worst {worst[-1]:.3g} of it"
    return worst


def _show(label, worst):
    print(f'RATIO {label}: ' + ' '.join(f"{k}' {w:.3f}" for k, w in zip('pmv', worst)))


def _one_step(ops, family, n, entry, lead, t, hi, w16=None, w_lead=8, zero_grad=True):
    """One launch from _state(family, n) -> (device state, worst ratios), with every assertion the forms share."""
    d = _Dev(_state(family, n), lead, w16, w_lead)
    assert d.takes_vector_kernel() == (lead == VECTOR and n >= 1024 and w_lead % 4 == 0)
    _launch(ops, d, entry, t, hi, zero_grad=zero_grad)
    ref, tol = _ref(family, n, t, hi)
    worst = _ratios(d.cpu()[:3], ref, tol[entry == 'dev'])
    d.assert_sentinels()
    if zero_grad:
        assert not bool(d.g.any())
    else:
        assert torch.equal(d.g.cpu(), _state(family, n)[3])
    if w16 is not None:
        d.assert_working_copy()
    return d, worst


# ---- a. a single step from an arbitrary state against float64 ------------------------------------------------------------------------
@pytest.mark.parametrize('hi', range(len(AR.HYPERS)), ids=lambda i: 'b1_%g-b2_%g-eps_%g-lr_%g' % AR.HYPERS[i])
@pytest.mark.parametrize('t', STEPS)
@pytest.mark.parametrize('kernel', ['vector', 'scalar'])
@pytest.mark.parametrize('entry', ['host', 'dev'])
def test_single_step_from_an_arbitrary_state(ops, entry, kernel, t, hi):
    worst = [0.0, 0.0, 0.0]
    for family in AR.FAMILIES:
        _, w = _one_step(ops, family, N, entry, VECTOR if kernel == 'vector' else SCALAR, t, hi, w16='bf16')
        worst = [max(a, b) for a, b in zip(worst, w)]
    _show(f'a {entry} {kernel} t={t} hyper {hi}', worst)


# ---- b. sizes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('entry', ['host', 'dev'])
def test_sizes_around_the_kernel_switch_and_the_partial_group(ops, entry, n):
    """n < 1024 takes the one-element kernel whatever the alignment; from 1024 on the aligned view takes the four-element kernel, whose
    last thread handles the n % 4 elements of a partial group one by one."""
    worst = [0.0, 0.0, 0.0]
    for lead in (VECTOR, SCALAR):
        for family, w16 in (('wide', 'bf16'), ('sparse', 'fp16'), ('matched', None)):
            _, w = _one_step(ops, family, n, entry, lead, 7, 0, w16=w16)
            worst = [max(a, b) for a, b in zip(worst, w)]
    _show(f'b {entry} n={n}', worst)


# ---- c. the forms give the same bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['host', 'dev'])
def test_every_form_leaves_the_same_bits(ops, entry):
    """Vector against scalar kernel, no / bf16 / fp16 working copy (16-byte and 8-byte aligned), gradient cleared or kept, and within
    the device entry gate absent against gate open: p', m', v' bit for bit those of one baseline launch."""
    t, hi = 3, 1
    base, worst = _one_step(ops, 'sparse', N, entry, VECTOR, t, hi)
    want = base.cpu()[:3]
    _show(f'c {entry}', worst)
    forms = 0
    for lead in (VECTOR, SCALAR):
        for w16, w_lead in ((None, 8), ('bf16', 8), ('fp16', 8), ('bf16', 4), ('fp16', 4), ('bf16', 1)):
            for zero_grad in (False, True):
                d, _ = _one_step(ops, 'sparse', N, entry, lead, t, hi, w16=w16, w_lead=w_lead, zero_grad=zero_grad)
                for a, b in zip(d.cpu()[:3], want):
                    assert torch.equal(a, b), (lead, w16, w_lead, zero_grad)
                forms += 1
    assert forms == 24
    if entry == 'dev':
        for lead in (VECTOR, SCALAR):
            for gate in (1, 17):
                d = _Dev(_state('sparse', N), lead, 'bf16')
                _launch(ops, d, 'dev', t, hi, gate=gate)
                for a, b in zip(d.cpu()[:3], want):
                    assert torch.equal(a, b), (lead, gate)
                assert not bool(d.g.any())
                d.assert_working_copy(); d.assert_sentinels()


# ---- d. device-scalar against host-scalar entry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hi', range(len(AR.HYPERS)))
@pytest.mark.parametrize('t', STEPS)
def test_device_scalars_against_host_scalars(ops, t, hi):
    """The two entries differ in where the bias corrections are formed (double on the host, fp32 in every workgroup's prologue): m' and v'
    are bit-identical, p' within the device entry's scalar error.  Measured on an MI355X: at most 0.895 of the bar (t = 3, beta2 = 0.99),
    on an element whose step is far below one ulp of p': the two p' are then equal or one ulp apart, one ulp of p' in [2^e, 2^(e+1)) is
    2u 2^e <= 2u|p'|, and the ratio approaches 1 only for p' just above a power of two."""
    b1, b2, eps, lr = AR.HYPERS[hi]
    worst = 0.0
    for family in AR.FAMILIES:
        for lead in (VECTOR, SCALAR):
            host, dev = (_Dev(_state(family, N), lead) for _ in range(2))
            _launch(ops, host, 'host', t, hi); _launch(ops, dev, 'dev', t, hi)
            (ph, mh, vh, _), (pd, md, vd, _) = host.cpu(), dev.cpu()
            assert torch.equal(mh, md) and torch.equal(vh, vd)
            bar = AR.entry_gap_bound(*_state(family, N), t, lr, b1, b2, eps)
            gap = (pd.double() - ph.double()).abs()
            assert bool((gap <= bar).all()), (family, lead, float((gap / bar.clamp_min(AR.TINY)).max()))
            worst = max(worst, float((gap / bar.clamp_min(AR.TINY)).max()))
            host.assert_sentinels(); dev.assert_sentinels()
    print(f"RATIO d t={t} hyper {hi}: p' {worst:.3f}")


# ---- e. gate and flag ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', ['vector', 'scalar'])
def test_a_closed_gate_moves_nothing_and_the_flag_is_cleared_either_way(ops, kernel):
    lead = VECTOR if kernel == 'vector' else SCALAR
    for gate in (0, -3, 1):
        d = _Dev(_state('wide', N), lead, 'fp16')
        assert d.takes_vector_kernel() == (kernel == 'vector')
        flag = _scalar(1, torch.int32)
        w0 = d.wbuf.clone()
        _launch(ops, d, 'dev', 5, 0, gate=gate, clear_flag=flag)
        assert int(flag.item()) == 0
        if gate <= 0:
            for a, b in zip(d.cpu()[:3], _state('wide', N)[:3]):
                assert torch.equal(a, b)
            assert torch.equal(d.wbuf.view(torch.int16), w0.view(torch.int16))
        else:
            ref, tol = _ref('wide', N, 5, 0)
            _ratios(d.cpu()[:3], ref, tol[True])
            d.assert_working_copy()
        d.assert_sentinels()


# ---- f. non-finite gradients stay where they are -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', ['vector', 'scalar'])
@pytest.mark.parametrize('entry', ['host', 'dev'])
def test_non_finite_gradients_stay_where_they_are(ops, entry, kernel):
    """g = +inf, -inf, NaN at an index inside a float4 group, in another workgroup's group and in the n % 4 tail: p' is NaN exactly there."""
    n, t, hi = 1027, 4, 0
    b1, b2, eps, lr = AR.HYPERS[hi]
    p, m, v, g = (x.clone() for x in _state('wide', n))
    where = {5: float('inf'), 514: float('-inf'), 1025: float('nan')}
    for i, x in where.items():
        g[i] = x
    keep = torch.ones(n, dtype=torch.bool); keep[list(where)] = False
    d = _Dev((p, m, v, g), VECTOR if kernel == 'vector' else SCALAR, 'bf16')
    assert d.takes_vector_kernel() == (kernel == 'vector')
    _launch(ops, d, entry, t, hi)
    got = d.cpu()[:3]
    assert torch.equal(got[0].isnan(), ~keep)
    ref = AR.adam_step_f64(p, m, v, g, t, lr, b1, b2, eps)
    assert torch.equal(ref[0].isnan(), ~keep)
    _show(f'f {entry} {kernel}', _ratios(got, ref, AR.adam_bounds(p, m, v, g, t, lr, b1, b2, eps, dev=entry == 'dev'), keep=keep))
    d.assert_sentinels()


# ---- g. a trajectory with skipped steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', ['vector', 'scalar'])
def test_trajectory_with_skipped_steps(ops, kernel):
    """60 iterations through perf_step_bookkeeping + perf_adam_step_dev, step count, iteration counter and learning-rate schedule on the
    device, the gate closed on every fifth.  Reference: adam_step_f64 chained over the taken iterations only, t = steps taken, lr = the
    schedule's row of the ITERATION (which advances on a skipped one).  Bar: twice the sum of the per-step bars along the float64
    trajectory (an fp32 emulation of 300 such iterations on the CPU reached 0.21 of it)."""
    iters, hi = 60, 0
    b1, b2, eps, _ = AR.HYPERS[hi]
    gen = torch.Generator().manual_seed(21)
    p0 = 0.3 * torch.randn(N, generator=gen)
    zeros = torch.zeros(N)
    d = _Dev((p0, zeros, zeros, zeros), VECTOR if kernel == 'vector' else SCALAR, 'bf16')
    assert d.takes_vector_kernel() == (kernel == 'vector')
    table = torch.stack([1e-2 * 0.98 ** torch.arange(iters, dtype=torch.float64), torch.linspace(0, 1, iters, dtype=torch.float64)], dim=1).float()
    table_dev = table.cuda()
    step, it = _scalar(0, torch.int32), _scalar(0, torch.int32)
    lr_out, ratio_out = _scalar(0.0, torch.float32), _scalar(0.0, torch.float32)
    eff = _scalar(0, torch.int64)
    counters = ops.step_counters('cuda')
    P, M, V = p0.double(), zeros.double(), zeros.double()
    bar = torch.zeros(N, dtype=torch.float64)
    taken = 0
    for i in range(iters):
        g = 128 * torch.randn(N, generator=gen)
        g[torch.rand(N, generator=gen) < 0.6] = 0.0
        d.g.copy_(g)
        gate = _scalar(0 if i % 5 == 4 else 17, torch.int64)
        ops.step_bookkeeping(step, gate, counters, _scalar(100, torch.int64), gate, eff_gate=eff, schedule=(table_dev, it, lr_out, ratio_out))
        ops.adam_step_dev(d.p, d.m, d.v, d.g, step, lr_out, b1, b2, eps, w16=d.w, zero_grad=True, gate=eff)
        if i % 5 != 4:
            taken += 1
            lr = float(table[i, 0])
            bar += AR.adam_bounds(P, M, V, g, taken, lr, b1, b2, eps, dev=True)[0]
            P, M, V = AR.adam_step_f64(P, M, V, g, taken, lr, b1, b2, eps)
    assert int(step.item()) == taken == 48 and int(it.item()) == iters
    assert counters.tolist()[:3] == [100 * iters, 17 * taken, iters]
    ratio = (d.p.cpu().double() - P).abs() / (2 * bar)
    print(f"RATIO g {kernel}: p' {float(ratio.max()):.3f}")
    assert bool((ratio <= 1).all()), float(ratio.max())
    d.assert_working_copy(); d.assert_sentinels()


# ---- h. the schedule, directly -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', [0, 3])
def test_schedule_rows_counters_and_the_step_that_follows(ops, first):
    """A table of 6 rows and 9 bookkeeping calls: Adam reads lr(iteration), the next loss head ratio(iteration + 1), the last row repeats
    beyond the table, the iteration counter advances on every call and the step count on taken ones only.  The Adam launch that follows
    is bit for bit the launch given the same step count and learning rate by hand."""
    rows, n, hi = 6, 1027, 2
    b1, b2, eps, _ = AR.HYPERS[hi]
    table = torch.tensor([[0.25 / (k + 1), 0.125 * k + 0.0625] for k in range(rows)], dtype=torch.float32)
    table_dev = table.cuda()
    step, it = _scalar(0, torch.int32), _scalar(first, torch.int32)
    lr_out, ratio_out = _scalar(-1.0, torch.float32), _scalar(-1.0, torch.float32)
    eff, flag = _scalar(-1, torch.int64), _scalar(0, torch.int32)
    # (gate, overflow flag, overflow_redone, marched, capacity) -> taken
    calls = [((17, 0, False, 500, 1000), True), ((0, 0, False, 500, 1000), False), ((17, 1, False, 500, 1000), False),
             ((17, 1, True, 500, 1000), True), ((17, 0, False, 1001, 1000), False), ((17, 0, False, 1000, 1000), True),
             ((0, 1, True, 500, 1000), False), ((17, 0, False, 500, 0), True), ((17, 0, False, 500, 1000), True)]
    assert len(calls) == 9
    d = _Dev(_state('matched', n), VECTOR)
    assert d.takes_vector_kernel()
    taken = 0
    for i, ((gate, raised, redone, marched, cap), want) in enumerate(calls):
        before = d.cpu()
        flag.fill_(raised)
        ops.step_bookkeeping(step, _scalar(gate, torch.int64), None, _scalar(marched, torch.int64), None, capacity=cap, overflow=flag,
                             eff_gate=eff, schedule=(table_dev, it, lr_out, ratio_out), overflow_redone=redone)
        taken += int(want)
        cur, nxt = min(first + i, rows - 1), min(first + i + 1, rows - 1)
        assert float(lr_out.item()) == float(table[cur, 0]) and float(ratio_out.item()) == float(table[nxt, 1]), i
        assert int(it.item()) == first + i + 1 and int(step.item()) == taken and int(eff.item()) == int(want) and int(flag.item()) == 0, i
        ops.adam_step_dev(d.p, d.m, d.v, d.g, step, lr_out, b1, b2, eps, gate=eff)
        if want:
            hand = _Dev(before, VECTOR)
            _launch(ops, hand, 'dev', taken, hi, zero_grad=False, lr=float(table[cur, 0]))
            for a, b in zip(d.cpu(), hand.cpu()):
                assert torch.equal(a, b), i
            assert not torch.equal(d.p.cpu(), before[0])
        else:
            for a, b in zip(d.cpu(), before):
                assert torch.equal(a, b), i
        d.assert_sentinels()
    assert taken == 5


# ---- i. the 16-bit conversions on every edge -------------------------------------------------------------------------------------------
def _from_bits(bits):
    """int64 tensor of 32-bit patterns -> float32"""
    return (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)


def _neighbours(x):
    """x (float32, finite, non-zero) -> (x, the fp32 below it in magnitude, the fp32 above)"""
    b = x.view(torch.int32)
    return torch.cat([x, (b - 1).view(torch.float32), (b + 1).view(torch.float32)])


def _bf16_edges():
    """every fp32 whose upper half is any of the 65,536 patterns and whose lower half is one of six: every tie, both neighbours of every
    tie, the exact values, subnormals, +-0, +-inf, NaNs"""
    hi = torch.arange(65536, dtype=torch.int64) << 16
    return torch.cat([_from_bits(hi | lo) for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)])


def _fp16_edges():
    """for every finite fp16 pattern of either sign: its value, the midpoint to the next pattern (for the largest, the overflow threshold
    65520) and that midpoint's two fp32 neighbours; the thresholds of overflow and underflow by name; fp32 subnormals, +-0, +-inf, NaNs"""
    k = torch.arange(31744, dtype=torch.int64)

    def value(k):
        e, f = k >> 10, (k & 1023).double()
        return torch.where(e == 0, f * 2.0 ** -24, (1024 + f) * torch.exp2((e - 25).double()))

    val, mid = value(k), (value(k) + value(k + 1)) / 2
    assert torch.equal(val.float().double(), val) and torch.equal(mid.float().double(), mid)
    assert torch.equal(val.float().to(torch.float16).view(torch.int16).long(), k)
    named = torch.tensor([65504.0, 65520.0, 65536.0, 1e10, 2.0 ** -25, 2.0 ** -24], dtype=torch.float32)
    special = _from_bits(torch.tensor([0x00000001, 0x00400000, 0x007FFFFF, 0x00800000, 0x00000000, 0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF]))
    pos = torch.cat([val.float(), _neighbours(mid.float()), _neighbours(named), special])
    return torch.cat([pos, -pos])


def _cast_and_compare(ops, x, dtype):
    n, t16 = x.numel(), _t16(dtype)
    buf = torch.full((n + PAD,), SENT16, dtype=torch.int16).view(t16).cuda()
    src = x.cuda()
    assert src.data_ptr() % 16 == 0
    ops.cast_params(src, dtype, out=buf[:n])
    got, want = buf[:n].cpu(), x.to(t16)
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)                        # (a NaN stays a NaN; its payload is not specified)
    gb, wb = got.view(torch.int16), want.view(torch.int16)
    bad = (gb != wb) & ~nan
    assert not bool(bad.any()), [(hex(a & 0xFFFFFFFF), hex(b & 0xFFFF), hex(c & 0xFFFF)) for a, b, c in
                                 zip(x.view(torch.int32)[bad][:8].tolist(), gb[bad][:8].tolist(), wb[bad][:8].tolist())]
    assert bool((buf.view(torch.int16)[n:] == SENT16).all())


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_cast_on_every_rounding_edge(ops, dtype):
    x = _bf16_edges() if dtype == 'bf16' else _fp16_edges()
    assert x.numel() < 500000
    _cast_and_compare(ops, x, dtype)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_cast_lengths_and_alignment(ops, dtype):
    """Whole and partial groups of four, nothing written behind the output; a source that is not 16-byte aligned is refused by the launcher
    before anything is launched."""
    from perf_amd._lib import PerfError
    x = _bf16_edges() if dtype == 'bf16' else _fp16_edges()
    x = x[torch.randperm(x.numel(), generator=torch.Generator().manual_seed(2))]
    for n in (1, 2, 3, 4, 5, 1023, 1025):
        _cast_and_compare(ops, x[:n].contiguous(), dtype)
    src = x[:1028].cuda()
    out = torch.full((1024,), SENT16, dtype=torch.int16).view(_t16(dtype)).cuda()
    assert src[1:].data_ptr() % 16 == 4
    with pytest.raises(PerfError):
        ops.cast_params(src[1:1025], dtype, out=out)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENT16).all())
