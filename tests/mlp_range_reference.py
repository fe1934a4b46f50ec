"""The exact-arithmetic cases of the MLP kernels, with their units as arguments, and a CPU emulation of the kernels' roundings.

1. The helpers of tests/test_gpu_exact_gradients.py part B (small-integer features, sparse small-integer weights, small-integer output
   gradients: every 16-bit rounding and every fp32 sum of the kernels is exact, so a float64 forward + autograd is THE answer).  The
   units s_feat / s_dout -- features and output gradients are integers times these -- default to that file's 2^-2 and 2^-3; any other
   power of two keeps every condition, which _exact_reference asserts at the units it is given.
2. range_cases(): the unit pairs that put one named quantity at an end of the 16-bit range (tests/test_gpu_mlp_range.py part A).
3. saturated_case(): the same networks at s_feat = 2 under an output activation, with a "compensated" output gradient
   g = fl32(r / act'(y)) for which the kernel's dY rounds to the integers r again (part B of that file).
4. emulate(): torch on the CPU with real 16-bit casts where the kernels round, and switches that make it wrong on purpose
   (tests/test_cpu_mlp_range_reference.py shows that the honest one IS the reference and that every wrong one fails a case)."""
import torch

DT = {'bf16': (torch.bfloat16, 256), 'fp16': (torch.float16, 2048)}      # integers up to this magnitude are exact in the type
S_FEAT, S_DOUT = 0.25, 0.125                                             # powers of two: features / output gradients are integers times these
MIN_NORMAL = {'bf16': 2.0 ** -126, 'fp16': 2.0 ** -14}
F32_SUB = 2.0 ** -149                                                    # one fp32 subnormal unit
EXP_OVERFLOW = 88.73                                                     # expf(a) is inf above this
EXP_CLAMP = 15.0                                                         # the backward multiplies by exp(min(y - shift, 15))


def _sparse_int(o, i, k, mag, g):
    """[o, i] matrix of small integers, k non-zeros per row, at most k * ceil(o / i) per column"""
    W = torch.zeros(o, i)
    for j in range(k):
        perm = torch.cat([torch.randperm(i, generator=g) for _ in range(-(-o // i))])[:o]
        W[torch.arange(o), perm] = torch.randint(1, mag + 1, (o,), generator=g).float() * (torch.randint(0, 2, (o,), generator=g) * 2 - 1).float()
    return W


def _exact_mlp(dt, nh, n_out, n_levels, n, seed, sel_mode, nnz=3, n_src=None, s_feat=S_FEAT, s_dout=S_DOUT, act='None', exp_shift=0.0):
    from perf_amd.grid import MlpConfig
    cfgm = MlpConfig(n_levels=n_levels, n_hidden_layers=nh, n_output_dims=n_out, output_activation=act, exp_shift=exp_shift)
    g = torch.Generator().manual_seed(seed)
    mag = 2 if n <= 5000 else 1                          # the value range shrinks with n: every fp32 sum over the samples stays below 2^24
    # (every column of W1 -- padded inputs included -- and every row of W_out -- rows >= n_out included -- holds weights)
    w = torch.cat([_sparse_int(o, i, nnz, mag, g).reshape(-1) for o, i in cfgm.shapes])
    rows = n if n_src is None else n_src
    feat = torch.randint(-mag, mag + 1, (n_levels, rows, 2), generator=g).float() * s_feat
    dout = torch.randint(-mag, mag + 1, (n, n_out), generator=g).float() * s_dout
    dout[0, 0] = s_dout                                  # (the first sample counts whatever the draw: batches of one, live counts of one)
    if sel_mode == 'zeros':
        sel = (torch.rand(n, generator=g) > 0.2).to(torch.uint8)
        sel[0] = 1
    else:
        sel = torch.ones(n, dtype=torch.uint8) if sel_mode == 'ones' else None
    return cfgm, w, feat, sel, dout


def _exact_reference(cfgm, w, feat, sel, dout, n_live, dt, activity=True, s_feat=S_FEAT, s_dout=S_DOUT, info=None):
    """float64 forward and autograd of the LINEAR network (no output activation); asserts the conditions under which it is what the
    kernels must give to the bit.  activity=False: the shares of active / tied / negative units are conditions on a population -- a
    caller that runs a few rows of one has asserted them on the whole of it.  info: a dict that receives the reference's inner
    quantities over the live rows (y, hidden pre-activations z, their gradients dz, the output gradient dy)."""
    tdt, cap = DT[dt]
    n = feat.shape[1]
    x = feat.permute(1, 0, 2).reshape(n, -1).double()
    x = torch.cat([x, x.new_zeros(n, cfgm.n_in_pad - x.shape[1])], 1).requires_grad_(True)
    Ws, off = [], 0
    for o, i in cfgm.shapes:
        Ws.append(w[off:off + o * i].view(o, i).double().requires_grad_(True))
        off += o * i
    h, zs, ins = x, [], []
    for W in Ws[:-1]:
        ins.append(h)
        z = h @ W.t()
        z.retain_grad()
        zs.append(z)
        h = torch.relu(z)
    ins.append(h)
    y = (h @ Ws[-1].t())[:, :cfgm.n_output_dims]
    y.retain_grad()
    out = y * (sel.double()[:, None] if sel is not None else 1.0)
    (out[:n_live] * dout[:n_live].double()).sum().backward()

    def exact16(t):
        return torch.equal(t.to(tdt).double(), t)
    # ---- the conditions (on the reference, before the GPU is touched)
    assert exact16(w.double()) and exact16(feat.double()) and exact16(y.grad)
    s = s_feat
    for z in zs:                                         # hidden pre-activations, and their gradients dH (masked): integers the type holds
        assert exact16(z.detach()) and float(z.detach().abs().max()) / s <= cap
        assert exact16(z.grad) and float(z.grad.abs().max()) / s_dout <= cap
        if not activity:
            continue
        live = z.detach()[:n_live]
        assert float((live > 0).double().mean()) >= 0.25, 'too few active hidden units'
        assert float((live == 0).double().mean()) >= 0.01, 'no ReLU ties'
        assert float((live < 0).double().mean()) >= 0.01
    # every fp32 sum: sum of |terms| below 2^24 units (forward rows, dX rows, and every dW entry summed over ALL samples)
    unit = s_feat * s_dout
    dzs = [z.grad for z in zs] + [torch.cat([y.grad, y.grad.new_zeros(n, 16 - y.grad.shape[1])], 1)]
    for W, a, dz in zip(Ws, ins, dzs):
        assert float((a.detach().abs() @ W.detach().abs().t()).max()) / s_feat < 2 ** 24
        assert float((dz.abs() @ W.detach().abs()).max()) / s_dout < 2 ** 24
        assert float((dz.abs().t() @ a.detach().abs()).max()) / unit < 2 ** 24
    dw = torch.cat([W.grad.reshape(-1) for W in Ws])
    dfeat = x.grad[:, :2 * cfgm.n_levels].reshape(n, cfgm.n_levels, 2).permute(1, 0, 2)
    for t in (out.detach(), dw, dfeat):
        assert torch.equal(t.float().double(), t)        # the answer itself is an fp32 number
    assert float(dw.abs().max()) > 0 and float(dfeat.abs().max()) > 0 and float(out.detach().abs().max()) > 0
    if info is not None:
        info.update(y=y.detach()[:n_live], z=[z.detach()[:n_live] for z in zs], dz=[z.grad[:n_live] for z in zs], dy=y.grad[:n_live], dw=dw)
    return out.detach().float(), dfeat.float().contiguous(), dw.float()


def _half_maxima(dfeat, n_levels):
    """level_absmax as mlp_bwd reports it TODAY: a lane accumulates ONE maximum over the levels of its half-wave, so level l receives
    the maximum over the levels l' with (l' >> 1) & 1 == (l >> 1) & 1 (mlp_reduce_device.hpp:32).  The rule for it is only ">= the
    level's own, tight overall" (_check_exact_mlp asserts no more); the end-to-end test needs the units the grid kernels derive from
    what mlp_bwd hands them, and a change of the sharing changes this function with it."""
    own = dfeat.abs().amax(dim=(1, 2)) if dfeat.shape[1] else torch.zeros(n_levels)
    half = [max([float(own[k]) for k in range(n_levels) if (k >> 1) & 1 == h], default=0.0) for h in (0, 1)]
    a = torch.zeros(24)
    for l in range(n_levels):
        a[l] = half[(l >> 1) & 1]
    return a, own


def _assert_backward_equal(cfgm, got, want, live):
    """dfeat, dw to the bit; level_absmax by the rule: each level at least its own maximum, tight overall, zeros past the last level"""
    (dfeat, dw, amax), (dfeat_ref, dw_ref) = got, want
    assert torch.equal(dfeat[:, :live], dfeat_ref[:, :live]), int((dfeat[:, :live] != dfeat_ref[:, :live]).sum())
    if not torch.equal(dw, dw_ref):
        bad = (dw != dw_ref).nonzero()[:, 0]
        raise AssertionError(f'dw: {len(bad)} of {dw.numel()} entries differ, first at {int(bad[0])}: kernel {float(dw[bad[0]])} reference {float(dw_ref[bad[0]])}')
    own = dfeat_ref[:, :live].abs().amax(dim=(1, 2))                   # per level: at least its own maximum; tight overall
    assert float(amax.max()) == float(own.max())
    assert bool((amax[:cfgm.n_levels] >= own).all()) and float(amax[cfgm.n_levels:].abs().sum()) == 0.0


def _run_kernels(ops, dt, cfgm, w, feat, sel, dout, n_live=None, index=None):
    """-> out (None through an index), (dfeat, dw, level_absmax), on the CPU"""
    tdt, _ = DT[dt]
    w16, f16 = w.to(tdt).cuda(), feat.to(tdt).cuda()
    sel_dev = None if sel is None else sel.cuda()
    n_dev = None if n_live is None else torch.tensor([n_live], dtype=torch.int64, device='cuda')
    out = None
    if index is None:
        out = ops.mlp_fwd(cfgm, w16, f16, sel_dev, n_dev=n_dev).cpu()
        fin = f16
    else:
        fin = ops.IndexedFeat(f16, index.cuda())
    dfeat, dw, amax = ops.mlp_bwd(cfgm, w16, fin, dout.cuda(), sel_dev, want_absmax=True, n_dev=n_dev)
    return out, (dfeat.cpu(), dw.cpu(), amax.cpu())


def _check_exact_mlp(ops, dt, cfgm, w, feat, sel, dout, n_live=None, index=None, activity=True, s_feat=S_FEAT, s_dout=S_DOUT, info=None):
    n = dout.shape[0]
    live = n if n_live is None else n_live
    src = feat if index is None else feat[:, index.long()]
    out_ref, dfeat_ref, dw_ref = _exact_reference(cfgm, w, src, sel, dout, live, dt, activity, s_feat, s_dout, info)
    out, back = _run_kernels(ops, dt, cfgm, w, feat, sel, dout, n_live, index)
    if out is not None:
        assert torch.equal(out[:live], out_ref[:live])
    _assert_backward_equal(cfgm, back, (dfeat_ref, dw_ref), live)
    return dfeat_ref, dw_ref


# ---- A: the ends of the 16-bit range ------------------------------------------------------------------------------------------------
# (s_feat, s_dout, the quantity at the edge).  'top_*' (fp16): the unit is derived per network so that the largest |z| (|dz|) of the
# case lies in [2^14, 2^15) -- at the listed 2^4 the largest hidden pre-activation of these networks is 12 or 72 units, 2^7.6 .. 2^10.2
UNIT_PAIRS = {
    'fp16': [(2.0 ** -2, 2.0 ** -24, 'dy_sub'), (2.0 ** -24, 2.0 ** -3, 'h_sub'), (2.0 ** -24, 2.0 ** -24, 'both_sub'),
             (2.0 ** 4, 2.0 ** -3, 'h_large'), (2.0 ** -2, 2.0 ** 4, 'dy_large'), (None, 2.0 ** -3, 'top_h'), (2.0 ** -2, None, 'top_dy')],
    'bf16': [(2.0 ** -2, 2.0 ** -133, 'dy_sub'), (2.0 ** -133, 2.0 ** -3, 'h_sub'), (2.0 ** 100, 2.0 ** -3, 'h_large'),
             (2.0 ** -2, 2.0 ** 100, 'dy_large'), (2.0 ** -70, 2.0 ** -70, 'prod_sub')],
}
RANGE_ARCHS = [(1, 1, 16), (1, 16, 8), (2, 3, 20), (2, 16, 24)]
RANGE_SIZES = [1, 40, 4003]            # a batch of one; two tiles, most waves idle; a ragged many-tile batch
RANGE_SELS = ['zeros', 'ones', None]


def range_cases():
    """(dt, nh, n_out, L, n, sel_mode, pair index): every (dtype, network, unit pair); n and the selector's form cycle as
    tests/test_gpu_exact_gradients.py:_exact_cases cycles them"""
    cases = []
    for di, dt in enumerate(DT):
        for ai, (nh, n_out, L) in enumerate(RANGE_ARCHS):
            for ui in range(len(UNIT_PAIRS[dt])):
                cases.append((dt, nh, n_out, L, RANGE_SIZES[(ai + ui + di) % 3], RANGE_SELS[(ai + 2 * ui + di) % 3], ui))
    return cases


def range_case_id(c):
    dt, nh, n_out, L, n, sel, ui = c
    return f'{dt}-nh{nh}-o{n_out}-L{L}-n{n}-sel_{sel}-{UNIT_PAIRS[dt][ui][2]}'


INDEXED_CASE, INDEXED_SRC = ('fp16', 2, 3, 20, 4003, 'zeros', 2), 6000        # features and gradients both subnormal, through ops.IndexedFeat


def indexed_rows(n, n_src):
    """an index that repeats rows and skips others (test_mlp_backward_through_an_index_is_exact's)"""
    g = torch.Generator().manual_seed(9)
    index = torch.randint(0, n_src // 2, (n,), generator=g) * 2          # even rows only, many of them twice
    index[:8] = index[8]
    index[-1] = n_src - 1
    assert len(set(index.tolist())) < n
    return index.to(torch.int32)


def _pow2_into_top_binade(largest_in_units):
    """the power of two that puts `largest_in_units` (an integer number of units) into [2^14, 2^15)"""
    k = 0
    while largest_in_units * 2.0 ** k < 2.0 ** 14:
        k += 1
    assert 2.0 ** 14 <= largest_in_units * 2.0 ** k < 2.0 ** 15
    return 2.0 ** k


def build_range_case(dt, nh, n_out, L, n, sel_mode, ui, n_src=None):
    """-> cfgm, w, feat, sel, dout, s_feat, s_dout, edge.  A batch of fewer than 64 samples is the head of a population of 64 (the rows
    with the largest gradients first), on which the shares of active / tied units have been asserted -- as in
    test_mlp_kernels_are_exact_on_exactly_representable_data."""
    s_feat, s_dout, edge = UNIT_PAIRS[dt][ui]
    seed = 600 + L + n_out
    if s_feat is None or s_dout is None:                 # derived units: measure the case at units of 1
        assert n_src is None
        probe = {}
        a = _exact_mlp(dt, nh, n_out, L, max(n, 64), seed, sel_mode, s_feat=1.0, s_dout=1.0)
        _exact_reference(*a, max(n, 64), dt, s_feat=1.0, s_dout=1.0, info=probe)
        if s_feat is None:
            s_feat = _pow2_into_top_binade(max(float(z.abs().max()) for z in probe['z']))
        else:
            s_dout = _pow2_into_top_binade(max(float(z.abs().max()) for z in probe['dz']))
    cfgm, w, feat, sel, dout = _exact_mlp(dt, nh, n_out, L, max(n, 64), seed, sel_mode, n_src=n_src, s_feat=s_feat, s_dout=s_dout)
    if n < 64:
        _, dfeat_pop, _ = _exact_reference(cfgm, w, feat, sel, dout, 64, dt, s_feat=s_feat, s_dout=s_dout)
        order = dfeat_pop.abs().sum(dim=(0, 2)).argsort(descending=True)[:n]
        feat, dout = feat[:, order].contiguous(), dout[order].contiguous()
        sel = None if sel is None else sel[order].contiguous()
        z0 = feat[:, 0].reshape(-1).double() @ w[:64 * cfgm.n_in_pad].view(64, -1)[:, :2 * L].double().t()
        assert bool((z0 > 0).any()) and bool((z0 == 0).any()) and bool((z0 < 0).any())      # (a batch of ONE has all three)
    return cfgm, w, feat, sel, dout, s_feat, s_dout, edge


def _share_below(t, bound):
    nz = t[t != 0].abs()
    assert nz.numel() > 0
    return float((nz < bound).double().mean())


def assert_edge_reached(edge, info, feat, dt):
    """the case really puts the named quantity at the end of the range (on the float64 reference's inner quantities, live rows only)"""
    tiny = MIN_NORMAL[dt]
    acts = torch.cat([torch.relu(z).reshape(-1) for z in info['z']])
    dzs = torch.cat([d.reshape(-1) for d in info['dz']])
    zmax, dzmax = float(torch.cat([z.reshape(-1) for z in info['z']]).abs().max()), float(dzs.abs().max())
    if edge in ('h_sub', 'both_sub'):                    # every feature and at least a quarter of the active hidden units: subnormal
        assert _share_below(feat.double(), tiny) == 1.0 and _share_below(acts, tiny) >= 0.25
    if edge in ('dy_sub', 'both_sub'):
        assert _share_below(info['dy'], tiny) == 1.0 and _share_below(dzs, tiny) >= 0.25
    if edge == 'prod_sub':                               # 16-bit operands of ordinary size whose fp32 products are fp32 subnormals
        assert _share_below(info['dw'], 2.0 ** -126) >= 0.25 and _share_below(acts, tiny) == 0.0 and _share_below(dzs, tiny) == 0.0
    if edge == 'h_large':                                # (what the listed unit reaches: see UNIT_PAIRS)
        assert zmax >= (2.0 ** 100 if dt == 'bf16' else 2.0 ** 6)
    if edge == 'dy_large':
        assert dzmax >= (2.0 ** 100 if dt == 'bf16' else 2.0 ** 6)
    if edge == 'top_h':
        assert 2.0 ** 14 <= zmax < 2.0 ** 15
    if edge == 'top_dy':
        assert 2.0 ** 14 <= dzmax < 2.0 ** 15


def mask_case(dt, n=4003, seed=77):
    """A case on which "the packed activation is not zero" and "the fp32 pre-activation is positive" DIFFER: features at the type's
    smallest subnormal unit and a first layer of integers / 4, so that hidden pre-activations are quarters of that unit.  The
    hidden activation's rounding is then a real one (0.25 and 0.5 units round to 0, 0.75 to 1, 1.5 to 2: nearest, ties to even) and the
    only one: everything behind it is exact again.  No autograd reference exists for it; the expectation is emulate() with float64
    sums.  -> cfgm, w, feat, sel, dout"""
    sub = {'fp16': 2.0 ** -24, 'bf16': 2.0 ** -133}[dt]
    cfgm, w, feat, sel, dout = _exact_mlp(dt, 1, 3, 16, n, seed, 'zeros', s_feat=sub)
    w = w.clone()
    w[:64 * cfgm.n_in_pad] *= 0.25
    tdt, _ = DT[dt]
    x = torch.cat([feat.permute(1, 0, 2).reshape(n, -1).double(), torch.zeros(n, cfgm.n_in_pad - 32, dtype=torch.float64)], 1)
    z = x @ w[:64 * cfgm.n_in_pad].view(64, -1).double().t()
    lost = (z > 0) & (z.to(tdt) == 0)
    assert float(lost.double().mean()) >= 0.05 and float(((z > 0) & ~lost).double().mean()) >= 0.05
    assert float((z.abs() / sub).max()) < 2 ** 10        # (and every later sum: integers of the units, far below 2^24)
    return cfgm, w, feat, sel, dout


# ---- B: output activations where they saturate ----------------------------------------------------------------------------------------
SAT_S_FEAT, SAT_S_DOUT = 2.0, 0.125
SAT_N = 4003


def linear_y(cfgm, w, feat, dt):
    """the network's linear output in float64, hidden activations as the kernels hold them (exact on the exact cases)"""
    tdt, _ = DT[dt]
    n = feat.shape[1]
    h = feat.permute(1, 0, 2).reshape(n, -1).double()
    h = torch.cat([h, h.new_zeros(n, cfgm.n_in_pad - h.shape[1])], 1)
    off = 0
    for k, (o, i) in enumerate(cfgm.shapes):
        W = w[off:off + o * i].view(o, i).double()
        off += o * i
        h = h @ W.t()
        if k < len(cfgm.shapes) - 1:
            h = torch.relu(h).to(tdt).double()
    return h[:, :cfgm.n_output_dims]


def act_derivative64(y, act, shift):
    if act == 'Exponential':
        return torch.exp((y - shift).clamp(max=EXP_CLAMP))
    s = torch.sigmoid(y)
    return s * (1 - s)


def act_truth(y, act, shift):
    """float64 activation of the exact y, rounded ONCE to fp32"""
    return (torch.exp(y - shift) if act == 'Exponential' else torch.sigmoid(y)).float()


def saturated_case(dt, nh, n_out, L, act, shift, seed, wo_scale):
    """-> dict.  The exact network at s_feat = 2 (y: even integers times wo_scale, a power of two on the output layer that spreads y
    over the activation's whole range), selector form 'zeros' with two rows masked on purpose -- the one with the largest argument and
    the one nearest 0 --, and the compensated output gradient: small integers r times s_dout on the entries inside the compensated
    range, g = fl32(r / act'(y)) there and 0 elsewhere.  The float64 LINEAR backward of r (masked entries 0) is then what the kernels
    must give to the bit.  All conditions are asserted here."""
    n = SAT_N
    cfgm, w, feat, sel, r = _exact_mlp(dt, nh, n_out, L, n, seed, 'zeros', s_feat=SAT_S_FEAT, s_dout=SAT_S_DOUT, act=act, exp_shift=shift)
    w = w.clone()
    w[-16 * 64:] *= wo_scale
    y = linear_y(cfgm, w, feat, dt)
    assert torch.equal(y.float().double(), y)
    arg = y - shift if act == 'Exponential' else y
    # ---- the masked rows: one whose exponential overflows in the forward, one in the middle
    sel = sel.clone()
    top = arg.amax(dim=1) if act == 'Exponential' else (-arg).amax(dim=1)          # (the sigmoid's expf(-y) overflows at the other end)
    i_hi, i_mid = int(top.argmax()), int(arg[:, 0].abs().argmin())
    sel[i_hi] = sel[i_mid] = 0
    assert i_hi != i_mid and float(top[i_hi]) > EXP_OVERFLOW + 1 and float(arg[i_mid, 0].abs()) <= 16
    # ---- the compensated range
    comp = (arg >= -80.0) if act == 'Exponential' else (y.abs() <= 6.0)
    r = torch.where(comp, r.double(), torch.zeros((), dtype=torch.float64)).float()
    d = act_derivative64(y, act, shift)
    g = torch.where(comp, r.double() / d, torch.zeros((), dtype=torch.float64)).float()
    assert bool(torch.isfinite(g).all())
    assert bool(((g.double() * d - r.double()).abs() <= 2.0 ** -16 * r.double().abs()).all())
    counted = comp & (r != 0) & (sel[:, None] != 0)                      # the compensated entries that reach dY
    shares = {}
    if act == 'Exponential':
        k = float(counted.sum())
        shares = {'above the clamp': float((counted & (arg > EXP_CLAMP)).sum()) / k, 'below -15': float((counted & (arg < -15.0)).sum()) / k,
                  'above the overflow point': int((counted & (arg > EXP_OVERFLOW)).sum())}
        assert shares['above the clamp'] >= 0.15 and shares['below -15'] >= 0.15 and shares['above the overflow point'] >= 1, shares
    else:
        assert float(counted.sum()) >= 0.05 * counted.numel() and float((y.abs() > 6.0).double().mean()) >= 0.25
        assert float(y.max()) >= 20.0                    # (both ends: 1 - s is 0 in fp32 from y = 17 on; the other end is `top` above)
    lin = {}
    out_lin, dfeat_ref, dw_ref = _exact_reference(cfgm, w, feat, sel, r, n, dt, s_feat=SAT_S_FEAT, s_dout=SAT_S_DOUT, info=lin)
    assert torch.equal(lin['y'], y)
    return dict(cfgm=cfgm, w=w, feat=feat, sel=sel, r=r, g=g, y=y, arg=arg, comp=comp, dfeat_ref=dfeat_ref, dw_ref=dw_ref, masked=(i_hi, i_mid),
                shares=shares)


SAT_ARCHS = [(1, 1, 16), (1, 3, 8), (1, 16, 20), (2, 1, 8), (2, 3, 16), (2, 16, 24)]      # n_out in {1, 3, 16} at both depths
SAT_ACTS = [('Exponential', 1.0), ('Exponential', 19.0), ('Sigmoid', 0.0)]
# (nh, n_out, L, act, shift, seed, wo_scale): where y falls depends on the draw -- with one output row of three weights it may have one
# sign only --, so for every network and activation the first seed from 700 on, at the smallest output scale of 1, 2, 4, whose draw
# meets the conditions saturated_case asserts (they are conditions on the reference; the kernels were not consulted).  With one
# hidden layer y has a standard deviation of about 15 at s_feat = 2 and the output layer is doubled.
SAT_TABLE = [
    (1, 1, 16, 'Exponential', 1.0, 702, 2.0), (1, 1, 16, 'Exponential', 19.0, 706, 2.0), (1, 1, 16, 'Sigmoid', 0.0, 705, 2.0),
    (1, 3, 8, 'Exponential', 1.0, 700, 2.0), (1, 3, 8, 'Exponential', 19.0, 701, 2.0), (1, 3, 8, 'Sigmoid', 0.0, 716, 1.0),
    (1, 16, 20, 'Exponential', 1.0, 700, 2.0), (1, 16, 20, 'Exponential', 19.0, 717, 2.0), (1, 16, 20, 'Sigmoid', 0.0, 702, 1.0),
    (2, 1, 8, 'Exponential', 1.0, 714, 1.0), (2, 1, 8, 'Exponential', 19.0, 707, 1.0), (2, 1, 8, 'Sigmoid', 0.0, 700, 1.0),
    (2, 3, 16, 'Exponential', 1.0, 700, 1.0), (2, 3, 16, 'Exponential', 19.0, 700, 1.0), (2, 3, 16, 'Sigmoid', 0.0, 700, 1.0),
    (2, 16, 24, 'Exponential', 1.0, 700, 1.0), (2, 16, 24, 'Exponential', 19.0, 735, 1.0), (2, 16, 24, 'Sigmoid', 0.0, 700, 1.0),
]
assert sorted({t[:5] for t in SAT_TABLE}) == sorted((*a, *b) for a in SAT_ARCHS for b in SAT_ACTS)


def saturated_cases():
    """(dt, nh, n_out, L, act, shift, seed, wo_scale): every row of SAT_TABLE in both types"""
    return [(dt,) + t for dt in DT for t in SAT_TABLE]


def saturated_case_id(c):
    dt, nh, n_out, L, act, shift, _, _ = c
    return f'{dt}-nh{nh}-o{n_out}-L{L}-{act}-shift{shift:g}'


def forward_units(got, y, act, shift):
    """-> (units, ok): the error of `got` against the float64 activation T rounded once to fp32, in units of 2^-24 |T| with a floor of
    one fp32 subnormal (results below 2^-126 are judged absolutely); entries where T is inf or 0 are judged by rule and carry 0 units:
    inf where T is inf; where T rounds to 0 at most one subnormal unit, never negative, never non-finite.  ok: every rule holds and
    nothing is NaN."""
    T = act_truth(y, act, shift).double()
    g = got.double()
    units = (g - T).abs() / (2.0 ** -24 * T.abs()).clamp(min=F32_SUB)
    inf, zero = torch.isinf(T), T == 0
    ok = bool((g[inf] == float('inf')).all()) and bool(((g[zero] >= 0) & (g[zero] <= F32_SUB)).all()) and not bool(torch.isnan(g).any())
    ok = ok and bool((g[~inf] >= 0).all()) and bool(torch.isfinite(g[~inf]).all())
    units = torch.where(inf | zero, torch.zeros_like(units), units)
    return units, ok, T


def forward_bars(y, act, shift):
    """4 x the worst error of torch's CPU fp32 exp / sigmoid on the same arguments, at least 4 units -- taken separately over the
    entries whose T is a normal fp32 number and over those whose T is subnormal (each at most the worst over both, which is the
    bar in one piece: where an fp32 sigmoid has lost its tail to the overflow of exp(-y), that does not excuse the rest).
    -> ((bar, emulation's worst) for normal T, the same for subnormal T), masks"""
    a32 = (y - shift).float() if act == 'Exponential' else y.float()
    emu = torch.exp(a32) if act == 'Exponential' else torch.sigmoid(a32)
    units, ok, T = forward_units(emu, y, act, shift)
    assert ok
    normal = T.abs() >= 2.0 ** -126
    worst = [float(units[m].max()) if bool(m.any()) else 0.0 for m in (normal, ~normal)]
    return [(4.0 * max(1.0, v), v) for v in worst], (normal, ~normal)


# ---- C: the kernels' roundings on the CPU ---------------------------------------------------------------------------------------------
def emulate(cfgm, w, feat, sel, dout, n_live, dt, acc=torch.float32, flush=(), mask_from='packed', clamp='arg', fwd_clamp=False,
            sel_by='select'):
    """mlp_fwd and mlp_bwd in torch on the CPU: real casts to the 16-bit type where the kernels round (weights, features, hidden
    activations, dY, every dH), sums in `acc`, the ReLU mask taken from the ROUNDED activation, the output activation and its
    derivative in `acc` by torch's own exp / sigmoid, a masked sample 0 by selection.  -> out, dfeat, dw.
    The switches make it wrong on purpose:
      flush      any of 'h', 'dy', 'dh': that 16-bit quantity is flushed to zero below the type's smallest normal
      mask_from  'pre': the ReLU mask of the backward is "the pre-activation in `acc` is positive"
      clamp      'none': dY = g exp(y - shift);  'y': dY = g exp(min(y, 15) - shift)      (honest 'arg': g exp(min(y - shift, 15)))
      fwd_clamp  the forward is exp(min(y - shift, 15)) too
      sel_by     'multiply': out = act(y) * sel"""
    tdt, _ = DT[dt]
    tiny = MIN_NORMAL[dt]
    n = feat.shape[1]

    def r16(t, name):
        t = t.to(tdt).to(acc)
        return torch.where(t.abs() < tiny, torch.zeros_like(t), t) if name in flush else t
    x = feat.to(tdt).to(acc).permute(1, 0, 2).reshape(n, -1)
    x = torch.cat([x, x.new_zeros(n, cfgm.n_in_pad - x.shape[1])], 1)
    Ws, off = [], 0
    for o, i in cfgm.shapes:
        Ws.append(w[off:off + o * i].view(o, i).to(tdt).to(acc))
        off += o * i
    h, ins, pres, acts = x, [], [], []
    for W in Ws[:-1]:
        ins.append(h)
        z = h @ W.t()
        h = r16(torch.relu(z), 'h')
        pres.append(z)
        acts.append(h)
    ins.append(h)
    n_out, act, shift = cfgm.n_output_dims, cfgm.output_activation, cfgm.exp_shift
    y = (h @ Ws[-1].t())[:, :n_out]
    sv = torch.ones(n, 1, dtype=acc) if sel is None else sel.to(acc)[:, None]
    if act == 'Exponential':
        a = torch.exp((y - shift).clamp(max=EXP_CLAMP) if fwd_clamp else y - shift)
    else:
        a = torch.sigmoid(y) if act == 'Sigmoid' else y
    out = a * sv if sel_by == 'multiply' else torch.where(sv != 0, a, torch.zeros_like(a))
    g = dout.to(acc) * sv
    g[n_live:] = 0
    if act == 'Exponential':
        g = g * torch.exp({'arg': (y - shift).clamp(max=EXP_CLAMP), 'none': y - shift, 'y': y.clamp(max=EXP_CLAMP) - shift}[clamp])
    elif act == 'Sigmoid':
        s = torch.sigmoid(y)
        g = g * s * (1 - s)
    dy = torch.cat([r16(g, 'dy'), g.new_zeros(n, 16 - n_out)], 1)
    dws = [None] * len(Ws)
    dws[-1] = dy.t() @ ins[-1]
    d = dy @ Ws[-1]
    for k in reversed(range(len(Ws) - 1)):
        active = (acts[k] != 0) if mask_from == 'packed' else (pres[k] > 0)
        dh = r16(torch.where(active, d, torch.zeros_like(d)), 'dh')
        dws[k] = dh.t() @ ins[k]
        d = dh @ Ws[k]
    dfeat = d[:, :2 * cfgm.n_levels].reshape(n, cfgm.n_levels, 2).permute(1, 0, 2).contiguous()
    return out.float(), dfeat.float(), torch.cat([t.reshape(-1) for t in dws]).float()
