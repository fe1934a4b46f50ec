"""Step riders (include/perf_hip_riders.h) on the GPU: the next batch's draw, lattice tables and the two marching passes as workgroups that
ride in the grid backward's tile-code launch (A), its replica reduction (B) and the optimizer's launch (C).

* every output array of every stage is torch.equal to what the stand-alone entry points write, called in the order A, B, C with the same
  arguments (rows nobody writes -- table entries beyond a row's count, mask words of dead chunks, sample rows beyond the marched count --
  are left out: they hold whatever the allocation held);
* every host launch computes the same bits with riders as without."""
import pytest
import torch

from tests import test_gpu_ops as GO

pytestmark = pytest.mark.gpu

RES, STEPS, STEP, NEAR, FAR = 128, 128, 0.007, 0.0, 1.5
AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
SEED = 4321


@pytest.fixture(scope='module')
def ops():
    from perf_amd import ops as o
    return o


def _occupancy(kind):
    g = torch.arange(RES, device='cuda', dtype=torch.float32)
    c = (g + 0.5) / RES * 2 - 1
    r = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2).sqrt()
    if kind == 'all':
        occ = torch.ones_like(r, dtype=torch.bool)
    elif kind == 'empty':
        occ = torch.zeros_like(r, dtype=torch.bool)
    else:                       # a thin shell: a few samples where a ray crosses it
        occ = (r > 0.40) & (r < 0.43)
    return occ.reshape(-1)


@pytest.fixture(scope='module')
def field(ops):
    """A field backward on the shapes of tests/test_gpu_ops.py::test_field_backward_in_one_boundary_call_equals_the_three_calls, and the
    flat gradient / headroom state it leaves WITHOUT riders (computed once)."""
    cfg = GO._grid_cfg()
    cfgm, w, feat, sel, tdt, _ = GO._mlp_case(ops, 'bf16', 1, 1, 'Exponential', n=20011, seed=5)
    g = torch.Generator().manual_seed(11)
    n = feat.shape[1]
    x = torch.rand(n, 3, generator=g).cuda()
    dout = (torch.randn(n, 1, generator=g) * 1e-2).cuda()
    case = dict(cfg=cfg, cfgm=cfgm, x=x, dout=dout, w16=w.to(tdt).cuda(), f16=feat.to(tdt).cuda(), sel=sel.cuda())

    def run(riders=None):
        hr = ops.headroom_state('cuda')
        ops.overflow_flag('cuda').zero_()
        grad = ops.field_bwd(cfg, cfgm, x, case['w16'], case['f16'], dout, case['sel'], fixed=True, redo=True, hr_state=hr, riders=riders)
        return grad, hr

    case['run'] = run
    case['grad'], case['hr'] = run()
    return case


@pytest.fixture(scope='module')
def adam(ops):
    """An optimizer step on a flat [network | table] parameter with a pair table, and what it leaves WITHOUT a rider."""
    g = torch.Generator().manual_seed(3)
    n_net, n = 3072, 3072 + 2 * 50000
    init = {k: torch.rand(n, generator=g).cuda() * s for k, s in (('p', 1.0), ('m', 1e-3), ('v', 1e-6), ('g', 1e-2))}
    step = torch.tensor([3], dtype=torch.int32, device='cuda'); lr = torch.tensor([1e-2], device='cuda')
    gate = torch.tensor([7], dtype=torch.int64, device='cuda')

    def run(rider=None, pair=True, dtype=torch.bfloat16):
        a = {k: v.clone() for k, v in init.items()}
        w16 = torch.zeros(n, dtype=dtype, device='cuda')
        table = torch.zeros((n - n_net) // 2, 2, dtype=torch.int32, device='cuda')
        flag = torch.ones(1, dtype=torch.int32, device='cuda')
        ops.adam_step_dev(a['p'], a['m'], a['v'], a['g'], step, lr, w16=w16, gate=gate, clear_flag=flag, pair=(table, 1, n_net) if pair else None, rider=rider)
        return a['p'], a['m'], a['v'], w16, table, flag

    return dict(run=run, ref={True: run(None, True), False: run(None, False)})


def _pool(n_pool=5000):
    g = torch.Generator().manual_seed(9)
    o = ((torch.rand(n_pool, 3, generator=g) - 0.5) * 0.2).cuda()
    d = torch.nn.functional.normalize(torch.randn(n_pool, 3, generator=g), dim=-1).cuda()
    c = torch.rand(n_pool, 3, generator=g).cuda(); t = torch.rand(n_pool, 1, generator=g).cuda(); nrm = torch.randn(n_pool, 3, generator=g).cuda()
    return o, d, c, t, nrm


def _standalone(ops, pool, R, bits, coarse, cap, want_bg, draw_no):
    o, d, c, t, nrm = pool
    counter = torch.full((1,), draw_no, dtype=torch.int64, device='cuda')
    a = ops.draw_train_batch(SEED, counter, 100, len(o), R, 0, o, d, c, t, nrm, want_bg=want_bg, want_indices=True)
    runs = ops.lattice_runs((a['jitter'], STEP, NEAR), STEP, STEPS)
    t0 = (a['jitter'], STEP, NEAR, runs)
    masks, counts = ops.occ_march_count(a['o'], a['d'], t0, bits, RES, AABB, FAR, STEP, STEPS, coarse)
    offsets, total = ops.exclusive_scan_i32(counts)
    ri, ts, te, packed, x01, sel = ops.occ_march_write(t0, masks, counts, offsets, cap, STEP, STEPS, a['o'], a['d'], AABB)
    return dict(a, counter=counter, runs=runs, masks=masks, counts=counts, offsets=offsets, total=total, ri=ri, ts=ts, te=te, packed=packed, x01=x01, sel=sel)


def _riders(ops, lib, pool, R, bits, coarse, cap, want_bg, draw_no, field, adam, pair, dtype=torch.bfloat16):
    o, d, c, t, nrm = pool
    dev = 'cuda'
    junk = lambda *s, dtype=torch.float32: torch.full(s, 77, dtype=dtype, device=dev)
    out = {'o': junk(R, 3), 'd': junk(R, 3), 'color': junk(R, 3), 'dist': junk(R, 1), 'normal': junk(R, 3), 'jitter': junk(R), 'noise': junk(R, 1),
           'bg': junk(R, 3) if want_bg else None, 'indices': junk(R, dtype=torch.int64)}
    counter = torch.full((1,), draw_no, dtype=torch.int64, device=dev)
    runs = junk(lib.perf_occ_lattice_runs_len(R), dtype=torch.int32)
    masks = junk(max(R * lib.perf_occ_mask_words(STEPS), 1), dtype=torch.int64)
    counts = junk(R, dtype=torch.int32); offsets = junk(R, dtype=torch.int32)
    total = torch.tensor([123], dtype=torch.int64, device=dev); keep = torch.zeros(1, dtype=torch.int64, device=dev)
    ri = junk(cap, dtype=torch.int64); ts = junk(cap); te = junk(cap); packed = junk(R, 2, dtype=torch.int32); x01 = junk(cap, 3); sel = junk(cap, dtype=torch.uint8)
    t0 = (out['jitter'], STEP, NEAR, runs)
    draw = ops.rider_draw(SEED, counter, 100, len(o), R, 0, o, d, c, t, nrm, out, STEP, NEAR, STEP, STEPS, runs, marched_live=total, marched_keep=keep)
    count = ops.rider_count(out['o'], out['d'], t0, bits, RES, AABB, FAR, STEP, STEPS, coarse, masks, counts)
    write = ops.rider_write(t0, masks, counts, offsets, total, cap, STEP, STEPS, out['o'], out['d'], AABB, ri, ts, te, packed, x01, sel)
    grad, hr = field['run'](riders=(draw, count))                 # stages A and B
    stepped = adam['run'](rider=write, pair=pair, dtype=dtype)      # stage C
    res = dict(out, counter=counter, runs=runs, masks=masks, counts=counts, offsets=offsets, total=total, ri=ri, ts=ts, te=te, packed=packed, x01=x01, sel=sel)
    return res, grad, hr, stepped, keep


def _check_stages(lib, a, b, R, cap):
    for k in ('o', 'd', 'color', 'dist', 'normal', 'jitter', 'noise', 'bg', 'indices', 'counter', 'counts', 'offsets', 'total', 'packed'):
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    # tables of runs: row = [n | ks[64] | bs[64] | dd[64]], written up to n
    stride = lib.perf_occ_lattice_runs_len(1)
    ra, rb = a['runs'].view(R, stride), b['runs'].view(R, stride)
    assert torch.equal(ra[:, 0], rb[:, 0]) and int(ra[:, 0].min()) > 0
    written = torch.arange(64, device='cuda')[None, :] < ra[:, :1]
    for seg in range(3):
        sa, sb = ra[:, 1 + 64 * seg:65 + 64 * seg], rb[:, 1 + 64 * seg:65 + 64 * seg]
        assert torch.equal(torch.where(written, sa, 0), torch.where(written, sb, 0)), ('runs', seg)
    # mask records: [live words | chunk masks], a chunk's mask written when its live bit is set
    words = lib.perf_occ_mask_words(STEPS)
    ma, mb = a['masks'][:R * words].view(R, words), b['masks'][:R * words].view(R, words)
    assert words == 3 and torch.equal(ma[:, 0], mb[:, 0])
    for q in range(2):
        live = ((ma[:, 0] >> q) & 1).bool()
        assert torch.equal(ma[live, 1 + q], mb[live, 1 + q]), ('masks', q)
    n = min(int(a['total'].item()), cap)
    for k in ('ri', 'ts', 'te', 'x01', 'sel'):
        assert torch.equal(a[k][:n], b[k][:n]), k
    return n


@pytest.mark.parametrize('R', [1, 5, 257, 1000])
@pytest.mark.parametrize('occ', ['all', 'empty', 'shell'])
def test_every_stage_writes_what_its_stand_alone_kernels_write(ops, field, adam, R, occ):
    from perf_amd import _lib
    lib = _lib.load()
    bits = ops.occ_pack_bits(_occupancy(occ).reshape(1, RES, RES, RES))
    coarse = ops.occ_build_coarse(bits, RES)
    pool = _pool()
    cap = R * STEPS
    a = _standalone(ops, pool, R, bits, coarse, cap, want_bg=(R % 2 == 1), draw_no=R)
    b, grad, hr, stepped, keep = _riders(ops, lib, pool, R, bits, coarse, cap, want_bg=(R % 2 == 1), draw_no=R, field=field, adam=adam, pair=(R != 5))
    n = _check_stages(lib, a, b, R, cap)
    per_ray = a['counts'].tolist()
    if occ == 'all':
        assert n == R * STEPS and min(per_ray) == STEPS
    elif occ == 'empty':
        assert n == 0
    else:
        assert 0 < n < R * 16 and max(per_ray) < 16
    assert int(b['counter'].item()) == R + 1 and int(keep.item()) == 123
    # the hosts: the same bits with riders as without
    assert torch.equal(grad, field['grad']) and torch.equal(hr, field['hr']) and float(grad.abs().max()) > 0
    for x, y in zip(stepped, adam['ref'][R != 5]):
        assert torch.equal(x, y)


def test_a_mixed_batch_and_a_truncating_capacity(ops, field, adam):
    """Rays with 0, a few and 128 samples in ONE batch (a shell plus an occupied half space; origins outside the box for a quarter of the
    pool), and a capacity below the marched count: the rays beyond it are cut off exactly as the stand-alone write pass cuts them."""
    from perf_amd import _lib
    lib = _lib.load()
    occ = _occupancy('shell').reshape(RES, RES, RES).clone()
    occ[RES // 2 + RES // 8:] = True
    bits = ops.occ_pack_bits(occ.reshape(1, RES, RES, RES))
    coarse = ops.occ_build_coarse(bits, RES)
    o, d, c, t, nrm = _pool()
    o = o.clone(); o[::4] += 5.0                                    # (outside the box, looking away or past it: no samples)
    o[1::4, 0] += 0.6                                               # (inside the occupied half space)
    d = d.clone(); d[1::4, 0] = d[1::4, 0].abs()
    d = torch.nn.functional.normalize(d, dim=-1)
    pool = (o, d, c, t, nrm)
    R = 257
    for cap in (R * STEPS, 4099):
        a = _standalone(ops, pool, R, bits, coarse, cap, want_bg=False, draw_no=2)
        b, grad, hr, stepped, keep = _riders(ops, lib, pool, R, bits, coarse, cap, want_bg=False, draw_no=2, field=field, adam=adam, pair=True)
        n = _check_stages(lib, a, b, R, cap)
        per_ray = a['counts'].tolist()
        assert min(per_ray) == 0 and max(per_ray) == STEPS and any(0 < k < 16 for k in per_ray)
        assert int(a['total'].item()) > 4099 and n == min(int(a['total'].item()), cap)
        assert torch.equal(grad, field['grad']) and torch.equal(hr, field['hr'])
        for x, y in zip(stepped, adam['ref'][True]):
            assert torch.equal(x, y)


def test_hosts_without_riders_are_what_they_were(ops, field, adam):
    """perf_field_bwd_riders / perf_adam_step_dev_riders with NULL jobs against the entry points they extend."""
    g1, hr = field['run'](riders=(None, None))
    assert torch.equal(g1, field['grad']) and torch.equal(hr, field['hr'])
    for pair in (True, False):
        got = adam['run'](rider=None, pair=pair)
        for x, y in zip(got, adam['ref'][pair]):
            assert torch.equal(x, y)


@pytest.mark.parametrize('pair', [True, False])
def test_the_fp16_optimizer_launches_carry_the_write_pass_too(ops, field, adam, pair):
    """The rider instantiations of the fp16 working copy (with and without a pair table): the same stage C, the same step."""
    from perf_amd import _lib
    lib = _lib.load()
    bits = ops.occ_pack_bits(_occupancy('shell').reshape(1, RES, RES, RES))
    coarse = ops.occ_build_coarse(bits, RES)
    pool, R = _pool(), 257
    a = _standalone(ops, pool, R, bits, coarse, R * STEPS, want_bg=False, draw_no=7)
    b, grad, hr, stepped, keep = _riders(ops, lib, pool, R, bits, coarse, R * STEPS, want_bg=False, draw_no=7, field=field, adam=adam, pair=pair,
                                         dtype=torch.float16)
    assert _check_stages(lib, a, b, R, R * STEPS) > 0
    ref = adam['run'](None, pair, dtype=torch.float16)
    assert ref[3].dtype == torch.float16 and float(ref[3].float().abs().max()) > 0
    for x, y in zip(stepped, ref):
        assert torch.equal(x, y)
