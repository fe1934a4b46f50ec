#!/usr/bin/env python
"""Every entry point of csrc/composite.hip on fixed inputs, every output saved: run it once per library build, compare the two files.

    python tools/exp/composite_same_bits.py run OUT.npz        (on an MI355X; the library the perf_amd package on the path loads)
    python tools/exp/composite_same_bits.py compare A.npz B.npz [RECORD.json]   -> np.array_equal per output, folded per entry point

Inputs: the six cases of tests/composite_reference.py (make_case at gains 0.05 / 1 / 20, with and without the empty tail; whole, where the
ray head runs its team instantiation, and the long rays alone, where it runs a wavefront per ray), the three _packed_case(21, ...) shapes of
tests/test_gpu_ops.py (maxc 200 / 17 / 5: wavefronts, quarter waves, 4-lane teams) and 524,288 rays of two samples (the BY16 instantiations).
Per-sample outputs are cut to the samples packed_info names (rows behind them are capacity, never written)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path += [ROOT, os.path.join(ROOT, 'tests')]


def flatten(prefix, v, out):
    import torch
    if v is None:
        return
    if isinstance(v, torch.Tensor):
        out[prefix] = v.detach().cpu().numpy()
    elif isinstance(v, dict):
        for k, x in v.items():
            flatten(f'{prefix}.{k}', x, out)
    else:
        for k, x in enumerate(v):
            flatten(f'{prefix}.{k}', x, out)


def entry_points(ops, name, packed, ts, te, sig, rgb, out, seed=5):
    """packed int32 [R, 2], ts / te / sig [>= S], rgb [>= S, 3] on the device"""
    import torch
    R, S, N = packed.shape[0], int(packed[:, 1].sum()), sig.numel()
    g = torch.Generator(device='cuda').manual_seed(seed)
    rnd = lambda *shape: torch.rand(*shape, device='cuda', generator=g)

    def keep(key, v):
        got = {}
        flatten(f'{name}/{key}', v, got)
        for k, a in got.items():
            out[k] = a[:S] if (a.ndim >= 1 and a.shape[0] == N and N > S) else a

    counts = packed[:, 1].contiguous()
    nc, ex = ops.visibility_count(sig, ts, te, packed, 1e-4, want_exsum=True)
    keep('visibility_count', (nc, ex))
    keep('visibility_count.tail', ops.visibility_count(sig, ts, te, packed, 1e-4, march_counts=(counts + 3).contiguous(), head_samples=4))
    x01, sel = rnd(N, 3), (rnd(N) * 255).to(torch.uint8)
    feat = (rnd(3, N, 2) - 0.5).to(torch.float16)
    keep('compact_prefix', ops.compact_prefix(packed, nc, ts, te, sig, x01=x01, sel=sel, feat=feat, index_features=False))
    keep('compact_prefix.index', ops.compact_prefix(packed, nc, ts, te, x01=x01, sel=sel, feat=feat, index_features=True))
    # the two-source kernels: the batch as head, the same rays in reverse sample order as tail
    ts2, te2, sig2 = ts.flip(0).contiguous(), te.flip(0).contiguous(), (sig * 0.01).contiguous()
    packed2 = torch.stack([N - packed[:, 0] - packed[:, 1], packed[:, 1]], -1).to(torch.int32).contiguous()
    nc2 = ops.visibility_count2((sig * 0.01, ts, te, packed), (sig2, ts2, te2, packed2), 1e-4)
    keep('visibility_count2', nc2)
    keep('compact_prefix2', ops.compact_prefix2((sig * 0.01, ts, te, packed, x01, sel), (sig2, ts2, te2, packed2, x01, sel), nc2, int(nc2.sum()),
                                                feat_h=feat, feat_t=feat))
    w, T, al, op, dist, col = ops.composite_fwd(sig, rgb, ts, te, packed)
    keep('composite_fwd', (w, T, al, op, dist, col))
    w2, T2, op2, dist2, col2, dl = ops.composite_distloss_fwd(sig, rgb, ts, te, packed)
    keep('composite_distloss_fwd', (w2, T2, op2, dist2, col2, dl))
    g_w, g_T, g_al = rnd(N) - 0.5, rnd(N) - 0.5, rnd(N) - 0.5
    g_op, g_d, g_col = rnd(R) - 0.5, rnd(R) - 0.5, rnd(R, 3) - 0.5
    keep('composite_bwd', ops.composite_bwd(sig, ts, te, packed, w, T, g_weights=g_w, g_opacity=g_op, g_distance=g_d, g_color=g_col, g_trans=g_T,
                                            g_alphas=g_al, want_drgb=True))
    keep('composite_bwd.plain', ops.composite_bwd(sig, ts, te, packed, w, T, g_opacity=g_op, g_distance=g_d))
    scale_dev = torch.tensor([0.7], device='cuda')
    keep('composite_distloss_bwd', ops.composite_distloss_bwd(sig, ts, te, packed, w, T, op, dist, g_op, g_d, 0.3, scale_dev=scale_dev))
    keep('distloss_fwd', ops.distloss_fwd(w, ts, te, packed))
    keep('distloss_bwd', ops.distloss_bwd(w, ts, te, packed, 0.3, scale_dev=scale_dev))
    keep('accumulate_fwd', (ops.accumulate_fwd(w, rgb, packed), ops.accumulate_fwd(w, None, packed)))
    gt_d, noise, gt_c, bg = rnd(R) * 1.5, rnd(R), rnd(R, 3), rnd(R, 3)
    ratio = torch.tensor([0.6], device='cuda')
    for tag, nz, rt, bgc in (('', noise, ratio, bg), ('.plain', None, None, None)):
        for bs in (R, 4 * R):
            keep(f'geo_loss{tag}.{bs // R}', ops.geo_loss(op, dist, gt_d, nz, dl, packed, bs, 1.0, 0.5, rt, 128.0))
            keep(f'app_loss{tag}.{bs // R}', ops.app_loss(op, col, bgc, gt_c, bs, 1.0, 128.0))
            keep(f'train_head_geo{tag}.{bs // R}', ops.train_head_geo(sig, rgb, ts, te, packed, gt_d, nz, bs, 1.0, 0.5, rt, 128.0))
            keep(f'train_head_app{tag}.{bs // R}', ops.train_head_app(sig, rgb, ts, te, packed, bgc, gt_c, bs, 1.0, 128.0))
    keep('train_head_geo.no_rgb', ops.train_head_geo(sig, None, ts, te, packed, gt_d, noise, R, 1.0, 0.5, ratio, 128.0))


def run(path):
    import torch
    from perf_amd import ops
    import composite_reference as CR
    import test_gpu_ops as TG
    dev = lambda *xs: [torch.as_tensor(np.ascontiguousarray(x)).cuda().contiguous() for x in xs]
    out = {}
    for gain in CR.GAINS:
        for tail_empty in (False, True):
            c = CR.make_case(gain, tail_empty)
            for tag, cc in (('teams', c), ('waves', CR.sub_case(c))):
                entry_points(ops, f'case gain {gain} tail_empty {tail_empty} {tag}', *dev(cc.packed, cc.ts, cc.te, cc.sig, cc.rgb), out)
    for maxc in (200, 17, 5):
        packed, _, ts, te, sig, rgb = TG._packed_case(21, R=300 if maxc == 200 else 1200, maxc=maxc)
        entry_points(ops, f'packed_case maxc {maxc}', *dev(packed, ts, te, sig, rgb), out)
    # sixteen rays per wave: 524,288 rays of two samples
    R = 524288
    g = torch.Generator(device='cuda').manual_seed(3)
    packed = torch.stack([torch.arange(R) * 2, torch.full((R,), 2)], -1).to(torch.int32).cuda()
    ts = torch.rand(2 * R, device='cuda', generator=g) * 1.5
    te, sig, rgb = ts + 5e-3, torch.exp(torch.randn(2 * R, device='cuda', generator=g) * 2 + 2), torch.rand(2 * R, 3, device='cuda', generator=g)
    big = {}
    nc, ex = ops.visibility_count(sig, ts, te, packed, 1e-4, want_exsum=True)
    flatten('by16/visibility_count', (nc, ex), big)
    flatten('by16/composite_fwd', ops.composite_fwd(sig, rgb, ts, te, packed), big)
    x01, sel = torch.rand(2 * R, 3, device='cuda', generator=g), torch.zeros(2 * R, dtype=torch.uint8, device='cuda')
    packed2 = torch.stack([2 * R - packed[:, 0] - 2, packed[:, 1]], -1).to(torch.int32).contiguous()
    head, tail = (sig * 0.01, ts, te, packed, x01, sel), (sig.flip(0).contiguous(), ts.flip(0).contiguous(), te.flip(0).contiguous(), packed2, x01, sel)
    nc2 = ops.visibility_count2(head[:4], tail[:4], 1e-4)
    flatten('by16/visibility_count2', nc2, big)
    flatten('by16/compact_prefix2', ops.compact_prefix2(head, tail, nc2, int(nc2.sum())), big)
    out.update(big)
    torch.cuda.synchronize()
    np.savez_compressed(path, **out)
    print(len(out), 'outputs ->', path)


def compare(a, b, record=None):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), sorted(set(A.files) ^ set(B.files))
    per_entry = {}
    for k in A.files:
        entry = k.split('/')[1].split('.')[0]
        e = per_entry.setdefault(entry, {'outputs': 0, 'equal': 0, 'differ': []})
        e['outputs'] += 1
        if A[k].shape == B[k].shape and np.array_equal(A[k], B[k], equal_nan=True):
            e['equal'] += 1
        else:
            e['differ'].append(k)
    res = {'outputs': len(A.files), 'all_equal': all(not e['differ'] for e in per_entry.values()), 'per_entry_point': per_entry}
    print(json.dumps(res, indent=1))
    if record:
        json.dump(res, open(record, 'w'), indent=1)
    return 0 if res['all_equal'] else 1


if __name__ == '__main__':
    sys.exit(run(sys.argv[2]) if sys.argv[1] == 'run' else compare(*sys.argv[2:]))
