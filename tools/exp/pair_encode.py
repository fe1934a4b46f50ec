#!/usr/bin/env python
"""Pair-encode probe (go / no-go of the pair table): ONE launch of hashgrid_fwd_pair_kernel on a pair table against the
sum of TWO perf_hashgrid_fwd launches on the two fields' own tables, same positions -- (train) 8192 rays x 128 lattice samples from one
origin in ray order, as bench.py's step encodes them; (random) as many uniform points.  HIP events in one process, the two sides
alternating in order from round to round; both feature arrays must be torch.equal to the single encodes'.

    python tools/exp/pair_encode.py [--out FILE]   (the JSON goes to standard output without --out) [--groupings 0,1,2,10] [--forms 0,1,5,6,2]

--groupings: values of PERF_PAIR_GROUPING, the level-grouping switch of tools/exp/pair_encode_variants.diff: 0 (the kept grouping, all
the committed library has) hashed levels alone + dense levels beside the finest hashed ones, 1 every level alone in two halves of
eight, 2 the single encode's {g, 15 - g}; + 10: features leave with non-temporal stores.  The committed library ignores the switch, so
anything but 0 is refused unless --variant-build says that the library was built with that diff applied; the JSON records which.

--forms: values of PERF_PAIR_FORM, the switch of tools/exp/pair_levels_variants.diff (the level-at-a-time body): 0 the kept
form (rolled levels, the kept grouping), 1 rolled levels with every level in a slot of its own, 5 and 6 the kept form held to 5 and 6
waves per SIMD, 2 two samples per thread (chunks of 512).  Same rule: anything but 0 needs --variant-build (a library built with THAT
diff).  --label names the library in the JSON (the parent commit's, this tree's, the variant build).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def samples(kind, dev):
    import torch
    g = torch.Generator().manual_seed(3)
    if kind == 'train':
        R, S = 8192, 128
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        t = (torch.arange(S)[None, :] + torch.rand(R, 1, generator=g)) * (0.99 / S)
        return (0.5 + 0.5 * d[:, None, :] * t[:, :, None]).reshape(-1, 3).contiguous().to(dev)
    return torch.rand(1 << 20, 3, generator=g).to(dev)


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--groupings', default='0')
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--forms', default=None)
    ap.add_argument('--label', default=None)
    ap.add_argument('--variant-build', action='store_true', help='the library was built with the variants diff of the switch in use applied')
    a = ap.parse_args()
    if a.groupings != '0' and not a.variant_build:
        sys.exit('--groupings other than 0 need a library built with tools/exp/pair_encode_variants.diff applied (--variant-build)')
    if a.forms not in (None, '0') and not a.variant_build:
        sys.exit('--forms other than 0 need a library built with tools/exp/pair_levels_variants.diff applied (--variant-build)')
    if a.forms is not None and a.groupings != '0':
        sys.exit('--forms and --groupings belong to two different variant builds')
    switch, key, values = ('PERF_PAIR_FORM', 'forms', a.forms) if a.forms is not None else ('PERF_PAIR_GROUPING', 'groupings', a.groupings)
    import torch
    from perf_amd import ops
    from perf_amd.grid import GridConfig
    dev = torch.device('cuda', 0)
    cfg = GridConfig()
    g = torch.Generator().manual_seed(1)
    ta = ops.cast_params(((torch.rand(cfg.n_params, generator=g) * 2 - 1) * 0.5).to(dev), a.dtype)
    tb = ops.cast_params(((torch.rand(cfg.n_params, generator=g) * 2 - 1) * 0.5).to(dev), a.dtype)
    pair = ops.pair_table(cfg, dev)
    ops.pair_fill(pair, 0, ta); ops.pair_fill(pair, 1, tb)
    assert torch.equal(pair[:, 0].contiguous().view(ta.dtype), ta) and torch.equal(pair[:, 1].contiguous().view(tb.dtype), tb)
    res = {'dtype': a.dtype, 'rounds': a.rounds, 'launches_per_round': a.reps, 'sets': {},
           'library': 'built with tools/exp/pair_%s_variants.diff applied' % ('levels' if a.forms is not None else 'encode') if a.variant_build else 'as committed (kept form only)'}
    if a.label:
        res['label'] = a.label
    for kind in ('train', 'random'):
        x = samples(kind, dev)
        fa, fb = ops.hashgrid_fwd(cfg, x, ta), ops.hashgrid_fwd(cfg, x, tb)

        def two():
            ops.hashgrid_fwd(cfg, x, ta); ops.hashgrid_fwd(cfg, x, tb)

        row = {'n': x.shape[0], key: {}}
        for grouping in values.split(','):
            os.environ[switch] = grouping

            def one():
                ops.hashgrid_fwd_pair(cfg, x, pair, a.dtype)

            pa, pb = ops.hashgrid_fwd_pair(cfg, x, pair, a.dtype)
            equal = bool(torch.equal(pa, fa) and torch.equal(pb, fb))
            for _ in range(3):
                one(); two()
            t_pair, t_two = [], []
            for r in range(a.rounds):
                for side in ((one, two) if r % 2 == 0 else (two, one)):
                    (t_pair if side is one else t_two).append(timed(side, a.reps))
            row[key][grouping] = {'torch_equal': equal, 'pair_ms': [round(t, 4) for t in t_pair], 'two_singles_ms': [round(t, 4) for t in t_two],
                                          'slowest_pair_over_fastest_two': round(max(t_pair) / min(t_two), 4)}
            print(kind, key[:-1], grouping, 'equal', equal, 'pair', [round(t, 4) for t in t_pair], 'two singles', [round(t, 4) for t in t_two], flush=True)
        res['sets'][kind] = row
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    else:
        print(json.dumps(res))


if __name__ == '__main__':
    main()
