#!/usr/bin/env python
"""ms per launch (HIP events, ops.start_kernel_timing) of the entry points of csrc/composite.hip that tools/exp/team_shape_ab.py does not
cover, at 8,192 rays x 128 samples and 8,192 rays x 2 samples: the ray heads, the compositing backward with and without the distortion
loss, the stand-alone distortion loss, accumulation, the loss kernels and the two-source visibility / compaction.  One JSON object; run it
once per library build, alternating the builds, and compare medians against the other build's spread."""
import json
import os
import sys

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from perf_amd import ops

R = 8192
out = {}
for spp in (128, 2):
    g = torch.Generator(device='cuda').manual_seed(spp)
    S = R * spp
    packed = torch.stack([torch.arange(R) * spp, torch.full((R,), spp)], -1).to(torch.int32).cuda()
    ts = torch.rand(S, device='cuda', generator=g) * 1.5
    te = ts + 5e-3
    sig = torch.exp(torch.randn(S, device='cuda', generator=g) * 2 - 1)
    rgb = torch.rand(S, 3, device='cuda', generator=g)
    gt_d, noise, gt_c, bg = (torch.rand(*s, device='cuda', generator=g) for s in ((R,), (R,), (R, 3), (R, 3)))
    ratio = torch.tensor([0.6], device='cuda')
    x01, sel = torch.rand(S, 3, device='cuda', generator=g), torch.zeros(S, dtype=torch.uint8, device='cuda')
    thin = (sig * 0.01).contiguous()

    def step():
        w, T, op, dist, col, dl = ops.composite_distloss_fwd(sig, rgb, ts, te, packed)
        g_op, g_d, sc = ops.geo_loss(op, dist, gt_d, noise, dl, packed, R, 1.0, 0.5, ratio, 128.0)
        ops.composite_distloss_bwd(sig, ts, te, packed, w, T, op, dist, g_op, g_d, 1.0, scale_dev=sc[2:3])
        g_col, _ = ops.app_loss(op, col, bg, gt_c, R, 1.0, 128.0)
        ops.composite_bwd(sig, ts, te, packed, w, T, g_opacity=g_op, g_distance=g_d, g_color=g_col, want_drgb=True)
        ops.train_head_geo(sig, rgb, ts, te, packed, gt_d, noise, R, 1.0, 0.5, ratio, 128.0)
        ops.train_head_app(sig, rgb, ts, te, packed, bg, gt_c, R, 1.0, 128.0)
        ops.distloss_fwd(w, ts, te, packed)
        ops.distloss_bwd(w, ts, te, packed, 0.3)
        ops.accumulate_fwd(w, rgb, packed)
        nc2 = ops.visibility_count2((thin, ts, te, packed), (thin, ts, te, packed), 1e-4)
        ops.compact_prefix2((thin, ts, te, packed, x01, sel), (thin, ts, te, packed, x01, sel), nc2, 2 * S)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ops.start_kernel_timing()
    for _ in range(20):
        step()
    k = ops.stop_kernel_timing()
    out[f'{spp} samples/ray, {R} rays'] = {n: round(ms, 5) for n, (c, ms) in k.items()}
print(json.dumps(out))
