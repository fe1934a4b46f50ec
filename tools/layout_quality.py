#!/usr/bin/env python
"""What the line-local table layouts cost and give when TRAINED (profiles/layout_quality.json).

  python tools/layout_quality.py [--out profiles/layout_quality.json] [--seeds 3] [--scenes room,doorway,pillars] [--no-quality]

Quality: the schedule of tests/psnr_parity_lib.py (256 x 512 panorama, 1,024-ray batches, 300 geometry + 300 colour iterations) through
NeRFScene(grid_conf=...) for tcnn / line_local / line_overlap at L16 and T = 18 / 16 (super-blocks of 8 x 8 x 4 vertices), each layout from
the module's own seeded initialisation: psnr@app150 / @app300, the depth error at the end of the geometry phase, and dPSNR against tcnn's
run of the same seed.  Speed (HIP events, same process): the fixed-point grid backward at L16 / T18 on 1 M uniform and 1 M ray-ordered
samples -- perf_hashgrid_bwd (tcnn layout) against perf_hashgrid_bwd_lines' LDS owners (with and without the tile-code pre-pass) and its
global-atomics scatter -- and at L20 with T = 22 / 24 (levels beyond 255 tiles: the scatter); the eager geometry step per layout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

GRID = {'n_levels': 16, 'sb_shift': (3, 3, 2), 'local_min_res': 64}
LAYOUTS = ('tcnn', 'line_local', 'line_overlap')


def _time(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2]


def _points(kind, n, g):
    if kind == 'uniform':
        return torch.rand(n, 3, generator=g, device='cuda')
    rays, per = n // 256, 256               # ray-ordered: 256 consecutive samples along each ray from a common origin region
    o = torch.rand(rays, 1, 3, generator=g, device='cuda') * 0.1 + 0.45
    d = torch.nn.functional.normalize(torch.randn(rays, 1, 3, generator=g, device='cuda'), dim=-1)
    t = torch.linspace(0.0, 0.45, per, device='cuda')[None, :, None]
    return (o + d * t).reshape(-1, 3).contiguous()


def speed():
    from perf_amd import ops
    from perf_amd.grid import GridConfig
    out = {}
    g = torch.Generator(device='cuda'); g.manual_seed(0)
    n = 1 << 20
    for kind in ('uniform', 'ray_ordered'):
        x = _points(kind, n, g)
        for L, T in ((16, 18), (20, 22), (20, 24)):
            dfeat = torch.randn(L, n, 2, generator=g, device='cuda') * 1e-2
            amax = torch.zeros(24, device='cuda'); amax[:L] = dfeat.abs().amax(dim=(1, 2))
            row = {}
            for layout in LAYOUTS:
                kw = {} if layout == 'tcnn' else {'sb_shift': GRID['sb_shift'], 'local_min_res': GRID['local_min_res']}
                cfg = GridConfig(n_levels=L, log2_hashmap_size=T, layout=layout, **kw)
                buf = torch.empty(cfg.n_params, device='cuda')
                if layout == 'tcnn':
                    row['tcnn_ms'] = _time(lambda: ops.hashgrid_bwd(cfg, x, dfeat, out=buf, level_absmax=amax))
                else:
                    row[layout + '_owners_ms'] = _time(lambda: ops.hashgrid_bwd_lines(cfg, x, dfeat, out=buf, level_absmax=amax))
                    row[layout + '_owners_no_codes_ms'] = _time(lambda: ops.hashgrid_bwd_lines(cfg, x, dfeat, out=buf, level_absmax=amax, use_codes=False))
                    row[layout + '_scatter_ms'] = _time(lambda: ops.hashgrid_bwd_lines(cfg, x, dfeat, out=buf, level_absmax=amax, use_owners=False))
                    row[layout + '_owner_levels'] = int(sum(1 for l in range(L) if cfg.local[l] and -(-int(cfg.size[l]) // 16384) <= 255))
            for layout in LAYOUTS[1:]:
                row[layout + '_owners_over_tcnn'] = row[layout + '_owners_ms'] / row['tcnn_ms']
                row[layout + '_scatter_over_owners'] = row[layout + '_scatter_ms'] / row[layout + '_owners_ms']
            out[f'{kind}_L{L}_T{T}'] = row
            print(kind, L, T, json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in row.items()}), flush=True)
    return out


def _grid_stats(grid):
    hashed_local = [l for l in range(grid.n_levels) if grid.hashed[l]]
    per = 0.75 if grid.layout == 'line_overlap' else 1.0
    return {'table_bytes_fp32': int(grid.n_params) * 4,
            'distinct_vertices_per_hashed_level': {int(l): int(int(grid.size[l]) * (per if grid.local[l] else 1.0)) for l in hashed_local}}


def train_run(layout, T, scene, draws, marks=(150, 300), n_geo=300, n_app=300, seed=0, batch=1024):
    from tests import psnr_parity_lib as P
    from perf_amd.scene import NeRFScene, Rays, SupInfoPool
    o, d, dist, rgb, occ = scene
    torch.manual_seed(seed)
    conf = {'n_levels': 16, 'log2_hashmap_size': T}
    if layout != 'tcnn':
        conf.update(GRID, layout=layout)
    sc = NeRFScene(dtype='fp16', grid_conf=conf)
    pool = SupInfoPool(); pool.register_rays(o.cuda(), d.cuda(), rgb.cuda(), dist.cuda())
    sc.train_conf.pixel_loss_batch_size = batch
    sc.set_train()
    sc.estimator.set_binaries(torch.from_numpy(occ.reshape(-1)).cuda())
    from perf_amd import tcnn           # (no reset_geo: for tcnn's layout it rebuilds the reference's L16 / T18 density grid)
    with torch.no_grad():       # the module's own initialisation under this seed (same draw for every layout)
        for net in (sc.nerf.geo_mlp, sc.nerf.app_mlp):
            net.params.copy_(tcnn._init_params(net.mlp, net.grid, tcnn.DEFAULT_SEED + seed, net.params.device))
    state = {'idx': None}
    pool.rand_ray_color_data = lambda bs, **kw: (Rays(pool.all_sup_rays.o[state['idx']], pool.all_sup_rays.d[state['idx']]),
                                                  pool.all_sup_colors[state['idx']], pool.all_sup_distances[state['idx']],
                                                  pool.all_sup_normals[state['idx']])
    rays = Rays(o.cuda(), d.cuda())
    res = {}
    oc = sc.train_conf.geo_optimizer
    opt = sc.make_optimizer(sc.nerf.geo_mlp, 0.0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(n_geo):
        dr = draws[i]; state['idx'] = dr['idx'].cuda()
        sc.update_lr(opt, oc, i / n_geo)
        sc.train_one_step_geo(opt, pool, progress=i / n_app, rand={k: dr[k].cuda() for k in ('jitter', 'bg', 'noise')})
    torch.cuda.synchronize()
    res['geo_step_ms_eager'] = (time.perf_counter() - t0) * 1e3 / n_geo
    ev = sc.render(rays, ['rgb', 'distance'])
    res['geo_end_depth_err'] = float((ev['distance'].cpu() - dist).abs().mean())
    sc.set_train()
    opt = sc.make_optimizer(sc.nerf.app_mlp, 0.0)
    for i in range(n_app):
        dr = draws[n_geo + i]; state['idx'] = dr['idx'].cuda()
        sc.update_lr(opt, oc, i / n_app)
        sc.train_one_step_app(opt, pool, progress=i / n_app, rand={k: dr[k].cuda() for k in ('jitter', 'bg', 'noise')})
        if i + 1 in marks:
            res[f'psnr@app{i + 1}'] = P.psnr(sc.render(rays, ['rgb'])['rgb'].cpu(), rgb); sc.set_train()
    res.update(_grid_stats(sc.nerf.geo_mlp.grid))
    return res


def quality(seeds, scenes):
    from tests import psnr_parity_lib as P
    rows = []
    warm = True
    for name in scenes:
        scene = P.make_scene(256, 512, name)
        if warm:        # (the first runs of a process pay one-time costs: not in any timed row)
            for layout in LAYOUTS:
                train_run(layout, 18, scene, P.make_draws(scene[0].shape[0], 1024, 40), marks=(), n_geo=20, n_app=20)
            warm = False
        for seed in range(seeds):
            draws = P.make_draws(scene[0].shape[0], 1024, 600, seed=seed)
            for T in (18, 16):
                base = None
                for layout in LAYOUTS:
                    r = train_run(layout, T, scene, draws, seed=seed)
                    r.update(scene=name, seed=seed, log2_hashmap_size=T, layout=layout)
                    if layout == 'tcnn':
                        base = r
                    else:
                        for k in ('psnr@app150', 'psnr@app300'):
                            r['d' + k] = r[k] - base[k]
                        r['d_geo_end_depth_err'] = r['geo_end_depth_err'] - base['geo_end_depth_err']
                    rows.append(r)
                    print(json.dumps({k: v for k, v in r.items() if k != 'distinct_vertices_per_hashed_level'}), flush=True)
    summary = {}
    for T in (18, 16):
        for layout in LAYOUTS[1:]:
            for k in ('dpsnr@app150', 'dpsnr@app300', 'd_geo_end_depth_err'):
                v = torch.tensor([r[k] for r in rows if r['layout'] == layout and r['log2_hashmap_size'] == T])
                if v.numel():
                    summary[f'{layout}_T{T}_{k}'] = {'mean': float(v.mean()), 'std': float(v.std()) if v.numel() > 1 else 0.0,
                                                     'min': float(v.min()), 'n': int(v.numel())}
    return rows, summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'layout_quality.json'))
    ap.add_argument('--seeds', type=int, default=3)
    ap.add_argument('--scenes', default='room,doorway,pillars')
    ap.add_argument('--no-quality', action='store_true')
    ap.add_argument('--no-speed', action='store_true')
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    rec = {'device': torch.cuda.get_device_name(0), 'grid': dict(GRID, sb_shift=list(GRID['sb_shift']))}
    if not a.no_speed:
        rec['speed_fixed_point_grid_bwd_1M'] = speed()
    if not a.no_quality:
        rec['quality_rows'], rec['quality_summary'] = quality(a.seeds, a.scenes.split(','))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
