"""End-to-end training of the line-local table layouts (NeRFScene(grid_conf=...)): L16 / T18, super-blocks of 8 x 8 x 4 vertices, on the
room of tests/psnr_parity_lib.py (256 x 512 panorama, 1,024-ray batches, 300 geometry + 300 colour iterations).  Every layout starts
from the module's own seeded initialisation, so the runs differ in the table layout only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import psnr_parity_lib as P  # noqa: E402

GRID = {'n_levels': 16, 'log2_hashmap_size': 18, 'sb_shift': (3, 3, 2), 'local_min_res': 64}
N_GEO, N_APP, BATCH = 300, 300, 1024


def _conf(layout):
    return dict(GRID, layout=layout) if layout != 'tcnn' else {'n_levels': 16, 'log2_hashmap_size': 18}


def _scene(layout, scene, batch=BATCH):
    from perf_amd.scene import NeRFScene, Rays, SupInfoPool
    o, d, dist, rgb, occ = scene
    torch.manual_seed(0)
    sc = NeRFScene(dtype='fp16', grid_conf=_conf(layout))
    pool = SupInfoPool(); pool.register_rays(o.cuda(), d.cuda(), rgb.cuda(), dist.cuda())
    sc.train_conf.pixel_loss_batch_size = batch
    sc.set_train()
    sc.estimator.set_binaries(torch.from_numpy(occ.reshape(-1)).cuda())
    sc.nerf.reset_geo()
    state = {'idx': None}
    pool.rand_ray_color_data = lambda bs, **kw: (Rays(pool.all_sup_rays.o[state['idx']], pool.all_sup_rays.d[state['idx']]),
                                                  pool.all_sup_colors[state['idx']], pool.all_sup_distances[state['idx']],
                                                  pool.all_sup_normals[state['idx']])
    return sc, pool, state


def _train(layout, scene, draws):
    from perf_amd.scene import Rays
    o, d, dist, rgb, occ = scene
    sc, pool, state = _scene(layout, scene)
    rays = Rays(o.cuda(), d.cuda())
    out = {'psnr@init': P.psnr(sc.render(rays, ['rgb'])['rgb'].cpu(), rgb)}
    sc.set_train()
    conf = sc.train_conf.geo_optimizer
    opt = sc.make_optimizer(sc.nerf.geo_mlp, 0.0)
    for i in range(N_GEO):
        dr = draws[i]; state['idx'] = dr['idx'].cuda()
        sc.update_lr(opt, conf, i / N_GEO)
        sc.train_one_step_geo(opt, pool, progress=i / N_APP, rand={k: dr[k].cuda() for k in ('jitter', 'bg', 'noise')})
    ev = sc.render(rays, ['rgb', 'distance'])
    out['geo_end_depth_err'] = float((ev['distance'].cpu() - dist).abs().mean())
    sc.set_train()
    opt_a = sc.make_optimizer(sc.nerf.app_mlp, 0.0)
    for i in range(N_APP):
        dr = draws[N_GEO + i]; state['idx'] = dr['idx'].cuda()
        sc.update_lr(opt_a, conf, i / N_APP)
        sc.train_one_step_app(opt_a, pool, progress=i / N_APP, rand={k: dr[k].cuda() for k in ('jitter', 'bg', 'noise')})
    out['psnr@app300'] = P.psnr(sc.render(rays, ['rgb'])['rgb'].cpu(), rgb)
    return out, sc, opt, opt_a


@pytest.fixture(scope='module')
def room():
    import __graft_entry__
    __graft_entry__.build()
    scene = P.make_scene(256, 512, 'room')
    draws = P.make_draws(scene[0].shape[0], BATCH, N_GEO + N_APP)
    return scene, draws


@pytest.fixture(scope='module')
def trained(room):
    scene, draws = room
    return {layout: _train(layout, scene, draws) for layout in ('tcnn', 'line_local', 'line_overlap')}


def _canonical(grid, t):
    return torch.equal(grid.canonicalize_(t.detach().clone()), t.detach())


def test_line_layouts_train_as_well_as_tcnns(trained):
    tc = trained['tcnn'][0]
    for layout in ('line_local', 'line_overlap'):
        r = trained[layout][0]
        print(layout, r, 'tcnn', tc)
        assert all(torch.isfinite(torch.tensor(v)) for v in r.values()), r
        assert r['psnr@app300'] >= r['psnr@init'] + 15.0, r
        assert r['psnr@app300'] >= tc['psnr@app300'] - 1.0, (layout, r, tc)


def test_line_overlap_copies_stay_equal_through_training(trained):
    """Adam is elementwise and both copies of a shared vertex receive the same gradient: master, moments and the 16-bit copy stay
    canonical bit for bit (no re-canonicalisation pass)."""
    _, sc, opt_g, opt_a = trained['line_overlap']
    for net, opt in ((sc.nerf.geo_mlp, opt_g), (sc.nerf.app_mlp, opt_a)):
        n_net = net.mlp.n_params
        for t in (net.params, opt.exp_avg, opt.exp_avg_sq, net.working_copy().float()):
            assert _canonical(net.grid, t[n_net:]), net.grid.layout


def test_line_layout_checkpoint_round_trip(trained, room):
    scene, _ = room
    _, sc, _, _ = trained['line_overlap']
    state = sc.state_dict()
    sc2, _, _ = _scene('line_overlap', scene)
    sc2.load_state_dict(state)
    assert sc2.nerf.geo_mlp.grid.layout == 'line_overlap'
    assert torch.equal(sc2.nerf.geo_mlp.params, sc.nerf.geo_mlp.params) and torch.equal(sc2.nerf.app_mlp.params, sc.nerf.app_mlp.params)
    tc, _, _ = _scene('tcnn', scene)
    with pytest.raises(ValueError, match='layout'):
        tc.load_state_dict(state)
    with pytest.raises(ValueError, match='layout'):
        sc2.load_state_dict(trained['tcnn'][1].state_dict())
    sc2.nerf.reset_geo()
    g = sc2.nerf.geo_mlp.grid
    assert (g.layout, g.sb_shift, g.log2_hashmap_size, g.n_levels) == ('line_overlap', (3, 3, 2), 18, 16)
    assert _canonical(g, sc2.nerf.geo_mlp.params[sc2.nerf.geo_mlp.mlp.n_params:])


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
def test_line_layout_graph_replay_equals_eager(room, layout):
    """A few geometry and colour steps captured as hipGraphs == the same steps eagerly, bit for bit."""
    scene, draws = room
    results = {}
    for mode in ('eager', 'graph'):
        sc, pool, state = _scene(layout, scene)
        state['idx'] = draws[0]['idx'].cuda()
        rand = {k: draws[0][k].cuda() for k in ('jitter', 'bg', 'noise')}
        sc.renderer.sample_capacity = BATCH * 128
        out = {}
        for kind in ('geo', 'app'):
            net = sc.nerf.geo_mlp if kind == 'geo' else sc.nerf.app_mlp
            opt = sc.make_optimizer(net, 0.0)
            step = sc.train_one_step_geo if kind == 'geo' else sc.train_one_step_app
            conf = sc.train_conf.geo_optimizer
            if mode == 'eager':
                for _ in range(5):
                    sc.update_lr(opt, conf, 0.1)
                    step(opt, pool, progress=0.5, rand=rand)
            else:
                wrapped = lambda o_, p_, progress, _s=step, **kw: _s(o_, p_, progress=progress, rand=rand)
                setattr(sc, 'train_one_step_geo' if kind == 'geo' else 'train_one_step_app', wrapped)
                sc.update_lr(opt, conf, 0.1)
                wrapped(opt, pool, progress=0.5)
                replay = sc.make_graphed_step(kind, opt, pool, warmup=0)
                for _ in range(4):
                    replay(sc.lr_at(conf, 0.1), 0.5)
            out[kind] = (net.params.detach().clone(), opt.exp_avg.clone(), int(opt.step_count))
        results[mode] = out
    for kind in ('geo', 'app'):
        pe, me, se = results['eager'][kind]; pg, mg, sg = results['graph'][kind]
        assert se == sg == 5
        assert torch.equal(pe, pg) and torch.equal(me, mg), kind


@pytest.mark.parametrize('conf', [None, {'n_levels': 16, 'log2_hashmap_size': 16}, dict(GRID, log2_hashmap_size=16, layout='line_local')])
def test_reset_geo_keeps_the_scenes_grid(conf):
    """NeRFScene(grid_conf=...) sizes BOTH fields, also across reset_geo (train_one_episode calls it every episode); no grid_conf
    is the reference's L16 / T18 density grid, bit for bit."""
    import __graft_entry__
    __graft_entry__.build()
    from perf_amd.grid import GridConfig
    from perf_amd.scene import NeRFScene
    sc = NeRFScene(dtype='fp16', grid_conf=conf)
    before = sc.nerf.geo_mlp.grid
    sc.nerf.reset_geo()
    g, app = sc.nerf.geo_mlp.grid, sc.nerf.app_mlp.grid
    for k in ('n_levels', 'log2_hashmap_size', 'layout', 'sb_shift', 'local_min_res', 'total'):
        assert getattr(g, k) == getattr(before, k) == getattr(app, k), k
    if conf is None:
        ref = GridConfig(n_levels=16, log2_hashmap_size=18)
        assert (g.total, g.layout) == (ref.total, 'tcnn') and sc.nerf.geo_mlp.encoding_config == {
            "otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 18, "base_resolution": 16,
            "per_level_scale": 1.4472692012786865}
    else:
        assert g.log2_hashmap_size == 16 and sc.nerf.geo_mlp.params.numel() == sc.nerf.geo_mlp.mlp.n_params + g.n_params
