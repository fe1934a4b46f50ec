"""Training with the step riders on and off (NeRFScene.step_riders; PERF_STEP_RIDERS): 40 geometry steps and 40 colour steps on a 64 x 32
panorama with the device generator, eager and graph-replayed, with one occupancy update and one capacity change (re-captured) in the middle
of the geometry phase.  The k-th batch consumed is the k-th batch drawn and every counter is booked to the step that consumes the batch:
parameters, Adam moments, sample counters, per-step losses and per-step marched counts are torch.equal either way."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH, STEPS = 1024, 40
UPDATE_AT, CAPACITY_AT = 15, 25


def _scene():
    from perf_amd import synthetic
    from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays
    torch.manual_seed(0)
    scene = NeRFScene(dtype='bf16')
    rays = gen_pano_rays(torch.eye(4), 32, 64)
    dist, rgb = synthetic.room(rays.d)
    pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
    scene.train_conf.pixel_loss_batch_size = BATCH
    scene.set_train(); scene.prepare_occupancy(pool); scene.nerf.reset_geo()
    scene.renderer.head_samples = None                       # the one-phase sampler
    scene.renderer.sample_capacity = BATCH * scene.TRAIN_SAMPLES_PER_RAY
    scene.auto_shrink_capacity = False
    return scene, pool


def _thicker(scene):
    """An occupancy update: every occupied cell's +x neighbour becomes occupied too."""
    b = scene.estimator.binaries.reshape(256, 256, 256)
    scene.estimator.set_binaries((b | torch.roll(b, 1, 0)).reshape(-1))


def _run(riders, graph):
    scene, pool = _scene()
    scene.step_riders = riders
    log = {'loss': [], 'marched': [], 'set': []}
    out = {}
    for kind in ('geo', 'app'):
        net = scene.nerf.geo_mlp if kind == 'geo' else scene.nerf.app_mlp
        conf = scene.train_conf.geo_optimizer if kind == 'geo' else scene.train_conf.app_optimizer
        opt = scene.make_optimizer(net, conf.init_lr)
        eager = scene.train_one_step_geo if kind == 'geo' else scene.train_one_step_app
        replay = None
        for i in range(STEPS):
            if kind == 'geo' and i == UPDATE_AT:
                _thicker(scene)
                replay = None
            if kind == 'geo' and i == CAPACITY_AT:
                scene.renderer.sample_capacity = BATCH * 96
                replay = None
            lr, progress = scene.lr_at(conf, i / STEPS), i / STEPS
            if graph and i >= 2:
                if replay is None:
                    replay = scene.make_graphed_step(kind, opt, pool, warmup=0)
                replay(lr, progress)
            else:
                scene.update_lr(opt, conf, i / STEPS)
                eager(opt, pool, progress=progress)
            log['loss'].append([float(v() if callable(v) else v) for _, v in sorted(scene.last_losses.items())])
            log['marched'].append(int(scene._last_counts[0].item()))
            log['set'].append(scene._march_set is not None)
        out[kind] = (net.params.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count)
    scene._riders_drop()
    out['counters'] = scene.sample_counters.clone()
    out['draws'] = int(scene._rng_counter.item())
    return out, log


@pytest.mark.parametrize('graph', [False, True])
def test_training_with_riders_equals_training_without(graph):
    off, log_off = _run(False, graph)
    on, log_on = _run(True, graph)
    # the riders really carried the geometry phase (and nothing of the colour phase: its steps take the stand-alone chain)
    assert log_on['set'] == [True] * STEPS + [False] * STEPS and not any(log_off['set'])
    assert on['draws'] == off['draws'] == 2 * STEPS
    assert log_on['marched'] == log_off['marched'] and min(log_on['marched']) > 0
    assert log_on['loss'] == log_off['loss']
    assert torch.equal(on['counters'], off['counters']) and int(on['counters'][2]) == 2 * STEPS
    for kind in ('geo', 'app'):
        for a, b in zip(on[kind][:3], off[kind][:3]):
            assert torch.equal(a, b), kind
        assert on[kind][3] == off[kind][3]
    assert on['geo'][3] > STEPS // 2 and on['app'][3] > STEPS // 2          # (steps were taken, not skipped)


def test_the_environment_switch_turns_the_riders_off(monkeypatch):
    from perf_amd.scene import NeRFScene
    monkeypatch.setenv('PERF_STEP_RIDERS', '0')
    assert NeRFScene(dtype='bf16').step_riders is False
    monkeypatch.delenv('PERF_STEP_RIDERS')
    assert NeRFScene(dtype='bf16').step_riders is True


def _interleaved(riders, captured_app):
    """Geometry replays with colour steps in between (eager, or replays of a captured colour step): both consume the one draw stream."""
    scene, pool = _scene()
    scene.step_riders = riders
    geo, app = scene.nerf.geo_mlp, scene.nerf.app_mlp
    og, oa = scene.make_optimizer(geo, 1e-3), scene.make_optimizer(app, 1e-3)
    scene.update_lr(og, scene.train_conf.geo_optimizer, 0.1); scene.update_lr(oa, scene.train_conf.app_optimizer, 0.1)
    scene.train_one_step_geo(og, pool, progress=0.5)
    scene.train_one_step_app(oa, pool, progress=0.5)
    replay_geo = scene.make_graphed_step('geo', og, pool, warmup=0)
    replay_app = scene.make_graphed_step('app', oa, pool, warmup=0) if captured_app else None
    held = replay_geo.state['set']
    marched, sets = [], []
    for rounds in range(3):
        for _ in range(3):
            replay_geo(1e-3, 0.5)
            marched.append(int(replay_geo.state['counts'][0].item()))      # (the captured step's own count: scene._last_counts is the last EAGER step's)
            sets.append(scene._march_set is not None and scene._march_set is replay_geo.state['set'])
        for _ in range(2):
            if captured_app:
                replay_app(1e-3, 0.5)
                marched.append(int(replay_app.state['counts'][0].item()))
            else:
                scene.train_one_step_app(oa, pool, progress=0.5)
                marched.append(int(scene._last_counts[0].item()))
    scene._riders_drop()
    torch.cuda.synchronize()
    return dict(geo=geo.params.detach().clone(), app=app.params.detach().clone(), mg=og.exp_avg.clone(), ma=oa.exp_avg.clone(),
                counters=scene.sample_counters.clone(), draws=int(scene._rng_counter.item()), marched=marched, sets=sets, held=held,
                steps=(og.step_count, oa.step_count))


@pytest.mark.parametrize('captured_app', [False, True])
def test_a_geometry_graph_replayed_after_a_colour_step_trains_on_the_next_batch_of_the_stream(captured_app):
    """A colour step between two replays of a captured geometry step takes the next draw of the stream and drops the set the geometry
    graph was captured on.  The graph keeps that set alive (no replay ever touches memory that went back to the allocator) and, finding
    it dropped, is captured again on a set filled with the draw that is next: the same training as with the riders off."""
    off = _interleaved(False, captured_app)
    on = _interleaved(True, captured_app)
    assert on['held'] is not None and off['held'] is None
    assert all(on['sets']) and not any(off['sets'])
    assert on['draws'] == off['draws'] == 2 + 3 * 5 and on['steps'] == off['steps']
    assert on['marched'] == off['marched'] and min(on['marched']) > 0
    for k in ('geo', 'app', 'mg', 'ma', 'counters'):
        assert torch.equal(on[k], off[k]), k
