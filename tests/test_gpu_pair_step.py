"""The pair table in the training steps (NeRFScene.pair_encode, include/perf_hip_pair.h): the Adam entry that keeps a half current, the MLP
forward through row indices, and the steps themselves -- with the pair encode on, every step leaves the parameters, optimizer moments,
counters and colours of the two-encode path, bit for bit, eagerly and graph-captured."""
import pytest
import torch

pytestmark = pytest.mark.gpu


# ---- 2. pair table maintenance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vector_path', [True, False])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_adam_with_pair_refresh(dtype, vector_path):
    from perf_amd import ops
    from perf_amd.grid import GridConfig
    cfg = GridConfig(log2_hashmap_size=10)
    n_net = 4098                                 # (even, not a multiple of 4: the table starts 4-byte, not 8- or 16-byte aligned in w16)
    n = n_net + cfg.n_params
    g = torch.Generator().manual_seed(4)
    t16 = ops.torch_dtype(dtype)

    def state():
        # (vector_path False: fp32 arrays that start 4 bytes into their allocation take the one-element-per-thread kernel)
        mk = lambda t: (t.cuda() if vector_path else torch.cat([torch.zeros(1), t]).cuda()[1:])
        gen = torch.Generator().manual_seed(9)
        p, m, v, gr = (mk(torch.randn(n, generator=gen) * s) for s in (0.1, 0.01, 1.0, 0.05))
        v = v.abs_() * 1e-4
        return p, m, v, gr, torch.zeros(n, dtype=t16, device='cuda')

    step = torch.tensor([3], dtype=torch.int32, device='cuda')
    lr = torch.tensor([1e-2], dtype=torch.float32, device='cuda')
    for field in (0, 1):
        for gate_value in (1, 0):
            gate = torch.tensor([gate_value], dtype=torch.int64, device='cuda')
            pair = torch.randint(-2 ** 31, 2 ** 31 - 1, (cfg.total, 2), generator=g, dtype=torch.int64).to(torch.int32).cuda()
            before = pair.clone()
            ref, got = state(), state()
            assert (got[0].data_ptr() % 16 == 0) == vector_path
            w0 = got[4].clone()
            ops.adam_step_dev(*ref[:4], step, lr, w16=ref[4], gate=gate)
            ops.adam_step_dev(*got[:4], step, lr, w16=got[4], gate=gate, pair=(pair, field, n_net))
            for a, b in zip(ref, got):
                assert torch.equal(a, b)
            assert torch.equal(pair[:, 1 - field], before[:, 1 - field])
            if gate_value:
                assert torch.equal(pair[:, field].contiguous().view(t16), got[4][n_net:]) and not torch.equal(got[4], w0)
            else:
                assert torch.equal(pair, before) and torch.equal(got[4], w0)      # gated off: nothing moves


# ---- 3. MLP forward through rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_levels', [16, 12])        # (12 levels: not a whole number of k-steps, the kernel's generic branch)
@pytest.mark.parametrize('n_hidden', [1, 2])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_mlp_forward_through_rows_equals_forward_on_materialised_rows(dtype, n_hidden, n_levels):
    from perf_amd import ops
    from perf_amd.grid import MlpConfig
    mlp = MlpConfig(n_levels=n_levels, n_hidden_layers=n_hidden, n_output_dims=1 if n_hidden == 1 else 3,
                    output_activation='Exponential' if n_hidden == 1 else 'Sigmoid')
    g = torch.Generator().manual_seed(n_hidden)
    t16 = ops.torch_dtype(dtype)
    w16 = (torch.randn(mlp.n_params, generator=g) * 0.15).to(t16).cuda()
    stride = 5003
    feat = (torch.randn(n_levels, stride, 2, generator=g) * 0.5).to(t16).cuda()
    for n in (1, 33, 4099):
        rows = {'repeated': torch.randint(0, 7, (n,), generator=g), 'random': torch.randint(0, stride, (n,), generator=g),
                'descending': torch.arange(stride - 1, stride - 1 - n, -1)}
        sel = (torch.rand(n, generator=g) > 0.2).to(torch.uint8).cuda()
        for name, idx in rows.items():
            idx = idx.to(torch.int32).cuda()
            want = ops.mlp_fwd(mlp, w16, feat[:, idx.long()].contiguous(), sel)
            got = ops.mlp_fwd(mlp, w16, ops.IndexedFeat(feat, idx), sel)
            assert torch.equal(got, want), (n, name)
            if n > 1:                            # a device-side count below n: the live rows are what they were
                live = n - n // 3
                n_dev = torch.tensor([live], dtype=torch.int64, device='cuda')
                got = ops.mlp_fwd(mlp, w16, ops.IndexedFeat(feat, idx), sel, n_dev=n_dev)
                assert torch.equal(got[:live], want[:live]), (n, name)


# ---- 4. step identity ------------------------------------------------------------------------------------------------------------------
R, S = 256, 32


def _scene(pair, eps, reuse, head=None, grid_conf=None, app_log2_t=None):
    from perf_amd import synthetic, tcnn
    from perf_amd.fields import _grid_cfg
    from perf_amd.scene import NeRFScene, Rays, SupInfoPool, gen_pano_rays
    torch.manual_seed(0)
    scene = NeRFScene(dtype='bf16', grid_conf=grid_conf)
    if app_log2_t is not None:                  # a colour field over another grid than the density field's
        scene.nerf.app_mlp = tcnn.NetworkWithInputEncoding(
            3, 3, _grid_cfg(16, app_log2_t), {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 64,
                                              "n_hidden_layers": 2}, dtype='bf16')
    rays = gen_pano_rays(torch.eye(4), 32, 64)
    dist, rgb = synthetic.room(rays.d)
    pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
    scene.train_conf.pixel_loss_batch_size = R
    scene.set_train()
    scene.estimator.set_binaries(torch.ones(256 ** 3, dtype=torch.uint8, device='cuda'))      # all-occupied: fixed-count marching
    r = scene.renderer
    r.render_step_size = 0.99 / S; r.far_plane = 1.5; r.max_steps = S; r.head_samples = head; r.early_stop_eps = eps
    r.sample_capacity = R * S
    scene.pair_encode = pair
    scene.reuse_sampling_features = reuse
    scene.nerf.reset_geo()
    scene.sample_counters.zero_()
    g = torch.Generator(device='cuda'); g.manual_seed(5)
    idx = torch.randint(0, len(pool), (R,), device='cuda', generator=g)
    pool.rand_ray_color_data = lambda bs, **kw: (Rays(pool.all_sup_rays.o[idx], pool.all_sup_rays.d[idx]), pool.all_sup_colors[idx],
                                                  pool.all_sup_distances[idx], pool.all_sup_normals[idx])
    rand = {'jitter': torch.rand(R, device='cuda', generator=g), 'noise': torch.rand(R, 1, device='cuda', generator=g),
            'bg': torch.rand(R, 3, device='cuda', generator=g)}
    return scene, pool, rand


def _run(pair, eps, reuse, graph):
    """4 geometry steps, 4 colour steps, 2 geometry steps, reset_geo, 2 geometry steps -> a snapshot after every step."""
    from perf_amd import ops
    scene, pool, rand = _scene(pair, eps, reuse)
    scene.count_graph_nodes = graph
    eager = {'geo': scene.train_one_step_geo, 'app': scene.train_one_step_app}
    shots, nodes = [], {}

    def snap(opt):
        shots.append((scene.nerf.geo_mlp.params.detach().clone(), scene.nerf.app_mlp.params.detach().clone(), opt.exp_avg.clone(),
                      opt.exp_avg_sq.clone(), scene.sample_counters.clone(), scene.last_colors.clone()))

    for kind, steps, reset in (('geo', 4, False), ('app', 4, False), ('geo', 2, False), ('geo', 2, True)):
        if reset:
            scene.nerf.reset_geo()
        net = scene.nerf.geo_mlp if kind == 'geo' else scene.nerf.app_mlp
        opt = scene.make_optimizer(net, 0.0)
        conf = scene.train_conf.geo_optimizer
        step = lambda o_, p_, progress, **kw: eager[kind](o_, p_, progress=progress, rand=rand)
        scene.update_lr(opt, conf, 0.1)
        step(opt, pool, progress=0.5); snap(opt)
        if graph:
            setattr(scene, 'train_one_step_' + kind, step)
            replay = scene.make_graphed_step(kind, opt, pool, warmup=0)
            setattr(scene, 'train_one_step_' + kind, eager[kind])
            nodes.setdefault(kind, scene.graph_nodes[kind])
        for i in range(steps - 1):
            if graph:
                replay(scene.lr_at(conf, 0.1), 0.5)
            else:
                scene.update_lr(opt, conf, 0.1)
                step(opt, pool, progress=0.5)
            snap(opt)
    # which encodes one more eager step of each kind launches (after the snapshots: HIP events around every C-ABI call)
    launches = {}
    for kind in ('geo', 'app'):
        opt = scene.make_optimizer(scene.nerf.geo_mlp if kind == 'geo' else scene.nerf.app_mlp, 0.0)
        scene.update_lr(opt, scene.train_conf.geo_optimizer, 0.1)
        ops.start_kernel_timing()
        eager[kind](opt, pool, progress=0.5, rand=rand)
        prof = ops.stop_kernel_timing()
        launches[kind] = tuple(prof.get(k, (0, 0.0))[0] for k in ('perf_hashgrid_fwd_pair', 'perf_hashgrid_fwd'))
    return shots, scene, nodes, launches


@pytest.mark.parametrize('reuse', [True, False])
@pytest.mark.parametrize('eps', [1e-4, 0.6])
def test_steps_with_the_pair_encode_equal_the_two_encode_steps(eps, reuse):
    """eps 1e-4: every marched sample is kept (a fresh field is nearly transparent).  eps 0.6: a fresh field's density exp(~0) = 1
    leaves T = exp(-t) along a ray of length 0.99, below 0.6 from t = 0.51 on -- about half of every ray is dropped, so the kept
    samples are rows of the marched ones (the case that exercises the row indices); asserted from the counters.
    reuse False is the strict two-evaluation order: the sampler's density pass stays a single encode and the geometry step's two
    encodes of the kept samples are ONE pair encode."""
    for graph in (False, True):
        off, scene_off, nodes_off, launched_off = _run(False, eps, reuse, graph)
        on, scene, nodes_on, launched_on = _run(True, eps, reuse, graph)
        assert len(on) == len(off) == 12
        assert scene.nerf.__dict__.get('_pair') is not None and scene_off.nerf.__dict__.get('_pair') is None
        # (pair launches, single-encode launches) of a geometry / a colour step
        assert launched_off == {'geo': (0, 2 if reuse else 3), 'app': (0, 2)}, launched_off
        assert launched_on == {'geo': (1, 0 if reuse else 1), 'app': (1, 0)}, launched_on
        if graph:                                # one node fewer in either captured step
            assert nodes_on['geo'] == nodes_off['geo'] - 1 and nodes_on['app'] == nodes_off['app'] - 1, (nodes_on, nodes_off)
        prev = torch.zeros(2, dtype=torch.int64)
        for k, (a, b) in enumerate(zip(off, on)):
            for x, y in zip(a, b):
                assert torch.equal(x, y), (graph, k)
            marched, kept = (b[4][:2].cpu() - prev).tolist()
            prev = b[4][:2].cpu()
            assert 0 < marched <= R * S and b[4][2].item() == k + 1, (k, b[4].tolist())
            assert (kept == marched) if eps < 1e-3 else (0 < kept < marched), (k, kept, marched)


# ---- 5. fallbacks ----------------------------------------------------------------------------------------------------------------------
LINE_LOCAL = {'n_levels': 16, 'log2_hashmap_size': 18, 'sb_shift': (3, 3, 2), 'local_min_res': 64, 'layout': 'line_local'}


@pytest.mark.parametrize('case', ['two_phase', 'unequal_grids', 'line_local'])
def test_fallbacks_take_the_two_encodes_and_give_their_results(case):
    kw = {'two_phase': {'head': 2}, 'unequal_grids': {'app_log2_t': 17}, 'line_local': {'grid_conf': LINE_LOCAL}}[case]
    out = {}
    for pair in (False, True):
        scene, pool, rand = _scene(pair, 1e-4, True, **kw)
        opt = scene.make_optimizer(scene.nerf.geo_mlp, 0.0)
        for i in range(2):
            scene.update_lr(opt, scene.train_conf.geo_optimizer, 0.1)
            scene.train_one_step_geo(opt, pool, progress=0.5, rand=rand)
        assert scene.nerf.__dict__.get('_pair') is None and getattr(scene.nerf.geo_mlp, '_pair_half', None) is None
        out[pair] = (scene.nerf.geo_mlp.params.detach().clone(), opt.exp_avg.clone(), scene.last_colors.clone())
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)


def test_unequal_grids_and_line_local_tables_are_not_paired():
    from perf_amd.fields import NGPNeRF
    from perf_amd.grid import GridConfig
    aabb = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    nerf = NGPNeRF(aabb, log2_hashmap_size=12)
    assert nerf.pair_supported() and nerf.use_pair(True) is not None
    for field, net in enumerate((nerf.geo_mlp, nerf.app_mlp)):          # both halves were filled from the working copies
        assert torch.equal(nerf._pair.buf[:, field].contiguous().view(net.working_copy().dtype), net.working_copy()[net.mlp.n_params:])
    nerf.reset_geo()                                                      # a new network: its half is stale until the next use
    nerf.use_pair(True)
    assert torch.equal(nerf._pair.buf[:, 0].contiguous().view(nerf.geo_mlp.working_copy().dtype), nerf.geo_mlp.working_copy()[nerf.geo_mlp.mlp.n_params:])
    with torch.no_grad():
        nerf.app_mlp.params.mul_(2.0)                                     # (load_state_dict and the like: the master's version moves)
    nerf.use_pair(True)
    assert torch.equal(nerf._pair.buf[:, 1].contiguous().view(nerf.app_mlp.working_copy().dtype), nerf.app_mlp.working_copy()[nerf.app_mlp.mlp.n_params:])
    assert nerf.use_pair(False) is None and nerf.geo_mlp._pair_half is None
    nerf.app_mlp.grid = GridConfig(log2_hashmap_size=11)
    assert not nerf.pair_supported()
    assert not NGPNeRF(aabb, log2_hashmap_size=12, layout='line_local', sb_shift=(3, 3, 2)).pair_supported()
    assert not NGPNeRF(aabb, n_levels=20, log2_hashmap_size=12).pair_supported()
