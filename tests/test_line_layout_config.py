"""Host-side plumbing of the line-local table layouts for training (no device needed): GridConfig.from_tcnn's optional layout keys,
the identity of the default configuration, and the refusals that need no GPU."""
import numpy as np
import pytest

from perf_amd.grid import LOCAL_MIN_RES, GridConfig

TCNN_CFG = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 18, "base_resolution": 16,
            "per_level_scale": 1.4472692012786865}


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ('scale', 'res', 'size', 'offset', 'hashed', 'local', 'nsx', 'nsxy')) \
        and a.total == b.total and a.layout == b.layout and a.sb_shift == b.sb_shift


def test_from_tcnn_without_layout_keys_is_todays_grid():
    g = GridConfig.from_tcnn(TCNN_CFG)
    assert g.layout == 'tcnn' and g.local_min_res == LOCAL_MIN_RES and not g.local.any()
    assert _same(g, GridConfig(n_levels=16, log2_hashmap_size=18))


@pytest.mark.parametrize('layout', ['line_local', 'line_overlap'])
def test_from_tcnn_reads_the_layout_keys(layout):
    g = GridConfig.from_tcnn(dict(TCNN_CFG, layout=layout, sb_shift=[3, 3, 2], local_min_res=32))
    ref = GridConfig(n_levels=16, log2_hashmap_size=18, layout=layout, sb_shift=(3, 3, 2), local_min_res=32)
    assert g.layout == layout and g.sb_shift == (3, 3, 2) and g.local_min_res == 32 and _same(g, ref)
    # the line-local levels are a suffix (what perf_hashgrid_bwd_lines requires)
    first = int(np.argmax(g.local))
    assert g.local[first:].all() and not g.local[:first].any() and all(g.res[:first] < 32) and all(g.res[first:] >= 32)
    with pytest.raises(ValueError):
        GridConfig.from_tcnn(dict(TCNN_CFG, layout='zorder'))


def test_default_scene_grid_config_is_unchanged():
    from perf_amd.fields import _grid_cfg
    assert _grid_cfg(16, 18) == TCNN_CFG
    assert _grid_cfg(16, 18, layout_kw=None) == TCNN_CFG


def test_line_overlap_init_is_canonical():
    import torch
    from perf_amd import tcnn
    from perf_amd.grid import MlpConfig
    g = GridConfig(n_levels=8, log2_hashmap_size=14, per_level_scale=2.0, layout='line_overlap', sb_shift=(3, 3, 2), local_min_res=32)
    p = tcnn._init_params(MlpConfig(8), g, 1337, 'cpu')
    t = p[MlpConfig(8).n_params:].clone()
    assert torch.equal(g.canonicalize_(t.clone()), t)


def test_scene_refuses_unknown_grid_conf_keys():
    from perf_amd.scene import NeRFScene
    with pytest.raises(ValueError, match='unknown keys'):
        NeRFScene(grid_conf={'layout': 'line_local', 'hashmap': 18})


def test_ops_refuse_without_a_device():
    import torch
    from perf_amd import ops
    x = torch.zeros(4, 3); d = torch.zeros(16, 4, 2)
    with pytest.raises(ValueError, match='hashgrid_bwd'):
        ops.hashgrid_bwd_lines(GridConfig(), x, d)                      # a tcnn grid goes through hashgrid_bwd
    g = GridConfig(layout='line_local', sb_shift=(3, 3, 2))
    with pytest.raises(ValueError, match='tcnn table layout'):
        ops.hashgrid_bwd_into(g, x, d, torch.zeros(g.n_params), shifts=torch.zeros(24, dtype=torch.int32), raw_fields=True)
