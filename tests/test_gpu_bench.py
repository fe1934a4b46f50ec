"""bench.py's plain run (no --full): the headline line alone, K timed steps, and --dump-outputs writing the last timed step's
results -- the same arrays, bit for bit, when the same arguments run twice."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--gpus', '1', '--rays-per-gpu', '1024', '--height', '128', '--width', '256']


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize('mode', ['train_geo', 'render'])
def test_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path, mode):
    runs = []
    for i in range(2):
        out = tmp_path / f'out{i}'
        line = _bench(SMALL + ['--mode', mode, '--steps', '7', '--warmup', '2', '--dump-outputs', str(out)])
        assert line['metric'].startswith('ray-samples/sec') and line['unit'] == 'ray-samples/s' and line['higher_is_better'] is True
        assert line['steps'] == 7 and line['warmup'] == 2 and line['ms_per_step'] > 0 and line['value'] > 0 and line['dtype'] in ('bf16', 'fp16')
        # what only --full measures is absent from a plain run
        for k in ('sustained', 'psnr', 'roofline', 'cpu_baseline', 'kernels'):
            assert line[k] is None, k
        for k in ('render', 'config4', 'config5', 'train_app', 'faithful', 'summary'):
            assert k not in line, k
        files = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        if mode == 'train_geo':
            assert {'geo_params', 'n_marched', 'n_kept', 'depth_loss', 'dist_loss'} <= set(files), sorted(files)
            assert files['geo_params'].ndim == 1 and np.isfinite(files['geo_params']).all()
            assert 0 < float(files['n_kept'].sum()) <= float(files['n_marched'].sum()) <= 1024 * 128
        else:
            assert {'rgb', 'distance', 'n_marched', 'n_kept'} <= set(files), sorted(files)
            assert files['rgb'].shape == (32768, 3) and np.isfinite(files['rgb']).all()
        runs.append(files)
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
