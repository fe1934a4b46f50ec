"""Dev tool: fp32-mode gradient tables of two builds of the library on the shapes of tests/test_gpu_bwd_owner_loop.py, compared to
the bit.  The owner loops keep the order in which entries enter a wave's queue, so a wave adds its floats in the same order under
either build; what the comparison cannot rule out is the order in which the sixteen waves of an owner reach one table entry, which is
not fixed from run to run.  Each library therefore runs TWICE (a process each): a case whose two runs of ONE library differ says
nothing about the other library.

    python tools/exp/bwd_owner_loop_fp32_ab.py A.so B.so        (on a GPU box; prints one JSON line)"""
import hashlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from perf_amd import _lib
_lib.LIB_PATH = {lib!r}
import numpy as np, torch
from perf_amd import ops
import test_gpu_bwd_owner_loop as T
out = {{}}
def put(tag, cfg, x, dfeat, n_dev=None):
    t = ops.hashgrid_bwd(cfg, x, dfeat, n_dev=n_dev)
    torch.cuda.synchronize()
    out[tag] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]
for log2_t in (18, 21):
    cfg = T._cfg(log2_hashmap_size=log2_t); g = torch.Generator().manual_seed(200 + log2_t)
    x = T._far_rows(4099, g); dfeat, _ = T._dfeat(cfg, 4099, g)
    put('far_T%d' % log2_t, cfg, x.cuda(), dfeat)
cfg = T._cfg()
for live in (5, 257):
    g = torch.Generator().manual_seed(400 + live)
    x = torch.rand(4096, 3, generator=g); x[live:] = float('nan'); dfeat, _ = T._dfeat(cfg, 4096, g)
    put('live_%d' % live, cfg, x.cuda(), dfeat, torch.tensor([live], dtype=torch.int64, device='cuda'))
for interpolation in ('Linear', 'Smoothstep'):
    for points in ('uniform', 'x_at_chunk_ends'):
        c = T._cfg(interpolation=interpolation); g = torch.Generator().manual_seed(500)
        x = torch.rand(4099, 3, generator=g)
        if points == 'x_at_chunk_ends': x[:, 0] = 0.999
        dfeat, _ = T._dfeat(c, 4099, g)
        put('dense_%s_%s' % (interpolation, points), c, x.cuda(), dfeat)
print('DIGESTS ' + json.dumps(out))
'''


def run(lib):
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), lib=os.path.abspath(lib))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f'{lib}: exit {r.returncode}\n{r.stderr[-3000:]}')
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('DIGESTS ')][0][8:])


a, b = sys.argv[1], sys.argv[2]
runs = {'a1': run(a), 'b1': run(b), 'a2': run(a), 'b2': run(b)}
res = {}
for case in runs['a1']:
    d = {k: v[case] for k, v in runs.items()}
    res[case] = {'a_reproducible': d['a1'] == d['a2'], 'b_reproducible': d['b1'] == d['b2'], 'a_equals_b': d['a1'] == d['b1'] and d['a2'] == d['b2']}
print(json.dumps({'a': a, 'b': b, 'cases': res}))
