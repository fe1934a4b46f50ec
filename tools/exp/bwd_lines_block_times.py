"""Dev tool: how long every workgroup of perf_hashgrid_bwd_lines takes (fixed point), by level -- the tcnn-rule prefix's owners
(hashgrid_bwd_kernel<true>, `BLOCKT`) and the line-local owners (hashgrid_bwd_lines_kernel<true>, `BLOCKT_LINES`).

Builds a copy of the library with -DPERF_BWD_BLOCK_TIMES (one thread of two workgroups per level and replica prints its wall-clock
duration), runs a few calls at L16 / T18, super-blocks 8 x 8 x 4, on uniform and on ray-ordered points and prints median / max / min
per level.  `python tools/exp/bwd_lines_block_times.py [n_samples] [line_local|line_overlap]` on a GPU box; nothing in the tree is
modified.  (line-local layouts.)"""
import collections, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from perf_amd import build as B

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
layout = sys.argv[2] if len(sys.argv) > 2 else 'line_local'
tmp = tempfile.mkdtemp(prefix='perf_blockt_lines_')
B.build()
hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
timed = ('hashgrid_bwd.hip', 'hashgrid_bwd_lines.hip')
for src in timed:
    subprocess.run([hipcc] + B.FLAGS + ['-DPERF_BWD_BLOCK_TIMES', '-c', os.path.join(B.CSRC, src), '-o', os.path.join(tmp, src.replace('.hip', '.o'))],
                   check=True)
objs = [os.path.join(tmp if s in timed else os.path.join(B.HERE, 'build'), s.replace('.hip', '.o')) for s in B.SOURCES]
lib = os.path.join(tmp, 'libperf_hip.so')
subprocess.run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib] + objs, check=True)

for kind in ('uniform', 'ray_ordered'):
    child = f'''
import sys; sys.path.insert(0, {ROOT!r})
from perf_amd import _lib
_lib.LIB_PATH = {lib!r}
import torch
from perf_amd import ops
from perf_amd.grid import GridConfig
cfg = GridConfig(n_levels=16, log2_hashmap_size=18, layout={layout!r}, sb_shift=(3, 3, 2), local_min_res=64); n = {n}
if {kind!r} == 'uniform':
    x = torch.rand(n, 3, device="cuda")
else:
    R = n // 128
    d = torch.nn.functional.normalize(torch.randn(R, 3, device="cuda"), dim=-1)
    t = (torch.arange(128, device="cuda") + 0.5) / 128
    x = ((d[:, None, :] * t[None, :, None]).reshape(-1, 3) * 0.45 + 0.5).contiguous()
dfeat = torch.randn(16, n, 2, device="cuda") * 1e-3
amax = torch.zeros(24, device="cuda"); amax[:16] = dfeat.abs().amax(dim=(1, 2))
hr = ops.headroom_state("cuda")
for _ in range(6):
    ops.hashgrid_bwd_lines(cfg, x, dfeat, level_absmax=amax, hr_state=hr)
torch.cuda.synchronize()
'''
    out = subprocess.run([sys.executable, '-c', child], capture_output=True, text=True)
    rows = [(m.group(1), *map(int, m.groups()[1:])) for m in
            re.finditer(r'(BLOCKT|BLOCKT_LINES) level (\d+) tile (\d+) rep (\d+) of (\d+) ticks (\d+)', out.stdout)]
    if not rows:
        sys.exit('no BLOCKT lines:\n' + out.stdout[-2000:] + out.stderr[-2000:])
    by = collections.defaultdict(list)
    for tag, l, t, r, reps, ticks in rows:
        by[(tag, l, reps)].append(ticks / 100.0)            # wall_clock64: 100 MHz
    print(f'{kind}: {len(rows)} reports, {n} samples, {layout} (us per workgroup; the minimum is the least disturbed by the printf)')
    for (tag, l, reps), v in sorted(by.items()):
        v.sort()
        print(f'  {tag:12s} level {l:2d} x {reps} replicas: median {v[len(v) // 2]:7.1f}  max {max(v):7.1f}  min {min(v):7.1f}')
