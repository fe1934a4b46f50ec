"""The register budget of the MLP forward kernels that stream level-major features (mlp_fwd_kernel, plain and ROWS, one or two hidden
layers, up to 16 levels): no scratch, no more unified registers than the figures below, at least three waves per SIMD.  The launchers
size their grids by these occupancies (mlp_blocks(n, nh == 1 ? 4 : 3)); an edit that costs registers lowers them without failing any
other test.  The figures are those of commit 319dba4 (the tree before the fragments were staged through LDS), bf16 and fp16 alike.
The three forward units are compiled device-only with the library's own flags and the compiler's resource-usage remarks are read,
as tests/test_pair_kernel_resources.py does."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('mlp_fwd_bf16.hip', 'mlp_fwd_fp16.hip', 'mlp_fwd_rows.hip')
# (hidden layers, k-steps, ROWS) -> VGPRs + AGPRs
MAX_REGISTERS = {(1, 1, False): 86, (1, 2, False): 114, (2, 1, False): 138, (2, 2, False): 154,
                 (1, 1, True): 104, (1, 2, True): 122, (2, 1, True): 142, (2, 2, True): 158}
MIN_WAVES = 3


def _hipcc():
    cand = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    return cand if os.path.exists(cand) else shutil.which('hipcc')


def _resource_usage(src):
    """{mangled kernel name: {field: int}} from -Rpass-analysis=kernel-resource-usage"""
    from perf_amd.build import FLAGS
    cmd = [_hipcc()] + FLAGS + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r'remark: +Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r'remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and name is not None:
            usage[name][m.group(1).strip()] = int(m.group(2))
    return usage


@pytest.mark.skipif(_hipcc() is None, reason='hipcc not found (HIPCC, /opt/rocm/bin/hipcc, PATH): the kernels cannot be compiled here')
def test_forward_kernels_keep_their_registers_and_waves():
    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        usages = list(ex.map(lambda u: _resource_usage(os.path.join(ROOT, 'perf_amd', 'csrc', u)), UNITS))
    seen = set()
    for usage in usages:
        for name, u in usage.items():
            # mlp_fwd_kernel<T16, NH, KS, FUSED, ROWS>: template arguments as the mangled name spells them
            m = re.search(r'mlp_fwd_kernelINS_\d(BF16|FP16)ELi(\d)ELi(\d)ELb(\d)ELb(\d)E', name)
            if not m or m.group(4) == '1':
                continue
            key = (int(m.group(2)), int(m.group(3)), m.group(5) == '1')
            if key not in MAX_REGISTERS:
                continue
            seen.add((m.group(1),) + key)
            registers = u['VGPRs'] + u.get('AGPRs', 0)
            print(m.group(1), key, u)
            assert u['ScratchSize'] == 0, (name, u)
            assert registers <= MAX_REGISTERS[key], (name, u)
            assert u['Occupancy'] >= MIN_WAVES, (name, u)
    assert seen == {(t,) + k for t in ('BF16', 'FP16') for k in MAX_REGISTERS}, sorted(seen)
