"""The register budget of hashgrid_fwd_pair_kernel: at most 64 VGPRs and no scratch, for both dtypes -- eight waves per SIMD.  The
kernel is paced by L1 misses in flight, a thread has the eight gathers of one level in flight, and what keeps a SIMD's
miss queue filled is the number of waves.  An edit that costs registers lowers the occupancy (65..72 VGPRs: seven waves; the joint
two-level body's 114: four) without failing any other test.  This is the guard: the file is compiled device-only with the library's
own flags and the compiler's resource-usage remarks are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_VGPRS = 64
WAVES = 8


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


@pytest.mark.skipif(_hipcc() is None, reason='hipcc not found (HIPCC, /opt/rocm/bin/hipcc, PATH): the kernel cannot be compiled here')
def test_pair_kernel_keeps_eight_waves_per_simd():
    usage = _resource_usage(os.path.join(ROOT, 'perf_amd', 'csrc', 'hashgrid_pair.hip'))
    kernels = {k: v for k, v in usage.items() if 'hashgrid_fwd_pair_kernel' in k}
    assert len(kernels) == 2 and any('BF16' in k for k in kernels) and any('FP16' in k for k in kernels), sorted(usage)
    for name, u in kernels.items():
        print(name, u)
        assert u['VGPRs'] <= MAX_VGPRS, (name, u)
        assert u.get('AGPRs', 0) == 0, (name, u)
        assert u['ScratchSize'] == 0, (name, u)
        assert u['Occupancy'] == WAVES, (name, u)
