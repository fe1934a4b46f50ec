"""The register budget of hashgrid_bwd_kernel: at most 128 VGPRs, no AGPRs and no scratch, for the fixed-point and the fp32
instantiation.  An owner workgroup is 1,024 threads = sixteen waves on the four SIMDs of a CU, i.e. four waves per SIMD, which a SIMD's
512 VGPRs per lane hold at 128 each; one register more and the workgroup does not fit a CU at all.  The owner loops (bwd_stream_masks,
bwd_stream_codes in perf_amd/csrc/hashgrid_bwd.hip) keep registers written by loads in flight next to everything an apply needs, and an
edit that spills them to scratch or moves them to AGPRs still passes every other test.  This is the guard, in the manner of
tests/test_pair_kernel_resources.py: the file is compiled device-only with the library's own flags and the compiler's resource-usage
remarks are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_VGPRS = 128         # 512 per SIMD lane / 4 waves per SIMD


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
def test_bwd_kernel_keeps_four_waves_per_simd_without_scratch():
    usage = _resource_usage(os.path.join(ROOT, 'perf_amd', 'csrc', 'hashgrid_bwd.hip'))
    # (_ZN4perf19hashgrid_bwd_kernelILb0EEEv... / ILb1E: the name is followed by its template argument, the atomics kernels' is not)
    kernels = {k: v for k, v in usage.items() if re.search(r'hashgrid_bwd_kernelILb[01]E', k)}
    assert len(kernels) == 2 and any('ILb1E' in k for k in kernels) and any('ILb0E' in k for k in kernels), sorted(usage)
    measured = {('fixed' if 'ILb1E' in k else 'fp32'): v['VGPRs'] for k, v in kernels.items()}
    for name, u in kernels.items():
        print(name, u)
        assert u['ScratchSize'] == 0, (name, u)
        assert u.get('AGPRs', 0) == 0, (name, u)
        assert u['VGPRs'] <= MAX_VGPRS, f'{name}: {u["VGPRs"]} VGPRs > {MAX_VGPRS} (VGPRs measured: {measured}); {u}'
