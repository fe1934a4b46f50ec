"""The register budget of the 24 packed-ray compositing kernels (perf_amd/csrc/composite.hip, built from composite_device.hpp): no scratch and
no more VGPRs than the figures below, which are those of commit 8a3c328 (the tree before the shared pieces were stated once).  The kernels
share __forceinline__ device functions; an edit of a shared piece that costs one of them registers lowers its occupancy without failing
any other test.  The unit is compiled device-only with the library's own flags and the compiler's resource-usage remarks are read, as
tests/test_mlp_fwd_resources.py does."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel (with its template arguments as the mangled name spells them) -> VGPRs
MAX_VGPRS = {'visibility_count_kernelILb1E': 49, 'visibility_count_kernelILb0E': 34,
             'visibility_count2_kernelILb1E': 44, 'visibility_count2_kernelILb0E': 36,
             'compact_prefix_kernel': 42, 'compact_prefix2_kernelILb1E': 52, 'compact_prefix2_kernelILb0E': 48,
             'composite_fwd_kernelILb1E': 85, 'composite_fwd_kernelILb0E': 77, 'composite_bwd_kernel': 42,
             'distloss_fwd_kernel': 34, 'distloss_bwd_kernel': 34, 'accumulate_kernel': 22, 'pack_info_kernel': 14,
             'head_tail_counts_kernel': 6, 'render_finish_eval_kernel': 10, 'pdf_resample_kernel': 14,
             'geo_loss_kernel': 19, 'app_loss_kernel': 14, 'app_loss_final_kernel': 6,
             'train_head_kernelILb0ELb1E': 77, 'train_head_kernelILb0ELb0E': 50,
             'train_head_kernelILb1ELb1E': 64, 'train_head_kernelILb1ELb0E': 42}


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
def test_compositing_kernels_keep_their_registers():
    usage = _resource_usage(os.path.join(ROOT, 'perf_amd', 'csrc', 'composite.hip'))
    seen = set()
    for name, u in usage.items():
        # _ZN4perf<len><kernel>[I<template arguments>E]E<parameters>: the kernel's name and its template arguments
        m = re.match(r'_ZN4perf\d+(\w+?_kernel)(?:(I(?:Lb\dE)+)E)?E', name)
        assert m, name
        key = m.group(1) + (m.group(2) or '')
        print(key, u)
        assert key in MAX_VGPRS, name
        seen.add(key)
        assert u['ScratchSize'] == 0, (name, u)
        assert u['VGPRs'] <= MAX_VGPRS[key], (name, u)
    assert seen == set(MAX_VGPRS), sorted(set(MAX_VGPRS) - seen)
