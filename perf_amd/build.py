"""Build libperf_hip.so (gfx950) in-tree with hipcc: one object per unit of SOURCES (meshnear.hip, the closest point of a mesh, is the newest), rebuilt
when a file it includes changed.  `python -m perf_amd.build [--force]`."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

from ._lib import _STAGED_UNITS, _UNITS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libperf_hip.so')
# (the MLP kernels are instantiated in six units of their own: one unit took 65 s, the longest of them now takes ~15 s)
SOURCES = ['mlp_bwd_bf16_nh2.hip', 'mlp_bwd_fp16_nh2.hip', 'mlp_bwd_bf16_nh1.hip', 'mlp_bwd_fp16_nh1.hip', 'mlp_fwd_bf16.hip', 'mlp_fwd_fp16.hip', 'mlp_fwd_rows.hip',
           'hashgrid_bwd.hip', 'hashgrid_bwd_lines.hip', 'hashgrid_fwd.hip', 'hashgrid_aux.hip', 'march.hip', 'misc.hip', 'composite.hip', 'mlp.hip', 'visibility.hip', 'field_normal.hip', 'field_normal_bwd.hip', 'sphere_field.hip', 'hashgrid_pair.hip', 'joint_align.hip', 'mesh.hip', 'brickmesh.hip', 'meshcc.hip', 'meshvis.hip', 'meshsimp.hip', 'meshcolor.hip', 'meshray.hip', 'meshtex.hip', 'meshquadric.hip', 'meshnear.hip']
HEADERS = ['common.hpp', 'grid_device.hpp', 'grid_fixed_point.hpp', 'mlp_reduce_device.hpp', 'step_book_device.hpp', 'mlp_device.hpp', 'field_normal_device.hpp', 'mesh_device.hpp', 'mesh_scan_device.hpp', 'mesh_filter_device.hpp', 'mesh_check_host.hpp', 'pano_lookup_device.hpp', 'march_device.hpp', 'step_riders_device.hpp', 'composite_device.hpp', 'meshtex_device.hpp']
# -amdgpu-mfma-vgpr-form: MFMA results land in VGPRs (no v_accvgpr_read per accumulator register before the epilogues)
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
         '-mllvm', '-amdgpu-mfma-vgpr-form=1']


def _newer(target, deps):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _includes(path):
    """path and, transitively, the files its `#include "..."` lines name: what a unit is rebuilt for"""
    names = re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', open(path).read(), re.M)
    return {path}.union(*(_includes(os.path.normpath(os.path.join(os.path.dirname(path), n))) for n in names))


def deps():
    """what the library as a whole is rebuilt for: the sources, the device headers and the public header of every unit of _lib's two tables"""
    return ([os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(CSRC, h) for h in HEADERS]
            + [os.path.join(HERE, '..', 'include', u.header) for u in _UNITS + _STAGED_UNITS])


def build(force=False, verbose=False):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not force and _newer(LIB, deps()):
        return LIB
    objdir = os.path.join(HERE, 'build')
    os.makedirs(objdir, exist_ok=True)

    def cc(src):
        obj = os.path.join(objdir, src.replace('.hip', '.o'))
        if not force and _newer(obj, _includes(os.path.join(CSRC, src))):
            return obj
        cmd = [hipcc] + FLAGS + ['-c', os.path.join(CSRC, src), '-o', obj]
        if verbose:
            print(' '.join(cmd))
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'hipcc failed on {src}:\n{r.stdout}\n{r.stderr}')
        if verbose and r.stderr:
            print(r.stderr)
        return obj

    # (at most 16 compilers at a time: on a shared host os.cpu_count() counts far more CPUs than one build may use)
    with ThreadPoolExecutor(max_workers=min(len(SOURCES), 16)) as ex:
        objs = list(ex.map(cc, SOURCES))
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'link failed:\n{r.stdout}\n{r.stderr}')
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
