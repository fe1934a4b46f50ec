#!/usr/bin/env python
"""Digest of the C ABI declared in include/perf_hip.h (`--ext`: of its extension, include/perf_hip_ext.h, versioned by
PERF_EXT_ABI_VERSION and recorded in include/perf_hip_ext.abi.json; `--sphere`: of the sphere distance field's header,
include/perf_hip_sphere.h, PERF_SPHERE_ABI_VERSION, include/perf_hip_sphere.abi.json; `--pair`: of the pair table's header,
include/perf_hip_pair.h, PERF_PAIR_ABI_VERSION, include/perf_hip_pair.abi.json; `--joint`: of the joint predictor's alignment step,
include/perf_hip_joint.h, PERF_JOINT_ABI_VERSION, include/perf_hip_joint.abi.json; `--mesh`: of surface nets on a dense lattice,
include/perf_hip_mesh.h, PERF_MESH_ABI_VERSION, include/perf_hip_mesh.abi.json; `--brickmesh`: of surface nets on the live bricks of a lattice,
include/perf_hip_brickmesh.h, PERF_BRICKMESH_ABI_VERSION, include/perf_hip_brickmesh.abi.json; `--meshcc`: of the connected components of a triangle mesh,
include/perf_hip_meshcc.h, PERF_MESHCC_ABI_VERSION, include/perf_hip_meshcc.abi.json; `--meshvis`: of the cull of the faces no panorama saw,
include/perf_hip_meshvis.h, PERF_MESHVIS_ABI_VERSION, include/perf_hip_meshvis.abi.json; `--meshsimp`: of the simplification by vertex clustering,
include/perf_hip_meshsimp.h, PERF_MESHSIMP_ABI_VERSION, include/perf_hip_meshsimp.abi.json; `--meshcolor`: of the colouring from the panoramas,
include/perf_hip_meshcolor.h, PERF_MESHCOLOR_ABI_VERSION, include/perf_hip_meshcolor.abi.json; `--meshray`: of the rays against a mesh on a uniform grid,
include/perf_hip_meshray.h, PERF_MESHRAY_ABI_VERSION, include/perf_hip_meshray.abi.json; `--meshtex`: of the texture atlas baked from the panoramas,
include/perf_hip_meshtex.h, PERF_MESHTEX_ABI_VERSION, include/perf_hip_meshtex.abi.json; `--meshquadric`: of the quadric error placement,
include/perf_hip_meshquadric.h, PERF_MESHQUADRIC_ABI_VERSION, include/perf_hip_meshquadric.abi.json; `--riders`: of the step riders,
include/perf_hip_riders.h, PERF_RIDERS_ABI_VERSION, include/perf_hip_riders.abi.json): sha256 over the comment-free, whitespace-normalised text of every
`perf_*` prototype, struct and #define, in file order.  `python tools/abi_digest.py` prints {version, digest};
`--write` records it in include/perf_hip.abi.json.  tests/test_cpu_oracle.py fails when the digest of the header differs
from the recorded one while PERF_ABI_VERSION is unchanged: every signature change must bump the version (the load-time
check of perf_amd/_lib.py can then catch a stale libperf_hip.so)."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'perf_hip.h')
RECORD = os.path.join(ROOT, 'include', 'perf_hip.abi.json')
EXT_HEADER = os.path.join(ROOT, 'include', 'perf_hip_ext.h')
EXT_RECORD = os.path.join(ROOT, 'include', 'perf_hip_ext.abi.json')
SPHERE_HEADER = os.path.join(ROOT, 'include', 'perf_hip_sphere.h')
SPHERE_RECORD = os.path.join(ROOT, 'include', 'perf_hip_sphere.abi.json')
PAIR_HEADER = os.path.join(ROOT, 'include', 'perf_hip_pair.h')
PAIR_RECORD = os.path.join(ROOT, 'include', 'perf_hip_pair.abi.json')
JOINT_HEADER = os.path.join(ROOT, 'include', 'perf_hip_joint.h')
JOINT_RECORD = os.path.join(ROOT, 'include', 'perf_hip_joint.abi.json')
MESH_HEADER = os.path.join(ROOT, 'include', 'perf_hip_mesh.h')
MESH_RECORD = os.path.join(ROOT, 'include', 'perf_hip_mesh.abi.json')
BRICKMESH_HEADER = os.path.join(ROOT, 'include', 'perf_hip_brickmesh.h')
BRICKMESH_RECORD = os.path.join(ROOT, 'include', 'perf_hip_brickmesh.abi.json')
MESHCC_HEADER = os.path.join(ROOT, 'include', 'perf_hip_meshcc.h')
MESHCC_RECORD = os.path.join(ROOT, 'include', 'perf_hip_meshcc.abi.json')
MESHVIS_HEADER = os.path.join(ROOT, 'include', 'perf_hip_meshvis.h')
MESHVIS_RECORD = os.path.join(ROOT, 'include', 'perf_hip_meshvis.abi.json')
MESHSIMP_HEADER = os.path.join(ROOT, 'include', 'perf_hip_meshsimp.h')
MESHSIMP_RECORD = os.path.join(ROOT, 'include', 'perf_hip_meshsimp.abi.json')
MESHCOLOR_HEADER = os.path.join(ROOT, 'include', 'perf_hip_meshcolor.h')
MESHCOLOR_RECORD = os.path.join(ROOT, 'include', 'perf_hip_meshcolor.abi.json')
MESHRAY_HEADER = os.path.join(ROOT, 'include', 'perf_hip_meshray.h')
MESHRAY_RECORD = os.path.join(ROOT, 'include', 'perf_hip_meshray.abi.json')
MESHTEX_HEADER = os.path.join(ROOT, 'include', 'perf_hip_meshtex.h')
MESHTEX_RECORD = os.path.join(ROOT, 'include', 'perf_hip_meshtex.abi.json')
MESHQUADRIC_HEADER = os.path.join(ROOT, 'include', 'perf_hip_meshquadric.h')
MESHQUADRIC_RECORD = os.path.join(ROOT, 'include', 'perf_hip_meshquadric.abi.json')
RIDERS_HEADER = os.path.join(ROOT, 'include', 'perf_hip_riders.h')
RIDERS_RECORD = os.path.join(ROOT, 'include', 'perf_hip_riders.abi.json')


def digest(path=HEADER, macro='PERF_ABI_VERSION'):
    text = open(path).read()
    version = int(re.search(r'#define\s+' + macro + r'\s+(\d+)', text).group(1))
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'#define\s+' + macro + r'\s+\d+', ' ', text)
    text = re.sub(r'\s+', ' ', text).strip()
    return {'version': version, 'digest': hashlib.sha256(text.encode()).hexdigest()}


if __name__ == '__main__':
    brickmesh = '--brickmesh' in sys.argv
    meshcc = '--meshcc' in sys.argv
    meshvis = '--meshvis' in sys.argv
    meshsimp = '--meshsimp' in sys.argv
    meshcolor = '--meshcolor' in sys.argv
    meshray = '--meshray' in sys.argv
    meshtex = '--meshtex' in sys.argv
    meshquadric = '--meshquadric' in sys.argv
    riders = '--riders' in sys.argv
    ext, sphere, pair, joint, mesh = '--ext' in sys.argv, '--sphere' in sys.argv, '--pair' in sys.argv, '--joint' in sys.argv, '--mesh' in sys.argv
    d = digest(RIDERS_HEADER, 'PERF_RIDERS_ABI_VERSION') if riders else digest(MESHQUADRIC_HEADER, 'PERF_MESHQUADRIC_ABI_VERSION') if meshquadric else digest(MESHTEX_HEADER, 'PERF_MESHTEX_ABI_VERSION') if meshtex else digest(MESHRAY_HEADER, 'PERF_MESHRAY_ABI_VERSION') if meshray else digest(MESHCOLOR_HEADER, 'PERF_MESHCOLOR_ABI_VERSION') if meshcolor else digest(MESHSIMP_HEADER, 'PERF_MESHSIMP_ABI_VERSION') if meshsimp else digest(MESHVIS_HEADER, 'PERF_MESHVIS_ABI_VERSION') if meshvis else digest(MESHCC_HEADER, 'PERF_MESHCC_ABI_VERSION') if meshcc else digest(BRICKMESH_HEADER, 'PERF_BRICKMESH_ABI_VERSION') if brickmesh else digest(MESH_HEADER, 'PERF_MESH_ABI_VERSION') if mesh else digest(JOINT_HEADER, 'PERF_JOINT_ABI_VERSION') if joint else digest(PAIR_HEADER, 'PERF_PAIR_ABI_VERSION') if pair else digest(SPHERE_HEADER, 'PERF_SPHERE_ABI_VERSION') if sphere else digest(EXT_HEADER, 'PERF_EXT_ABI_VERSION') if ext else digest()
    record = RIDERS_RECORD if riders else MESHQUADRIC_RECORD if meshquadric else MESHTEX_RECORD if meshtex else MESHRAY_RECORD if meshray else MESHCOLOR_RECORD if meshcolor else MESHSIMP_RECORD if meshsimp else MESHVIS_RECORD if meshvis else MESHCC_RECORD if meshcc else BRICKMESH_RECORD if brickmesh else MESH_RECORD if mesh else JOINT_RECORD if joint else PAIR_RECORD if pair else SPHERE_RECORD if sphere else EXT_RECORD if ext else RECORD
    if '--write' in sys.argv:
        json.dump(d, open(record, 'w'), indent=1)
        open(record, 'a').write('\n')
    print(json.dumps(d))
