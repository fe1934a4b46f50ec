"""The pair table's header (include/perf_hip_pair.h) checked without a GPU: the fourth header, its binding table, its recorded digest and
the library agree; the three older ABIs are untouched and the four name sets are disjoint; refusals happen before a launch."""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERF_E_INVALID = -1          # include/perf_hip.h
FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch
NAMES = ['perf_adam_step_dev_pair', 'perf_hashgrid_fwd_pair', 'perf_mlp_fwd_rows', 'perf_pair_fill', 'perf_pair_version']


def test_header_binding_record_and_library_agree():
    from perf_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import abi_digest
    header = open(os.path.join(ROOT, 'include', 'perf_hip_pair.h')).read()
    version = int(re.search(r'#define\s+PERF_PAIR_ABI_VERSION\s+(\d+)', header).group(1))
    record = json.load(open(os.path.join(ROOT, 'include', 'perf_hip_pair.abi.json')))
    now = abi_digest.digest(abi_digest.PAIR_HEADER, 'PERF_PAIR_ABI_VERSION')
    lib = _lib.load()
    assert version == 1 and _lib.PAIR_ABI_VERSION == 1 and record['version'] == 1 and lib.perf_pair_version() == 1
    assert now == record, 'include/perf_hip_pair.h changed: bump PERF_PAIR_ABI_VERSION, then `python tools/abi_digest.py --pair --write`'
    plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = sorted(set(re.findall(r'\b(perf_[a-z0-9_]+)\s*\(', plain)))
    assert declared == sorted(_lib._SIGS_PAIR) == NAMES
    for name, (_, args) in _lib._SIGS_PAIR.items():
        params = re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', plain, re.S).group(1).strip()
        assert (0 if params in ('', 'void') else len(params.split(','))) == len(args), name
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes or []) == len(args)
    # the three older ABIs are what they were, and the four name sets are disjoint
    for rec, hdr, macro, ver in (('perf_hip.abi.json', abi_digest.HEADER, 'PERF_ABI_VERSION', 16),
                                 ('perf_hip_ext.abi.json', abi_digest.EXT_HEADER, 'PERF_EXT_ABI_VERSION', 1),
                                 ('perf_hip_sphere.abi.json', abi_digest.SPHERE_HEADER, 'PERF_SPHERE_ABI_VERSION', 1)):
        old = json.load(open(os.path.join(ROOT, 'include', rec)))
        assert old['version'] == ver and abi_digest.digest(hdr, macro) == old, rec
    assert lib.perf_version() == 16 and lib.perf_ext_version() == 1 and lib.perf_sphere_version() == 1
    sets = [set(_lib._SIGS), set(_lib._SIGS_EXT), set(_lib._SIGS_SPHERE), set(_lib._SIGS_PAIR)]
    assert all(not (a & b) for i, a in enumerate(sets) for b in sets[i + 1:])
    assert _lib.exported_symbols() == sorted(_lib._SIGS)


def _fwd(cfg, **kw):
    from perf_amd import _lib
    lib = _lib.load()
    a = {'x': FAKE, 'pair': FAKE, 'fa': FAKE, 'fb': FAKE, 'dtype': 0, 'n': 64}
    a.update(kw)
    d = cfg.desc()
    rc = lib.perf_hashgrid_fwd_pair(ctypes.byref(d), a['x'], a['pair'], a['fa'], a['fb'], a['n'], None, a['dtype'], None)
    return rc, (lib.perf_last_error() or b'').decode()


def test_pair_encode_refuses_what_is_not_built():
    from perf_amd.grid import GridConfig
    for layout in ('line_local', 'line_overlap'):
        rc, msg = _fwd(GridConfig(layout=layout, sb_shift=(3, 3, 2)))
        assert rc == PERF_E_INVALID and 'tcnn' in msg, msg
    rc, msg = _fwd(GridConfig(n_levels=20))
    assert rc == PERF_E_INVALID and '20 levels' in msg, msg
    for kw in ({'x': None}, {'pair': None}, {'fa': None}, {'fb': None}):
        rc, msg = _fwd(GridConfig(), **kw)
        assert rc == PERF_E_INVALID and 'NULL pointer' in msg, (kw, msg)
    rc, msg = _fwd(GridConfig(), dtype=7)
    assert rc == PERF_E_INVALID and 'dtype' in msg, msg
    rc, msg = _fwd(GridConfig(), n=-1)
    assert rc == PERF_E_INVALID and 'n out of range' in msg, msg
    rc, msg = _fwd(GridConfig(), pair=ctypes.c_void_p(68))
    assert rc == PERF_E_INVALID and '8-byte aligned' in msg, msg
    assert _fwd(GridConfig(), n=0, x=None)[0] == 0          # (an empty call launches nothing)


def test_pair_fill_refusals():
    from perf_amd import _lib
    lib = _lib.load()
    for args, word in (((None, 0, FAKE, 64), 'NULL pointer'), ((FAKE, 0, None, 64), 'NULL pointer'), ((FAKE, 2, FAKE, 64), 'field 2'),
                       ((FAKE, 0, FAKE, -1), 'n_entries'), ((ctypes.c_void_p(68), 0, FAKE, 64), 'aligned'), ((FAKE, 0, ctypes.c_void_p(66), 64), 'aligned')):
        assert lib.perf_pair_fill(*args, None) == PERF_E_INVALID
        assert word in (lib.perf_last_error() or b'').decode(), args
    assert lib.perf_pair_fill(FAKE, 1, FAKE, 0, None) == 0
