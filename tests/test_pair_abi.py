"""The pair table's header (include/perf_hip_pair.h) checked without a GPU: the header's constants and parameter types are the binding's (that
header, binding, record and library agree is tests/test_abi_units.py's); refusals happen before a launch."""
import ctypes

from tests import abi_units
from tests.abi_units import PERF_E_INVALID

FAKE = ctypes.c_void_p(64)   # never dereferenced: every call of this file is refused before a launch


def test_header_binding_record_and_library_agree():
    """(the agreement every unit owes is [pair] of tests/test_abi_units.py; this is what is particular to this header)"""
    from perf_amd import _lib
    header, _ = abi_units.header('pair')
    assert abi_units.const(header, 'PERF_PAIR_ABI_VERSION') == _lib.PAIR_ABI_VERSION == 1
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
