#!/usr/bin/env python
"""Digest of one C ABI of the library: sha256 over the comment-free, whitespace-normalised text of every `perf_*` prototype, struct
and #define of its header, in file order.  The units are the rows of perf_amd/_lib.py's two tables (a staged unit's header and record
lie in include/staged/); a unit NAME has the header
include/perf_hip_NAME.h, the version macro PERF_NAME_ABI_VERSION and the record include/perf_hip_NAME.abi.json, and the core is
include/perf_hip.h, PERF_ABI_VERSION, include/perf_hip.abi.json.  `python tools/abi_digest.py` prints {version, digest} of the core,
`--NAME` (`--ext` ... `--riders`) of that unit; `--write` records it.  tests/test_abi_units.py fails when the digest of a header differs
from the recorded one while its version is unchanged: every signature change must bump the version (the load-time check of
perf_amd/_lib.py can then catch a stale libperf_hip.so)."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from perf_amd._lib import _STAGED_UNITS, _UNITS  # noqa: E402

UNITS = {u.name: u for u in _UNITS + _STAGED_UNITS}


def header_path(name='core'):
    return os.path.join(ROOT, 'include', UNITS[name].header)


def record_path(name='core'):
    return os.path.join(ROOT, 'include', UNITS[name].record)


def digest(path=header_path(), macro=UNITS['core'].macro):
    text = open(path).read()
    version = int(re.search(r'#define\s+' + macro + r'\s+(\d+)', text).group(1))
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'#define\s+' + macro + r'\s+\d+', ' ', text)
    text = re.sub(r'\s+', ' ', text).strip()
    return {'version': version, 'digest': hashlib.sha256(text.encode()).hexdigest()}


def digest_unit(name='core'):
    return digest(header_path(name), UNITS[name].macro)


if __name__ == '__main__':
    options = [a[2:] for a in sys.argv[1:] if a.startswith('--') and a != '--write']
    if len(options) > 1 or any(o == 'core' or o not in UNITS for o in options):
        print('usage: abi_digest.py [' + ' | '.join('--' + n for n in UNITS if n != 'core') + '] [--write]    (no unit option: the core, perf_hip.h)',
              file=sys.stderr)
        sys.exit(2)
    name = options[0] if options else 'core'
    d = digest_unit(name)
    if '--write' in sys.argv:
        json.dump(d, open(record_path(name), 'w'), indent=1)
        open(record_path(name), 'a').write('\n')
    print(json.dumps(d))
