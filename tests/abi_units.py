"""What the ABI tests share: a unit's header read once, the header's constants and parameter lists, a refused call with its message,
and the workspace formulas of the mesh headers."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERF_E_INVALID = -1          # include/perf_hip.h


def header(name):
    """(text, comment-free text) of include/perf_hip_<name>.h; 'core' is include/perf_hip.h"""
    text = open(os.path.join(ROOT, 'include', 'perf_hip.h' if name == 'core' else f'perf_hip_{name}.h')).read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def const(text, macro):
    return int(re.search(r'#define\s+' + macro + r'\s+(\d+)', text).group(1))


def params(plain, function):
    """the text between the parentheses of a prototype of the comment-free header"""
    return re.search(r'\b' + function + r'\s*\((.*?)\)\s*;', plain, re.S).group(1)


def abi_digest():
    """tools/abi_digest.py as a module"""
    if os.path.join(ROOT, 'tools') not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import abi_digest
    return abi_digest


def build_deps():
    """the files perf_amd/build.py rebuilds the whole library for, paths normalised"""
    from perf_amd import build
    return {os.path.normpath(p) for p in build.deps()}


def refused(name, *args):
    """(return code, perf_last_error's message) of one call"""
    from perf_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, (lib.perf_last_error() or b'').decode()


def levels(n):
    """L(n) of the headers: the words of the scan's levels of 256 above n words, down to the level of one word."""
    words = 0
    while True:
        n = -(-n // 256)
        words += n
        if n <= 1:
            return words


def group_words(n):
    """S(n) of the headers."""
    return 0 if n == 0 else -(-n // 256) + levels(-(-n // 256))


def slots(n):
    """T(n) of the headers."""
    t = 256
    while t < 2 * n:
        t *= 2
    return t
