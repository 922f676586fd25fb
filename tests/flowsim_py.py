"""ctypes face of tests/native/libflowsim.so — TEST-ONLY host replay of stream mode: the flow routines of hg_core.h driven
the way hg_flow_scan_kernel drives them (pieces, slices by start position, OR of end states, the write-end rules), raw ends
per expression, and hg_nfa_scan over the concatenation (see tests/native/flowsim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

from hypergrep_amd.utils import ExprExt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "flowsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libflowsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")

_lib = None


def build() -> None:
    deps = [SRC, os.path.join(REPO, "include", "hypergrep_amd.h")] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_flow_rules.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, SRC, os.path.join(CSRC, "hg_compile.cpp")])
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.flowsim_compile.restype = ctypes.c_void_p
        _lib.flowsim_compile.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                         ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_char_p, ctypes.c_size_t]
        _lib.flowsim_free.argtypes = [ctypes.c_void_p]
        _lib.flowsim_hold.restype = ctypes.c_uint32
        _lib.flowsim_hold.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _lib.flowsim_group_span.restype = ctypes.c_uint32
        _lib.flowsim_group_span.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _lib.flowsim_words.restype = ctypes.c_uint32
        _lib.flowsim_words.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _lib.flowsim_block.restype = ctypes.c_long
        _lib.flowsim_block.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
        _lib.flowsim_deliver.restype = ctypes.c_long
        _lib.flowsim_deliver.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                         ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
        _lib.flowsim_run.restype = ctypes.c_long
        _lib.flowsim_run.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
    return _lib


class Db:
    def __init__(self, patterns, flags, ids=None, exts=None):
        n = len(patterns)
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        self._exts = [e if e is None else ctypes.pointer(e) for e in (exts or [None] * n)]
        ea = (ctypes.POINTER(ExprExt) * n)(*self._exts)
        err = ctypes.create_string_buffer(512)
        self.n = n
        self.h = lib().flowsim_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n))),
                                       ea, n, err, 512)
        self.error = None if self.h else err.value.decode()

    def hold(self, i: int) -> bool:
        return bool(lib().flowsim_hold(self.h, i))

    def group_span(self, g: int) -> int:
        """Words of tables of hg_flow_scan_kernel's group g (`hi - lo`: staged in LDS up to HG_BLOCK_SMALL_POOL words)."""
        return lib().flowsim_group_span(self.h, g)

    def words(self, i: int) -> int:
        return lib().flowsim_words(self.h, i)

    def block(self, data: bytes):
        """{(expression, end)} of hg_nfa_scan over data."""
        cap = (len(data) + 2) * self.n + 16
        out = (ctypes.c_uint32 * (2 * cap))()
        k = lib().flowsim_block(self.h, data, len(data), out, cap)
        assert 0 <= k <= cap
        return [(out[2 * j], out[2 * j + 1]) for j in range(k)]

    def run(self, data: bytes, cuts, piece: int = 4096, lanes: int = 8, min_slice: int = 8):
        """[(call, expression, end)] of the flow replay: data written at `cuts`, then closed (call len(cuts) + 1)."""
        cap = (len(data) + 2) * self.n * 2 + 16
        out = (ctypes.c_uint32 * (3 * cap))()
        c = (ctypes.c_uint32 * max(1, len(cuts)))(*cuts)
        k = lib().flowsim_run(self.h, data, len(data), c, len(cuts), piece, lanes, min_slice, out, cap)
        assert 0 <= k <= cap
        return [(out[3 * j], out[3 * j + 1], out[3 * j + 2]) for j in range(k)]

    def deliver(self, data: bytes, cuts, raw):
        """Face A's report rules over run()'s raw ends: [(call, id, to)] in delivery order."""
        flat = [v for r in raw for v in r]
        ra = (ctypes.c_uint32 * max(1, len(flat)))(*flat)
        c = (ctypes.c_uint32 * max(1, len(cuts)))(*cuts)
        cap = len(raw) + 16
        out = (ctypes.c_uint32 * (3 * cap))()
        k = lib().flowsim_deliver(self.h, ra, len(raw), len(data), c, len(cuts), out, cap)
        assert 0 <= k <= cap
        return [(out[3 * j], out[3 * j + 1], out[3 * j + 2]) for j in range(k)]

    def __del__(self):
        if getattr(self, "h", None):
            lib().flowsim_free(self.h)
            self.h = None
