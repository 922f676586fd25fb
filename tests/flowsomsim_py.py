"""ctypes face of tests/native/libflowsomsim.so — TEST-ONLY host replay of start of match in stream mode: the SOM flow
routines of hg_core.h with the carried starts stored and reloaded at every write, the plain flow routines for the other
expressions, the report rules of hg_flow_rules.h; and the block-mode reference (hg_nfa_scan + hg_hit_som) over the
concatenation (see tests/native/flowsomsim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

from hypergrep_amd.utils import ExprExt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "flowsomsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libflowsomsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
WIDTH = {"small": 2, "medium": 4, "large": 8}
HBITS = {"small": 16, "medium": 32, "large": 0}
PAST = (1 << 64) - 1

_lib = None


def build() -> None:
    deps = [SRC, os.path.join(REPO, "include", "hypergrep_amd.h")] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_flow_rules.h", "hg_som.h")]
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
        u32, u64p = ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)
        _lib.fss_compile.restype = ctypes.c_void_p
        _lib.fss_compile.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                     ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_char_p, ctypes.c_size_t]
        _lib.fss_free.argtypes = [ctypes.c_void_p]
        _lib.fss_header.restype = u32
        _lib.fss_header.argtypes = [ctypes.c_void_p, u32]
        _lib.fss_run.restype = ctypes.c_long
        _lib.fss_run.argtypes = [ctypes.c_void_p, ctypes.c_char_p, u32, ctypes.POINTER(u32), u32, u32, u32, u64p, ctypes.c_size_t]
        _lib.fss_block.restype = ctypes.c_long
        _lib.fss_block.argtypes = [ctypes.c_void_p, ctypes.c_char_p, u32, u32, u64p, ctypes.c_size_t]
    return _lib


class Db:
    def __init__(self, patterns, flags, ids=None, exts=None):
        n = len(patterns)
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        self._exts = [e if e is None else ctypes.pointer(e) for e in (exts or [None] * n)]
        ea = (ctypes.POINTER(ExprExt) * n)(*self._exts)
        err = ctypes.create_string_buffer(512)
        self.n = n
        self.h = lib().fss_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n))),
                                   ea, n, err, 512)
        self.error = None if self.h else err.value.decode()

    def header(self, i: int) -> int:
        return lib().fss_header(self.h, i)

    def run(self, data: bytes, cuts, horizon: str = "large"):
        """[(call, id, from, to)] delivered by the replayed stream: data written at `cuts`, then closed (call len(cuts) + 1)."""
        cap = (len(data) + 2) * self.n * 2 + 16
        out = (ctypes.c_uint64 * (4 * cap))()
        c = (ctypes.c_uint32 * max(1, len(cuts)))(*cuts)
        k = lib().fss_run(self.h, data, len(data), c, len(cuts), WIDTH[horizon], HBITS[horizon], out, cap)
        assert 0 <= k <= cap
        return [tuple(out[4 * j:4 * j + 4]) for j in range(k)]

    def block(self, data: bytes, horizon: str = "large"):
        """[(id, from, to)] of hs_scan(data) on the block-mode twin, `from` cut at the horizon."""
        cap = (len(data) + 2) * self.n + 16
        out = (ctypes.c_uint64 * (3 * cap))()
        k = lib().fss_block(self.h, data, len(data), HBITS[horizon], out, cap)
        assert 0 <= k <= cap
        return [tuple(out[3 * j:3 * j + 3]) for j in range(k)]

    def __del__(self):
        if getattr(self, "h", None):
            lib().fss_free(self.h)
            self.h = None
