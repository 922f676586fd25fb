"""ctypes face of tests/native/libctxsim.so — TEST-ONLY host mirror of the stream pass's first level with one byte of
context (see tests/native/ctxsim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "ctxsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libctxsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
DEFAULT_FLAGS = 14

SCAN_FIELDS = ("dwords", "l1_old", "l1_new", "cands_old", "cands_new", "violations", "rows", "rows_old", "rows_new", "dropped")

_lib = None


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"  # (built aside and renamed into place: parallel test workers)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, SRC, os.path.join(CSRC, "hg_compile.cpp")])
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.ctxsim_compile.restype = ctypes.c_void_p
        _lib.ctxsim_free.argtypes = [ctypes.c_void_p]
        _lib.ctxsim_tune.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        _lib.ctxsim_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        _lib.ctxsim_windows.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        _lib.ctxsim_windows.restype = ctypes.c_uint32
        _lib.ctxsim_scan.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    return _lib


class Db:
    def __init__(self, patterns, flags=None, ids=None):
        n = len(patterns)
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        pa = (ctypes.c_char_p * n)(*enc)
        fa = (ctypes.c_uint * n)(*(flags if flags else [DEFAULT_FLAGS] * n))
        ia = (ctypes.c_uint * n)(*(ids if ids else [0] * n))
        err = ctypes.create_string_buffer(256)
        self.h = lib().ctxsim_compile(pa, fa, ia, n, err, 256)
        self.error = err.value.decode() if not self.h else None

    def ok(self) -> bool:
        return bool(self.h)

    def tune(self, sample: bytes) -> int:
        return lib().ctxsim_tune(self.h, sample, len(sample))

    def info(self) -> dict:
        out = (ctypes.c_uint32 * 9)()
        lib().ctxsim_info(self.h, out)
        return dict(zip(("filter_log2", "wide", "dense", "fold_mask", "windows", "has_ctx", "used_slots", "ctx_slots", "use_ctx"), out))

    def windows(self):
        """(violations, checks) of ctxsim_windows: every window of every literal against the context test."""
        checks = ctypes.c_uint64(0)
        bad = lib().ctxsim_windows(self.h, ctypes.byref(checks))
        return bad, checks.value

    def scan(self, data: bytes) -> dict:
        out = (ctypes.c_uint64 * 10)()
        lib().ctxsim_scan(self.h, data, len(data), out)
        return dict(zip(SCAN_FIELDS, (int(x) for x in out)))

    def __del__(self):
        if getattr(self, "h", None):
            lib().ctxsim_free(self.h)
            self.h = None
