"""ctypes face of tests/native/libcombsim.so — TEST-ONLY host harness around the product's compiler and the scalar routines
of the combination pass, hypergrep_amd/csrc/hg_comb.h (see tests/native/combsim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "combsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libcombsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")

_lib = None


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_comb.h", "hg_post.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"  # built aside and renamed into place (parallel test workers)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, SRC, os.path.join(CSRC, "hg_compile.cpp")])
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.combsim_compile.restype = ctypes.c_void_p
        _lib.combsim_free.argtypes = [ctypes.c_void_p]
        _lib.combsim_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        _lib.combsim_tier.restype = ctypes.c_uint32
        _lib.combsim_tier.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _lib.combsim_digest.restype = ctypes.c_size_t
        _lib.combsim_digest.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
        _lib.combsim_eval.restype = ctypes.c_int
        _lib.combsim_eval.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64]
        _lib.combsim_operands.restype = ctypes.c_uint32
        _lib.combsim_operands.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        _lib.combsim_piece.restype = ctypes.c_long
        _lib.combsim_piece.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
    return _lib


class Db:
    def __init__(self, patterns, flags, ids):
        n = len(patterns)
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        err = ctypes.create_string_buffer(512)
        self.h = lib().combsim_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*ids), n, err, 512)
        self.error = None if self.h else err.value.decode()

    def ok(self) -> bool:
        return bool(self.h)

    def info(self) -> dict:
        out = (ctypes.c_uint32 * 4)()
        lib().combsim_info(self.h, out)
        return {"ncomb": out[0], "nquiet": out[1], "records": out[2], "feed": out[3]}

    def tier(self, i: int) -> int:
        return lib().combsim_tier(self.h, i)

    def digest(self, n_keep: int) -> bytes:
        size = lib().combsim_digest(self.h, n_keep, None, 0)
        buf = ctypes.create_string_buffer(size)
        lib().combsim_digest(self.h, n_keep, buf, size)
        return buf.raw

    def eval(self, k: int, status: int) -> bool:
        return bool(lib().combsim_eval(self.h, k, status))

    def operands(self, k: int):
        ids = (ctypes.c_uint32 * 64)()
        pat = ctypes.c_uint32()
        n = lib().combsim_operands(self.h, k, ids, ctypes.byref(pat))
        return list(ids[:n]), pat.value

    def piece(self, reports):
        """reports: [(id, to, pattern)] of one piece after the report rules, in (id, to) order -> delivered [(id, to, pattern)]."""
        m = len(reports)
        flat = (ctypes.c_uint32 * max(3 * m, 1))(*[v for r in reports for v in r])
        cap = 4 * m + 64 * 64 + 16
        out = (ctypes.c_uint32 * (3 * cap))()
        n = lib().combsim_piece(self.h, flat, m, out, cap)
        assert n >= 0
        return [tuple(out[3 * i:3 * i + 3]) for i in range(n)]

    def __del__(self):
        if getattr(self, "h", None):
            lib().combsim_free(self.h)
            self.h = None
