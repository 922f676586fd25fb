"""ctypes face of tests/native/libsegpartssim.so — TEST-ONLY host harness around the product's compiler, the rules of
hypergrep_amd/csrc/hg_segparts.h and the walk of hg_parts.h (see tests/native/segpartssim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "segpartssim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libsegpartssim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
COMPILER = os.path.join(CSRC, "hg_compile.cpp")

_lib = None


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_som.h", "hg_parts.h", "hg_segments.h", "hg_invert.h",
                                                    "hg_segparts.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"  # built aside and renamed into place (parallel test workers)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, SRC, COMPILER])
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        u64, p64, p32 = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        _lib.segpartssim_compile.restype = ctypes.c_void_p
        _lib.segpartssim_free.argtypes = [ctypes.c_void_p]
        _lib.segpartssim_run.restype = ctypes.c_long
        _lib.segpartssim_run.argtypes = [ctypes.c_void_p, ctypes.c_char_p, p64, p32, u64, p64, u64, p64, p64, u64, p64, ctypes.c_int]
    return _lib


class Db:
    def __init__(self, patterns, flags):
        n = len(patterns)
        err = ctypes.create_string_buffer(512)
        self.h = lib().segpartssim_compile((ctypes.c_char_p * n)(*[p.encode() for p in patterns]), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*range(1, n + 1)), n,
                                           err, 512)
        assert self.h, err.value.decode()

    def run(self, data: bytes, records, segment, starts, first_record, exact: bool = True):
        """The stage over the surviving records of a segment pass (segments_ref.replay's records, segment, first_record):
        ([(line, from, to, pattern)], part_segment, first_part)."""
        n, n_seg = len(records), len(starts)
        u64, u32 = ctypes.c_uint64, ctypes.c_uint32
        recs = (u64 * (5 * n + 1))()
        for i, r in enumerate(records):
            recs[5 * i:5 * i + 5] = list(r[:5])
        cap = sum(r[4] for r in records) + 1  # (parts are never empty: a piece has at most len of them)
        out, first_part = (u64 * (5 * cap))(), (u64 * (n_seg + 1))()
        got = lib().segpartssim_run(self.h, data, recs, (u32 * (n + 1))(*segment), n, (u64 * (n_seg + 1))(*starts), n_seg, (u64 * (n_seg + 1))(*first_record), out, cap,
                                    first_part, 1 if exact else 0)
        assert got >= 0, {-1: "more parts than bytes", -2: "the write pass disagrees with the count pass"}[got]
        rows = [tuple(out[5 * i:5 * i + 4]) for i in range(got)]
        return rows, [out[5 * i + 4] for i in range(got)], list(first_part)

    def __del__(self):
        if getattr(self, "h", None):
            lib().segpartssim_free(self.h)
            self.h = None
