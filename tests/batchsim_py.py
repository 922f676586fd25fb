"""ctypes face of tests/native/libbatchsim.so — TEST-ONLY host replay of the batched block scan: the packing, the
shard / round / team / slice walk and the per-item report rules of hypergrep_amd/csrc/hg_batch.h driven the way
hg_scan_blocks and hg_block_batch_kernel drive them (see tests/native/batchsim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "batchsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libbatchsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")

_lib = None


def build() -> None:
    deps = [SRC, os.path.join(REPO, "include", "hypergrep_amd.h")] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_batch.h")]
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
        _lib.batchsim_compile.restype = ctypes.c_void_p
        _lib.batchsim_compile.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.c_uint,
                                          ctypes.c_char_p, ctypes.c_size_t]
        _lib.batchsim_free.argtypes = [ctypes.c_void_p]
        _lib.batchsim_block.restype = ctypes.c_long
        _lib.batchsim_block.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
        _lib.batchsim_run.restype = ctypes.c_long
        _lib.batchsim_run.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
    return _lib


class Db:
    def __init__(self, patterns, flags, ids=None):
        n = len(patterns)
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        err = ctypes.create_string_buffer(512)
        self.n = n
        self.h = lib().batchsim_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n))), n, err, 512)
        self.error = None if self.h else err.value.decode()

    def block(self, data: bytes):
        """[(expression, end)] of hg_nfa_scan over data alone."""
        cap = (len(data) + 2) * self.n + 16
        out = (ctypes.c_uint32 * (2 * cap))()
        k = lib().batchsim_block(self.h, data, len(data), out, cap)
        assert 0 <= k <= cap
        return [(out[2 * j], out[2 * j + 1]) for j in range(k)]

    def run(self, items, lanes: int = 256, ppw: int = 32, nshards: int = 1):
        """[[(id, to)] per item] of the replayed batch, each item's reports in delivery order."""
        n = len(items)
        blob = b"".join(items)
        offs, at = [], 0
        for d in items:
            offs.append(at)
            at += len(d)
        cap = (len(blob) + 2 * n) * self.n + 16
        out = (ctypes.c_uint32 * (3 * cap))()
        k = lib().batchsim_run(self.h, blob, (ctypes.c_uint64 * max(1, n))(*offs), (ctypes.c_uint32 * max(1, n))(*[len(d) for d in items]), n, lanes, ppw, nshards,
                               out, cap)
        assert 0 <= k <= cap, f"batchsim_run returned {k}"
        res = [[] for _ in range(n)]
        last = -1
        for j in range(k):
            assert out[3 * j] >= last, "reports are not grouped in item order"
            last = out[3 * j]
            res[last].append((out[3 * j + 1], out[3 * j + 2]))
        return res

    def __del__(self):
        if getattr(self, "h", None):
            lib().batchsim_free(self.h)
            self.h = None
