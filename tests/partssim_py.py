"""ctypes face of tests/native/libpartssim.so — TEST-ONLY host harness around the product's compiler and the parts routines of
hypergrep_amd/csrc/hg_parts.h (see tests/native/partssim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import invert_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "partssim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libpartssim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
COMPILER = os.path.join(CSRC, "hg_compile.cpp")

_lib = None


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_som.h", "hg_parts.h")]
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
        _lib.partssim_compile.restype = ctypes.c_void_p
        _lib.partssim_free.argtypes = [ctypes.c_void_p]
        _lib.partssim_refusal.restype = ctypes.c_char_p
        _lib.partssim_refusal.argtypes = [ctypes.c_void_p]
        _lib.partssim_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        _lib.partssim_piece.restype = ctypes.c_long
        _lib.partssim_piece.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
        p32 = ctypes.POINTER(ctypes.c_uint32)
        _lib.partssim_pattern_info.restype = ctypes.c_uint32
        _lib.partssim_pattern_info.argtypes = [ctypes.c_void_p, ctypes.c_uint32, p32]
        _lib.partssim_piece_grouped.restype = ctypes.c_long
        _lib.partssim_piece_grouped.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, p32, ctypes.c_size_t, p32, ctypes.c_size_t, p32]
    return _lib


class Db:
    def __init__(self, patterns, flags, ids=None, min_offsets=None):
        """ids default to 0, 1, 2 ...; min_offsets: per expression, non-zero = compiled with that hs_expr_ext_t min_offset"""
        n = len(patterns)
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        err = ctypes.create_string_buffer(512)
        ext = (ctypes.c_ulonglong * n)(*min_offsets) if min_offsets is not None else None
        self.h = lib().partssim_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n))), ext, n,
                                        err, 512)
        self.error = None if self.h else err.value.decode()

    def ok(self) -> bool:
        return bool(self.h)

    def refusal(self):
        assert self.h, self.error
        text = lib().partssim_refusal(self.h)
        return text.decode() if text else None

    def info(self) -> dict:
        assert self.h, self.error
        out = (ctypes.c_uint32 * 3)()
        lib().partssim_info(self.h, out)
        return {"max_nw": out[0], "simple0": out[1], "nnodes0": out[2]}

    def piece(self, data: bytes):
        """[(from, to, pattern)] of one trimmed piece, in order."""
        cap = len(data) + 1
        out = (ctypes.c_uint32 * (3 * cap))()
        n = lib().partssim_piece(self.h, data, len(data), out, cap)
        assert n >= 0
        return [tuple(out[3 * i:3 * i + 3]) for i in range(n)]

    def pattern_info(self, index: int) -> dict:
        """{"nw", "simple", "nnodes"} of expression `index`."""
        assert self.h, self.error
        out = (ctypes.c_uint32 * 3)()
        n = lib().partssim_pattern_info(self.h, index, out)
        assert index < n, (index, n)
        return {"nw": out[0], "simple": out[1], "nnodes": out[2]}

    def n_patterns(self) -> int:
        assert self.h, self.error
        return lib().partssim_pattern_info(self.h, 0xFFFFFFFF, (ctypes.c_uint32 * 3)())

    def piece_grouped(self, data: bytes):
        """The replay of the kernels' decomposition (groups of 64 starts, first-byte rule, ballot / cursor / base loop) of one
        trimmed piece: ([(from, to, pattern)], ties, trace).  ties[i]: an expression of another bitmap word reaches part i's
        end too; trace: [(base, ballot rounds, outrun starts)] per group."""
        cap = len(data) + 1
        out = (ctypes.c_uint32 * (4 * cap))()
        trace = (ctypes.c_uint32 * (3 * cap))()
        groups = ctypes.c_uint32()
        n = lib().partssim_piece_grouped(self.h, data, len(data), out, cap, trace, cap, ctypes.byref(groups))
        assert n >= 0, n
        return ([tuple(out[4 * i:4 * i + 3]) for i in range(n)], [out[4 * i + 3] for i in range(n)],
                [tuple(trace[3 * i:3 * i + 3]) for i in range(groups.value)])

    def text(self, data: bytes, buffer_size: int = 1 << 20, line_base: int = 0):
        """[(line_number, from, to, pattern)] over every piece of a text that has a part."""
        rows = []
        for i, (_a, piece) in enumerate(invert_ref.pieces(data, buffer_size)):
            rows += [(line_base + i, f, t, p) for f, t, p in self.piece(piece)]
        return rows

    def __del__(self):
        if getattr(self, "h", None):
            lib().partssim_free(self.h)
            self.h = None
