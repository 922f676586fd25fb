"""ctypes face of tests/native/libextsim.so — TEST-ONLY host harness around hgc_compile_ext: the whole-pipeline host replay
of hostsim.cpp on databases with extended parameters, a byte-for-byte database digest and per-piece automaton runs with
their start of match (see tests/native/extsim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import hgsim_py
from hypergrep_amd.utils import ExprExt  # hs_expr_ext_t

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "extsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libextsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
INCLUDE = os.path.join(REPO, "include", "hypergrep_amd.h")

HS_EXT_FLAG_MIN_OFFSET, HS_EXT_FLAG_MAX_OFFSET, HS_EXT_FLAG_MIN_LENGTH = 1, 2, 4
HS_EXT_FLAG_EDIT_DISTANCE, HS_EXT_FLAG_HAMMING_DISTANCE = 8, 16


def ext(edit: int = 0, hamming: int = 0, min_offset=None, max_offset=None, min_length=None, flags=None) -> ExprExt:
    x = ExprExt()
    f = 0
    if edit:
        f |= HS_EXT_FLAG_EDIT_DISTANCE
        x.edit_distance = edit
    if hamming:
        f |= HS_EXT_FLAG_HAMMING_DISTANCE
        x.hamming_distance = hamming
    for bit, name, value in ((HS_EXT_FLAG_MIN_OFFSET, "min_offset", min_offset), (HS_EXT_FLAG_MAX_OFFSET, "max_offset", max_offset),
                             (HS_EXT_FLAG_MIN_LENGTH, "min_length", min_length)):
        if value is not None:
            f |= bit
            setattr(x, name, value)
    x.flags = f if flags is None else flags
    return x


_lib = None


def build() -> None:
    deps = [SRC, INCLUDE, os.path.join(REPO, "tests", "native", "hostsim.cpp")] + [
        os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_post.h", "hg_som.h")]
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
        _lib.extsim_compile.restype = ctypes.c_void_p
        _lib.extsim_compile.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                        ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t,
                                        ctypes.POINTER(ctypes.c_int)]
        _lib.hgsim_free.argtypes = [ctypes.c_void_p]
        _lib.extsim_digest.restype = ctypes.c_size_t
        _lib.extsim_digest.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        _lib.extsim_pattern.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        _lib.extsim_nfa.restype = ctypes.c_long
        _lib.extsim_nfa.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
        _lib.hgsim_scan.restype = ctypes.c_long
        _lib.hgsim_scan.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int,
                                    ctypes.POINTER(ctypes.POINTER(hgsim_py.SimHit)), ctypes.POINTER(ctypes.c_uint64)]
        _lib.hgsim_free_hits.argtypes = [ctypes.POINTER(hgsim_py.SimHit)]
    return _lib


class Db:
    """mode "ext": hgc_compile_ext(ext) (entries may be None); "plain": hgc_compile; "null": hgc_compile_ext(NULL)."""

    def __init__(self, patterns, flags, ids=None, exts=None, mode: str = "ext"):
        n = len(patterns)
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        self._exts = [e if e is None else ctypes.pointer(e) for e in (exts or [None] * n)]
        ea = (ctypes.POINTER(ExprExt) * n)(*self._exts)
        err = ctypes.create_string_buffer(512)
        bad = ctypes.c_int(-1)
        self.h = lib().extsim_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n))),
                                      ea, n, {"plain": 0, "ext": 1, "null": 2}[mode], err, 512, ctypes.byref(bad))
        self.error = None if self.h else err.value.decode()
        self.bad = bad.value

    def digest(self) -> bytes:
        n = lib().extsim_digest(self.h, None, 0)
        buf = ctypes.create_string_buffer(n)
        lib().extsim_digest(self.h, buf, n)
        return buf.raw

    def pattern(self, i: int) -> dict:
        out = (ctypes.c_uint32 * 10)()
        lib().extsim_pattern(self.h, i, out)
        return dict(zip(("tier", "nw", "nnodes", "max_len", "lit_lead", "literal_only", "mode", "single", "lo", "hi"), out))

    def nfa(self, i: int, data: bytes):
        """[(to, from)] of expression i over one trimmed piece."""
        cap = len(data) + 2
        out = (ctypes.c_uint32 * (2 * cap))()
        n = lib().extsim_nfa(self.h, i, data, len(data), out, cap)
        assert n >= 0
        return [(out[2 * j], out[2 * j + 1]) for j in range(n)]

    def scan(self, data: bytes, buffer_size: int = 262140):
        """The host replay of the GPU pipeline: [(line_no, id, to)] after the report rules."""
        out = ctypes.POINTER(hgsim_py.SimHit)()
        stats = (ctypes.c_uint64 * 5)()
        n = lib().hgsim_scan(self.h, data, len(data), buffer_size, ctypes.byref(out), stats)
        if n < 0:
            raise RuntimeError(f"hgsim_scan rc {n}")
        hits = [(out[i].line_no, out[i].id, out[i].to) for i in range(n)]
        lib().hgsim_free_hits(out)
        return hits

    def __del__(self):
        if getattr(self, "h", None):
            lib().hgsim_free(self.h)
            self.h = None
