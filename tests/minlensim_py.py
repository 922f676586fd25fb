"""ctypes face of tests/native/libminlensim.so — TEST-ONLY host harness around the product's compiler, hg_nfa_scan, the
match-length / start-of-match reference routines of hypergrep_amd/csrc/hg_som.h and the combination routines (see
tests/native/minlensim.cpp) — and the independent expectation every min_length test uses: Python `re` brute force."""
from __future__ import annotations

import ctypes
import os
import subprocess

import comb_ref
import regex_gen
from extsim_py import ExprExt, ext  # noqa: F401  (hs_expr_ext_t and its builder)
from somsim_py import start_by_brute_force

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "minlensim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libminlensim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
INCLUDE = os.path.join(REPO, "include", "hypergrep_amd.h")
SOM, SINGLE, COMBINATION, QUIET = 256, 8, 512, 1024

_lib = None


def build() -> None:
    deps = [SRC, INCLUDE] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_som.h", "hg_comb.h", "hg_post.h")]
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
        _lib.minlensim_compile.restype = ctypes.c_void_p
        _lib.minlensim_compile.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                           ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_char_p, ctypes.c_size_t]
        _lib.minlensim_free.argtypes = [ctypes.c_void_p]
        _lib.minlensim_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        _lib.minlensim_long_enough.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        _lib.minlensim_piece.restype = ctypes.c_long
        _lib.minlensim_piece.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_uint32)]
    return _lib


def exts_for(min_lengths):
    """[ExprExt or None] for a list of min_length values (None: no parameters)."""
    return [None if v is None else ext(min_length=v) for v in min_lengths]


class Db:
    def __init__(self, patterns, flags, ids=None, exts=None):
        """ids default to 0, 1, 2 ...; exts: one ExprExt or None per expression"""
        n = len(patterns)
        self.n = n
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        self._exts = [e if e is None else ctypes.pointer(e) for e in (exts or [None] * n)]
        ea = (ctypes.POINTER(ExprExt) * n)(*self._exts)
        err = ctypes.create_string_buffer(512)
        self.h = lib().minlensim_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n))),
                                         ea, n, err, 512)
        self.error = None if self.h else err.value.decode()

    def ok(self) -> bool:
        return bool(self.h)

    def info(self) -> dict:
        assert self.h, self.error
        out = (ctypes.c_uint32 * (3 + 4 * self.n))()
        lib().minlensim_info(self.h, out)
        per = [dict(zip(("min_length", "single", "reverse_tables", "tier"), out[3 + 4 * i:7 + 4 * i])) for i in range(self.n)]
        return {"filtering": out[0], "nsom": out[1], "pool_words": out[2], "patterns": per}

    def long_enough(self, pattern: int, data: bytes, to: int, min_len: int) -> bool:
        return bool(lib().minlensim_long_enough(self.h, pattern, data, len(data), to, min_len))

    def piece(self, data: bytes):
        """([(id, to, from, pattern)] of one trimmed piece in (id, to) order, reports before the filter)."""
        cap = 4 * len(data) * 8 + 64
        out = (ctypes.c_uint32 * (4 * cap))()
        n_raw = ctypes.c_uint32()
        n = lib().minlensim_piece(self.h, data, len(data), out, cap, ctypes.byref(n_raw))
        assert n >= 0
        return [tuple(out[4 * i:4 * i + 4]) for i in range(n)], n_raw.value

    def __del__(self):
        if getattr(self, "h", None):
            lib().minlensim_free(self.h)
            self.h = None


# ---- the expectation: Python `re` brute force, nothing of the library under test

def spans(pat: str, flags: int, line: bytes):
    """[(leftmost start, to)] of every end of one expression in one trimmed piece."""
    return [(start_by_brute_force(pat, flags, line, to), to) for to in regex_gen.ends_by_brute_force(pat, flags & 7, line)]


def expected_piece(pats, flags, ids, min_lengths, line: bytes):
    """The delivered [(id, to, from)] of one trimmed piece, in (id, to) order: per expression keep an end t iff a start s
    with t - s >= min_length exists (the leftmost start decides), then the report rules (SINGLEMATCH expressions of an id:
    the smallest surviving end; an identical (id, to) once), then combinations and QUIET (comb_ref), and for SOM ids `from` =
    the smallest start over the expressions whose own report at `to` survives (0 for the other ids)."""
    multi, single, start = {}, {}, {}
    for i, pat in enumerate(pats):
        if flags[i] & COMBINATION:
            continue
        need = min_lengths[i] or 0
        for s, to in spans(pat, flags[i], line):
            if to - s < need:
                continue
            (single if flags[i] & SINGLE else multi).setdefault(ids[i], set()).add(to)
            if flags[i] & SOM:
                start[(ids[i], to)] = min(s, start.get((ids[i], to), s))
    reports = set()
    for rid, tos in multi.items():
        reports |= {(rid, to) for to in tos}
    for rid, tos in single.items():
        reports.add((rid, min(tos)))
    reports = sorted(reports)
    if any(f & (COMBINATION | QUIET) for f in flags):
        reports = comb_ref.CombSet(list(pats), list(flags), list(ids)).piece(reports)
    return [(rid, to, start.get((rid, to), 0)) for rid, to in reports]
