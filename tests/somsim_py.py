"""ctypes face of tests/native/libsomsim.so — TEST-ONLY host harness around the product's compiler, hg_nfa_scan and the
start-of-match reference routine of hypergrep_amd/csrc/hg_som.h (see tests/native/somsim.cpp)."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import regex_gen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "somsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libsomsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
SOM = 256

_lib = None


def build() -> None:
    deps = [SRC, os.path.join(REPO, "include", "hypergrep_amd.h")] + [os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_som.h")]
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
        _lib.somsim_compile.restype = ctypes.c_void_p
        _lib.somsim_free.argtypes = [ctypes.c_void_p]
        _lib.somsim_info.restype = ctypes.c_uint64
        _lib.somsim_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        _lib.somsim_piece.restype = ctypes.c_long
        _lib.somsim_piece.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
        _lib.somsim_start.restype = ctypes.c_uint32
        _lib.somsim_start.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
        _lib.somsim_compile_ext.restype = ctypes.c_void_p
        _lib.somsim_pattern.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        _lib.somsim_nfa_som.restype = ctypes.c_uint32
        _lib.somsim_nfa_som.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
        _lib.somsim_nfa_minlen.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        _lib.somsim_walk.restype = None
        _lib.somsim_walk.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    return _lib


NONE32 = 0xFFFFFFFF
EXITS = ("died", "lo", "start", "early")  # how somsim_walk ended: state died, q == lo, piece start, early exit


class Db:
    def __init__(self, patterns, flags, ids=None, exts=None):
        """ids default to 0, 1, 2 ...: one report id per expression; exts: one extsim_py.ExprExt or None per expression"""
        n = len(patterns)
        self.n = n
        enc = [p.encode() if isinstance(p, str) else p for p in patterns]
        err = ctypes.create_string_buffer(512)
        pa, fa, ia = (ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n)))
        if exts is None:
            self.h = lib().somsim_compile(pa, fa, ia, n, err, 512)
        else:
            self._exts = [e if e is None else ctypes.pointer(e) for e in exts]
            ea = (ctypes.c_void_p * n)(*[None if e is None else ctypes.cast(e, ctypes.c_void_p) for e in self._exts])
            self.h = lib().somsim_compile_ext(pa, fa, ia, ea, n, err, 512)
        self.error = None if self.h else err.value.decode()

    def ok(self) -> bool:
        return bool(self.h)

    def info(self) -> dict:
        assert self.h, self.error
        out = (ctypes.c_uint32 * 4)()
        words = lib().somsim_info(self.h, out)
        return {"pool_words": words, "nsom": out[0], "tier0": out[1], "nw0": out[2], "literal_only0": out[3]}

    def piece(self, data: bytes):
        """[(id, to, from, pattern)] of one trimmed piece, in (id, to) order."""
        cap = 4 * len(data) * 8 + 64
        out = (ctypes.c_uint32 * (4 * cap))()
        n = lib().somsim_piece(self.h, data, len(data), out, cap)
        assert n >= 0
        return [tuple(out[4 * i:4 * i + 4]) for i in range(n)]

    def start(self, pattern: int, data: bytes, to: int) -> int:
        return lib().somsim_start(self.h, pattern, data, len(data), to)

    def pattern(self, i: int) -> dict:
        """The compiler's read-out of expression i."""
        out = (ctypes.c_uint32 * 8)()
        lib().somsim_pattern(self.h, i, out)
        return dict(zip(("nw", "max_len", "literal_only", "som_next", "flags", "min_length", "tier", "reverse_tables"), out))

    def nfa_som(self, pattern: int, data: bytes, to: int) -> int:
        """hg_nfa_som: the scalar loop (NONE32 when no match of the expression ends at `to`)."""
        return lib().somsim_nfa_som(self.h, pattern, data, len(data), to)

    def nfa_minlen(self, pattern: int, data: bytes, to: int, min_len: int) -> bool:
        return bool(lib().somsim_nfa_minlen(self.h, pattern, data, len(data), to, min_len))

    def walk(self, pattern: int, text: bytes, a: int, length: int, to: int, early: bool = False, limit: int = 0) -> dict:
        """somsim_walk, the restatement of the kernel's chunked walk, on the piece text[a, a + length): result, exit (EXITS),
        the lowest and highest text offset loaded, the 64-byte rounds."""
        out = (ctypes.c_uint64 * 5)()
        lib().somsim_walk(self.h, pattern, text, len(text), a, length, to, int(early), limit, out)
        return {"result": out[0], "exit": EXITS[out[1]], "lowest": out[2], "highest": out[3], "rounds": out[4]}

    def __del__(self):
        if getattr(self, "h", None):
            lib().somsim_free(self.h)
            self.h = None


def pieces(data: bytes, buffer_size: int):
    """(piece index, offset of the first scanned byte, scanned bytes) per piece, the gzgets rules of the reference
    (pieces of at most buffer_size - 1 bytes ending after '\\n', leading NULs skipped, cut at the first NUL)."""
    bs1 = buffer_size - 1
    out, pos, idx = [], 0, 0
    while pos < len(data):
        nl = data.find(b"\n", pos, pos + bs1)
        end = nl + 1 if nl >= 0 else min(pos + bs1, len(data))
        a = pos
        while a < end and data[a] == 0:
            a += 1
        z = data.find(b"\0", a, end)
        z = end if z < 0 else z
        out.append((idx, a, data[a:z]))
        pos, idx = end, idx + 1
    return out


_START_RE_CACHE: dict = {}


def start_by_brute_force(pat: str, flags: int, line: bytes, to: int) -> int | None:
    """min(s for s in range(to) if the expression matches exactly [s, to) of `line` in its real context): the lookahead to
    \\Z that regex_gen.ends_by_brute_force builds keeps `$` / `\\b` honest at `to`, `pos` keeps `^` / `\\b` honest at s."""
    key = (pat, flags & 7, len(line) - to)
    cre = _START_RE_CACHE.get(key)
    if cre is None:
        cre = _START_RE_CACHE[key] = re.compile(b"(?:" + pat.encode() + b")(?=(?s:.{%d})\\Z)" % (len(line) - to), regex_gen.py_flags(flags))
    return next((s for s in range(to) if cre.match(line, s)), None)
