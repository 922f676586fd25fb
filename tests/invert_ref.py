"""Inverted match (grep -v): the plain Python reference every invert test uses, and the ctypes face of
tests/native/libinvertsim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_invert.h (see tests/native/invertsim.cpp).

The reference knows nothing of tiles: split at '\\n', cut into pieces of buffer_size - 1 bytes, apply the trim rule, and drop
the pieces whose number is among the matching lines."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "invertsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libinvertsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
HG_ID_INVERT = 0xFFFFFFFF

_lib = None


def pieces(data: bytes, buffer_size: int):
    """[(offset of the first scanned byte, scanned bytes)] per line piece, in order."""
    bs1 = buffer_size - 1
    out = []
    pos = 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        line_end = nl + 1 if nl >= 0 else len(data)
        while pos < line_end:  # the line's pieces
            end = min(pos + bs1, line_end)
            a = pos
            while a < end and data[a] == 0:
                a += 1
            z = data.find(b"\0", a, end)
            z = end if z < 0 else z
            out.append((a, data[a:z]))
            pos = end
    return out


def expected(data: bytes, buffer_size: int, matching_lines, line_base: int = 0):
    """[(line_number, HG_ID_INVERT, 0, start, len)] of the selected pieces: what Scanner.hits() gives after an inverted scan.
    matching_lines: the line numbers (line_base included) that have a delivered report."""
    matching = set(matching_lines)
    return [(line_base + i, HG_ID_INVERT, 0, a, len(p)) for i, (a, p) in enumerate(pieces(data, buffer_size)) if line_base + i not in matching]


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_invert.h", "hg_core.h", "hg_db.h", "hg_post.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"  # built aside and renamed into place (parallel test workers)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-o", tmp, SRC])
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        u64 = ctypes.c_uint64
        _lib.invertsim_run.restype = ctypes.c_long
        _lib.invertsim_run.argtypes = [ctypes.c_char_p, u64, u64, u64, u64, ctypes.POINTER(u64), u64, ctypes.POINTER(u64), u64, ctypes.POINTER(u64)]
    return _lib


def replay(data: bytes, tile: int, buffer_size: int, hit_lines, line_base: int = 0):
    """The host replay of the invert stage over tiles of `tile` bytes: ([(line_number, id, to, start, len)], n_pieces).
    hit_lines: the line numbers of the scan's hits, ascending (a line may repeat)."""
    hit_lines = list(hit_lines)
    cap = len(data) + 1
    out = (ctypes.c_uint64 * (6 * cap))()
    n_pieces = ctypes.c_uint64()
    n = lib().invertsim_run(data, len(data), tile, buffer_size - 1, line_base, (ctypes.c_uint64 * len(hit_lines))(*hit_lines), len(hit_lines), out, cap,
                            ctypes.byref(n_pieces))
    assert n >= 0, {-1: "output too small", -2: "a tile's count and its walk disagree", -3: "the tiles' first piece numbers do not chain"}[n]
    rows = []
    for i in range(n):
        line, start, length, rid, to, pattern = out[6 * i:6 * i + 6]
        assert pattern == 0xFFFFFFFF
        rows.append((line, rid, to, start, length))
    return rows, n_pieces.value
