"""ctypes face of tests/native/libranksim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_values.h and hg_rank.h (see
tests/native/ranksim.cpp): the passes of the rank stage over a text, its records and its parts."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "ranksim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libranksim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")

_lib = None


def build() -> None:
    deps = [SRC, os.path.join(REPO, "include", "hypergrep_amd.h")] + [os.path.join(CSRC, f) for f in ("hg_rank.h", "hg_values.h", "hg_partlines.h", "hg_gather.h", "hg_parts.h", "hg_core.h",
                                                                                                      "hg_db.h")]
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
        u32, u64, p8, p32, p64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        _lib.ranksim_run.restype = ctypes.c_long
        _lib.ranksim_run.argtypes = [p8, u64, u64, p64, u64, p64, u64, ctypes.c_int, p64, u32, u32, u64, u32, u32, u64, u64, ctypes.POINTER(ctypes.c_uint8), u64, p64, p64, p64, p32,
                                     p64, p32, p64, p64, p64, p64]
        _lib.ranksim_trace.restype = ctypes.c_long
        _lib.ranksim_trace.argtypes = _lib.ranksim_run.argtypes + [p64, p64, p64, p64]
        _lib.ranksim_sizes.argtypes = [p32]
    return _lib


SIZES = ("sizeof_params", "sizeof_result", "p.flags", "p.hash_bits", "p.table_log2", "p.reserved", "p.top", "r.n_values", "r.n_distinct", "r.n_parts", "r.n_bytes", "r.d_bytes",
         "r.d_off", "r.d_count", "r.d_first", "r.d_pattern", "r.d_line_number", "r.d_segment", "r.d_first_value", "r.d_seg_distinct", "r.d_seg_parts", "r.n_seg", "r.table_log2",
         "r.rank_us", "r.reserved", "by_pattern", "per_segment", "sizeof_values_params", "sizeof_values_result")


def sizes() -> dict:
    out = (ctypes.c_uint32 * len(SIZES))()
    lib().ranksim_sizes(out)
    return dict(zip(SIZES, out))


PART_COLS = ("tier", "home", "slot", "probes", "wrapped", "claimed", "key")  # tier: 0 none, 1 lane, 2 wave
SEG_COLS = ("first_group", "seg_distinct", "seg_parts", "kept")
CALL_COLS = ("n_groups", "count_bits", "seg_bits", "slots")


def replay(text: bytes, records, parts, by_pattern: bool = False, per_segment: bool = False, top: int = 0, seg_start=None, hash_bits: int = 0, table_log2: int = 0,
           order_seed: int = 0, tile: int = 16384, base: int = 0, trace: bool = False):
    """The stage over `parts`, (line, from, to, pattern, segment) rows, and `records`, (line, start, len, segment) rows, both in the
    scan's order.  seg_start: the files' offsets (the scan had segments).  Returns (arrays as rank_ref.arrays gives them, the
    per-segment arrays or None, {"n_distinct", "n_long"}); with trace the dict also has "parts" (a dict of PART_COLS per part),
    "segs" (one of SEG_COLS per segment; one segment without per_segment), "placed" (per group of the final order, 1 or 0 for
    cut) and "call" (CALL_COLS): ranksim.cpp, Trace."""
    n, nr = len(parts), len(records)
    segments = seg_start is not None
    n_seg = len(seg_start) if segments else 0
    c_recs = (ctypes.c_uint64 * max(4 * nr, 1))(*[v for r in records for v in (r[0], r[1] + (0 if segments else base), r[2], r[3])])
    c_parts = (ctypes.c_uint64 * max(5 * n, 1))(*[v for p in parts for v in p])
    c_seg = (ctypes.c_uint64 * max(n_seg, 1))(*[s + base for s in seg_start]) if segments else None
    cap = sum(p[2] - p[1] for p in parts) + 32
    out = (ctypes.c_uint8 * cap)()
    off, count, first, line = ((ctypes.c_uint64 * (n + 1))() for _ in range(4))
    pattern, segment = ((ctypes.c_uint32 * (n + 1))() for _ in range(2))
    first_value, seg_distinct, seg_parts = ((ctypes.c_uint64 * (n_seg + 1))() for _ in range(3))
    totals = (ctypes.c_uint64 * 4)()
    flags = (1 if by_pattern else 0) | (2 if per_segment else 0)
    args = (text, len(text), base, c_recs, nr, c_parts, n, 1 if segments else 0, c_seg, n_seg, flags, top, hash_bits, table_log2, order_seed, tile, out, cap, off, count, first, pattern,
            line, segment, first_value, seg_distinct, seg_parts, totals)
    n_rank_seg = n_seg if per_segment else 1
    if trace:
        t_part, t_seg, t_group, t_call = ((ctypes.c_uint64 * max(k, 1))() for k in (len(PART_COLS) * n, len(SEG_COLS) * n_rank_seg, n, len(CALL_COLS)))
        rc = lib().ranksim_trace(*args, t_part, t_seg, t_group, t_call)
    else:
        rc = lib().ranksim_run(*args)
    assert rc == 0, f"ranksim_run returned {rc}"
    nv, nb = totals[0], totals[1]
    seg_arrays = {"first_value": list(first_value[:n_seg + 1]), "seg_distinct": list(seg_distinct[:n_seg]), "seg_parts": list(seg_parts[:n_seg])} if per_segment else None
    arrays = {"bytes": bytes(out[:nb]), "off": list(off[:nv + 1]), "count": list(count[:nv]), "first": list(first[:nv]), "pattern": list(pattern[:nv]),
              "line_number": list(line[:nv]), "segment": list(segment[:nv]) if segments else None}
    info = {"n_distinct": totals[2], "n_long": totals[3]}
    if trace:
        info["parts"] = [dict(zip(PART_COLS, t_part[len(PART_COLS) * q:len(PART_COLS) * (q + 1)])) for q in range(n)]
        info["segs"] = [dict(zip(SEG_COLS, t_seg[len(SEG_COLS) * k:len(SEG_COLS) * (k + 1)])) for k in range(n_rank_seg)]
        info["placed"] = list(t_group[:totals[2]])
        info["call"] = dict(zip(CALL_COLS, t_call))
    return (arrays, seg_arrays, info)
