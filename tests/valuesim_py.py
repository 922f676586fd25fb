"""ctypes face of tests/native/libvaluesim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_values.h (see
tests/native/valuesim.cpp): the passes of the values stage over a text, its records and its parts."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "valuesim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libvaluesim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")

_lib = None


def build() -> None:
    deps = [SRC, os.path.join(REPO, "include", "hypergrep_amd.h")] + [os.path.join(CSRC, f) for f in ("hg_values.h", "hg_partlines.h", "hg_gather.h", "hg_parts.h", "hg_core.h", "hg_db.h")]
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
        _lib.valuesim_run.restype = ctypes.c_long
        _lib.valuesim_run.argtypes = [p8, u64, u64, p64, u64, p64, u64, ctypes.c_int, p64, u32, u32, u32, u64, u64, ctypes.POINTER(ctypes.c_uint8), u64, p64, p64, p64, p32, p64,
                                      p32, p64]
        _lib.valuesim_trace.restype = ctypes.c_long
        _lib.valuesim_trace.argtypes = _lib.valuesim_run.argtypes + [p64, p64, p64]
        _lib.valuesim_hash.restype = u64
        _lib.valuesim_hash.argtypes = [p8, u64, u64, u32, u32, u32, u32, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        _lib.valuesim_sizes.argtypes = [p32]
    return _lib


SIZES = ("sizeof_params", "sizeof_result", "p.flags", "p.hash_bits", "p.table_log2", "p.reserved", "r.n_values", "r.n_parts", "r.n_bytes", "r.d_bytes", "r.d_off", "r.d_count",
         "r.d_first", "r.d_pattern", "r.d_line_number", "r.d_segment", "r.table_log2", "r.values_us", "lane_max", "by_pattern", "sizeof_part_lines_result", "sizeof_lines_result",
         "sizeof_counts_result", "sizeof_parts_result")


def sizes() -> dict:
    out = (ctypes.c_uint32 * len(SIZES))()
    lib().valuesim_sizes(out)
    return dict(zip(SIZES, out))


def hash_of(text: bytes, s: int, length: int, which: int, by_pattern: bool = False, pattern: int = 0, hash_bits: int = 64) -> int:
    """The hash of text[s:s + length] by the byte-wise definition (which 0), the lanes' dword path (1) or a wave's shares (2)."""
    bad = ctypes.c_int()
    h = lib().valuesim_hash(text, len(text), s, length, 1 if by_pattern else 0, pattern, hash_bits, which, ctypes.byref(bad))
    assert not bad.value, "a read left the text"
    return h


PART_COLS = ("tier", "home", "slot", "probes", "wrapped", "claimed", "same_tag", "other_tag")  # tier: 0 none, 1 lane, 2 wave
WAVE_COLS = ("path", "leader", "mask")  # path: 0 no counted lane, 1 one add by the leader, 2 lane by lane
CALL_COLS = ("n_long", "long_iterations", "last_slot_occupied", "n_values", "sort_bits", "slots", "long_waves", "no_value")


def replay(text: bytes, records, parts, by_pattern: bool = False, seg_start=None, hash_bits: int = 0, table_log2: int = 0, order_seed: int = 0, tile: int = 16384, base: int = 0,
           trace: bool = False):
    """The stage over `parts`, (line, from, to, pattern, segment) rows, and `records`, (line, start, len, segment) rows, both in the
    scan's order.  seg_start: the files' offsets (the scan had segments).  Returns (arrays as values_ref.arrays gives them,
    {"probes", "n_long"}); with trace also {"parts": a dict of PART_COLS per part, "waves": one of WAVE_COLS per wave of the
    insert pass, "call": one of CALL_COLS} (valuesim.cpp, Trace)."""
    n, nr = len(parts), len(records)
    segments = seg_start is not None
    c_recs = (ctypes.c_uint64 * max(4 * nr, 1))(*[v for r in records for v in (r[0], r[1] + (0 if segments else base), r[2], r[3])])
    c_parts = (ctypes.c_uint64 * max(5 * n, 1))(*[v for p in parts for v in p])
    c_seg = (ctypes.c_uint64 * max(len(seg_start), 1))(*[s + base for s in seg_start]) if segments else None
    cap = sum(p[2] - p[1] for p in parts) + 32
    out = (ctypes.c_uint8 * cap)()
    off, count, first, line = ((ctypes.c_uint64 * (n + 1))() for _ in range(4))
    pattern, segment = ((ctypes.c_uint32 * (n + 1))() for _ in range(2))
    totals = (ctypes.c_uint64 * 4)()
    args = (text, len(text), base, c_recs, nr, c_parts, n, 1 if segments else 0, c_seg, 1 if by_pattern else 0, hash_bits, table_log2, order_seed, tile, out, cap, off, count, first,
            pattern, line, segment, totals)
    n_waves = (n + 63) // 64
    if trace:
        t_part, t_wave, t_call = (ctypes.c_uint64 * max(len(PART_COLS) * n, 1))(), (ctypes.c_uint64 * max(len(WAVE_COLS) * n_waves, 1))(), (ctypes.c_uint64 * len(CALL_COLS))()
        rc = lib().valuesim_trace(*args, t_part, t_wave, t_call)
    else:
        rc = lib().valuesim_run(*args)
    assert rc == 0, f"valuesim_run returned {rc}"
    nv, nb = totals[0], totals[1]
    info = {"probes": totals[2], "n_long": totals[3]}
    if trace:
        info["parts"] = [dict(zip(PART_COLS, t_part[len(PART_COLS) * q:len(PART_COLS) * (q + 1)])) for q in range(n)]
        info["waves"] = [dict(zip(WAVE_COLS, t_wave[len(WAVE_COLS) * w:len(WAVE_COLS) * (w + 1)])) for w in range(n_waves)]
        info["call"] = dict(zip(CALL_COLS, t_call))
    return ({"bytes": bytes(out[:nb]), "off": list(off[:nv + 1]), "count": list(count[:nv]), "first": list(first[:nv]), "pattern": list(pattern[:nv]),
             "line_number": list(line[:nv]), "segment": list(segment[:nv]) if segments else None}, info)
