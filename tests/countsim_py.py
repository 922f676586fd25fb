"""ctypes face of tests/native/libcountsim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_counts.h (see
tests/native/countsim.cpp): the head rule, the bin lookup and the split into runs over a record list."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "countsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libcountsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")

_lib = None


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_counts.h", "hg_core.h", "hg_db.h")]
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
        u32, u64, p32, p64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        _lib.countsim_run_length.restype = u32
        _lib.countsim_lds_bins.restype = u32
        _lib.countsim_bin.restype = u32
        _lib.countsim_bin.argtypes = [p32, u32, u32]
        _lib.countsim_run.restype = u64
        _lib.countsim_run.argtypes = [p64, u64, ctypes.c_int, p32, u32, u32, u64, p64, p64, p32, p32]
    return _lib


def bin_of(ids, rid: int) -> int:
    return lib().countsim_bin((ctypes.c_uint32 * max(len(ids), 1))(*ids), len(ids), rid)


def replay(records, ids, run_len: int, n_seg: int | None = None, totals=None):
    """The stage over `records`, (segment, line, id) rows in the scan's order, with bins `ids` (ascending) and runs of run_len
    records.  n_seg: also the per-segment matrices (the list then has a segment array).  totals: (n_lines, n_reports) lists to
    add to (accumulate).  Returns (n_lines, n_reports, seg_lines or None, seg_reports or None, skipped)."""
    n, nb = len(records), len(ids)
    recs = (ctypes.c_uint64 * max(3 * n, 1))(*[v for r in records for v in r])
    c_ids = (ctypes.c_uint32 * max(nb, 1))(*ids)
    lines = (ctypes.c_uint64 * max(nb, 1))(*(totals[0] if totals else [0] * nb))
    reports = (ctypes.c_uint64 * max(nb, 1))(*(totals[1] if totals else [0] * nb))
    cells = (n_seg or 0) * nb
    seg_lines = (ctypes.c_uint32 * max(cells, 1))() if n_seg is not None else None
    seg_reports = (ctypes.c_uint32 * max(cells, 1))() if n_seg is not None else None
    skipped = lib().countsim_run(recs, n, 1 if n_seg is not None else 0, c_ids, nb, n_seg or 0, run_len, lines, reports, seg_lines, seg_reports)
    rows = lambda m: [list(m[s * nb:(s + 1) * nb]) for s in range(n_seg)]  # noqa: E731
    return list(lines[:nb]), list(reports[:nb]), rows(seg_lines) if n_seg is not None else None, rows(seg_reports) if n_seg is not None else None, skipped
