"""Context lines of many files in one scan: the plain Python reference the tests use, and the ctypes face of
tests/native/libsegctxsim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_segctx.h (tests/native/segctxsim.cpp).

The reference uses nothing of the product and knows nothing of packs, tiles or line bases: it cuts the packed bytes at the
segments, scans each segment's bytes ALONE, keeps the records the per-segment limit keeps, and asks context_ref (the
single-buffer reference) for the context of those lines in those bytes.  The limit rule in plain words: keep lines until the
running record count reaches m; the context then ends before the next matching line."""
from __future__ import annotations

import ctypes
import os
import subprocess

import context_ref
import invert_ref
import segments_ref as sr

REPO = sr.REPO
SRC = os.path.join(REPO, "tests", "native", "segctxsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libsegctxsim.so")
CSRC = sr.CSRC
CONTEXTS = [(1, 0), (0, 1), (2, 3), (1000, 1000)]

_lib = None


def expected(data, starts, ends, scan_alone, buffer_size, before, after, limit=0):
    """Per segment the context rows [(line, HG_ID_CONTEXT, 0, start, len)], file-relative.  scan_alone(bytes) -> (ordered
    records (line, ...), n_lines), as for segments_ref.expected."""
    out = []
    for a, z in zip(starts, ends):
        own = data[a:z]
        records, _ = scan_alone(own)
        kept = sr.limited(records, limit)
        rows, _owed, _tails = context_ref.expected(own, buffer_size, [r[0] for r in kept], before, after)
        if len(kept) < len(records):  # the limit removed records: nothing from the first removed line on
            rows = [r for r in rows if r[0] < records[len(kept)][0]]
        out.append(rows)
    return out


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_segctx.h", "hg_segments.h", "hg_context.h", "hg_invert.h", "hg_core.h", "hg_db.h", "hg_post.h")]
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
        u64, p64, p32 = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        _lib.segctxsim_run.restype = ctypes.c_long
        _lib.segctxsim_run.argtypes = [ctypes.c_char_p, u64, u64, u64, p64, u64, p64, p64, u64, u64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, p64, p32, u64, p64, p64]
    return _lib


ERRORS = {-1: "output too small", -2: "a tile's count and its walk disagree", -3: "the tiles do not chain", -4: "the records' segments do not ascend",
          -5: "malformed segments"}


def replay(data, tile, buffer_size, records, starts, ends, before, after, limit=0, invert=False):
    """The host replay of the stage over tiles of `tile` bytes.  records: the PACKED scan's ordered records (line, id, to,
    start, len).  Returns a dict: rows (file-relative context records), segment (per row), first_context, kept, tiles_read."""
    n, n_seg = len(records), len(starts)
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    recs = (u64 * (6 * n + 1))()
    for i, (line, rid, to, start, length) in enumerate(records):
        recs[6 * i:6 * i + 6] = [line, rid, to, start, length, 0xFFFFFFFF if rid == invert_ref.HG_ID_INVERT else rid]
    cap = len(data) + 1
    out, out_seg, first, info = (u64 * (6 * cap))(), (u32 * cap)(), (u64 * (n_seg + 1))(), (u64 * 2)()
    got = lib().segctxsim_run(data, len(data), tile, buffer_size - 1, recs, n, (u64 * (n_seg + 1))(*starts), (u64 * (n_seg + 1))(*ends), n_seg, limit,
                              1 if invert else 0, before, after, out, out_seg, cap, first, info)
    assert got >= 0, ERRORS[got]
    rows = []
    for i in range(got):
        line, rid, to, start, length, pattern = out[6 * i:6 * i + 6]
        assert pattern == 0xFFFFFFFF
        rows.append((line, rid, to, start, length))
    return {"rows": rows, "segment": list(out_seg[:got]), "first_context": list(first[:n_seg + 1]), "kept": info[0], "tiles_read": info[1]}
