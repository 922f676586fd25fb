"""Segments (many files in one scan): the plain Python reference the segment tests use, the cases they share, and the ctypes
face of tests/native/libsegsim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_segments.h (tests/native/segsim.cpp).

The reference knows nothing of tiles or line bases: it cuts the packed bytes at the segments, takes each segment's records
from a scan of those bytes ALONE (any function that maps bytes to ordered records), and applies the per-segment limit."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import invert_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "segsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libsegsim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
PAD = b"\0\n"
TILE = 16384

_lib = None


def pack(files):
    """The packing rule: (packed bytes, seg_start, seg_end).  A file that is empty or ends in a newline is packed as it is,
    any other is followed by the two pad bytes."""
    data, starts, ends = bytearray(), [], []
    for f in files:
        starts.append(len(data))
        data += f
        ends.append(len(data))
        if f and not f.endswith(b"\n"):
            data += PAD
    return bytes(data), starts, ends


def limited(records, limit):
    """Rule (d): the records up to and including the line on which the running record count reaches `limit`."""
    if limit <= 0 or len(records) < limit:
        return list(records)
    cut = records[limit - 1][0]
    return [r for r in records if r[0] <= cut]


def expected(data, starts, ends, scan_alone, limit=0):
    """Per segment (records, n_lines, n_selected): scan_alone(bytes) -> (ordered records (line, ...), n_lines) run on each
    segment's own bytes, the limit applied."""
    out = []
    for a, z in zip(starts, ends):
        records, n_lines = scan_alone(data[a:z])
        records = limited(records, limit)
        out.append((records, n_lines, len({r[0] for r in records})))
    return out


def re_scan(patterns, buffer_size, invert=False):
    """A stand-in scan for the host tests: bytes -> ([(line, id, to, start, len)], n_lines) with Python's `re` run on every
    piece's scanned bytes (patterns: [(id, bytes regex)]; one record per match end), or its complement for invert."""
    compiled = [(i, re.compile(p)) for i, p in patterns]

    def scan(data):
        pieces = invert_ref.pieces(data, buffer_size)
        hits = []
        for line, (a, scanned) in enumerate(pieces):
            found = sorted({(i, m.end()) for i, rx in compiled for m in rx.finditer(scanned) if m.end() > m.start()})
            hits += [(line, i, to, a, len(scanned)) for i, to in found]
        if invert:
            return invert_ref.expected(data, buffer_size, [h[0] for h in hits]), len(pieces)
        return hits, len(pieces)

    return scan


def packed_records(data, starts, ends, scan, buffer_size, invert):
    """The records the stage gets from the PACKED buffer.  Plain: scan(data)'s hits.  Inverted: the hits that lie in a pad are
    removed first (the replay's hg_seg_pad_hit), then the pieces without a hit are selected, pads and all."""
    hits, _ = scan(data)
    if not invert:
        return hits
    u64 = ctypes.c_uint64
    n = len(starts)
    sa, ea = (u64 * (n + 1))(*starts), (u64 * (n + 1))(*ends)
    kept = [h for h in hits if not lib().segsim_pad_hit(sa, ea, n, h[3])]
    return invert_ref.expected(data, buffer_size, [h[0] for h in kept])


def filler(n, word=b"xy abc z\n"):
    """n bytes of lines that end in a newline (n >= 1)."""
    return (word * (n // len(word) + 1))[:n - 1] + b"\n"


def cases(tile, buffer_size, multiples=(1, 2)):
    """[(name, [file bytes])]: the geometry every segment test runs, for tiles of `tile` bytes and pieces of buffer_size - 1.
    multiples: the k of the unterminated last lines of k * (buffer_size - 1) + {0, -1, -2, 1} bytes."""
    bs1 = buffer_size - 1
    out = [
        ("boundary_at_tile_end", [filler(tile), b"abc 1\n", b"no\nab\n"]),
        ("boundary_before_tile_end", [filler(tile - 1), b"abc 2\n", b"q\n"]),
        ("boundary_after_tile_end", [filler(tile + 1), b"abc 3\n", b"q\n"]),
        ("300_one_line_segments", [b"abc\n" if i % 3 else b"q\n" for i in range(300)]),
        ("empty_segments", [b"", b"", b"abc\nq\n", b"", b"", b"", b"zz abc", b"", b"q\nab\n", b"", b""]),
        ("three_tiles", [b"abc\n", filler(2 * tile + tile // 2), b"tail abc"]),
        ("whole_buffer", [filler(tile + tile // 3)]),
        ("whole_buffer_unterminated", [filler(tile // 2 + 5) + b"abc"]),
        ("nul_only_last_line", [b"abc\n\0\0\0", b"abc\n", b"\0", b"q abc\n"]),
        ("inner_nul_last_line", [b"q\nxabc\0yabc", b"abc\n", b"\0abc\0", b"abc"]),
        ("nul_lines", [b"\0\0abc\n\0\n\0\0\n", b"abc\0\n"]),
    ]
    for k in multiples:
        for d in (0, -1, -2, 1):
            n = k * bs1 + d
            if n >= 1:
                out.append((f"unterminated_{k}x{'%+d' % d}", [b"abc\n" + (b"abc" * n)[:n], b"q\n", (b"zabc" * n)[:n], b"abc\n"]))
    return out


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_segments.h", "hg_invert.h", "hg_core.h", "hg_db.h", "hg_post.h")]
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
        _lib.segsim_pad_hit.argtypes = [p64, p64, u64, u64]
        _lib.segsim_run.restype = ctypes.c_long
        _lib.segsim_run.argtypes = [ctypes.c_char_p, u64, u64, u64, p64, p32, u64, p64, p64, u64, u64, ctypes.c_int, p64, p32, p32, p64, p64, p64, p64, p32, p64]
    return _lib


class Malformed(Exception):
    """The replay's argument check refused the segments; args[0]: the HG_SEG_BAD_* bits."""


def replay(data, tile, buffer_size, records, starts, ends, limit=0, invert=False, froms=None):
    """The host replay of the segment stage over tiles of `tile` bytes.  records: the PACKED scan's ordered records
    (line, id, to, start, len).  Returns a dict: records (file-relative), from, segment (per record), first_record, n_lines,
    n_selected, base, tiles_walked."""
    n, n_seg = len(records), len(starts)
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    recs = (u64 * (6 * n + 1))()
    for i, (line, rid, to, start, length) in enumerate(records):
        recs[6 * i:6 * i + 6] = [line, rid, to, start, length, 0xFFFFFFFF if rid == invert_ref.HG_ID_INVERT else rid]
    frm = (u32 * (n + 1))(*(froms if froms is not None else range(n)))
    out_recs, out_from, out_seg = (u64 * (6 * n + 1))(), (u32 * (n + 1))(), (u32 * (n + 1))()
    first, n_lines, n_sel, base = (u64 * (n_seg + 1))(), (u64 * (n_seg + 1))(), (u64 * (n_seg + 1))(), (u64 * (n_seg + 1))()
    bad, walked = u32(), u64()
    kept = lib().segsim_run(data, len(data), tile, buffer_size - 1, recs, frm, n, (u64 * (n_seg + 1))(*starts), (u64 * (n_seg + 1))(*ends), n_seg, limit,
                            1 if invert else 0, out_recs, out_from, out_seg, first, n_lines, n_sel, base, ctypes.byref(bad), ctypes.byref(walked))
    if kept == -1:
        raise Malformed(bad.value)
    assert kept >= 0, {-2: "the piece walk and the per-chunk finish disagree on a line base", -3: "a boundary got no line base"}[kept]
    return {
        "records": [tuple(out_recs[6 * i:6 * i + 5]) for i in range(kept)],
        "from": list(out_from[:kept]),
        "segment": list(out_seg[:kept]),
        "first_record": list(first[:n_seg + 1]),
        "n_lines": list(n_lines[:n_seg]),
        "n_selected": list(n_sel[:n_seg]),
        "base": list(base[:n_seg]),
        "tiles_walked": walked.value,
    }
