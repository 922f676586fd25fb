"""The gathered parts (hg_gather_parts): the plain Python reference every parts-gather test uses, and the ctypes face of
tests/native/libpartlinesim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_partlines.h (tests/native/partlinesim.cpp).

The reference knows nothing of records, lower bounds or tiles: it takes the text, the pieces {(segment, line): (S, start, len)}
(S: where the piece's scanned bytes lie in the text; start: hg_hit_aux_t.start, which the offset prefix prints), the parts
[(line, from, to, pattern, segment)] (parts_ref.expected's rows with their file) and writes every entry out by the definition
in include/hypergrep_amd.h."""
from __future__ import annotations

import ctypes
import os
import subprocess

import invert_ref

REPO = invert_ref.REPO
SRC = os.path.join(REPO, "tests", "native", "partlinesim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libpartlinesim.so")
CSRC = invert_ref.CSRC
NUMBER, BYTE_OFFSET, TERMINATE, LINE = 1, 2, 4, 8
FIRST, LAST = 1, 2
ALL_FLAGS = range(16)
COLOR = (b"\x1b[01;31m\x1b[K", b"\x1b[m\x1b[K")  # GNU grep's default match colour (GREP_COLORS unset or empty)

_lib = None


def expected(data: bytes, pieces, parts, flags: int = 0, mark=(b"", b""), byte_base: int = 0):
    """(entries, arrays): the entry of every part as bytes, and line_number / kind / pattern / segment per entry."""
    out, arrays = [], {"line_number": [], "kind": [], "pattern": [], "segment": []}
    key = lambda p: (p[4], p[0])  # noqa: E731
    for q, p in enumerate(parts):
        line, frm, to, pattern, seg = p
        first = q == 0 or key(parts[q - 1]) != key(p)
        last = q + 1 == len(parts) or key(parts[q + 1]) != key(p)
        b = b""
        if key(p) in pieces:  # (the parts stage leaves no part without its piece's record; the rules give such a part no bytes)
            S, start, length = pieces[key(p)]
            if not flags & LINE or first:
                if flags & NUMBER:
                    b += b"%d:" % ((line + 1) % 2**64)
                if flags & BYTE_OFFSET:
                    b += b"%d:" % ((byte_base + start + (0 if flags & LINE else frm)) % 2**64)
            if flags & LINE:
                b += data[S + (0 if first else parts[q - 1][2]):S + frm]
            b += mark[0] + data[S + frm:S + to] + mark[1]
            end = to
            if flags & LINE and last:
                b += data[S + to:S + length]
                end = length
            if flags & TERMINATE and (not flags & LINE or last) and data[S + end - 1:S + end] != b"\n":
                b += b"\n"
        out.append(b)
        for name, v in (("line_number", line), ("kind", (FIRST if first else 0) | (LAST if last else 0)), ("pattern", pattern), ("segment", seg)):
            arrays[name].append(v)
    return out, arrays


def pieces_of(data: bytes, buffer_size: int, line_base: int = 0, segment: int = 0, at: int = 0):
    """{(segment, line): (S, start, len)} of one text scanned alone (`at`: where it lies in a pack)."""
    return {(segment, line_base + i): (at + a, a, len(p)) for i, (a, p) in enumerate(invert_ref.pieces(data, buffer_size))}


def joined(entries, arrays):
    """Line mode: the entries of every piece joined, as Scanner.part_lines() gives them."""
    out = []
    for b, kind in zip(entries, arrays["kind"]):
        if kind & FIRST:
            out.append(b)
        else:
            out[-1] += b
    return out


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_partlines.h", "hg_gather.h", "hg_parts.h", "hg_som.h", "hg_context.h", "hg_invert.h", "hg_core.h", "hg_db.h", "hg_post.h")]
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
        u64, u32, p64, p32 = ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        _lib.partlinesim_run.restype = ctypes.c_long
        _lib.partlinesim_run.argtypes = [ctypes.c_char_p, u64, u64, p64, u64, p64, u64, ctypes.c_int, p64, u32, u64, ctypes.c_char_p, u32, ctypes.c_char_p, u32, u64,
                                         ctypes.c_char_p, u64, p64, p64, p32, p32, p32, p64]
        _lib.partlinesim_digits.restype = u32
        _lib.partlinesim_digits.argtypes = [u64]
        _lib.partlinesim_sizes.restype = None
        _lib.partlinesim_sizes.argtypes = [p32]
    return _lib


ERRORS = {-1: "output too small", -2: "a text read left [0, nbytes rounded up to 4)", -3: "the lanes' chunks and the byte-by-byte definition disagree"}


def replay(data: bytes, tile: int, records, parts, flags: int = 0, mark=(b"", b""), byte_base: int = 0, seg_start=None, base: int = 0):
    """The host replay of the stage with output spans of `tile` bytes.  records: the scan's final records as (line, start, len,
    segment) rows in order (several per line allowed); parts as for expected().  seg_start: the files' offsets after a scan
    with segments.  base (a multiple of 4) is added to every start (to seg_start with segments) and taken off again where the
    text is read.  Returns (entries, arrays)."""
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    n, m = len(records), len(parts)
    recs = (u64 * (4 * n + 1))()
    for i, (line, start, length, seg) in enumerate(records):
        recs[4 * i:4 * i + 4] = [line, start + (0 if seg_start is not None else base), length, seg]
    rows = (u64 * (5 * m + 1))()
    for i, p in enumerate(parts):
        rows[5 * i:5 * i + 5] = list(p)
    starts = (u64 * (len(seg_start) + 1))(*[s + base for s in seg_start]) if seg_start is not None else None
    cap = sum(r[2] for r in records) + m * (2 * 21 + 34) + sum(p[2] - p[1] for p in parts) + 64
    out = ctypes.create_string_buffer(cap)
    entry_off, line_number, totals = (u64 * (m + 2))(), (u64 * (m + 1))(), (u64 * 2)()
    kind, pattern, segment = (u32 * (m + 1))(), (u32 * (m + 1))(), (u32 * (m + 1))()
    rc = lib().partlinesim_run(data, len(data), base, recs, n, rows, m, 1 if seg_start is not None else 0, starts, flags, byte_base, bytes(mark[0]), len(mark[0]),
                               bytes(mark[1]), len(mark[1]), tile, out, cap, entry_off, line_number, kind, pattern, segment, totals)
    assert rc == 0, ERRORS[rc]
    ne, nb = totals[0], totals[1]
    blob = out.raw[:nb]
    assert ne == m and entry_off[0] == 0 and entry_off[ne] == nb
    return [blob[entry_off[j]:entry_off[j + 1]] for j in range(ne)], {"line_number": list(line_number[:ne]), "kind": list(kind[:ne]), "pattern": list(pattern[:ne]),
                                                                        "segment": list(segment[:ne])}
