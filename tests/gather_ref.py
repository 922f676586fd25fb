"""The gathered lines (hg_gather_lines): the plain Python reference every gather test uses, and the ctypes face of
tests/native/libgathersim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_gather.h (see tests/native/gathersim.cpp).

The reference knows nothing of records, ranks or tiles: it takes invert_ref.pieces (split at '\\n', cut into pieces of
buffer_size - 1 bytes, trimmed), the set of selected line numbers, optionally context_ref.classify's classes, and writes
every entry out by the definition in include/hypergrep_amd.h."""
from __future__ import annotations

import ctypes
import os
import subprocess

import context_ref
import invert_ref

REPO = invert_ref.REPO
SRC = os.path.join(REPO, "tests", "native", "gathersim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libgathersim.so")
CSRC = invert_ref.CSRC
CONTEXT, TERMINATE, NUMBER, SEPARATOR = 1, 2, 4, 8
MATCH, KIND_CONTEXT, KIND_TAIL = 0, 1, 2
ALL_FLAGS = range(16)

_lib = None


def render(items, flags):
    """items: [(segment, line_number, kind, body)] in output order -> the entries as a list of bytes."""
    out, prev = [], None
    for seg, line, kind, body in items:
        b = b""
        if flags & SEPARATOR and prev is not None and (seg != prev[0] or line != prev[1] + 1):
            b += b"--\n"
        if flags & NUMBER:
            b += str(line + 1).encode() + (b":" if kind == MATCH else b"-")
        b += body
        if flags & TERMINATE and not body.endswith(b"\n"):
            b += b"\n"
        out.append(b)
        prev = (seg, line)
    return out


def items_of(data: bytes, buffer_size: int, selected_lines, line_base: int = 0, classes=None, flags: int = 0, segment: int = 0):
    """[(segment, line_number, kind, body)] of one text: its pieces whose number is selected, and with CONTEXT those that
    `classes` ({piece number: HG_ID_CONTEXT | HG_ID_CONTEXT_TAIL}, context_ref.classify's) names, in line order."""
    selected = set(selected_lines)
    classes = classes if (flags & CONTEXT and classes) else {}
    out = []
    for i, (_a, body) in enumerate(invert_ref.pieces(data, buffer_size)):
        q = line_base + i
        if q in selected:
            out.append((segment, q, MATCH, body))
        elif q in classes:
            out.append((segment, q, KIND_TAIL if classes[q] == context_ref.HG_ID_CONTEXT_TAIL else KIND_CONTEXT, body))
    return out


def expected(data: bytes, buffer_size: int, selected_lines, flags: int, line_base: int = 0, context=None, carry_after: int = 0, tail: bool = False):
    """(entries, items) of a text scanned alone.  selected_lines: the line numbers (line_base included) the scan delivers a
    record for (the matching lines, or their complement for an inverted scan); context = (before, after) of the scan."""
    classes = None
    if context is not None or carry_after or tail:
        before, after = context or (0, 0)
        classes, _ = context_ref.classify(len(invert_ref.pieces(data, buffer_size)), selected_lines, before, after, line_base, carry_after, tail)
    items = items_of(data, buffer_size, selected_lines, line_base, classes, flags)
    return render(items, flags), items


def expected_files(files, buffer_size: int, selected_per_file, flags: int, context_per_file=None):
    """(entries, items, first_entry) of a pack of files.  selected_per_file[s]: the file-relative line numbers file s keeps a
    record for; context_per_file[s]: the file-relative numbers of its context pieces (from a per-file reference), or None."""
    items, first = [], [0]
    for s, f in enumerate(files):
        classes = {q: context_ref.HG_ID_CONTEXT for q in context_per_file[s]} if context_per_file is not None else None
        items += items_of(f, buffer_size, selected_per_file[s], 0, classes, flags, s)
        first.append(len(items))
    return render(items, flags), items, first


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_gather.h", "hg_context.h", "hg_invert.h", "hg_core.h", "hg_db.h", "hg_post.h")]
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
        _lib.gathersim_run.restype = ctypes.c_long
        _lib.gathersim_run.argtypes = [ctypes.c_char_p, u64, u64, p64, u64, u64, ctypes.c_int, p64, p64, p64, u64, ctypes.c_uint32, u64, ctypes.c_char_p, u64, p64, p64, p32,
                                       p32, p64, p64]
        _lib.gathersim_digits.restype = ctypes.c_uint32
        _lib.gathersim_digits.argtypes = [u64]
        _lib.gathersim_tile.restype = ctypes.c_uint32
    return _lib


ERRORS = {-1: "output too small", -2: "a text read left [0, nbytes rounded up to 4)", -3: "the lanes' chunks and the byte-by-byte definition disagree"}


def replay(data: bytes, tile: int, main, ctx, flags: int, segments=None, base: int = 0):
    """The host replay of the stage with output spans of `tile` bytes.  main / ctx: the scan's two record lists as
    (line, id, to, start, len) rows, with the segment of each as a sixth column when `segments` = (seg_start, first_record,
    first_context or None) is given (ctx is ignored without the CONTEXT flag, as the stage ignores it).  base is added to every
    start and taken off again where the text is read.  Returns a dict: entries, line_number, kind, segment, first_entry."""
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    ctx = list(ctx) if flags & CONTEXT else []
    rows = list(main) + ctx
    n = len(rows)
    recs = (u64 * (5 * n + 1))()
    for i, r in enumerate(rows):  # (with segments the records are file-relative: the base travels in seg_start)
        recs[5 * i:5 * i + 5] = [r[0], r[1], r[3] + (0 if segments else base), r[4], r[5] if segments else 0]
    n_seg = len(segments[0]) if segments else 0
    seg_start = first_record = first_context = None
    if segments:
        seg_start = (u64 * (n_seg + 1))(*[s + base for s in segments[0]])
        first_record = (u64 * (n_seg + 1))(*segments[1])
        first_context = (u64 * (n_seg + 1))(*segments[2]) if segments[2] is not None and ctx else None
    cap = sum(r[4] + 32 for r in rows) + 64
    out = ctypes.create_string_buffer(cap)
    entry_off, line_number, totals = (u64 * (n + 2))(), (u64 * (n + 1))(), (u64 * 2)()
    kind, segment, first_entry = (u32 * (n + 1))(), (u32 * (n + 1))(), (u64 * (n_seg + 1))()
    rc = lib().gathersim_run(data, len(data), base, recs, len(main), len(ctx), 1 if segments else 0, seg_start, first_record, first_context, n_seg, flags, tile, out, cap,
                             entry_off, line_number, kind, segment, first_entry, totals)
    assert rc == 0, ERRORS[rc]
    ne, nb = totals[0], totals[1]
    blob = out.raw[:nb]
    assert entry_off[0] == 0 and entry_off[ne] == nb
    return {"entries": [blob[entry_off[j]:entry_off[j + 1]] for j in range(ne)], "line_number": list(line_number[:ne]), "kind": list(kind[:ne]),
            "segment": list(segment[:ne]) if segments else None, "first_entry": list(first_entry[:n_seg + 1]) if segments else None}
