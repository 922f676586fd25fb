"""Face B's delivery: the ctypes face of tests/native/libdeliversim.so, a TEST-ONLY C face over hypergrep_amd/csrc/hg_deliver.h
(see tests/native/deliversim.cpp), the chunk inputs it is fed, and the plain Python expectation, which knows nothing of chunks.

A case is a text, the set of its matching lines with their reports (and, for parts mode, their parts), `before` / `after`, the
match limit, the ring's batch size and the lines at which the text is cut into chunks.  `play` does what scan_file's loop does:
per chunk it asks the state object for the context stage's parameters, makes the chunk's records (context and tail records
from context_ref.classify), hands them over, and stops when told to."""
from __future__ import annotations

import ctypes
import os
import subprocess

import context_ref
import invert_ref

REPO = invert_ref.REPO
SRC = os.path.join(REPO, "tests", "native", "deliversim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libdeliversim.so")
CSRC = invert_ref.CSRC
HEADERS = ("hg_deliver.h", "hg_reader.h", "hg_context.h", "hg_invert.h", "hg_parts.h", "hg_som.h", "hg_core.h", "hg_db.h", "hg_post.h")
BUFFER_SIZE = 64  # (above every line of the tests' texts: a line is a piece)
PATTERN_IDS = (11, 7, 4000000000)  # the report ids of expressions 0, 1, 2 (parts carry the expression, results the id)

_lib = None


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, h) for h in HEADERS]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"  # built aside and renamed into place (parallel test workers)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-pthread", "-o", tmp, SRC, "-lz", "-ldl"])
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        u64, u32, p64, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
        lists = [ctypes.c_char_p, p64, u64, p64, u64, p64, u64, ctypes.POINTER(u32), u32]
        _lib.deliversim_new.restype = vp
        _lib.deliversim_new.argtypes = [ctypes.c_int, u32, u32, u64, ctypes.c_int, ctypes.c_int]
        _lib.deliversim_free.argtypes = [vp]
        _lib.deliversim_context_params.argtypes = [vp, p64]
        _lib.deliversim_line_base.restype = u64
        _lib.deliversim_line_base.argtypes = [vp]
        _lib.deliversim_chunk.argtypes = [vp] + lists + [u64, u64]
        _lib.deliversim_file.argtypes = [vp] + lists
        _lib.deliversim_flush.argtypes = [vp]
        _lib.deliversim_sizes.argtypes = [vp, p64]
        _lib.deliversim_read.argtypes = [vp, p64, ctypes.c_char_p, p64]
        _lib.deliversim_cut.restype = u64
        _lib.deliversim_cut.argtypes = [ctypes.c_char_p, u64, u64]
    return _lib


def cut(buf: bytes, bs1: int) -> int:
    return lib().deliversim_cut(buf, len(buf), bs1)


def _words(rows):
    flat = [v for row in rows for v in row]
    return (ctypes.c_uint64 * max(1, len(flat)))(*flat)


class Text:
    """A text with its pieces: piece q is data[start[q] : start[q] + len(piece[q])]; lines_end[q] is where line q ends."""

    def __init__(self, lines, final_newline=True):
        self.data = b"\n".join(lines) + (b"\n" if lines and final_newline else b"")
        pcs = invert_ref.pieces(self.data, BUFFER_SIZE)
        assert len(pcs) == len(lines)
        self.start = [a for a, _ in pcs]
        self.piece = [p for _, p in pcs]
        self.n = len(pcs)
        self.line_end = [self.data.find(b"\n", a) + 1 or len(self.data) for a in self.start]


def read_results(handle):
    sizes = (ctypes.c_uint64 * 3)()
    lib().deliversim_sizes(handle, sizes)
    rows = (ctypes.c_uint64 * max(1, 3 * sizes[0]))()
    data = ctypes.create_string_buffer(max(1, sizes[1]))
    batches = (ctypes.c_uint64 * max(1, sizes[2]))()
    lib().deliversim_read(handle, rows, data, batches)
    out, at = [], 0
    for i in range(sizes[0]):
        rid, line, length = rows[3 * i:3 * i + 3]
        out.append((rid, line, data.raw[at:at + length]))
        at += length
    return out, list(batches[:sizes[2]])


def chunk_lists(text: Text, a: int, b: int, reports, parts, cls):
    """The records of the chunk of the lines [a, b), offsets relative to the chunk's first byte.  reports: {line: [(to, id)] in the
    order they are handed over}; parts: {line: [(from, to, expression)]}; cls: context_ref.classify's classes of the chunk."""
    origin = text.start[a] if a < text.n else len(text.data)
    end = text.line_end[b - 1] if b > a else origin
    hits = [(q, rid, to, text.start[q] - origin, len(text.piece[q])) for q in range(a, b) for to, rid in reports.get(q, ())]
    ctx = [(q, cls[q], text.start[q] - origin, len(text.piece[q])) for q in sorted(cls)]
    prt = [(q, f, t, e) for q in range(a, b) if q in reports for f, t, e in parts.get(q, ())]
    return text.data[origin:end], hits, ctx, prt


def play(text: Text, edges, reports, before, after, limit, buffer_count, parts=None, record=None):
    """The call over the chunks edges[i] .. edges[i + 1]: ([(id, line, bytes)], batch sizes, chunks read).  record: a list that receives the
    call as the words of deliversim's stand-alone replay."""
    L = lib()
    handle = L.deliversim_new(1 if parts is not None else 0, before, after, limit, buffer_count, BUFFER_SIZE)
    ids = (ctypes.c_uint32 * len(PATTERN_IDS))(*PATTERN_IDS)
    chunks = []
    try:
        params = (ctypes.c_uint64 * 4)()
        for a, b in zip(edges, edges[1:]):
            L.deliversim_context_params(handle, params)
            assert L.deliversim_line_base(handle) == a
            cls, owed = ({}, 0) if parts is not None else context_ref.classify(b - a, [q for q in reports if a <= q < b], params[0], params[1], a, params[2], bool(params[3]))
            data, hits, ctx, prt = chunk_lists(text, a, b, reports, parts or {}, cls)
            chunks.append([len(data)] + list(data) + [len(hits)] + [v for r in hits for v in r] + [len(ctx)] + [v for r in ctx for v in r] + [len(prt)] + [v for r in prt for v in r] + [b - a, owed])
            if L.deliversim_chunk(handle, data, _words(hits), len(hits), _words(ctx), len(ctx), _words(prt), len(prt), ids, len(PATTERN_IDS), b - a, owed):
                break
        L.deliversim_flush(handle)
        if record is not None:
            record += [1, 1 if parts is not None else 0, before, after, limit, buffer_count, BUFFER_SIZE, len(PATTERN_IDS)] + list(PATTERN_IDS) + [len(chunks)] + [v for c in chunks for v in c]
        return read_results(handle) + (len(chunks),)
    finally:
        L.deliversim_free(handle)


def play_file(text: Text, reports, before, after, buffer_count, parts=None):
    """The whole text through the line routines of the packed route (the stages have settled limit and context already)."""
    L = lib()
    handle = L.deliversim_new(1 if parts is not None else 0, before, after, 0, buffer_count, BUFFER_SIZE)
    try:
        cls = {} if parts is not None else context_ref.classify(text.n, list(reports), before, after)[0]
        data, hits, ctx, prt = chunk_lists(text, 0, text.n, reports, parts or {}, cls)
        L.deliversim_file(handle, data, _words(hits), len(hits), _words(ctx), len(ctx), _words(prt), len(prt), (ctypes.c_uint32 * len(PATTERN_IDS))(*PATTERN_IDS), len(PATTERN_IDS))
        return read_results(handle)
    finally:
        L.deliversim_free(handle)


def expected(text: Text, reports, before, after, limit, parts=None):
    """[(id, line, bytes)] of the whole call, from the whole text: the sorted merge of the matches and the context lines, cut by
    the limit: delivery stops after the first line at which the delivered reports reach it, and with `after` the context
    lines that directly follow that line still go out, `after` at most, up to the next matching line or the end of the text."""
    context = {} if parts is not None else {r[0] for r in context_ref.expected(text.data, BUFFER_SIZE, list(reports), before, after)[0]}
    out, delivered = [], 0
    for q in range(text.n):
        if q in reports:
            if parts is not None:
                out += [(PATTERN_IDS[e], q, text.piece[q][f:t]) for f, t, e in parts.get(q, ())]
            else:
                out += [(rid, q, text.piece[q]) for _to, rid in sorted(reports[q])]
            delivered += len(reports[q])
            if limit and delivered >= limit:
                follow = q + 1
                while after and parts is None and follow < text.n and follow <= q + after and follow not in reports:
                    out.append((context_ref.HG_ID_CONTEXT, follow, text.piece[follow]))
                    follow += 1
                break
        elif q in context:
            out.append((context_ref.HG_ID_CONTEXT, q, text.piece[q]))
    return out


def expected_chunks(text: Text, edges, reports, after, limit, parts=None):
    """How many chunks the call reads: all, unless the limit is reached; then through the chunk of the line that settles the
    trailing context: the first matching line behind the stopping line, or the `after`-th line behind it, whichever comes first."""
    delivered = 0
    for q in sorted(reports):
        delivered += len(reports[q])
        if limit and delivered >= limit:
            settles = q
            if after and parts is None:
                settles = min([m for m in reports if m > q] + [q + after, text.n - 1])
            return next(i + 1 for i, b in enumerate(edges[1:]) if settles < b)
    return len(edges) - 1
