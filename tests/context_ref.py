"""Context lines (grep -A / -B / -C): the plain Python reference every context test uses, and the ctypes face of
tests/native/libcontextsim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_context.h (see tests/native/contextsim.cpp).

The reference knows nothing of tiles: it takes invert_ref.pieces (split at '\\n', cut into pieces of buffer_size - 1 bytes,
trimmed), the set of matching lines, A, B, the carry and the tail flag, and classifies every piece by the definition in
include/hypergrep_amd.h, one piece at a time."""
from __future__ import annotations

import ctypes
import os
import subprocess

import invert_ref

REPO = invert_ref.REPO
SRC = os.path.join(REPO, "tests", "native", "contextsim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libcontextsim.so")
CSRC = invert_ref.CSRC
HG_ID_CONTEXT = 0xFFFFFFFE
HG_ID_CONTEXT_TAIL = 0xFFFFFFFD

_lib = None


def classify(n_pieces: int, matching_lines, before: int, after: int, line_base: int = 0, carry_after: int = 0, tail: bool = False):
    """({piece number: HG_ID_CONTEXT | HG_ID_CONTEXT_TAIL} of the context and tail pieces, owed_after)."""
    end = line_base + n_pieces
    matching = sorted(set(m for m in matching_lines if line_base <= m < end))
    covered = set()
    for m in matching:  # (clipped to the buffer first: A and B may be 2^32 - 1)
        covered.update(range(max(line_base, m - before), min(end, m + after + 1)))
    covered.update(range(line_base, min(end, line_base + carry_after)))
    out = {}
    match_set = set(matching)
    for q in range(line_base, end):
        if q in match_set:
            continue
        if q in covered:
            out[q] = HG_ID_CONTEXT
        elif tail and q >= end - before:
            out[q] = HG_ID_CONTEXT_TAIL
    owed = max(0, matching[-1] + after - (end - 1)) if matching else max(0, carry_after - n_pieces)
    return out, owed


def expected(data: bytes, buffer_size: int, matching_lines, before: int, after: int, line_base: int = 0, carry_after: int = 0, tail: bool = False):
    """([(line_number, id, 0, start, len)] of the context and tail pieces in line order: what Scanner.context() gives,
    owed_after, n_tail).  matching_lines: the line numbers (line_base included) the call delivers a record for."""
    pcs = invert_ref.pieces(data, buffer_size)
    cls, owed = classify(len(pcs), matching_lines, before, after, line_base, carry_after, tail)
    rows = [(q, cls[q], 0, pcs[q - line_base][0], len(pcs[q - line_base][1])) for q in sorted(cls)]
    return rows, owed, sum(1 for r in rows if r[1] == HG_ID_CONTEXT_TAIL)


def chain(n_pieces_per_buffer, matching_lines, before: int, after: int):
    """The chaining identity on piece numbers alone: the buffers hold n_pieces_per_buffer[i] pieces each, one after the other
    from piece 0.  Returns the merged context piece numbers (tail records kept by the rule of include/hypergrep_amd.h)."""
    matching = sorted(set(matching_lines))
    out, base, carry = [], 0, 0
    held = []  # tail candidates of the buffers so far, still undecided
    for n in n_pieces_per_buffer:
        cls, owed = classify(n, matching, before, after, base, carry, tail=True)
        first = next((m for m in matching if base <= m < base + n), None)
        if first is not None:
            out += [q for q in held if q >= first - before]
            held = []
        out += [q for q in sorted(cls) if cls[q] == HG_ID_CONTEXT]
        tails = [q for q in sorted(cls) if cls[q] == HG_ID_CONTEXT_TAIL]
        held = (held + tails)[-before:] if before else []
        base += n
        carry = owed
    return sorted(out)


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_context.h", "hg_invert.h", "hg_core.h", "hg_db.h", "hg_post.h")]
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
        _lib.contextsim_run.restype = ctypes.c_long
        _lib.contextsim_run.argtypes = [ctypes.c_char_p, u64, u64, u64, u64, ctypes.POINTER(u64), u64, ctypes.c_uint32, ctypes.c_uint32, u64, ctypes.c_int,
                                        ctypes.POINTER(u64), u64, ctypes.POINTER(u64)]
    return _lib


ERRORS = {-1: "output too small", -2: "a tile's count and its walk disagree", -3: "the tiles' first piece numbers do not chain",
          -4: "the tail count and the walk's tail records disagree"}


def replay(data: bytes, tile: int, buffer_size: int, hit_lines, before: int, after: int, line_base: int = 0, carry_after: int = 0, tail: bool = False):
    """The host replay of the context stage over tiles of `tile` bytes: ([(line_number, id, to, start, len)], owed_after,
    n_tail, n_pieces).  hit_lines: the line numbers of the call's records, ascending (a line may repeat)."""
    hit_lines = list(hit_lines)
    cap = len(data) + 1
    out = (ctypes.c_uint64 * (6 * cap))()
    info = (ctypes.c_uint64 * 3)()
    n = lib().contextsim_run(data, len(data), tile, buffer_size - 1, line_base, (ctypes.c_uint64 * len(hit_lines))(*hit_lines), len(hit_lines), before, after,
                             carry_after, 1 if tail else 0, out, cap, info)
    assert n >= 0, ERRORS[n]
    rows = []
    for i in range(n):
        line, start, length, rid, to, pattern = out[6 * i:6 * i + 6]
        assert pattern == 0xFFFFFFFF
        rows.append((line, rid, to, start, length))
    return rows, info[0], info[1], info[2]
