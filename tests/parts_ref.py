"""Matched parts (grep -o over all expressions): the plain Python reference every parts test uses.  It knows nothing of the
kernel or of hg_parts.h: pieces come from invert_ref.pieces, "expression p matches exactly [s, e)" is decided by Python `re`
with the construction somsim_py.start_by_brute_force uses (a lookahead that pins the distance to the piece's end keeps `$`,
`\\b`, `\\Z` honest at e; `pos` keeps `^`, `\\b` honest at s), and the parts loop is the definition in
include/hypergrep_amd.h written out."""
from __future__ import annotations

import re

import invert_ref
import regex_gen

_RE_CACHE: dict = {}


def _exact_re(pat: str, flags: int, tail: int):
    key = (pat, flags & 7, tail)
    cre = _RE_CACHE.get(key)
    if cre is None:
        if len(_RE_CACHE) > 20000:
            _RE_CACHE.clear()
        cre = _RE_CACHE[key] = re.compile(b"(?:" + pat.encode() + b")(?=(?s:.{%d})\\Z)" % tail, regex_gen.py_flags(flags))
    return cre


def matches_exactly(pat: str, flags: int, piece: bytes, s: int, e: int) -> bool:
    return _exact_re(pat, flags, len(piece) - e).match(piece, s) is not None


def _plain_re(pat: str, flags: int):
    key = (pat, flags & 7, None)
    cre = _RE_CACHE.get(key)
    if cre is None:
        cre = _RE_CACHE[key] = re.compile(b"(?:" + pat.encode() + b")", regex_gen.py_flags(flags))
    return cre


def piece_parts(pats, flags, piece: bytes):
    """[(from, to, pattern)] of one piece's scanned bytes, by the definition: from a cursor the smallest start at which any
    expression matches exactly some [s, e), the largest such e, the lowest expression that matches exactly [s, e)."""
    n = len(piece)
    out = []
    cursor = 0
    while cursor < n:
        found = None
        for s in range(cursor, n):
            # (an expression that has no match at s at all has no exact one either: spares the per-end tries)
            live = [j for j in range(len(pats)) if _plain_re(pats[j], flags[j]).match(piece, s)]
            if not live:
                continue
            for e in range(n, s, -1):
                who = [j for j in live if matches_exactly(pats[j], flags[j], piece, s, e)]
                if who:
                    found = (s, e, who[0])
                    break
            if found:
                break
        if not found:
            break
        out.append(found)
        cursor = found[1]
    return out


def expected(data: bytes, buffer_size: int, pats, flags, hit_lines, line_base: int = 0):
    """[(line_number, from, to, pattern)] for the pieces whose number (line_base included) is in hit_lines: what
    Scanner.parts() gives after a parts scan whose hits have those distinct line numbers."""
    wanted = set(hit_lines)
    out = []
    for i, (_a, piece) in enumerate(invert_ref.pieces(data, buffer_size)):
        if line_base + i in wanted:
            out += [(line_base + i, f, t, p) for f, t, p in piece_parts(pats, flags, piece)]
    return out


def matching_lines(data: bytes, buffer_size: int, pats, flags, line_base: int = 0):
    """The piece numbers in which some expression matches anywhere: the distinct line numbers of a scan's hits when every
    expression reports (no limits, no QUIET)."""
    out = []
    for i, (_a, piece) in enumerate(invert_ref.pieces(data, buffer_size)):
        if any(_plain_re(p, f).search(piece) for p, f in zip(pats, flags)):
            out.append(line_base + i)
    return out
