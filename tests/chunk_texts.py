"""Texts for the stage suites' pipeline tests: more than 2048 tiles, so that HG_CHUNK_TILES=1024 (the smallest chunk the
engine honours: one tile-scan block) gives three pipeline chunks with cuts at 16 MiB and 32 MiB.

The references stay affordable because the text is long runs of a few repeated filler lines; the stage's interesting lines
stand in clusters around the cuts: the last line before the first cut ends on the cut's last byte and the next one begins on
its first; one line lies across the second cut.  Every line is shorter than the scan buffer the tests use (1000), so pieces
are lines, and a reference that evaluates each DISTINCT line once covers the text (distinct / expand below)."""
from __future__ import annotations

TILE = 16384
CHUNK_ENV = {"HG_CHUNK_TILES": "1024"}
CUTS = (1024 * TILE, 2048 * TILE)
SIZE = 2052 * TILE + 321
MAX_LINE = 990


def build(cluster, fillers, size: int = SIZE) -> bytes:
    """cluster: four lists of lines (each ends with a newline) put before and behind the first cut and before and behind the
    second; the last line of the third list is the one that lies across the second cut.  fillers: the lines repeated between."""
    assert all(ln.endswith(b"\n") and ln.count(b"\n") == 1 and len(ln) <= MAX_LINE for part in list(cluster) + [fillers] for ln in part)
    out, pos, turn = [], 0, 0

    def fill_to(target):
        nonlocal pos, turn
        assert target >= pos
        while pos + len(fillers[turn % len(fillers)]) <= target:
            out.append(fillers[turn % len(fillers)])
            pos += len(out[-1])
            turn += 1
        while pos < target:  # lines of dots up to the exact byte
            n = min(target - pos, 700)
            out.append(b"." * (n - 1) + b"\n")
            pos += n

    def put(lines):
        nonlocal pos
        out.extend(lines)
        pos += sum(len(ln) for ln in lines)

    fill_to(CUTS[0] - sum(len(ln) for ln in cluster[0]))
    put(cluster[0])
    assert pos == CUTS[0]
    put(cluster[1])
    across = cluster[2][-1]
    assert len(across) >= 4
    fill_to(CUTS[1] - sum(len(ln) for ln in cluster[2]) + len(across) // 2)
    put(cluster[2])
    put(cluster[3])
    fill_to(size)
    text = b"".join(out)
    assert len(text) == size and text[CUTS[0] - 1] == 10 and text[CUTS[1] - 1] != 10 and text[CUTS[1]] != 10 and text[-1] == 10
    return text


def distinct(text: bytes):
    """(mini, which, starts): `mini` holds each distinct line of the text once, in the order of first appearance; which[i] is
    the index in `mini` of the text's line i and starts[i] that line's offset in the text."""
    assert text.endswith(b"\n")
    lines = text.split(b"\n")[:-1]
    index, which, starts, pos = {}, [], [], 0
    for ln in lines:
        assert len(ln) < MAX_LINE
        which.append(index.setdefault(ln, len(index)))
        starts.append(pos)
        pos += len(ln) + 1
    return b"".join(ln + b"\n" for ln in index), which, starts


def expand(mini_rows, mini: bytes, which, starts, line_base: int = 0):
    """mini_rows: (line, id, to, start, len) records of a scan of `mini`, ordered by line -> the records of the whole text."""
    mini_starts, pos = [], 0
    for ln in mini.split(b"\n")[:-1]:
        mini_starts.append(pos)
        pos += len(ln) + 1
    by_line = {}
    for r in mini_rows:
        by_line.setdefault(r[0], []).append(r)
    out = []
    for i, j in enumerate(which):
        for r in by_line.get(j, ()):
            out.append((line_base + i, r[1], r[2], starts[i] + (r[3] - mini_starts[j]), r[4]) + tuple(r[5:]))
    return out
