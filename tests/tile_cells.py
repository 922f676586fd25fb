"""Cells for the tile scan (hg_tile_reduce / spine / apply / inner_kernel) and an exact reference for them.

The tile scan turns the stream pass's per-tile newline summaries into the state at every tile's start: where the line that
is open there began, and the number of the piece that begins there.  Every report's (line number, start, length) is that
state plus arithmetic inside the tile, so the state of a tile is seen from outside by a report in the tile's carry-in line
(its state alone) and by reports behind its first and its last newline (its state plus the tile's own summary).

A cell is a geometry (newline positions chosen by hand, filler elsewhere), a size, a scan buffer, the scanner's environment
and a line base.  Markers (one literal, all-matches, so every occurrence reports) are planted at each tile's start, behind
its first newline and behind its last one.  tags() reads the classes a cell covers off its geometry; the tests assert that
every class the suite is written for occurs (tests/test_tile_cells.py) instead of hoping for it.

reference(): numpy over the newline positions alone, by the definition of a piece: a line is cut into
pieces of at most bs1 = buffer_size - 1 bytes, pieces are numbered from line_base, a marker reports on the piece that holds
it whole.  No tiles, nothing of hg_post.h.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

TILE = 16384
BLOCK = 1024          # tiles of a tile-scan block: 256 threads x 4
MARKER = b"TqMark7Z"  # not in the filler, no overlap with itself
MARKER_ID = 7
FLAGS = 6             # DOTALL | MULTILINE: every occurrence reports
M = len(MARKER)
DEFAULT_BS = 262140


# ---------------------------------------------------------------------------------------------------- the reference
@dataclass
class Pieces:
    starts: np.ndarray  # line starts
    lens: np.ndarray    # line lengths (the newline included)
    first: np.ndarray   # number of the line's first piece, from 0
    total: int
    bs1: int


def pieces(nl: np.ndarray, nbytes: int, bs1: int) -> Pieces:
    nl = nl[nl < nbytes]
    starts = np.concatenate([[0], nl + 1]).astype(np.int64)
    if nbytes == 0 or starts[-1] == nbytes:
        starts = starts[:-1]
    lens = np.diff(np.concatenate([starts, [nbytes]]))
    per = -(-lens // bs1)
    first = np.cumsum(per) - per
    return Pieces(starts, lens, first, int(per.sum()), bs1)


def reference(nl: np.ndarray, nbytes: int, bs1: int, line_base: int, markers: np.ndarray):
    """(rows, n_lines): rows[i] = (line_no, id, to, start, len) of the markers that report, in text order (one id: the order of
    delivery); a marker that a forced break or the text's end cuts reports nowhere."""
    p = pieces(nl, nbytes, bs1)
    x = np.sort(markers[markers < nbytes]).astype(np.int64)
    i = np.searchsorted(p.starts, x, side="right") - 1
    k = (x - p.starts[i]) // bs1
    ps = p.starts[i] + k * bs1
    plen = np.minimum(bs1, p.lens[i] - k * bs1)
    ok = x + M <= ps + plen
    rows = np.stack([line_base + p.first[i] + k, np.full(len(x), MARKER_ID), x + M - ps, ps, plen], axis=1)[ok]
    return rows.astype(np.uint64), p.total


def tile_states(nl: np.ndarray, nbytes: int, bs1: int, line_base: int):
    """(cs, L) at every tile's start, by the same definition: the line open there (the one that begins there, if one does) and
    the number of its first piece."""
    p = pieces(nl, nbytes, bs1)
    t0 = np.arange((nbytes + TILE - 1) // TILE, dtype=np.int64) * TILE
    i = np.searchsorted(p.starts, t0, side="right") - 1
    return p.starts[i], line_base + p.first[i]


def summaries(nl: np.ndarray, nbytes: int, bs1: int):
    """The tile summaries (nl_count, first_nl, last_nl, inner) of a text, as the stream pass and hg_tile_inner_kernel leave them,
    worked out from the newline positions and the piece table."""
    nl = nl[nl < nbytes].astype(np.int64)
    ntiles = (nbytes + TILE - 1) // TILE
    out = np.zeros((ntiles, 4), dtype=np.uint32)
    out[:, 1:3] = 0xFFFFFFFF
    if len(nl):
        t = nl // TILE
        lo = np.searchsorted(t, np.arange(ntiles), side="left")
        hi = np.searchsorted(t, np.arange(ntiles), side="right")
        has = hi > lo
        out[:, 0] = hi - lo
        out[has, 1] = (nl[lo[has]] % TILE).astype(np.uint32)
        out[has, 2] = (nl[hi[has] - 1] % TILE).astype(np.uint32)
        # the whole lines between the tile's first and last newline: lines lo + 1 .. hi - 1 (line j ends with newline j)
        p = pieces(nl, nbytes, bs1)
        per = -(-p.lens // bs1)
        cum = np.concatenate([[0], np.cumsum(per)])
        out[has, 3] = (cum[hi[has]] - cum[lo[has] + 1]).astype(np.uint32)
    return out


# ---------------------------------------------------------------------------------------------------------- texts
class Geo:
    """Newline positions of a text, chosen stretch by stretch; everything else is filler."""

    def __init__(self, ntiles: int, extra: int = 0):
        self.size = ntiles * TILE + extra
        self.nl = []

    def at(self, *pos):
        self.nl += [p for p in pos if 0 <= p < self.size]
        return self

    def tile(self, t: int, *offsets):
        return self.at(*[t * TILE + o for o in offsets])

    def lines(self, a: int, b: int, lens):
        """Lines of the cycled lengths `lens` from byte a on: a newline ends each, none at or behind b."""
        pos, i = a, 0
        while True:
            pos += lens[i % len(lens)]
            if pos > b:
                return self
            self.nl.append(pos - 1)
            i += 1

    def array(self) -> np.ndarray:
        out = np.unique(np.array(self.nl, dtype=np.int64))
        return out[out < self.size]


def busy(g: Geo, t0: int, t1: int):
    """Tiles [t0, t1) of everyday text: by turns many newlines, one on the tile's first byte, one on its last, two, and one on
    the last byte followed by one on the next tile's first (an empty line across the edge)."""
    for t in range(t0, t1):
        kind = t % 5
        if kind == 0:
            g.lines(t * TILE + 3, (t + 1) * TILE, [70, 1, 211, 38, 1900, 9])
        elif kind == 1:
            g.tile(t, 0)
        elif kind == 2:
            g.tile(t, TILE - 1)
        elif kind == 3:
            g.tile(t, 5000, 5100)
        else:
            g.tile(t, 0, TILE - 1)
    return g


def _edges():
    """2050 tiles (the prefixes of every size are cut from it).  Runs of tiles without a newline: 1 (tile 9, off a thread's
    first tile), 3 (12-14, from a thread's first tile), 4 (17-20), 5 (24-28, from a thread's first); a line of 5 tiles + 7
    bytes (from inside tile 31); a newline on the last byte before tile 1024 and one on its first byte; a run of 1020 from
    tile 1026, a line across tile 2048."""
    g = Geo(2050)
    busy(g, 0, 9)
    g.tile(10, 100).tile(11, 16383)
    g.tile(15, 0, 7000).tile(16, 9)
    busy(g, 21, 24)
    g.tile(29, 40).tile(30, 16000)
    x = 31 * TILE + 1234
    g.at(x, x + 5 * TILE + 7)   # the line behind x: 5 tiles + 7 bytes; tiles 32-35 without a newline
    busy(g, 37, 1023)
    g.tile(1023, 300, TILE - 1).tile(1024, 0, 77).tile(1025, 16383)
    g.tile(2046, 5, 600, 601, 9000)  # tiles 1026-2045 without one; the line behind 2046:9000 crosses tile 2048
    g.tile(2049, 100, 16000)
    return g


def _blocks():
    """3100 tiles.  A run of 1023 tiles without a newline from tile 4 (a thread's first tile; across the edge of block 0), one
    newline per tile alternating between its first and its last byte up to tile 2047, a line of exactly 1025 tiles from tile
    2048 (a block's first tile: block 2 whole, and beyond it) and everyday text to the end."""
    g = Geo(3100)
    busy(g, 0, 4)
    for t in range(1027, 2047):
        g.tile(t, 0 if t % 2 else TILE - 1)
    g.tile(2047, TILE - 1).tile(3072, TILE - 1)
    busy(g, 3073, 3100)
    return g


def _hole():
    """2100 tiles, three pipeline chunks of 1024 tiles: the middle one (tiles 1024-2047, a whole block) holds no newline, nor does
    tile 2048 (a run of 1025 from a block's first tile), so one line crosses both cuts.  Before it one newline a tile on its first byte, behind it on its last."""
    g = Geo(2100, 77)
    for t in range(0, 1024):
        g.tile(t, 0)
    for t in range(2049, 2100):
        g.tile(t, TILE - 1)
    return g


def _none():
    return Geo(1025, 1)


def _only_last():
    g = Geo(1025, 1)
    return g.at(g.size - 1)


def _only_first():
    return Geo(1025, 1).at(0)


def _small(bs1: int):
    """9 tiles for a scan buffer below a tile: tiles with many, no, one and two newlines; lines of exactly bs1, bs1 + 1 and
    2 * bs1 bytes between two newlines of one tile (tile 3; at 16383 only the first fits) and the same three across a tile's
    edge (tiles 4-7); two newlines in tile 8."""
    def make():
        g = Geo(9, 1)
        g.lines(0, TILE, [bs1, 1, bs1 + 1, 3 * bs1 + 2, 5, 2 * bs1])   # tile 0: many
        g.tile(2, 4000)                                                # tile 1 none, tile 2 one
        if 4 * bs1 + 8 <= TILE:
            a = 3 * TILE + 3
            g.at(a - 1, a + bs1 - 1, a + 2 * bs1, a + 4 * bs1)         # tile 3: lines of bs1, bs1 + 1 and 2 * bs1 bytes inside it
        else:
            g.tile(3, 0, TILE - 1)                                     # (16383: the line of bs1 bytes fills the tile between its two newlines)
        for t, n in ((4, bs1), (5, bs1 + 1), (6, 2 * bs1)):            # across the edge between tiles t and t + 1
            a = (t + 1) * TILE - min(n, TILE) // 2
            g.at(a - 1, a + n - 1)
        g.tile(8, 12000, 12007)                                        # two
        return g
    make.__name__ = f"_small_{bs1}"
    return make


@functools.lru_cache(maxsize=None)
def geometry(fn):
    g = fn()
    return g.array(), g.size


def next_newline(nl: np.ndarray, y: np.ndarray, size: int) -> np.ndarray:
    """The first newline at or behind each y (size: none)."""
    return np.concatenate([nl, [size]])[np.searchsorted(nl, y, side="left")]


def marker_sites(nl: np.ndarray, size: int, bs1s) -> np.ndarray:
    """Where the markers stand: at each tile's start (the carry-in line), behind its first newline and behind its last.  A
    site moves forward, up to 64 bytes, off a newline and off a forced break of every scan buffer in `bs1s`, staying in its
    line; if none of the 64 places is free the marker stands where it is and the reference says what it reports."""
    ntiles = (size + TILE - 1) // TILE
    t = nl // TILE
    lo = np.searchsorted(t, np.arange(ntiles), side="left")
    hi = np.searchsorted(t, np.arange(ntiles), side="right")
    want = [np.arange(ntiles, dtype=np.int64) * TILE, nl[lo[hi > lo]] + 1, nl[hi[hi > lo] - 1] + 1]
    x = np.unique(np.concatenate(want))
    x = x[x + M <= size]
    starts = np.concatenate([[0], nl + 1])
    chosen = np.full(len(x), -1, dtype=np.int64)
    for shift in range(64):
        y = x + shift
        free = next_newline(nl, y, size) >= y + M
        free &= np.searchsorted(nl, x, side="left") == np.searchsorted(nl, y, side="left")  # still the same line
        s = starts[np.searchsorted(starts, y, side="right") - 1]
        for bs1 in bs1s:
            free &= (y - s) % bs1 + M <= bs1
        take = free & (chosen < 0)
        chosen[take] = y[take]
    chosen[chosen < 0] = x[chosen < 0]
    # none holds a newline; no two markers overlap
    chosen = np.unique(chosen)
    chosen = chosen[(next_newline(nl, chosen, size) >= chosen + M) & (chosen + M <= size)]
    keep = np.concatenate([[True], np.diff(chosen) >= M])
    while not keep.all():
        chosen = chosen[keep]
        keep = np.concatenate([[True], np.diff(chosen) >= M])
    return chosen


def straddlers(nl: np.ndarray, size: int, bs1: int, count: int = 3) -> np.ndarray:
    """Markers put ACROSS the first forced breaks of the text's long lines on purpose: they report nowhere."""
    p = pieces(nl, size, bs1)
    return (p.starts[p.lens > bs1 + M][:count] + bs1 - 3).astype(np.int64)


@dataclass(frozen=True)
class TextKey:
    geo: object
    bs1s: tuple       # the scan buffers the markers keep off
    straddle: int = 0  # a scan buffer whose first forced breaks get a marker across them (0: none)


@functools.lru_cache(maxsize=None)
def text_markers(key: TextKey) -> np.ndarray:
    nl, size = geometry(key.geo)
    x = marker_sites(nl, size, key.bs1s)
    if key.straddle:
        extra = straddlers(nl, size, key.straddle)
        x = np.unique(np.concatenate([x[np.all(np.abs(x[:, None] - extra[None, :]) >= M, axis=1)], extra]))
    return x


def text_array(key: TextKey) -> np.ndarray:
    """The text's bytes (numpy uint8)."""
    nl, size = geometry(key.geo)
    buf = np.full(size, ord("."), dtype=np.uint8)
    buf[nl] = 10
    x = text_markers(key)
    for j, c in enumerate(MARKER):
        buf[x + j] = c
    return buf


# ---------------------------------------------------------------------------------------------------------- cells
@dataclass
class Cell:
    name: str
    key: TextKey
    nbytes: int
    buffer_size: int = DEFAULT_BS
    env: dict = field(default_factory=dict)
    line_base: int = 0
    claim: dict = field(default_factory=dict)  # stream_launches_min / stream_launches: asserted on the GPU

    @property
    def bs1(self):
        return self.buffer_size - 1


def cell_reference(cell: Cell):
    nl, _ = geometry(cell.key.geo)
    return reference(nl, cell.nbytes, cell.bs1, cell.line_base, text_markers(cell.key))


def chunk_cuts(cell: Cell):
    """Tile ranges of the scan's tile-scan launches as the engine's plan gives them: pipeline chunks of HG_CHUNK_TILES (whole
    blocks, honoured from 1024 upward) for a whole-buffer pass."""
    ntiles = (cell.nbytes + TILE - 1) // TILE
    v = int(cell.env.get("HG_CHUNK_TILES", 0))
    step = v // BLOCK * BLOCK if v >= BLOCK else max(ntiles, 1)
    return [(a, min(a + step, ntiles)) for a in range(0, ntiles, step)]


def segment_ranges(cell: Cell, nsegments: int):
    """(tile_lo, tile_hi, own_hi tile) of the passes of a segmented scan (HgScanner::scan_segments)."""
    ntiles = (cell.nbytes + TILE - 1) // TILE
    reach = (cell.bs1 >> 14) + 2
    seg = ((ntiles + nsegments - 1) // nsegments + 15) // 16 * 16
    out = []
    for lo in range(0, ntiles, seg):
        last = lo + seg >= ntiles
        out.append((lo, ntiles if last else min(ntiles, lo + seg + reach), ntiles if last else lo + seg))
    return out


def raw_reports(cell: Cell, lo_tile: int, hi_tile: int) -> int:
    """Raw reports of the pieces that begin in tiles [lo_tile, hi_tile): the all-matches expression runs over the whole piece
    once per occurrence, so a piece with k markers yields k * k (tests/finalize_cells.py states the same rule)."""
    rows, _ = cell_reference(cell)
    own = rows[(rows[:, 3] >= lo_tile * TILE) & (rows[:, 3] < hi_tile * TILE)]
    _, counts = np.unique(own[:, 3], return_counts=True)
    return int((counts.astype(np.int64) ** 2).sum())


def planned_segments(cell: Cell) -> int:
    """In how many segments the engine scans the cell under its HG_HIT_LIMIT: 1, or the first power of two at which no
    segment's raw reports pass the limit."""
    limit = max(1024, int(cell.env.get("HG_HIT_LIMIT", 1 << 28)))
    ntiles = (cell.nbytes + TILE - 1) // TILE
    if raw_reports(cell, 0, ntiles) <= limit:
        return 1
    n = 2
    while any(raw_reports(cell, lo, own_hi) > limit for lo, _, own_hi in segment_ranges(cell, n)):
        n *= 2
    return n


def tags(cell: Cell) -> set:
    """The classes of the issue's list that this cell covers, read off its geometry."""
    nl, _ = geometry(cell.key.geo)
    nl = nl[nl < cell.nbytes]
    n, bs1 = cell.nbytes, cell.bs1
    ntiles = (n + TILE - 1) // TILE
    out = {f"tiles-{n // TILE}" if n % TILE == 0 else f"tiles-{n // TILE}+{n % TILE}"}
    s = summaries(nl, n, bs1)
    empty = s[:, 0] == 0
    # runs of tiles without a newline
    edge = np.flatnonzero(np.diff(np.concatenate([[0], empty.astype(np.int8), [0]])))
    for a, b in zip(edge[::2], edge[1::2]):
        out.add(f"run-{b - a}")
        out.add("run-from-thread-first" if a % 4 == 0 else "run-off-thread-first")
        if a % BLOCK == 0:
            out.add("run-from-block-first")
        if a // BLOCK != (b - 1) // BLOCK:
            out.add("run-across-block-edge")
        if any(a <= k * BLOCK and (k + 1) * BLOCK <= b for k in range(ntiles // BLOCK + 1)):
            out.add("block-without-newline")
    if len(nl) == 0:
        out.add("no-newline")
    if len(nl) == 1 and nl[0] == n - 1:
        out.add("only-newline-last-byte")
    if len(nl) == 1 and nl[0] == 0:
        out.add("only-newline-first-byte")
    one = s[:, 0] == 1
    at0, at_end = one & (s[:, 1] == 0), one & (s[:, 1] == TILE - 1)
    if at0.any():
        out.add("one-newline-byte-0")
    if at_end.any():
        out.add("one-newline-byte-16383")
    if (at0[:-1] & at_end[1:]).any() and (at_end[:-1] & at0[1:]).any():
        out.add("one-newline-alternating")
    p = pieces(nl, n, bs1)
    if bs1 >= TILE:
        out.add(f"bs1-{bs1}")
        if (p.lens > bs1).any():
            out.add("forced-break")
            if (p.lens == 5 * TILE + 7).any():
                out.add("forced-break-line-5-tiles-7")
            if (p.lens == 1025 * TILE).any():
                out.add("forced-break-line-1025-tiles")
            # a piece that begins inside a tile without a newline
            long = np.flatnonzero(p.lens > bs1)
            for i in long[:50]:
                ks = np.arange(1, min(-(-int(p.lens[i]) // bs1), 70))
                if empty[(p.starts[i] + ks * bs1) // TILE].any():
                    out.add("piece-begins-in-newline-free-tile")
    else:
        out.add(f"small-bs1-{bs1}")
        for c, name in ((0, "0"), (1, "1"), (2, "2")):
            if (s[:, 0] == c).any():
                out.add(f"small-tile-{name}-newlines")
        if (s[:, 0] > 8).any():
            out.add("small-tile-many-newlines")
        if (s[:, 0] >= 2).any() and (s[s[:, 0] >= 2, 3] != s[s[:, 0] >= 2, 0] - 1).any():
            out.add("small-inner-split")
        t_first, t_last = p.starts // TILE, (p.starts + p.lens - 1) // TILE
        # "inside one tile": between two newlines of that tile (what hg_tile_inner_kernel prices)
        prev_in_tile = (p.starts > 0) & ((p.starts - 1) // TILE == t_first)
        for length, name in ((bs1, "bs1"), (bs1 + 1, "bs1+1"), (2 * bs1, "2bs1")):
            hit = p.lens == length
            if (hit & (t_first == t_last) & prev_in_tile).any():
                out.add(f"small-line-{name}-inside-tile")
            if (hit & (t_first != t_last)).any():
                out.add(f"small-line-{name}-across-edge")
    cuts = chunk_cuts(cell)
    if len(cuts) >= 3:
        out.add("chunks-3")
        starts_set = set(p.starts.tolist())
        nlset = nl
        for a, _ in cuts[1:]:
            cut = a * TILE
            if cut not in starts_set:
                out.add("chunk-line-across-cut")
            if np.isin(cut - 1, nlset):
                out.add("chunk-newline-before-cut")
            if np.isin(cut, nlset):
                out.add("chunk-newline-behind-cut")
        if any(empty[a:b].all() for a, b in cuts[1:-1]):
            out.add("chunk-middle-without-newline")
        if cell.env.get("HG_JOINER") == "0":
            out.add("chunks-no-joiner")
        if "HG_NO_EARLY_FINALIZE" in cell.env:
            out.add("chunks-no-early-finalize")
    if "HG_HIT_LIMIT" in cell.env:
        k = planned_segments(cell)
        out.add(f"segments-{k}")
        if k > 1:
            starts_set = set(p.starts.tolist())
            for lo, _, _ in segment_ranges(cell, k)[1:]:
                if lo % BLOCK:
                    out.add("segment-start-off-block")
                if lo * TILE not in starts_set and (p.lens[np.searchsorted(p.starts, lo * TILE, side="right") - 1] > 4 * TILE):
                    out.add("segment-long-line-across-start")
    if cell.line_base:
        out.add(f"line-base-{cell.line_base}")
    rows, _ = cell_reference(cell)
    if len(rows) < len(text_markers(cell.key)[text_markers(cell.key) + M <= n]):
        out.add("marker-across-forced-break")
    return out


SIZES = (1, 2, 3, 4, 5, 8, 9, 1023, 1024, 1025, 2047, 2048, 2049)
BIG_BS1 = (16384, 16385, 40000, DEFAULT_BS - 1)
EDGES = TextKey(_edges, BIG_BS1)
EDGES_SMALL = {b: TextKey(_edges, (b,)) for b in (16383, 1000, 8)}
BLOCKS = TextKey(_blocks, BIG_BS1)
HOLE = TextKey(_hole, BIG_BS1)
CHUNK3 = {"HG_CHUNK_TILES": "1024"}

REQUIRED = (
    {f"tiles-{k}" for k in SIZES} | {f"tiles-{k}+1" for k in SIZES} | {f"tiles-{k}+16383" for k in SIZES}
    | {f"run-{k}" for k in (1, 3, 4, 5, 1020, 1023, 1024, 1025)}
    | {"run-from-thread-first", "run-off-thread-first", "run-from-block-first", "run-across-block-edge", "block-without-newline", "no-newline", "only-newline-last-byte",
       "only-newline-first-byte", "one-newline-byte-0", "one-newline-byte-16383", "one-newline-alternating"}
    | {"bs1-16384", "bs1-16385", "bs1-40000", "forced-break", "forced-break-line-5-tiles-7", "forced-break-line-1025-tiles", "piece-begins-in-newline-free-tile",
       "marker-across-forced-break"}
    | {f"small-bs1-{b}" for b in (16383, 1000, 8)} | {f"small-tile-{k}-newlines" for k in ("0", "1", "2", "many")} | {"small-inner-split"}
    | {f"small-line-{n}-{w}" for n in ("bs1", "bs1+1", "2bs1") for w in ("inside-tile", "across-edge")}
    | {"chunks-3", "chunk-line-across-cut", "chunk-newline-before-cut", "chunk-newline-behind-cut", "chunk-middle-without-newline", "chunks-no-joiner", "chunks-no-early-finalize"}
    | {"segments-2", "segments-4", "segment-start-off-block", "segment-long-line-across-start", f"line-base-{2**33 + 5}"}
)
# Classes of the list that no text can hold, and why:
#  * a line of bs1 + 1 or of 2 * bs1 bytes between two newlines of ONE tile, at bs1 = 16383: it would be 16384 or 32766 bytes
#    between two newlines that lie at most 16383 bytes apart.  The classes occur at bs1 = 1000 and 8.
#  * a segment start that is no multiple of 4 tiles: HgScanner::scan_segments aligns segments to 16 tiles.  What a segment start
#    can be is off a block's first tile (every thread's group of four then covers other tiles than in the whole-buffer pass);
#    ranges that begin on tiles 1, 2, 3 and 5 run in the host replay (tests/native/tilesim.cpp).


def cells():
    out = []
    size_of = lambda fn: geometry(fn)[1]
    for k in SIZES:  # the sizes, each also with a ragged last tile
        for extra in (0, 1, 16383):
            out.append(Cell(f"size-{k}" + (f"+{extra}" if extra else ""), EDGES, k * TILE + extra))
    # forced breaks at and above a tile
    for bs1 in (16384, 16385, 40000):
        out.append(Cell(f"breaks-edges-{bs1}", TextKey(_edges, BIG_BS1, straddle=bs1), size_of(_edges), buffer_size=bs1 + 1))
        out.append(Cell(f"breaks-blocks-{bs1}", TextKey(_blocks, BIG_BS1, straddle=bs1), size_of(_blocks), buffer_size=bs1 + 1))
    out.append(Cell("blocks-default", BLOCKS, size_of(_blocks)))
    out.append(Cell("hole-default", HOLE, size_of(_hole)))
    for fn in (_none, _only_last, _only_first):
        out.append(Cell(fn.__name__.strip("_").replace("_", "-"), TextKey(fn, BIG_BS1), size_of(fn)))
        out.append(Cell(fn.__name__.strip("_").replace("_", "-") + "-16384", TextKey(fn, BIG_BS1), size_of(fn), buffer_size=16385))
    # small-buffer mode
    for bs1 in (16383, 1000, 8):
        small = _small_fn(bs1)
        out.append(Cell(f"small-lines-{bs1}", TextKey(small, (bs1,)), size_of(small), buffer_size=bs1 + 1))
        out.append(Cell(f"small-edges-9-{bs1}", EDGES_SMALL[bs1], 9 * TILE + 1, buffer_size=bs1 + 1))
    for bs1 in (16383, 1000):
        out.append(Cell(f"small-edges-1025-{bs1}", EDGES_SMALL[bs1], 1025 * TILE + 16383, buffer_size=bs1 + 1))
    # chunk chaining: three chunks of the pipeline, the state handed on through *state
    for tag, env in (("", {}), ("-nojoiner", {"HG_JOINER": "0"}), ("-noearly", {"HG_NO_EARLY_FINALIZE": "1"})):
        out.append(Cell(f"chunks-edges{tag}", EDGES, size_of(_edges), env={**CHUNK3, **env}, claim={"stream_launches_min": 3}))
        out.append(Cell(f"chunks-hole{tag}", HOLE, size_of(_hole), env={**CHUNK3, **env}, claim={"stream_launches_min": 3}))
    out.append(Cell("chunks-blocks-16385", BLOCKS, size_of(_blocks), buffer_size=16386, env=CHUNK3, claim={"stream_launches_min": 3}))
    out.append(Cell("chunks-edges-small-1000", EDGES_SMALL[1000], size_of(_edges), buffer_size=1001, env=CHUNK3, claim={"stream_launches_min": 3}))
    # segmented scans: a segment's first tile takes its state from the pass before it
    for limit in SEGMENT_LIMITS:
        out.append(Cell(f"segments-limit-{limit}", EDGES, size_of(_edges), env={"HG_HIT_LIMIT": str(limit)}))
    out.append(Cell("line-base", EDGES, 1025 * TILE + 1, line_base=2**33 + 5))
    out.append(Cell("line-base-breaks", TextKey(_blocks, BIG_BS1), size_of(_blocks), buffer_size=40001, line_base=2**33 + 5))
    assert len({c.name for c in out}) == len(out)
    return out


_SMALL_FNS = {}


def _small_fn(bs1):
    if bs1 not in _SMALL_FNS:
        _SMALL_FNS[bs1] = _small(bs1)
    return _SMALL_FNS[bs1]


# HG_HIT_LIMIT values under which the 2050-tile text scans in two and in four segments: test_tile_cells.py asserts that
# planned_segments() says so, the GPU test that the scan made as many stream launches.
SEGMENT_LIMITS = (17000, 9000)

CELLS = cells()


# ------------------------------------------------------------------------------------------------ the large cell
BIG_TILES = (4 << 30) // TILE + (16 << 20) // TILE + 5  # 258 tile-scan blocks: two rounds of the spine
BIG_BYTES = BIG_TILES * TILE + 123
BIG_LINE = 1 << 20


def big_geometry(seed: int = 20):
    """Newline positions of the large cell: lines of about 1 MiB (the default scan buffer forces breaks in every one), and
    around the first tiles of blocks 0, 1, 255, 256, 257 and a few hundred seeded random tiles short lines as well."""
    rng = np.random.default_rng(seed)
    base = np.arange(BIG_LINE + 1000, BIG_BYTES, BIG_LINE + 4099, dtype=np.int64)  # (a step that is no multiple of a tile)
    base = base + rng.integers(-40000, 40000, size=len(base))
    tiles = np.concatenate([[0, 1, 2, 3], np.array([1, 255, 256, 257])[:, None].repeat(4, 1).ravel() * BLOCK + np.tile([-2, -1, 0, 1], 4),
                            [BIG_TILES - 2, BIG_TILES - 1], rng.integers(0, BIG_TILES, size=600)])
    local = []
    for t in np.unique(tiles):
        kind = int(t) % 4
        offs = [[0], [TILE - 1], [17, 9000], [0, 5, 300, 8000, TILE - 1]][kind]
        local += [int(t) * TILE + o for o in offs]
    nl = np.unique(np.concatenate([base, np.array(local, dtype=np.int64)]))
    return nl[(nl >= 0) & (nl < BIG_BYTES)], np.unique(tiles)


def big_markers(nl: np.ndarray, tiles: np.ndarray) -> np.ndarray:
    """Markers at the chosen tiles' starts, behind their first and last newline, and behind every second line's start."""
    t = nl // TILE
    lo, hi = np.searchsorted(t, tiles, side="left"), np.searchsorted(t, tiles, side="right")
    has = hi > lo
    x = np.concatenate([tiles * TILE, (tiles + 1) * TILE, nl[lo[has]] + 1, nl[hi[has] - 1] + 1, nl[::2] + 1 + 300000])
    x = np.unique(x[(x >= 0) & (x + M <= BIG_BYTES)])
    x = x[np.concatenate([[True], np.diff(x) >= M])]
    return x[next_newline(nl, x, BIG_BYTES) >= x + M]
