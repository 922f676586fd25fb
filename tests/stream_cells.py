"""The stream pass's instantiations as test cells (hypergrep_amd/csrc/hg_stream.hip), an exact literal reference and the texts
that drive each cell through its paths.  Test infrastructure: imported by test_stream_variants*.py and test_stream_resources.py.

A cell is one instantiation of hg_stream_kernel / hg_stream_join_kernel, or one of the runtime variants that share an
instantiation but take another path through it, together with a deterministic literal set that the compiler maps to it.
The joiner cells reuse the literal sets of the stream cells with the same (filter, mode, fold)."""
from __future__ import annotations

import os
import random
import re
from dataclasses import dataclass

import numpy as np

STREAM_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hypergrep_amd", "csrc", "hg_stream.hip")
TILE = 16384  # HG_TILE_BYTES: one wave's tile
ROW = 1024  # one wave iteration (64 lanes x 16 bytes)
ALNUM = "abcdefghijklmnopqrstuvwxyz0123456789"
FLAGS = 6  # DOTALL | MULTILINE: no SINGLEMATCH, every occurrence is reported
FLAGS_CASELESS = 7
SPACES = " " * 8  # the case mask folds NUL onto ' ': zeros past the end of the text look like this literal
# Literals whose bytes fold onto others under | 0x20 ('@' / '`', '[' / '{', '\\' / '|', ']' / '}', '^' / '~').  Caseless
# sets carry them; the texts hold the other byte of each pair, which must not match.
LOOKALIKE_LITS = ["q`z{w|x}", "k~m`p{r|", "t}u~v`y{"]
LOOKALIKE_PAIRS = {ord("`"): ord("@"), ord("{"): ord("["), ord("|"): ord("\\"), ord("}"): ord("]"), ord("~"): ord("^")}
# Residues of the text length modulo the tile at which the partial last tile is tested.
RESIDUES = (0, 1, 15, 16, 17, 1023, 1025, 16383)


@dataclass(frozen=True)
class Cell:
    name: str
    # what the compiler must select
    log2: int
    wide: bool
    dense: int  # 0: dword windows; 1 / 2: byte-aligned probing with that step
    fold: bool  # fold_mask != 0
    joiner: bool = False
    window_bytes: int = 4
    # the literal set: `count` literals of `length` bytes over ALNUM, the first round(count * caseless) of them caseless
    count: int = 0
    length: int = 8
    caseless: float = 0.0
    seed: int = 1

    @property
    def instantiation(self) -> tuple:
        """The kernel this cell runs: ("stream", log2, wide, dense, FOLD) or ("join", log2, dense, FOLD).  Only the dword
        single-probe variants have a FOLD = false instantiation; the others fold (a no-op with a zero mask) always."""
        fold_t = self.fold if (not self.wide and self.dense == 0) else True
        if self.joiner:
            return ("join", self.log2, self.dense, fold_t)
        return ("stream", self.log2, self.wide, self.dense, fold_t)

    @property
    def modes(self) -> set:
        m = {"wide" if self.wide else ("dense%d" % self.dense if self.dense else "dword")}
        if self.fold:
            m.add("fold")
        return m


def _c(name, log2, wide, dense, fold, count, length, caseless=0.0, seed=1, window_bytes=4):
    return Cell(name, log2, wide, dense, fold, False, window_bytes, count, length, caseless, seed)


# One cell per hg_stream_kernel instantiation plus the runtime variants (counts found with hgsim_py.Db(...).selfcheck()).
STREAM_CELLS = [
    # dword-aligned windows, single-probe filter, nothing folded (FOLD = false)
    _c("dword11", 11, False, 0, False, 4, 8),
    _c("dword12", 12, False, 0, False, 250, 8),
    _c("dword13", 13, False, 0, False, 400, 8),
    _c("dword14", 14, False, 0, False, 600, 8),
    _c("dword15", 15, False, 0, False, 1500, 8),
    # ... with the text folded (more than 64 caseless literals)
    _c("dword11_fold", 11, False, 0, True, 80, 8, caseless=1.0),
    _c("dword12_fold", 12, False, 0, True, 200, 8, caseless=1.0),
    _c("dword13_fold", 13, False, 0, True, 400, 8, caseless=1.0),
    _c("dword14_fold", 14, False, 0, True, 600, 8, caseless=1.0),
    _c("dword15_fold", 15, False, 0, True, 1500, 8, caseless=1.0),
    # byte-aligned probing, a window at every byte
    _c("dense1_11", 11, False, 1, False, 600, 4),
    _c("dense1_12", 12, False, 1, False, 1000, 4),
    _c("dense1_13", 13, False, 1, False, 1500, 4),
    _c("dense1_14", 14, False, 1, False, 3000, 4),
    _c("dense1_15", 15, False, 1, False, 6000, 4),
    # ... at every second byte (all literals of at least 5 bytes)
    _c("dense2_11", 11, False, 2, False, 200, 5),
    _c("dense2_12", 12, False, 2, False, 600, 5),
    _c("dense2_13", 13, False, 2, False, 900, 5),
    _c("dense2_14", 14, False, 2, False, 1500, 5),
    _c("dense2_15", 15, False, 2, False, 3000, 5),
    # wide (two-probe) filters
    _c("wide13", 13, True, 0, False, 3000, 8),
    _c("wide14_fold", 14, True, 0, True, 6000, 8, caseless=1.0),
    _c("wide15", 15, True, 0, False, 12000, 8),
    # runtime variants: 3-byte windows; caseless literals stored in every case variant (nothing folded); byte-aligned
    # probing of a folded text
    _c("dense1_12_w3", 12, False, 1, False, 1500, 3, window_bytes=3),
    _c("dword_expand", 11, False, 0, False, 12, 8, caseless=1.0),
    _c("dense2_12_fold", 12, False, 2, True, 600, 5, caseless=0.5),
]


def _joiner(src: str) -> Cell:
    c = next(c for c in STREAM_CELLS if c.name == src)
    return Cell("join_" + src, c.log2, c.wide, c.dense, c.fold, True, c.window_bytes, c.count, c.length, c.caseless, c.seed)


# One cell per hg_stream_join_kernel instantiation: filters of 2-8 KiB, single-probe, every mode
JOIN_CELLS = [_joiner(n) for n in ("dword11", "dword12", "dword13", "dword11_fold", "dword12_fold", "dword13_fold",
                                   "dense1_11", "dense1_12", "dense1_13", "dense2_11", "dense2_12", "dense2_13")]
CELLS = STREAM_CELLS + JOIN_CELLS
BY_NAME = {c.name: c for c in CELLS}


def instantiation_of_symbol(symbol: str):
    """The cell key (Cell.instantiation) of a mangled hg_stream_kernel / hg_stream_join_kernel name; None for other kernels."""
    m = re.match(r"_Z16hg_stream_kernelILi(\d+)ELb([01])ELi(\d)ELi\d+ELb([01])E", symbol)
    if m:
        return ("stream", int(m[1]), m[2] == "1", int(m[3]), m[4] == "1")
    m = re.match(r"_Z21hg_stream_join_kernelILi(\d+)ELi(\d)ELb([01])E", symbol)
    if m:
        return ("join", int(m[1]), int(m[2]), m[3] == "1")
    return None


def residues(cell: Cell) -> tuple:
    """Partial-last-tile residues of a stream cell: four per cell, consecutive cells of the same mode take the next four, so
    that every residue meets every mode (test_residues_meet_every_mode)."""
    primary = sorted(cell.modes)[0] if len(cell.modes) == 1 else "fold"
    group = [c for c in STREAM_CELLS if (sorted(c.modes)[0] if len(c.modes) == 1 else "fold") == primary]
    k = group.index(cell)
    return tuple(RESIDUES[(4 * k + j) % len(RESIDUES)] for j in range(4))


# ------------------------------------------------------------------ literal sets
def literal_set(cell: Cell):
    """(literals as bytes, caseless flags) of the cell: distinct over ASCII case, one report id each (its index)."""
    rng = random.Random(cell.seed * 1_000_003 + cell.count * 31 + cell.length)
    ncase = round(cell.count * cell.caseless)
    seen, lits = set(), []
    while len(lits) < cell.count:
        s = "".join(rng.choice(ALNUM) for _ in range(cell.length))
        if s not in seen:
            seen.add(s)
            lits.append(s)
    caseless = [i < ncase for i in range(cell.count)]
    if cell.caseless:
        extra = LOOKALIKE_LITS + ([SPACES] if cell.fold else [])
        lits += extra
        caseless += [True] * len(extra)
    return [s.encode() for s in lits], caseless


def patterns_of(lits) -> list:
    """The literals as expressions (regex metacharacters escaped)."""
    return [re.sub(rb"([\\^$.|?*+()\[\]{}])", rb"\\\1", s).decode() for s in lits]


def flags_of(caseless) -> list:
    return [FLAGS_CASELESS if c else FLAGS for c in caseless]


# ------------------------------------------------------------------ exact reference
_UPPER_TO_LOWER = np.arange(256, dtype=np.uint8)
_UPPER_TO_LOWER[ord("A"):ord("Z") + 1] += 32


def _pack(a: np.ndarray, k: int, n: int) -> np.ndarray:
    """Little-endian uint64 keys of the first k (<= 8) bytes of every window of a that starts in [0, n)."""
    key = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        key |= a[j:j + n].astype(np.uint64) << np.uint64(8 * j)
    return key


def line_table(text: bytes):
    """(newline offsets, n_lines) of a text: a last line without a newline counts."""
    a = np.frombuffer(text, dtype=np.uint8)
    nl = np.flatnonzero(a == 10).astype(np.uint64)
    nlines = len(nl) + (1 if len(text) and text[-1:] != b"\n" else 0)
    return nl, nlines


def reference_hits(text: bytes, literals, caseless, ids) -> np.ndarray:
    """Every occurrence of every literal in a text of lines, as a sorted uint64 array [n, 5] of the oracle's tuples
    (line, id, to, line_off, line_len): 0-based line, `to` the end offset in the line, line_len with the '\\n'.
    Overlapping occurrences are all reported.  Caseless literals match an ASCII-folded copy (A-Z only).  The literals hold no
    newline and the lines are shorter than the scan buffer, so an occurrence is one in its line."""
    a = np.frombuffer(text, dtype=np.uint8)
    folded = _UPPER_TO_LOWER[a]
    n = len(a)
    rows = []
    groups = {}
    for i, (lit, cl) in enumerate(zip(literals, caseless)):
        groups.setdefault((len(lit), bool(cl)), []).append(i)
    for (length, cl), idx in groups.items():
        if length == 0 or length > n:
            continue
        hay = folded if cl else a
        lits = np.array([np.frombuffer(literals[i], dtype=np.uint8) for i in idx], dtype=np.uint8)
        if cl:
            lits = _UPPER_TO_LOWER[lits]
        k = min(length, 8)
        npos = n - length + 1
        keys = _pack(hay, k, npos)
        lkeys = np.zeros(len(idx), dtype=np.uint64)
        for j in range(k):
            lkeys |= lits[:, j].astype(np.uint64) << np.uint64(8 * j)
        order = np.argsort(lkeys, kind="stable")
        skeys = lkeys[order]
        pos = np.flatnonzero(np.isin(keys, skeys))
        if not len(pos):
            continue
        lo = np.searchsorted(skeys, keys[pos], "left")
        hi = np.searchsorted(skeys, keys[pos], "right")
        cnt = hi - lo
        rep = np.repeat(pos, cnt)
        first = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt) + np.arange(cnt.sum())
        which = order[first]
        if length > 8:  # the bytes past the key
            win = np.lib.stride_tricks.sliding_window_view(hay, length)
            ok = (win[rep, 8:] == lits[which, 8:]).all(axis=1)
            rep, which = rep[ok], which[ok]
        rows.append((rep.astype(np.uint64), np.asarray(ids, dtype=np.uint64)[np.asarray(idx)[which]], length))
    if not rows:
        return np.zeros((0, 5), dtype=np.uint64)
    nl, _ = line_table(text)
    starts = np.concatenate([[0], nl + 1]).astype(np.uint64)  # line i: [starts[i], ends[i])
    ends = np.concatenate([nl + 1, [n]]).astype(np.uint64)
    out = []
    for pos, rid, length in rows:
        line = np.searchsorted(nl, pos)  # newlines before the occurrence
        start = starts[line]
        out.append(np.stack([line.astype(np.uint64), rid, pos + np.uint64(length) - start, start, ends[line] - start], axis=1))
    return sort_hits(np.concatenate(out))


def sort_hits(h: np.ndarray) -> np.ndarray:
    h = np.asarray(h, dtype=np.uint64).reshape(-1, 5)
    return h[np.lexsort(tuple(h[:, c] for c in range(4, -1, -1)))]


# ------------------------------------------------------------------ texts
FILLER = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789 .,=-_:;/", dtype=np.uint8)


def near_misses(lit: bytes, rng: random.Random):
    """The literal with its first, middle or last byte changed: passes the windows of some part of it, must not match."""
    out = []
    for at in (0, len(lit) // 2, len(lit) - 1):
        b = bytearray(lit)
        b[at] = ord(rng.choice("!#%&*+<>?" if b[at] != ord("!") else "#"))
        out.append(bytes(b))
    return out


def case_variant(lit: bytes, rng: random.Random) -> bytes:
    return bytes(c - 32 if 97 <= c <= 122 and rng.random() < 0.5 else c for c in lit)


def cell_text(cell: Cell, lits, caseless, size: int, seed: int = 0) -> bytes:
    """A text of `size` bytes (rounded up to whole tiles) that drives the cell through the stream pass's paths: the queue
    full at every iteration, every kind of newline geometry of a tile, occurrences at every chunk offset and across every
    chunk / row / tile boundary, near misses, case variants and fold look-alikes.  No NUL; every line is shorter than 64 KiB."""
    rng = random.Random(seed * 7919 + cell.count + 100 * cell.length)
    nprng = np.random.default_rng(seed * 7919 + cell.count)
    ntiles = max(48, -(-size // TILE))
    n = ntiles * TILE
    buf = nprng.choice(FILLER, size=n)
    buf[nprng.random(n) < 1 / 70] = 10  # lines of ~70 bytes
    t = bytearray(buf.tobytes())
    real = [l for l in lits if l != SPACES.encode()]
    cased = [l for l, c in zip(lits, caseless) if c and l != SPACES.encode()]

    def put(at: int, b: bytes):
        t[at:at + len(b)] = b

    def pick():
        return rng.choice(real)

    def as_text(lit: bytes) -> bytes:  # an occurrence of the literal as a text may hold it
        return case_variant(lit, rng) if lit in cased_set else lit

    cased_set = set(cased)

    # tiles 0-7: lines of back-to-back literals, every chunk queued, every row drained
    at = 0
    while at < 8 * TILE:
        line = b"".join(as_text(pick()) for _ in range(rng.randrange(4, 200)))[: 8 * TILE - at - 1]
        put(at, line + b"\n")
        at += len(line) + 1
    # tile 8: only newlines (16384: the top of the rank field)
    put(8 * TILE, b"\n" * TILE)
    # tile 9: no newline at all, occurrences in it
    t[9 * TILE:10 * TILE] = bytes(c if c != 10 else 32 for c in t[9 * TILE:10 * TILE])
    for _ in range(40):
        put(9 * TILE + rng.randrange(0, TILE - 16), as_text(pick()))
    # tile 10: newlines at bytes 0 and 16383 only
    body = bytes(c if c != 10 else 32 for c in t[10 * TILE:11 * TILE])
    put(10 * TILE, b"\n" + body[1:-1] + b"\n")
    for _ in range(40):
        put(10 * TILE + 1 + rng.randrange(0, TILE - 18), as_text(pick()))
    # tile 11: newlines in the first rows only, none in the last row (the last newline comes from a reload)
    t[11 * TILE + 3 * ROW:12 * TILE] = bytes(c if c != 10 else 32 for c in t[11 * TILE + 3 * ROW:12 * TILE])
    for _ in range(40):
        put(11 * TILE + rng.randrange(0, TILE - 16), as_text(pick()))
    # tile 12: a newline in the last row at the last chunk's first byte, none after
    put(12 * TILE + TILE - 16, b"\n" + bytes(c if c != 10 else 32 for c in t[12 * TILE + TILE - 15:13 * TILE]))
    # tiles 13-15: short lines, most chunks with several newlines (the wave scan of the newline prefix)
    at = 13 * TILE
    while at < 16 * TILE - 32:
        r = rng.random()
        line = as_text(pick()) if r < 0.15 else bytes(rng.choice(b"xyz.,") for _ in range(rng.randrange(0, 6)))
        line = line[: 16 * TILE - at - 1]
        put(at, line + b"\n")
        at += len(line) + 1
    # tiles 16-23: an occurrence starting at every offset 0-31 of a 32-byte pair of chunks, for many literals
    at, off = 16 * TILE, 0
    while at < 24 * TILE - 64:
        lit = as_text(pick())
        p = at - at % 32 + off
        put(p, lit)
        if rng.random() < 0.3:
            put(p + len(lit) + rng.randrange(1, 8), b"\n")
        at = p + len(lit) + 3
        off = (off + 1) % 32
    # tiles 24-31: near misses of every literal (the first level passes, the second level or the verify must not), case
    # variants and fold look-alikes
    at, end = 24 * TILE, 32 * TILE
    for lit in real:
        if at >= end - 64:
            break
        for miss in near_misses(lit, rng) + ([case_variant(lit, rng)] if lit in cased_set else []):
            put(at, miss + b" ")
            at += len(miss) + 1
        if rng.random() < 0.2:
            put(at, b"\n")
            at += 1
    if cased:
        for lit in LOOKALIKE_LITS:
            lit = lit.encode()
            for j, c in enumerate(lit):
                if c in LOOKALIKE_PAIRS and at < end - 64:
                    b = bytearray(lit)
                    b[j] = LOOKALIKE_PAIRS[c]
                    put(at, bytes(b) + b" " + case_variant(lit, rng) + b"\n")
                    at += 2 * len(lit) + 2
    # the rest: occurrences across every chunk / row / tile boundary from tile 32 on, sprinkled occurrences and near misses
    for tile in range(32, ntiles):
        base = tile * TILE
        for bound, step in ((TILE, TILE), (ROW, ROW * 3), (16, 16 * 37)):
            for edge in range(base + (bound if bound < TILE else 0), base + TILE, step):
                lit = as_text(pick())
                put(edge - rng.randrange(1, len(lit)), lit)
        for _ in range(8):
            lit = pick()
            put(base + rng.randrange(0, TILE - 16), rng.choice([as_text(lit)] + near_misses(lit, rng)))
    t = bytes(t)
    assert b"\x00" not in t
    return t


def truncated(text: bytes, lits, nbytes: int, rng: random.Random) -> bytes:
    """The text's first nbytes with an occurrence of a literal ending at its last byte (where there is room for one)."""
    t = bytearray(text[:nbytes])
    real = [l for l in lits if l != SPACES.encode()]
    lit = rng.choice(real)
    if nbytes >= len(lit):
        t[nbytes - len(lit):] = lit
    return bytes(t)
