"""Cells for the finalize stage (hg_fin_* and the compact finalize) and an exact reference for them.

The finalize orders a pass's raw reports by (line, id, to), applies the SINGLEMATCH and duplicate rules and compacts the
result.  Which of its paths runs depends on how many raw reports land in a bucket (one wave up to 64, a block in LDS up to
512, a block in a scratch area up to 4096, the compact array beyond), on the width of the sort key and on the pipeline.  A
cell is a text, a set of LITERAL expressions, a buffer size, the environment of its scanner, and the geometry it claims; the
tests assert the claim (tests/test_finalize_cells.py from the model below, tests/test_finalize_cells_gpu.py from
Scanner.finalize_info()) instead of hoping for it.

reference(): plain Python.  Overlapping occurrences by bytes.find per piece of a line, then the three report rules of
hg_post.h: SINGLEMATCH expressions that share an id yield the smallest end per (line, id); other expressions every
distinct end; identical (id, to) reports are delivered once.  Its output is the ordered list (line, id, to, start, len), per
record the expression indices that may stand in hg_hit_aux_t.pattern, and per line the raw reports.

Raw reports.  A SINGLEMATCH literal yields one raw report per occurrence.  An all-matches expression is run over the whole
piece once per verified occurrence (hg_confirm), so k occurrences on a piece yield k * k raw reports: every end k times.
reference() states this in its `raw` lists; the GPU test compares its per-bucket counts with the fill levels the device reports, so the model
itself is under test.  The texts keep every literal free of overlaps with itself.
"""
from __future__ import annotations

import bisect
import functools
import itertools
import random
from collections import Counter, namedtuple
from dataclasses import dataclass, field

Expr = namedtuple("Expr", "lit id single")  # a literal expression: its bytes, report id, HS_FLAG_SINGLEMATCH

FLAG_SINGLE, FLAG_MULTI, FLAG_SOM = 14, 6, 256  # DOTALL | MULTILINE (| SINGLEMATCH); HS_FLAG_SOM_LEFTMOST
TILE = 16384
HIT_CAP0 = 1 << 16  # hit records of a fresh scanner for texts of up to 64 MiB (HgScanner::ensure)
MAX_BUCKETS = 1 << 22


def flags_of(exprs, som=False):
    return [FLAG_SINGLE if e.single else FLAG_MULTI | (FLAG_SOM if som else 0) for e in exprs]


# ---------------------------------------------------------------------------------------------------- the reference
def split_pieces(text: bytes, buffer_size: int):
    """(starts, lengths) of the line pieces: at most buffer_size - 1 bytes, ending after a newline (the oracle's splitter)."""
    bs1 = buffer_size - 1
    starts, lens = [], []
    pos, n = 0, len(text)
    while pos < n:
        limit = min(pos + bs1, n)
        nl = text.find(b"\n", pos, limit)
        end = nl + 1 if nl >= 0 else limit
        starts.append(pos)
        lens.append(end - pos)
        pos = end
    return starts, lens


Scan = namedtuple("Scan", "records admissible raw_ref raw starts lens")


def reference(text: bytes, exprs, buffer_size: int = 262140, line_base: int = 0) -> Scan:
    """records: [(line, id, to, start, len)] in delivery order; admissible: per record the expression indices hg_hit_aux_t.pattern
    may hold; raw_ref: {piece: occurrences over all expressions}; raw: {piece: [(id, to, single, expression)]}, the raw reports
    of the product (see the module text); starts / lens: the pieces."""
    assert b"\0" not in text, "the cells' texts hold no NUL byte"
    starts, lens = split_pieces(text, buffer_size)
    occ = {}
    for j, e in enumerate(exprs):
        pos = text.find(e.lit)
        while pos >= 0:
            k = bisect.bisect_right(starts, pos) - 1
            if pos + len(e.lit) <= starts[k] + lens[k]:  # (an occurrence cut by a forced break is in no piece)
                occ.setdefault(k, []).append((j, pos + len(e.lit) - starts[k]))
            pos = text.find(e.lit, pos + 1)
    records, admissible, raw_ref, raw = [], [], {}, {}
    for k in sorted(occ):
        here = occ[k]
        raw_ref[k] = len(here)
        times = Counter(j for j, _ in here)
        raw[k] = [(exprs[j].id, to, 1 if exprs[j].single else 0, j) for j, to in here for _ in range(1 if exprs[j].single else times[j])]
        first_single = {}
        for j, to in here:
            if exprs[j].single:
                first_single[exprs[j].id] = min(to, first_single.get(exprs[j].id, to))
        kept = {}
        for j, to in here:
            if not exprs[j].single or to == first_single[exprs[j].id]:
                kept.setdefault((exprs[j].id, to), set()).add(j)
        for rid, to in sorted(kept):
            records.append((line_base + k, rid, to, starts[k], lens[k]))
            admissible.append(frozenset(kept[(rid, to)]))
    return Scan(records, admissible, raw_ref, raw, starts, lens)


def bucket_fill(scan: Scan, fin_shift: int, fin_nb: int):
    """Raw reports per finalize bucket: a report goes to the bucket of its piece's start."""
    fill = [0] * fin_nb
    for k, recs in scan.raw.items():
        fill[scan.starts[k] >> fin_shift] += len(recs)
    return fill


def bucket_sorted(scan: Scan, fin_shift: int, bucket: int):
    """The raw reports of one bucket in the order its sort gives them: (piece start, id, to, single, expression); reports with
    equal keys in expression order (any order among them is a correct sort)."""
    out = []
    for k, recs in scan.raw.items():
        if scan.starts[k] >> fin_shift == bucket:
            out += [(scan.starts[k], rid, to, single, j) for rid, to, single, j in recs]
    return sorted(out)


def groups_of(sorted_raw):
    """[(first position, last position, records)] of the (line, id) groups of a bucket's sorted raw reports."""
    out, i = [], 0
    for _, g in itertools.groupby(sorted_raw, key=lambda r: r[:2]):
        g = list(g)
        out.append((i, i + len(g) - 1, g))
        i += len(g)
    return out


# ------------------------------------------------------------------------------------------- the engine's pass plan
def bits_for(v: int) -> int:
    b = 1
    while b < 64 and (v >> b):
        b += 1
    return b


def plan_buckets(nbytes: int, expect_prev: int, target: int, hit_cap: int = HIT_CAP0):
    """(fin_shift, fin_nb, fin_cap) of a whole-buffer pass (HgScanner::plan_pass): expect_prev is the raw report count of the
    scanner's last pass (0: a fresh scanner), target HG_FIN_TARGET."""
    shift, nb = 10, 1
    if nbytes:
        expect = max(expect_prev, nbytes >> 13)
        want = 1
        while want * target < expect and want < MAX_BUCKETS:
            want <<= 1
        while ((nbytes - 1) >> shift) >= want:
            shift += 1
        nb = ((nbytes - 1) >> shift) + 1
    return shift, nb, hit_cap // nb


def plan_path(fin_shift: int, max_id: int, buffer_size: int, line_base: int, nbytes: int, n_pieces: int, env) -> str:
    id_bits, to_bits = bits_for(max_id + 1), bits_for(buffer_size)
    if (fin_shift <= 24 and fin_shift + id_bits + to_bits + 1 <= 64 and bits_for(line_base + nbytes + 1) <= 40 and "HG_NO_BUCKET_FINALIZE" not in env):
        return "bucketed"
    return "compact_packed" if bits_for(line_base + n_pieces + 1) + id_bits + to_bits + 1 <= 64 else "compact_wide"


# ---------------------------------------------------------------------------------------------------------- texts
class Layout:
    """A text of filler lines (dots: no expression occurs in them) with planted lines at exact offsets."""

    def __init__(self, fill_len: int = 200):
        self.parts, self.cur, self.fill_len = [], 0, fill_len

    def fill_to(self, x: int):
        assert x >= self.cur, (x, self.cur)
        full, rest = divmod(x - self.cur, self.fill_len)
        if rest == 0 and full:
            full, rest = full - 1, self.fill_len
        if full:
            self.parts.append((b"." * (self.fill_len - 1) + b"\n") * full)
        if rest:
            self.parts.append(b"." * (rest - 1) + b"\n")
        self.cur = x
        return self

    def put(self, *lines: bytes):
        for line in lines:
            assert line.endswith(b"\n") and line.count(b"\n") == 1
            self.parts.append(line)
            self.cur += len(line)
        return self

    def at(self, x: int, *lines: bytes):
        return self.fill_to(x).put(*lines)

    def bytes(self, size: int | None = None) -> bytes:
        if size is not None:
            self.fill_to(size)
        return b"".join(self.parts)


A, B, C = 7, 9, 4095
# shared id A: two SINGLEMATCH and two all-matches literals; pairs that END TOGETHER wherever the longer one occurs: two
# all-matches expressions (kTie7 / Tie7: equal sort keys from different expressions) and a SINGLEMATCH with an all-matches
# one (gDup8 / Dup8: the duplicate rule across kinds); and a pair whose ends are NEIGHBOURS wherever the longer one occurs
# (hAdj / hAdjo: ends p and p + 1, on even and odd p: reports that differ in the lowest bit of `to` alone)
BASE = [Expr(b"sAx1", A, True), Expr(b"sBy2", A, True), Expr(b"mCz3", A, False), Expr(b"mDw4", A, False), Expr(b"qEv5", B, True), Expr(b"mFu6", C, False),
        Expr(b"kTie7", A, False), Expr(b"Tie7", A, False), Expr(b"gDup8", A, True), Expr(b"Dup8", A, False), Expr(b"wGt9", C, True),
        Expr(b"hAdj", A, False), Expr(b"hAdjo", A, False)]
SINGLES = [b"sAx1", b"sBy2", b"qEv5", b"wGt9"]


def words_raw(words) -> int:
    """Raw reports (raw_model) of a line made of these BASE words."""
    c = Counter(words)
    n = sum(c[w] for w in SINGLES) + c[b"mCz3"] ** 2 + c[b"mDw4"] ** 2 + c[b"mFu6"] ** 2
    return n + 2 * c[b"kTie7"] ** 2 + c[b"gDup8"] + c[b"gDup8"] ** 2 + 2 * c[b"hAdjo"] ** 2


def line_of(n: int, rng: random.Random, rich: bool = True) -> bytes:
    """One line with exactly n raw reports: where n allows, all-matches literals that occur twice or three times (every end
    two or three times in the raw reports), the pairs that end together, and SINGLEMATCH literals before, between and behind
    them (a SINGLEMATCH report earlier in its group, later, and duplicated)."""
    words = []
    if rich:
        for extra in ([b"mCz3"] * 3, [b"kTie7"], [b"gDup8"], [b"hAdjo"], [b"mDw4"] * 2, [b"mFu6"] * 2):
            if words_raw(words + extra) <= n:
                words += extra
    while words_raw(words) < n:
        words.append(SINGLES[len(words) % len(SINGLES)])
    assert words_raw(words) == n
    rng.shuffle(words)
    return b" ".join(words) + b"\n"


def lines_of(n: int, per_line: int, rng: random.Random):
    """n raw reports spread over lines of up to per_line each, with report-free lines between some of them."""
    out = []
    while n:
        k = min(n, rng.randint(1, per_line))
        out.append(line_of(k, rng))
        n -= k
        if n and rng.random() < 0.3:
            out.append(b"." * rng.randint(0, 30) + b"\n")
    return out


CLASS_EDGES = (1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096)
MIB = 1 << 20


def fill_text(placing, size: int, shift: int, seed: int, newline_at_end: bool = True) -> bytes:
    """placing: {bucket: (raw reports, "line" | "spread", offset of the first planted line in the bucket; negative: from the bucket's end)}."""
    rng = random.Random(seed)
    lay = Layout()
    for b in sorted(placing):
        n, how, off = placing[b]
        at = (b << shift) + off if off >= 0 else ((b + 1) << shift) + off
        lay.at(at, *([line_of(n, rng)] if how == "line" else lines_of(n, 7 if n <= 600 else 40, rng)))
        assert lay.cur - len(lay.parts[-1]) < (b + 1) << shift, "the bucket's last planted line starts inside it"
    text = lay.bytes(size)
    return text if newline_at_end else text[:-1]


# ---------------------------------------------------------------------------------------------------------- cells
@dataclass
class Cell:
    name: str
    text: object  # () -> bytes
    exprs: list
    buffer_size: int = 262140
    env: dict = field(default_factory=dict)
    line_base: int = 0
    prelude: object = None  # () -> bytes: a first scan on the same scanner (its results are checked as well)
    second: object = None   # () -> bytes: a scan behind the cell's on the same scanner, checked for exact results
    claim: dict = field(default_factory=dict)
    # claim: path, fin_shift, fin_nb, fin_cap, early_beside_stream, joiner_launches_min; fills {bucket: raw reports}; classes (fill levels that must occur); reruns_min;
    # left_bucketed; early_buckets; scan_blocks; second_path; first_plan (the plan of the pass that overflows); positions: a function (cell) -> None that asserts the sorted
    # positions the cell is named for
    som: bool = False
    big: bool = False


@functools.lru_cache(maxsize=None)
def _text(fn):
    return fn()


def cell_text(cell: Cell) -> bytes:
    return _text(cell.text)


def cell_scan(cell: Cell, which: str = "text") -> Scan:
    return _scan(getattr(cell, which), tuple(cell.exprs), cell.buffer_size, cell.line_base if which == "text" else 0)


@functools.lru_cache(maxsize=64)
def _scan(fn, exprs, buffer_size, line_base):
    return reference(_text(fn), exprs, buffer_size, line_base)


def target_of(cell: Cell) -> int:
    return max(4, int(cell.env.get("HG_FIN_TARGET", 48)))


FRESH8 = {"HG_FIN_TARGET": "8"}  # 1 MiB on a fresh scanner: 16 buckets of 64 KiB, 4096 records each


def _fills_a():
    # every class once, all reports of a bucket on ONE line; neighbours of different classes, empty buckets between others;
    # the first bucket and the last one hold the largest classes; lines that start on a bucket's first and last byte
    placing = {0: (4096, "line", 0), 1: (1, "line", 77), 3: (64, "line", -1), 4: (65, "line", 1000), 6: (512, "line", 5000), 7: (513, "line", 0),
               9: (63, "line", 1), 10: (2, "line", -40000), 11: (511, "line", 300), 13: (4095, "line", 123), 15: (4096, "line", 20000)}
    return fill_text(placing, MIB, 16, 101)


def _fills_b():
    # the same classes spread over the bucket's lines, in another arrangement; the last bucket is only partly covered by the
    # text, which ends without a newline
    placing = {0: (65, "spread", 0), 1: (4096, "spread", 0), 2: (4095, "spread", 64), 4: (513, "spread", 100), 5: (512, "spread", 0), 6: (511, "spread", 7),
               8: (64, "spread", 10), 9: (63, "spread", 0), 10: (2, "spread", 65000), 12: (1, "spread", -1), 15: (64, "spread", 0)}
    return fill_text(placing, MIB - 40000, 16, 102, newline_at_end=False)


def _fills_c():
    # the small classes in the first bucket, the 513+ class in a partly covered last bucket
    placing = {0: (63, "spread", 0), 1: (64, "line", 0), 2: (65, "line", 0), 14: (2, "line", 0), 15: (4096, "spread", 3)}
    return fill_text(placing, MIB - 30000, 16, 103)


def _overflow():
    return fill_text({2: (64, "spread", 0), 3: (4097, "line", 100), 4: (65, "line", 0), 9: (600, "spread", 0)}, MIB, 16, 104)


def _regrow():
    # 32 KiB buckets of 2048 records; one with 3000 reports: the bucket regions grow, the scanner stays with buckets
    return fill_text({1: (5, "line", 0), 6: (3000, "line", 100), 7: (70, "spread", 0), 20: (300, "spread", 0)}, MIB, 15, 105)


# -- rule positions: (line, id) groups of mixed kinds at chosen positions of a bucket's sorted reports
def _group_line(words) -> bytes:
    return b" ".join(words) + b"\n"


def _pad_lines(n: int, rng):
    """n raw reports of id A on lines that sort in front of / between the planted groups (SINGLEMATCH literals only: one report each)."""
    out = []
    while n:
        k = min(n, 5)
        out.append(b" ".join([b"sAx1", b"sBy2", b"sAx1", b"sBy2", b"sAx1"][:k]) + b"\n")
        n -= k
    return out


def _positions_text():
    rng = random.Random(106)
    lay = Layout()
    # bucket 1: 64 reports, the last (line, id) group begins at sorted position 63: 63 reports of id A, one of id B, one line
    lay.at(1 << 16, _group_line([b"qEv5"] + [b"mCz3"] * 3 + [b"kTie7"] + [b"gDup8"] + [b"mDw4"] * 2 + [b"sAx1", b"sBy2"] * 23))
    # bucket 2: 64 reports, ONE group spans positions 0-63
    lay.at(2 << 16, _group_line([b"sBy2"] + [b"mCz3"] * 6 + [b"mDw4"] * 4 + [b"gDup8"] + [b"sAx1"] * 9))
    # buckets 4 (65-512) and 6 (513-4096): 62 reports, a group over positions 62-66 whose duplicate pair sits on 63|64 (a
    # SINGLEMATCH report in front of it), 60 more, a group from 127 whose duplicate pair sits on 127|128 (SINGLEMATCH behind)
    for b, total in ((4, 200), (6, 700)):
        lines = _pad_lines(62, rng) + [_group_line([b"sAx1", b"mCz3", b"mCz3"])] + _pad_lines(60, rng) + [_group_line([b"mDw4", b"mDw4", b"sBy2", b"gDup8"])]
        lines += _pad_lines(total - 62 - 5 - 60 - 7, rng)
        lay.at(b << 16, *lines)
    # bucket 8: one group of 66: its last report is a SINGLEMATCH one, and the one that rules it out is 65 positions in front
    lay.at(8 << 16, _group_line([b"sBy2"] + [b"mCz3"] * 8 + [b"sAx1"]))
    return lay.bytes(MIB)


def _check_positions(cell):
    scan = cell_scan(cell)
    g1 = groups_of(bucket_sorted(scan, 16, 1))
    assert g1[-1][0] == 63 and g1[-1][1] == 63 and len(g1) == 2, "bucket 1: the last group begins at position 63"
    g2 = groups_of(bucket_sorted(scan, 16, 2))
    assert [(a, z) for a, z, _ in g2] == [(0, 63)], "bucket 2: one group over positions 0-63"
    assert {r[3] for r in g2[0][2]} == {0, 1}
    for b in (4, 6):
        s = bucket_sorted(scan, 16, b)
        spans = [(a, z) for a, z, _ in groups_of(s)]
        assert (62, 66) in spans and (127, 133) in spans, (b, spans)
        assert s[62][3] == 1 and s[63][:4] == s[64][:4] and s[63][3] == 0, "a duplicate pair on positions 63|64 behind a SINGLEMATCH report"
        assert s[127][:4] == s[128][:4] and s[127][3] == 0 and any(r[3] == 1 for r in s[129:134]), "a duplicate pair on 127|128, SINGLEMATCH behind it"
    s8 = bucket_sorted(scan, 16, 8)
    assert len(s8) == 66 and s8[0][3] == 1 and s8[65][3] == 1 and all(r[3] == 0 for r in s8[1:65]) and len(groups_of(s8)) == 1


# -- every small group once: up to three (kind, end) reports over ends a < b < c, all sharing one id.  One family of literals
# per (end, kinds): U<f>VW, S<f>TU<f>VW, Q<f>RS<f>TU<f>VW end together wherever the longest occurs.
KINDS = list(itertools.product((True, False), repeat=3))


def _family(f: int):
    u = b"U%02dVW" % f
    s = b"S%02dT" % f + u
    return [u, s, b"Q%02dR" % f + s]


GROUP_EXPRS = [Expr(lit, A, kinds[i]) for slot in range(3) for kc, kinds in enumerate(KINDS) for i, lit in enumerate(_family(slot * 8 + kc))]
SMALL_GROUPS = [g for n in (1, 2, 3) for g in itertools.combinations_with_replacement([(single, end) for end in range(3) for single in (True, False)], n)]


def _group_words(group):
    words = []
    for end in range(3):
        kinds = sorted((single for single, e in group if e == end), reverse=True)  # SINGLEMATCH ones first, as KINDS lists them
        if kinds:
            kc = next(i for i, k in enumerate(KINDS) if list(k[:len(kinds)]) == kinds)
            words.append(_family(end * 8 + kc)[len(kinds) - 1])
    return words


def _groups_text(copies: int, spread: bool):
    def make():
        lay = Layout()
        lines = [_group_line(_group_words(g)) for _ in range(copies) for g in SMALL_GROUPS]
        if not spread:
            return lay.put(*lines).bytes()
        for i in range(0, len(lines), 6):  # six groups to a 64 KiB bucket: at most 18 reports, one wave orders them
            lay.at((i // 6) << 16, *lines[i:i + 6])
        return lay.bytes(MIB)
    return make


GROUPS_ONE, GROUPS_BIG, GROUPS_SPREAD = _groups_text(1, False), _groups_text(5, False), _groups_text(1, True)

# -- key width
WIDE_IDS = [0, 1, 4095, 0x7FFFFFFF, 0xFFFFFFF0, 0xFFFFFFFF]
WIDE = [Expr(b"sAx1", 0xFFFFFFFF, True), Expr(b"sBy2", 0xFFFFFFFF, True), Expr(b"mCz3", 0xFFFFFFFF, False), Expr(b"mDw4", 0xFFFFFFF0, False), Expr(b"qEv5", 0x7FFFFFFF, True),
        Expr(b"mFu6", 4095, False), Expr(b"kTie7", 1, False), Expr(b"Tie7", 1, False), Expr(b"gDup8", 0xFFFFFFFF, True), Expr(b"Dup8", 0xFFFFFFFF, False), Expr(b"wGt9", 0, True),
        Expr(b"hAdj", 0xFFFFFFF0, False), Expr(b"hAdjo", 0xFFFFFFF0, False)]
assert [e.lit for e in WIDE] == [e.lit for e in BASE] and {e.id for e in WIDE} == set(WIDE_IDS)
SMALL_IDS = [Expr(e.lit, i % 5, e.single) for i, e in enumerate(BASE)]
# ids that differ in their lowest bit alone, SINGLEMATCH and all-matches expressions on either: the bit that separates two
# (line, id) groups is the lowest one above `to` in the sort key
NEIGHBOUR_IDS = [Expr(e.lit, 6 + (i * 5 // 3) % 2, e.single) for i, e in enumerate(BASE)]


def _neighbour_text():
    # lines of each sort class: 50 and 60 reports (one wave), 300 and 400 (a block in LDS), 700 and 2000 (a block in scratch)
    return fill_text({1: (50, "line", 0), 3: (60, "spread", 9), 5: (300, "line", 100), 7: (400, "spread", 0), 9: (700, "line", 1), 11: (2000, "spread", 0)}, MIB, 16, 110)


SOM_SET = [Expr(e.lit, (A if e.lit != b"qEv5" else B) if e.single else C, e.single) for e in BASE]


def _dense_prelude():
    # 400 reports on 400 lines: the next pass on this scanner expects as many and plans 1 KiB buckets for a text of 64 KiB
    return b"".join(b"sAx1 " + b"." * (i % 50) + b"\n" for i in range(400))


def _key_text():
    rng = random.Random(107)
    lines = []
    for i in range(1100):
        lines.append(line_of(rng.choice((0, 0, 1, 3, 13, 30)), rng) if i % 3 == 0 else b"." * rng.randint(60, 120) + b"\n")
    return b"".join(lines)[:65536].rsplit(b"\n", 1)[0] + b"\n"


def _small_text():
    return fill_text({0: (40, "spread", 0), 2: (300, "spread", 0), 5: (30, "line", -1), 9: (700, "spread", 0), 15: (9, "line", 0)}, MIB, 16, 108)


# -- ranges: three pipeline chunks; the buckets that the first two chunks complete are finalized beside the third's side passes
RANGES_SIZE, RANGES_B, RANGES_SHIFT = 48 * MIB, 32 * MIB, 22
RANGES_X = 28 * MIB - 1  # a planted line on the LAST byte of bucket 6
RANGES_ENV = {"HG_CHUNK_TILES": "1024", "HG_FIN_TARGET": "384"}  # 16 MiB chunks; 12 buckets of 4 MiB, 5461 records each


def _ranges_text():
    rng = random.Random(109)
    lay = Layout(fill_len=3000)
    for b, n, how in ((3, 600, "spread"), (4, 40, "spread"), (5, 300, "spread"), (6, 700, "spread")):  # every class below the settled limit
        lay.at((b << RANGES_SHIFT) + 12345, *([line_of(n, rng)] if how == "line" else lines_of(n, 7, rng)))
    # the long line: reports at its start and around every place where a scan buffer of B - X - 1, B - X or B - X + 1 bytes ends
    # its first piece, i.e. just below and beyond the last chunk's start B
    span = RANGES_B - RANGES_X
    head = b"sAx1 mCz3 sBy2 mCz3 "
    far = b" ".join([b"mDw4", b"sAx1", b"kTie7", b"qEv5", b"gDup8", b"mDw4"])
    body = head + b"." * (span - 20 - len(head) - 1) + far
    long_line = body + b"." * (span + 40 - len(body)) + b" sBy2 mFu6 mFu6\n"
    lay.at(RANGES_X, long_line)
    for b, n in ((8, 50), (9, 400), (10, 600)):  # ... and beyond it
        lay.at((b << RANGES_SHIFT) + 777, *lines_of(n, 7, rng))
    lay.at(RANGES_SIZE - 30, line_of(3, rng))
    return lay.bytes(RANGES_SIZE)


def _ranges_cells():
    out = []
    # default: the engine decides about a joiner; -joiner: a joiner launch per later chunk, so the early range is finalized
    # beside the last stream launch (hg_fin_scan_kernel<512>); -nojoiner / -noearly: beside the last side passes / not at all
    for tag, env in (("", {}), ("-noearly", {"HG_NO_EARLY_FINALIZE": "1"}), ("-nojoiner", {"HG_JOINER": "0"}), ("-joiner", {"HG_JOINER": "1"})):
        for d in (-1, 0, 1):  # the long line starts at B - bs1 - 1, B - bs1, B - bs1 + 1
            bs1 = RANGES_B - RANGES_X + d
            settled = (RANGES_B - bs1) >> RANGES_SHIFT
            claim = {"path": "bucketed", "fin_shift": RANGES_SHIFT, "fin_nb": 12, "fin_cap": HIT_CAP0 // 12, "stream_launches": 3,
                     "early_buckets": 0 if "HG_NO_EARLY_FINALIZE" in env else settled, "classes_each_side": settled}
            if tag:
                claim["early_beside_stream"] = settled if tag == "-joiner" else 0
            if tag == "-joiner":
                claim["joiner_launches_min"] = 1
            out.append(Cell(f"ranges{tag}-start{d:+d}", _ranges_text, BASE, buffer_size=bs1 + 1, env={**RANGES_ENV, **env}, big=True, claim=claim))
    return out


# -- many buckets: more than 8192 in one range, so the position scan runs several blocks
MANY_SIZE = 24 * MIB + 1024
MANY_NB = MANY_SIZE >> 10
MANY_BLOCKS = (MANY_NB + 8191) // 8192
MANY_SPAN = ((MANY_NB + MANY_BLOCKS - 1) // MANY_BLOCKS + 1023) // 1024 * 1024  # buckets per block of hg_fin_scan_kernel<1024>


def _many_prelude():
    # 70 000 reports, 16 to a KiB: the next pass plans 1 KiB buckets for any text of up to 32 MiB
    return (b"sAx1" + b"." * 59 + b"\n") * 70000


def _many_buckets():
    edges = {0, 1, MANY_NB - 2, MANY_NB - 1}
    for k in range(1, MANY_BLOCKS):
        edges |= {k * 8192 - 1, k * 8192, k * MANY_SPAN - 1, k * MANY_SPAN}
    return sorted(edges)


def _many_text():
    lay = Layout(fill_len=500)
    samples = [b"sAx1 mCz3 sBy2\n", b"mCz3 sAx1 mCz3\n", b"gDup8 qEv5\n", b"kTie7 mFu6\n", b"sBy2\n"]  # at most 5 reports to a bucket
    for i, b in enumerate(_many_buckets()):
        lay.at((b << 10) + (i * 37) % 900, samples[i % len(samples)])
    return lay.bytes(MANY_SIZE)


def _line_base_cells():
    out = []
    n = MIB
    for bits, tag in ((40, "40bits"), (41, "41bits")):
        base = (1 << 40) - n - 1 - (1 if bits == 40 else 0)  # line_base + nbytes + 1 == 2^40 - 1 (40 bits) or 2^40 (41 bits)
        out.append(Cell(f"linebase-{tag}", _small_text, SMALL_IDS, env=FRESH8, line_base=base,
                        claim={"path": "bucketed" if bits == 40 else "compact_packed", "fin_shift": 16, "fin_nb": 16, "bound_bits": bits}))
    return out


def cells():
    out = [
        Cell("fill-one-line", _fills_a, BASE, env=FRESH8,
             claim={"path": "bucketed", "fin_shift": 16, "fin_nb": 16, "fin_cap": 4096,
                    "fills": {0: 4096, 1: 1, 2: 0, 3: 64, 4: 65, 5: 0, 6: 512, 7: 513, 8: 0, 9: 63, 10: 2, 11: 511, 12: 0, 13: 4095, 14: 0, 15: 4096}, "classes": CLASS_EDGES}),
        Cell("fill-spread", _fills_b, BASE, env=FRESH8,
             claim={"path": "bucketed", "fin_shift": 16, "fin_nb": 16, "fin_cap": 4096,
                    "fills": {0: 65, 1: 4096, 2: 4095, 3: 0, 4: 513, 5: 512, 6: 511, 7: 0, 8: 64, 9: 63, 10: 2, 11: 0, 12: 1, 15: 64}, "classes": CLASS_EDGES}),
        Cell("fill-first-last", _fills_c, BASE, env=FRESH8,
             claim={"path": "bucketed", "fin_shift": 16, "fin_nb": 16, "fin_cap": 4096, "fills": {0: 63, 1: 64, 2: 65, 14: 2, 15: 4096}}),
        Cell("overflow-4097", _overflow, BASE, env=FRESH8, second=_fills_b,
             claim={"path": "compact_packed", "reruns_min": 1, "left_bucketed": True, "second_path": "compact_packed", "first_plan": (16, 16, 4096), "max_fill": 4097}),
        Cell("regrow-3000", _regrow, BASE, env={"HG_FIN_TARGET": "4"},
             claim={"path": "bucketed", "reruns_min": 1, "left_bucketed": False, "first_plan": (15, 32, 2048), "max_fill": 3000}),
        Cell("rule-positions", _positions_text, BASE, env=FRESH8,
             claim={"path": "bucketed", "fin_shift": 16, "fin_nb": 16, "fills": {1: 64, 2: 64, 4: 200, 6: 700, 8: 66}, "positions": _check_positions}),
        Cell("rule-groups-one-bucket", GROUPS_ONE, GROUP_EXPRS, claim={"path": "bucketed", "fin_nb": 1, "fill_class": (65, 512)}),
        Cell("rule-groups-big-bucket", GROUPS_BIG, GROUP_EXPRS, claim={"path": "bucketed", "fin_nb": 1, "fill_class": (513, 4096)}),
        Cell("rule-groups-small-buckets", GROUPS_SPREAD, GROUP_EXPRS, env=FRESH8, claim={"path": "bucketed", "fin_shift": 16, "fin_nb": 16, "fill_class": (1, 64)}),
        # starts of match behind the finalize: HS_FLAG_SOM_LEFTMOST on the all-matches expressions, which then share no id with a
        # SINGLEMATCH one (the compiler's rule); the pairs that end together have different starts, either may be reported
        Cell("som-starts", _small_text, SOM_SET, env=FRESH8, som=True, claim={"path": "bucketed", "fin_shift": 16, "fin_nb": 16, "fills": {0: 40, 2: 300, 5: 30, 9: 700, 15: 9}}),
        Cell("neighbour-ids", _neighbour_text, NEIGHBOUR_IDS, env=FRESH8,
             claim={"path": "bucketed", "fin_shift": 16, "fin_nb": 16, "fills": {1: 50, 3: 60, 5: 300, 7: 400, 9: 700, 11: 2000}, "neighbour_ids": (1, 5, 9)}),
        # fin_shift + id_bits + to_bits + 1 == 10 + 33 + 20 + 1 == 64: still bucketed
        Cell("key-64-bits", _key_text, WIDE, buffer_size=(1 << 19) + 5, env={"HG_FIN_TARGET": "4"}, prelude=_dense_prelude,
             claim={"path": "bucketed", "fin_shift": 10, "fin_nb": 64, "id_bits": 33, "to_bits": 20, "key_bits": 64}),
        # one `to` bit more: 65 bits, the compact array; 10 line bits + 33 + 21 + 1 > 64: two sorts
        Cell("key-65-bits", _key_text, WIDE, buffer_size=1 << 20, env={"HG_FIN_TARGET": "4"}, prelude=_dense_prelude,
             claim={"path": "compact_wide", "fin_shift": 10, "fin_nb": 64, "id_bits": 33, "to_bits": 21, "key_bits": 65}),
        Cell("key-packed-no-buckets", _small_text, SMALL_IDS, env={"HG_NO_BUCKET_FINALIZE": "1", "HG_FIN_TARGET": "8"}, claim={"path": "compact_packed", "id_bits": 3}),
        *_line_base_cells(),
        *_ranges_cells(),
        Cell("many-buckets", _many_text, BASE, env={"HG_FIN_TARGET": "4"}, prelude=_many_prelude, big=True,
             claim={"path": "bucketed", "fin_shift": 10, "fin_nb": MANY_NB, "scan_blocks": MANY_BLOCKS, "kept_buckets": _many_buckets()}),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


CELLS = cells()
