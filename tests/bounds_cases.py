"""Window scans of a larger text: the cases, their windows and what every window claims.  Test infrastructure: imported by
test_text_bounds.py and test_text_bounds_gpu.py.

hg_scan_device and every call built on it take (d_text, nbytes) and must treat [0, nbytes) as the whole world.  A case keeps
one base text in memory and scans the window [lo, hi) of it with d_text = base + lo (lo a multiple of 16), so the bytes around
the window are the real continuation of the text: a routine that looks one byte too far finds exactly the bytes that complete
a match, add a line or change a context.  The reference is the stage's own reference run on data[lo:hi] alone.

A case is one expression set of one tier (placement asserted by test_text_bounds.py), a base text of at most five tiles and a
frame of two tiles and 1 KiB of ordinary match-bearing lines behind it, so that every load a correct or slightly wrong routine
makes stays inside mapped, initialised memory.  Every line of the text that is not a planted event is a "good line": filler
and one complete match, the expressions in turn, so what follows any `hi` holds newlines and complete matches.

Window classes (d = hi - lo is what the kernels see as nbytes; rows and tiles count from lo):

    R1  hi inside a required literal, at every residue d % 16 for literals of 8, 16, 17 and 32 bytes; one caseless literal
    R2  the required literal complete, the match needs bytes behind hi
    R3  hi one byte before a newline, on it, one byte after it
    R4  context at the end: \\b, $, \\B where text[hi] flips the answer
    R5  a right event of class R1-R4 with hi at a 1 KiB row edge -1 / 0 / +1 or at a tile edge -1 / 0 / +1 ("R5/tile+1:R2")
    R6  the huge expression with its closing literal behind hi
    L1  lo inside a required literal: its head lies before the window
    L2  text[lo - 1] is a word byte: ^ and \\b at window offset 0 must hold, \\B must not
    L3  text[lo - 1] is a newline in one window and is not in another: line 0 starts at lo either way
    L4  an always-on match in progress at lo

Every window carries k, the smallest leak its class is about: the reference on the window widened by k bytes (to the right
for R, to the left for L) differs from the reference on the window itself.  test_text_bounds.py proves that for every
window; a window whose surroundings would not change the answer proves nothing."""
from __future__ import annotations

import bisect
import functools
from dataclasses import dataclass

import numpy as np

import always_on_cells as ac
import confirm_cells as cc
import somsim_py

TILE = cc.TILE
ROW = 1024
DEFAULT_BS = cc.DEFAULT_BS
SIZES = (DEFAULT_BS, 64)
FILL = b"#%&~;!"  # no word byte, no letter, no digit, no '@': no expression matches across filler
MAX_BODY = 5 * TILE
FRAME = 2 * TILE + ROW
RIGHT = ("R1", "R2", "R3", "R4", "R5", "R6")
LEFT = ("L1", "L2", "L3", "L4")
GEOMETRY = ("R3", "L3")  # judged on all five columns and n_lines; every other class on where which id reports
# the (case, class) pairs that make sense: always-on expressions have no required literal, R6 is the huge automaton's
SENSIBLE = {
    "literal": ("R1", "R2", "R3", "R4", "R5", "L1", "L2", "L3"),
    "always_on_free": ("R2", "R3", "R5", "L3", "L4"),  # no boundary conditions: no byte beside a match is looked at
    "always_on_ctx": ("R2", "R3", "R4", "R5", "L2", "L3", "L4"),
    "huge": ("R1", "R3", "R5", "R6", "L1", "L3"),
}


def fill(n: int, salt: int = 0) -> bytes:
    return bytes(FILL[(i * 7 + salt * 3 + (i >> 3)) % len(FILL)] for i in range(n))


@dataclass(frozen=True)
class Ev:
    cls: str
    blob: bytes  # one line (a '\n' is added unless it ends in one); it starts a line of the text
    cut: int  # the window edge falls in front of blob[cut]
    k: int  # the leak the event is about, in bytes
    sub: str = ""
    residues: tuple = (15, 0, 1, 7)  # right events: d % 16 of the windows
    som: bool = False  # the leak changes a start of match only


@dataclass(frozen=True)
class BExpr:
    pattern: str
    flags: int
    good: bytes  # a complete match between filler bytes
    events: tuple = ()
    mode: int | None = None  # literal tier: hg_confirm_mode
    bol: bool = False
    eol: bool = False


@dataclass(frozen=True)
class Window:
    cls: str
    tag: str
    lo: int
    hi: int
    k: int
    expr: int
    som: bool = False

    @property
    def side(self):
        return "R" if self.cls in RIGHT else "L"

    @property
    def base_cls(self):
        """R5 windows: the class of the event at the edge."""
        return self.tag.split(":")[1].split("/")[0] if self.cls == "R5" else self.cls


@dataclass
class Case:
    name: str
    tier: str
    exprs: tuple
    data: bytes
    windows: list
    body_end: int
    line_starts: list

    @property
    def patterns(self):
        return [e.pattern for e in self.exprs]

    @property
    def flags(self):
        return [e.flags for e in self.exprs]

    def ids(self, shared: bool):
        return [0] * len(self.exprs) if shared else list(range(len(self.exprs)))

    def what(self, w: Window) -> str:
        return f"{self.name} window [{w.lo}, {w.hi}) d={w.hi - w.lo} ({(w.hi - w.lo) % 16} mod 16) {w.tag} expr {w.expr} {self.exprs[w.expr].pattern!r}"


# ------------------------------------------------------------------ expression sets
def _lit(n: int) -> bytes:
    s = (b"ndl_%02d_" % n + b"abcdefghijklmnopqrstuvwxyz")[:n]
    assert len(s) == n
    return s


def _r1(lit: bytes, text: bytes | None = None, residues=tuple(range(16)), tail: bytes = b"") -> tuple:
    """hi inside the literal, the cut moving with the residue; the leak is the rest of the match."""
    text = text or lit
    out = []
    for r in residues:
        c = 1 + (r * 3 + len(lit)) % (len(lit) - 1)
        out.append(Ev("R1", fill(5, r) + text + tail + fill(4, r + 1), 5 + c, len(text) + len(tail) - c, f"lit{len(lit)}", (r,)))
    return tuple(out)


def _l1(lit: bytes, text: bytes | None = None, tail: bytes = b"") -> tuple:
    text = text or lit
    return tuple(Ev("L1", fill(6, c) + text + tail + fill(5, c + 1), 6 + c, c, f"lit{len(lit)}") for c in sorted({1, len(lit) // 2, len(lit) - 1}))


def _r3(good: bytes, e: BExpr | None = None) -> tuple:
    """hi one byte before the line's newline, on it, one byte behind it.  The line has a report, so its len is compared."""
    body = (b"" if e and e.bol else fill(2, 1)) + good + fill(3, 2) + b"c"
    return tuple(Ev("R3", body + b"\n", len(body) + d, 1, ("nl-1", "nl", "nl+1")[d + 1], (r,)) for d, r in ((-1, 15), (0, 0), (1, 1), (-1, 6), (0, 9), (1, 12)))


def _l3(good: bytes) -> tuple:
    return (Ev("L3", good + fill(4, 3), 0, 1, "after_newline"), Ev("L3", fill(7, 2) + fill(5, 4) + good + fill(3, 1), 7, 1, "mid_line"))


L8, L16, L17, L32 = _lit(8), _lit(16), _lit(17), _lit(32)

LITERAL = (
    BExpr(L8.decode(), 14, L8, _r1(L8) + _l1(L8), mode=0),
    BExpr(L16.decode(), 14, L16, _r1(L16) + _l1(L16) + _l3(L16), mode=0),
    BExpr(L17.decode(), 14, L17, _r1(L17) + _l1(L17) + _r3(L17), mode=0),
    BExpr(L32.decode(), 14, L32, _r1(L32) + _l1(L32), mode=0),
    BExpr("Ndl_Ci_Folded", 15, b"nDL_cI_fOLDED", _r1(b"nDL_cI_fOLDED", residues=(15, 0, 1, 3, 9)) + _l1(b"nDL_cI_fOLDED"), mode=0),
    BExpr("needle_sa_[0-9]+x", 14, b"needle_sa_123x", _r1(b"needle_sa_", residues=(15, 0, 1, 6), tail=b"12x") + _l1(b"needle_sa_", tail=b"7x") + (
        Ev("R2", fill(3) + b"needle_sa_123x" + fill(3, 1), 3 + 13, 1, "digits|x"),
        # SINGLEMATCH: the line's first (and only reported) match end lies behind hi, a second occurrence follows it
        Ev("R2", fill(2) + b"needle_sa_1" + b"2x" + fill(3, 1) + b"needle_sa_3x", 2 + 11, 2, "singlematch"),
    ) + _r3(b"needle_sa_123x") + _l3(b"needle_sa_9x"), mode=1),
    BExpr(r"needle_cb_foo\b", 14, b"needle_cb_foo", (Ev("R4", fill(4) + b"needle_cb_foo" + b"x" + fill(3, 1), 4 + 13, 1, r"\b|word"),) + _r3(b"needle_cb_foo"), mode=2),
    BExpr("needle_ce_foo$", 14, b"needle_ce_foo", (Ev("R4", fill(4, 2) + b"needle_ce_foo" + fill(3, 1), 4 + 13, 1, "$|not_newline"),), mode=2, eol=True),
    BExpr(r"needle_cg_foo\B", 14, b"needle_cg_fooz", (Ev("R4", fill(4, 3) + b"needle_cg_fooz" + fill(3, 1), 4 + 13, 1, r"\B|word"),), mode=2),
    BExpr("^needle_la_abc", 14, b"needle_la_abc", (Ev("L2", fill(3) + b"w" + b"needle_la_abc" + fill(4), 4, 1, "^"),), mode=2, bol=True),
    BExpr(r"\bneedle_lb_abc", 14, b"needle_lb_abc", (Ev("L2", fill(3, 1) + b"w" + b"needle_lb_abc" + fill(4), 4, 1, r"\b"),), mode=2),
    BExpr(r"\Bneedle_lc_abc", 14, b"qneedle_lc_abc", (Ev("L2", fill(3, 2) + b"w" + b"needle_lc_abc" + fill(4), 4, 1, r"\B"),), mode=2),
    BExpr("needle_ga_[0-9]*", 6, b"needle_ga_123", (Ev("R2", fill(3, 4) + b"needle_ga_12345" + fill(3, 1), 3 + 11, 4, "all_matches"),) + _r3(b"needle_ga_12") + _l3(b"needle_ga_7"), mode=3),
    BExpr(r"[a-z]{0,20}needle_cf_11[0-9]{1,20}\b", 14, b"abcneedle_cf_1112345", (
        Ev("R2", fill(3, 5) + b"abcneedle_cf_11" + b"7" + fill(3, 1), 3 + 15, 1, "literal|digit"),
        Ev("R4", fill(3, 6) + b"abcneedle_cf_11123" + fill(3, 1), 3 + 16, 1, r"digit\b|digit"),
    ), mode=2),
)

W2 = ac.S_W2_0["good"][0]
NT4 = b"1adgjmpyzy2"
NT4U = b"1adgjmpYZY2"
SCB = ac.S_SC_B["good"][0]


def _r2_last(good: bytes, sub: str = "last_byte") -> tuple:
    return (Ev("R2", fill(3, 1) + good + fill(3, 2), 3 + len(good) - 1, 1, sub),)


def _l4_half(good: bytes) -> tuple:
    c = len(good) // 2
    return (Ev("L4", fill(6, 2) + good + fill(4, 1), 6 + c, c, "in_progress"),)


AO_FREE = (
    BExpr("[0-9]+x", 14, b"123x", _r2_last(b"123x", "digits|x") + _r3(b"45x") + _l3(b"6x") + (Ev("L4", fill(6) + b"1234x" + fill(3, 1), 6 + 2, 2, "digits_before_lo", som=True),)),
    BExpr("[a-z]+@[a-z]+", 6, b"bob@example", (Ev("R2", fill(3) + b"bob@example" + fill(2, 1), 3 + 4, 1, "@|"),) + _r3(b"al@b") + (Ev("L4", fill(6, 1) + b"bob@example" + fill(3), 6 + 4, 4, "@_before_lo"),)),
    BExpr("[X-Z]{2,3}", 6, b"XYZ", _r2_last(b"XYZ") + _l3(b"YZ") + (Ev("L4", fill(6, 3) + b"XYZ" + fill(3), 6 + 1, 1, "in_progress"),)),
    BExpr(ac.P_NT4, 14, NT4, _r2_last(NT4) + _r3(NT4) + _l4_half(NT4)),
    BExpr(ac.P_W2_0, 14, W2, _r2_last(W2) + _r3(W2) + _l3(W2) + _l4_half(W2)),
)


def _r4_word(good: bytes) -> tuple:
    return (Ev("R4", fill(4, 1) + good + b"_" + fill(3, 2), 4 + len(good), 1, r"\b|word"),)


def _l2_word(good: bytes, sub: str = r"\b") -> tuple:
    return (Ev("L2", fill(3, 2) + b"w" + good + fill(4, 1), 4, 1, sub),)


AO_CTX = (
    BExpr(r"\b[A-C][0-9]{2,4}[g-i]\b", 14, b"A123g", (Ev("R2", fill(3) + b"A123g" + fill(3, 1), 3 + 4, 1, "last_byte"),) + _r4_word(b"A123g") + _l2_word(b"A123g") + _r3(b"B45h") + _l3(b"C67i") + _l4_half(b"A1234g")),
    BExpr("[A-C][D-F]{2,4}$", 14, b"ADEF", (Ev("R4", fill(4) + b"ADEF" + fill(3, 1), 4 + 4, 1, "$|not_newline"), Ev("R2", fill(4) + b"ADEF", 4 + 3, 1, "last_byte")), eol=True),
    BExpr("^[j-l][m-o]{2,4}", 6, b"jmno", (Ev("L2", fill(3) + b"w" + b"jmno" + fill(4), 4, 1, "^"), Ev("R2", b"jmno" + fill(4), 2, 1, "all_matches")), bol=True),
    BExpr(rf"\b{ac.P_NT4}\b".replace("[yz]", "[YZ]"), 14, NT4U, _r2_last(NT4U) + _r4_word(NT4U) + _l2_word(NT4U) + _r3(NT4U) + _l4_half(NT4U)),
    BExpr(rf"\b{ac.P_W2_0}\b", 14, W2, _r2_last(W2) + _r4_word(W2) + _l2_word(W2) + _l3(W2) + _l4_half(W2)),
    BExpr(ac.E_SC_B.pattern, 14, SCB, _r2_last(SCB) + _r3(SCB) + _l3(SCB) + _l4_half(SCB)),
)

HG_HEAD, HG_TAIL = b"needle_hg", b"thread"


def _huge_events() -> tuple:
    out = []
    for i, gap in enumerate((3, 40, 700, 3000, 4990)):
        for j in ((0, 3, 5) if gap <= 700 else (2,)):  # hi in front of / inside the closing literal
            out.append(Ev("R6", fill(4, i) + HG_HEAD + fill(gap, i + j) + HG_TAIL + fill(5), 4 + len(HG_HEAD) + gap + j, len(HG_TAIL) - j, f"gap{gap}", (15, 0, 1, 4 + j) if gap <= 700 else (0, 11)))
    short = HG_HEAD + fill(12, 3) + HG_TAIL
    for r in range(16):
        c = 1 + (r * 3) % (len(HG_HEAD) - 1)
        out.append(Ev("R1", fill(5, r) + short + fill(4), 5 + c, len(short) - c, "lit9", (r,)))
    for c in (1, 4, 8):
        out.append(Ev("L1", fill(6, c) + short + fill(5), 6 + c, c, "lit9"))
    out.append(Ev("L1", fill(6, 2) + HG_HEAD + fill(2500, 1) + HG_TAIL + fill(5), 6 + 5, 5, "lit9_long"))
    return tuple(out) + _r3(short) + _r3(HG_HEAD + fill(900, 2) + HG_TAIL) + _l3(short) + _l3(HG_HEAD + fill(1500, 4) + HG_TAIL)


HUGE = (BExpr(r"needle_hg[^\n]{0,5000}thread", 14, HG_HEAD + fill(20, 1) + HG_TAIL, _huge_events(), mode=4),)

SETS = {"literal": ("literal", LITERAL), "always_on_free": ("always_on", AO_FREE), "always_on_ctx": ("always_on", AO_CTX), "huge": ("huge", HUGE)}
NAMES = tuple(SETS)


# ------------------------------------------------------------------ texts and windows
class _Builder:
    def __init__(self, exprs):
        self.exprs = exprs
        self.buf = bytearray()
        self.turn = 0

    def good_line(self, n: int) -> bytes:
        """A line of n bytes, the '\\n' included: filler around one complete match where it fits, the expressions in turn."""
        e = self.exprs[self.turn % len(self.exprs)]
        room = n - 1 - len(e.good)
        if room < (0 if e.bol or e.eol else 2) or (e.bol and e.eol and room):
            return fill(n - 1, n) + b"\n"
        self.turn += 1
        front = 0 if e.bol else room if e.eol else 1 + room // 3
        return fill(front, n) + e.good + fill(room - front, n + 1) + b"\n"

    def pad_to(self, target: int) -> None:
        gap = target - len(self.buf)
        assert gap >= 0, (target, len(self.buf))
        longest = max(len(e.good) for e in self.exprs)
        while gap > 0:
            n = min(gap, longest + 12 + len(self.buf) % 29)
            if 0 < gap - n < 12:
                n = gap if gap <= longest + 60 else n - 12
            self.buf += self.good_line(n)
            gap -= n

    def plant(self, blob: bytes, cut: int, residue: int | None, aligned: bool) -> int:
        """Put the line `blob` so that the offset of blob[cut] has the residue mod 16 (aligned: is a multiple of 16); good
        lines make up the distance.  Returns the offset of blob[cut]."""
        at = len(self.buf) + cut
        want = 0 if aligned else residue
        pad = (want - at) % 16
        if pad:
            pad += 16 * (pad < 2)  # (a pad line needs its newline and is better not empty)
            self.pad_to(len(self.buf) + pad)
        at = len(self.buf) + cut
        assert at % 16 == want
        self.buf += blob if blob.endswith(b"\n") else blob + b"\n"
        return at


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    tier, exprs = SETS[name]
    b = _Builder(exprs)
    b.pad_to(160)
    lefts, rights = [], []
    for ei, e in enumerate(exprs):  # the left events first: the right ones lie more than a tile into the text (R5)
        for ev in e.events:
            if ev.cls in LEFT:
                lefts.append((ev, ei, b.plant(ev.blob, ev.cut, None, True)))
                b.pad_to(len(b.buf) + 100 + 7 * len(lefts) % 50)
    b.pad_to(max(len(b.buf), TILE + ROW + 200))
    for ei, e in enumerate(exprs):
        for ev in e.events:
            if ev.cls in RIGHT:
                for r in ev.residues:
                    rights.append((ev, ei, b.plant(ev.blob, ev.cut, r, False)))
    body_end = len(b.buf)
    assert body_end <= MAX_BODY, (name, body_end)
    b.pad_to(body_end + FRAME + 64)
    data = bytes(b.buf)
    line_starts = [0] + [i + 1 for i in range(len(data) - 1) if data[i] == 10]
    windows = []
    for n, (ev, ei, lo) in enumerate(lefts):
        assert lo % 16 == 0 and lo >= 16
        hi = line_starts[bisect.bisect_left(line_starts, lo + 150 + 61 * (n % 7))]  # a line end: nothing planted at this edge
        windows.append(Window(ev.cls, f"{ev.cls}/{ev.sub}", lo, hi, ev.k, ei, ev.som))
    edge_count = {}
    for n, (ev, ei, hi) in enumerate(rights):
        lo = (hi - max(120 + 53 * (n % 11), ev.cut + 40)) & ~15  # (the event's own line lies inside the window)
        windows.append(Window(ev.cls, f"{ev.cls}/{ev.sub}", lo, hi, ev.k, ei, ev.som))
        d = {15: -1, 0: 0, 1: 1}.get(hi % 16)
        if d is None:
            continue
        for edge, span in (("row", ROW * (1 + n % 3)), ("tile", TILE)):  # hi - lo = span + d: hi at the edge of a row / of the tile
            key = (edge, d, ev.cls)
            if edge_count.get(key, 0) < (2 if edge == "row" else 1) and hi - d - span >= 16:
                edge_count[key] = edge_count.get(key, 0) + 1
                windows.append(Window("R5", f"R5/{edge}{d:+d}:{ev.cls}/{ev.sub}", hi - d - span, hi, ev.k, ei, ev.som))
    assert all(w.lo % 16 == 0 and 16 <= w.lo < w.hi <= body_end for w in windows)
    return Case(name, tier, exprs, data, windows, body_end, line_starts)


# ------------------------------------------------------------------ references
_REF = {}


def reference(name: str, lo: int, hi: int, bs: int = DEFAULT_BS, shared: bool = False, flags=None):
    """(sorted uint64 [n, 5] of (line, id, to, start, len), n_lines) of data[lo:hi] scanned alone (confirm_cells.reference)."""
    key = (name, lo, hi, bs, shared, tuple(flags) if flags else None)
    if key not in _REF:
        c = case(name)
        rows, nlines, _ = cc.reference(c.data[lo:hi], c.patterns, list(flags) if flags else c.flags, c.ids(shared), bs)
        _REF[key] = (rows, nlines)
    return _REF[key]


def window_reference(name: str, w: Window, bs: int = DEFAULT_BS, shared: bool = False, flags=None):
    return reference(name, w.lo, w.hi, bs, shared, flags)


def widened(w: Window) -> tuple:
    """(lo, hi) of the window widened by the leak its class is about."""
    return (w.lo, w.hi + w.k) if w.side == "R" else (w.lo - w.k, w.hi)


def starts_of(c: Case, piece_of, rows) -> list:
    """The leftmost start (brute force over Python `re`) of every row, offsets inside the piece; piece_of(row) -> bytes."""
    out = []
    for r in rows:
        line, rid, to = int(r[0]), int(r[1]), int(r[2])
        e = c.exprs[rid]
        out.append(somsim_py.start_by_brute_force(e.pattern, e.flags, piece_of(r), to))
    return out


def claim(name: str, lo: int, hi: int, origin: int, geometry: bool, som: bool):
    """What a scan of data[lo:hi] says, in the terms a window of the class is judged in, with offsets counted from `origin`
    (the window's own lo, so that the widened scan is re-based): geometry classes all five columns and n_lines; the others the
    set of (match end, id), with the match start where the leak can change nothing else."""
    c = case(name)
    rows, nlines = reference(name, lo, hi)
    shift = lo - origin
    if geometry:
        return ([(int(r[0]), int(r[1]), int(r[2]), int(r[3]) + shift, int(r[4])) for r in rows], nlines)
    ends = [(int(r[3]) + int(r[2]) + shift, int(r[1])) for r in rows]
    if som:
        data = c.data[lo:hi]
        froms = starts_of(c, lambda r: data[int(r[3]):int(r[3]) + int(r[4])], rows)
        ends = [(e, rid, int(r[3]) + f + shift) for (e, rid), r, f in zip(ends, rows, froms)]
    return sorted(ends)


def is_hostile(name: str, w: Window) -> bool:
    geometry = w.base_cls in GEOMETRY
    wlo, whi = widened(w)
    return claim(name, w.lo, w.hi, w.lo, geometry, w.som) != claim(name, wlo, whi, w.lo, geometry, w.som)


def diff_report(c: Case, w: Window, got: np.ndarray, want: np.ndarray, limit: int = 4) -> str:
    rows = lambda a: np.ascontiguousarray(a).view([("", np.uint64)] * 5).ravel()  # noqa: E731
    show = lambda hs: [tuple(int(x) for x in h) for h in hs[:limit]]  # noqa: E731
    return f"{c.what(w)}: {len(got)} hits, want {len(want)}; missing {show(np.setdiff1d(rows(want), rows(got)))}; extra {show(np.setdiff1d(rows(got), rows(want)))}"


def block_reference(c: Case, data: bytes, flags=None, som: bool = False) -> list:
    """Face A's reports of one block, in delivery order (to, id): no expression of the cases matches across a newline or
    tells a line's edge from the block's (every one has MULTILINE), so they are the lines' reports shifted; SINGLEMATCH holds
    for the block.  (id, from, to) with som."""
    flags = flags or c.flags
    rows, _, _ = cc.reference(data, c.patterns, [f & 7 for f in flags], c.ids(False), DEFAULT_BS)  # (every end; SINGLEMATCH below)
    froms = starts_of(c, lambda r: data[int(r[3]):int(r[3]) + int(r[4])], rows) if som else [0] * len(rows)
    out = sorted(((int(r[3]) + int(r[2]), int(r[1]), int(r[3]) + f) for r, f in zip(rows, froms)))
    seen, kept = set(), []
    for to, rid, frm in out:
        if flags[rid] & 8:
            if rid in seen:
                continue
            seen.add(rid)
        kept.append((rid, frm, to) if som else (rid, to))
    return kept


def files_of(c: Case, w: Window):
    """The window as a pack of three files: the pack begins at lo, the last file ends at nbytes == hi (an unterminated last
    line there has no pad behind it: what follows is the base text), the inner cuts are line starts."""
    inner = [s - w.lo for s in c.line_starts if w.lo < s < w.hi]
    cuts = sorted({inner[len(inner) // 3], inner[2 * len(inner) // 3]}) if len(inner) >= 3 else inner[:1]
    starts = [0] + cuts
    return starts, cuts + [w.hi - w.lo]
