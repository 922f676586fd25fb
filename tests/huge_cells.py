"""The routines of the huge automata (hypergrep_amd/csrc/hg_huge.hip: huge_run_reg<1 / 2 / 4>, huge_run with staged tables
and with tables in L2) under their three callers (the always-on kernel, the confirm kernel, block mode) as test cells, the
texts that drive each cell through the word, slab, exception, chunk, condition and caller geometry, and the reference.  Test
infrastructure: imported by test_huge_cells.py and test_huge_cells_gpu.py.

A cell is a small set of expressions plus what hugesim_py must say of each (routine label, state words, ctxfree).  The
routine labels are restated in hugesim_py from huge_stage_words, clamp_stage and huge_prepare:

    reg1 / reg2 / reg4   the tables fit the staging cap and nw <= 64 / 128 / 256: huge_run_reg<K>
    lds_staged           they fit and nw > 256: huge_run on staged tables
    lds_l2               they do not fit: huge_run on the tables in L2

Every planted case carries a tag "class/subcase[:miss|:any]" (":miss": the reference must stay silent for the case's
expression, ":any": not judged, no suffix: it must report):

    word       one live bit that crosses every word edge: repeat counts n - 1, n, n + 1; the body without its head
    slab       the same against the slab edges of huge_run_reg (words 63->64, 127->128, 191->192): the bit dies right behind
               the edge; an exception detour taken while the live bit sits in slab 1, 2, 3
    exc        hits that exist only through an exception edge: into a higher slab, into a lower word, beyond the live words
    chunk      pieces of 1 ... 129 bytes, match ends on the 64th / 65th byte of a 64-byte text chunk and at the end of a piece
               whose length is a multiple of 64, piece starts at many residues mod 64
    ctx        \\b and \\B on both sides, ^ and $, the end of the text without a newline
    always_on  (tier 1) line starts at every residue mod 64, empty lines, tile edges, the NUL rules, forced breaks
    confirm    (tier 0) the literal 1 ... 200 bytes behind its line start, carried lines, overlapping literals, pieces k > 0
    block      (hs_scan) the buffer as one unit: BLOCKS of the cell

Filler bytes come from confirm_cells.FILLER (no word byte); the long bodies come from BODY, which holds none of the letters
the expressions use as heads and tails, so a planted case is judged on its own.

clamp_stage below huge_stage_words: the cap shrinks when 2 * huge_max_nw + huge_stage_words exceeds the 40896 words of
clamp_stage's room.  huge_stage_words is at most 12288, so huge_max_nw would have to exceed 14304 words = 457 728 nodes, and
the compiler bounds an expression by 400 000 Thompson instructions (HG_HUGE_MAX_PROGRAM), each node taking at least one:
the largest automaton kept here (a{32767} x 12, 12288 words) leaves 16320 words, more than any staged table.  No compilable
set reaches the clamp, so there is no such cell; test_huge_cells.py::test_clamp_is_out_of_reach holds the arithmetic."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import confirm_cells as cc
from confirm_cells import FILLER, diff_report, diff_tags, fill, reference, sort_hits  # noqa: F401  (re-exported for the tests)

TILE = cc.TILE
DEFAULT_BS = cc.DEFAULT_BS
MAX_TEXT = 8 * TILE  # 128 KiB
BREAK_BS1 = (63, 100, 512, 4096, 16384, 20000)  # buffer_size - 1 of the forced-break texts
CLASSES = ("word", "slab", "exc", "chunk", "ctx", "always_on", "confirm", "block")
BODY = b"bcdefghijlmnoprstuvw"  # no a (the monster), no head or tail letter of any expression
MONSTER = "a{32767}" * 12  # the largest automaton kept in the suite: 393 204 nodes, 12288 state words


@functools.lru_cache(maxsize=None)
def body(n: int, salt: int = 0) -> bytes:
    """n lower-case letters of BODY, deterministic."""
    return bytes(BODY[(i * 7 + salt * 5 + (i >> 4)) % len(BODY)] for i in range(n))


def digits(n: int, salt: int = 0) -> bytes:
    return bytes(b"0123456789"[(i * 3 + salt + (i >> 3)) % 10] for i in range(n))


@dataclass(frozen=True)
class Expr:
    pattern: str
    flags: int
    routine: str  # what hugesim_py must say ("" for an expression that is not huge)
    ctxfree: bool
    samples: tuple  # (tag, line bytes without the newline)
    nw: int = 0  # exact state words (0: not asserted)
    short: tuple = ()  # (head, tail): head + up to 40 arbitrary bytes + tail is a match (the geometry sweeps plant these)
    lit: bytes = b""  # tier 0: the required literal
    shape: str = ""  # "walk", "dense", "exc", "loop", "init", "idle"
    needs: tuple = ()  # what hugesim_py must also say: "lower", "crosses_slab", "sources", "beyond"


def walk(head: str, n: int, tail: str, routine: str, nw: int = 0, flags: int = 14, lit: bytes = b"") -> Expr:
    """One live bit: head [a-z]{n} tail."""
    h, t = head.encode(), tail.encode()
    s = [("word/n", fill(3) + h + body(n) + t + fill(2)), ("word/n-1:miss", h + body(n - 1) + t), ("word/n+1:miss", fill(1) + h + body(n + 1) + t),
         ("word/headless:miss", body(n + 40, 3) + t), ("word/twice", h + body(n, 1) + t + h + body(n, 2) + t)]
    words = (n + 2 + len(head) - 1 + len(tail) - 1 + 31) // 32
    for k in range(1, (words - 1) // 64 + 1):  # the bit dies on the first node of slab k, and one node in front of it
        at = 64 * 32 * k - len(head)  # body bytes consumed when the live bit sits on node 2048 k
        s.append((f"slab/dies_behind_{64 * k - 1}-{64 * k}:miss", h + body(at, k) + b"#" + body(n - at - 1, k) + t))
        s.append((f"slab/dies_before_{64 * k - 1}-{64 * k}:miss", h + body(at - 1, k) + b"#" + body(n - at, k) + t))
        s.append((f"slab/crosses_{64 * k - 1}-{64 * k}", fill(k) + h + body(n, 3 + k) + t))
    return Expr(f"{head}[a-z]{{{n}}}{tail}", flags, routine, True, tuple(s), nw=nw, lit=lit, shape="walk")


def dense(head: str, n: int, tail: str, routine: str, nw: int = 0, flags: int = 6, lit: bytes = b"", ctx: bool = False) -> Expr:
    """Every bit live: head .{0,n} tail; the head's exception edge reaches every word (beyond the live ones).  ctx: \\b on both
    sides (head and tail are word bytes)."""
    h, t = head.encode(), tail.encode()
    s = [("exc/beyond_live_words", fill(2) + h + t + fill(2)), ("exc/higher_slab", fill(1) + h + fill(n, 1) + t + fill(1)), ("exc/higher_slab:miss", h + fill(n + 1, 2) + t),
         ("word/all_live", h + fill(300) + t + fill(7) + t + fill(2)), ("word/all_live:miss", h + fill(300) + t[:-1] if len(t) > 1 else fill(9) + t)]
    if ctx:
        s += [("ctx/\\b_left:miss", b"b" + h + fill(4) + t), ("ctx/\\b_right:miss", h + fill(4) + t + b"_"), ("ctx/\\b_both", fill(2) + h + fill(4) + t)]
    pat = f"{head}.{{0,{n}}}{tail}"
    return Expr(f"\\b{pat}\\b" if ctx else pat, flags, routine, not ctx, tuple(s), nw=nw, short=(h, t), lit=lit, shape="dense", needs=("beyond", "sources"))


def slabexc(head: str, seg: int, nseg: int, tail: str, routine: str) -> Expr:
    """head ([a-z]{seg}(?:AB|CD)){nseg} [a-z]{90} tail: the entry of C and the exit of B are exception edges, one pair per
    junction, junction k in slab k."""
    h, t = head.encode(), tail.encode()

    def line(choice, salt=0):
        return h + b"".join(body(seg, salt + k) + c for k, c in enumerate(choice)) + body(90, salt) + t

    s = [("slab/exc_all_AB", line([b"AB"] * nseg))]
    for k in range(nseg):
        pick = [b"AB"] * nseg
        pick[k] = b"CD"
        s.append((f"slab/exc_in_slab{k + 1}", fill(2) + line(pick, k)))
        pick[k] = b"AD"
        s.append((f"slab/exc_in_slab{k + 1}:miss", line(pick, k)))
        pick[k] = b"CB"
        s.append((f"slab/exc_in_slab{k + 1}_CB:miss", line(pick, k)))
    return Expr(head + f"[a-z]{{{seg}}}(?:AB|CD)" * nseg + "[a-z]{90}" + tail, 14, routine, True, tuple(s), shape="exc", needs=("sources",))


def optional(n: int, routine: str) -> Expr:
    """x(ab?c?){n}y: two exception sources per repeat, target ranges of two words, some across a slab edge."""
    def reps(k, salt=0):
        return b"".join((b"a", b"ab", b"ac", b"abc")[(i * 5 + salt + (i >> 2)) % 4] for i in range(k))

    s = [("exc/heavy", fill(2) + b"x" + reps(n) + b"y"), ("exc/heavy_all_a", b"x" + b"a" * n + b"y"), ("exc/heavy_n-1:miss", b"x" + reps(n - 1) + b"y"),
         ("exc/heavy_n+1:miss", b"x" + reps(n + 1, 1) + b"y"), ("exc/heavy_broken:miss", b"x" + reps(n // 2) + b"abb" + reps(n - n // 2 - 1, 2) + b"y")]
    return Expr(f"x(ab?c?){{{n}}}y", 14, routine, True, tuple(s), shape="exc", needs=("sources", "crosses_slab"))


def alternation(n: int, routine: str) -> Expr:
    """(abc|def){n}!: an exception edge every third byte, in every word."""
    def reps(k, salt=0):
        return b"".join((b"abc", b"def")[((i * 3 + salt) >> 1) & 1] for i in range(k))

    s = [("exc/every_third_byte", fill(2) + reps(n) + b"!"), ("exc/every_third_byte_abc", b"abc" * n + b"!"), ("exc/every_third_byte_def", b"#" + b"def" * n + b"!"),
         ("exc/every_third_byte_n-1:miss", b"#" + reps(n - 1) + b"!"), ("exc/every_third_byte_broken:miss", reps(n // 2) + b"abd" + reps(n - n // 2 - 1) + b"!")]
    return Expr(f"(abc|def){{{n}}}!", 14, routine, True, tuple(s), shape="exc", needs=("sources",))


def loop(n: int, routine: str) -> Expr:
    """(?:k[0-9]{n}-){2,}z: the loop's edge leads back to a lower word."""
    def reps(k, salt=0):
        return b"".join(b"k" + digits(n, salt + i) + b"-" for i in range(k))

    s = [("exc/lower_word_2", fill(2) + reps(2) + b"z"), ("exc/lower_word_3", reps(3, 1) + b"z"), ("exc/lower_word_5", fill(1) + reps(5, 2) + b"z"), ("exc/lower_word_1:miss", reps(1) + b"z"),
         ("exc/lower_word_broken:miss", reps(2) + b"k" + digits(n - 1) + b"-z")]
    return Expr(f"(?:k[0-9]{{{n}}}-){{2,}}z", 14, routine, True, tuple(s), shape="loop", needs=("sources", "lower"))


def allinit(n: int, routine: str) -> Expr:
    """(a?){n}b: no exception edge, every word holds start nodes (init_hi = nw)."""
    s = [("word/every_init", b"ca" * 3 + b"a" * n + b"b"), ("word/every_init_short", fill(3) + b"aab" + fill(3) + b"b"), ("word/every_init:miss", b"a" * 80 + b"c")]
    return Expr(f"(a?){{{n}}}b", 6, routine, True, tuple(s), short=(b"", b"b"), shape="init")


def ctx_bol_wb(head: str, n: int, routine: str, nw: int = 0) -> Expr:
    """^head[a-z]{n}\\b with MULTILINE."""
    h = head.encode()
    s = [("ctx/^_piece_start+\\b_right", h + body(n) + b"#" + fill(3)), ("ctx/^_behind_bytes:miss", b"#" + h + body(n) + b"#"), ("ctx/\\b_right:miss", h + body(n, 1) + b"_"),
         ("ctx/^+\\b_before_newline", h + body(n, 2))]
    return Expr(f"^{head}[a-z]{{{n}}}\\b", 14, routine, False, tuple(s), nw=nw, shape="walk")


def ctx_nwb_eol(head: str, n: int, routine: str, nw: int = 0) -> Expr:
    """\\Bhead[a-z]{n}$ without MULTILINE: $ is taken before a final newline and at the end."""
    h = head.encode()
    s = [("ctx/\\B_left+$_before_final_newline", fill(2) + b"b" + h + body(n)), ("ctx/\\B_left:miss", fill(2) + h + body(n, 1)), ("ctx/$_bytes_behind:miss", b"b" + h + body(n, 2) + b"#")]
    return Expr(f"\\B{head}[a-z]{{{n}}}$", 10, routine, False, tuple(s), nw=nw, shape="walk")


def ctx_wb_nwb(head: str, n: int, routine: str, nw: int = 0) -> Expr:
    """\\bhead[a-z]{n}\\B. : \\b on the left, \\B on the right."""
    h = head.encode()
    s = [("ctx/\\b_left+\\B_right", fill(2) + h + body(n) + b"_" + fill(2)), ("ctx/\\b_left:miss", b"b" + h + body(n, 1) + b"_"), ("ctx/\\B_right:miss", fill(1) + h + body(n, 2) + b"#")]
    return Expr(f"\\b{head}[a-z]{{{n}}}\\B.", 14, routine, False, tuple(s), nw=nw, shape="walk")


def classes_walk(head: str, ranges, n: int, tail: str, routine: str, ctx: bool, nw: int = 0) -> Expr:
    """head [r0]{n} [r1]{n} ... tail: one byte class per range, so that the tables outgrow the staging area."""
    h, t = head.encode(), tail.encode()

    def line(counts, salt=0):
        return h + b"".join(bytes(ord(r[0]) + (i * 3 + salt + k) % (ord(r[-1]) - ord(r[0]) + 1) for i in range(c)) for k, (r, c) in enumerate(zip(ranges, counts))) + t

    full = [n] * len(ranges)
    s = [("word/n", fill(2) + line(full) + fill(2)), ("word/n-1:miss", fill(2) + line(full[:-1] + [n - 1]) + fill(2)), ("word/n+1:miss", fill(2) + line([n + 1] + full[1:], 1) + fill(2)),
         ("word/headless:miss", line(full, 2)[len(h):] + fill(1))]
    if ctx:
        s += [("ctx/\\b_left:miss", b"_" + line(full, 3) + fill(2)), ("ctx/\\b_right:miss", fill(2) + line(full, 4) + b"_"), ("ctx/\\b_both", line(full, 5))]
    pat = head + "".join(f"[{r[0]}-{r[-1]}]{{{n}}}" for r in ranges) + tail
    return Expr(f"\\b{pat}\\b" if ctx else pat, 14, routine, not ctx, tuple(s), nw=nw, shape="walk")


def monster() -> Expr:
    """Its literal (a run of a) occurs once, in a short line: the automaton is staged, runs a few bytes and dies."""
    return Expr(MONSTER, 14, "lds_l2", True, (("word/idle_monster:miss", fill(3) + b"a" * 48 + fill(3)),), nw=12288, lit=b"a" * 8, shape="idle")


@dataclass(frozen=True)
class Cell:
    name: str
    tier: int  # of every huge expression but the monster (tier 0)
    exprs: tuple
    excluded: dict = field(default_factory=dict)  # class -> why the cell does not plant it
    floor: int = 0  # reports of the reference over all texts, sizes and both id modes: at least this many (profiles/huge_cells.txt)

    @property
    def patterns(self):
        return [e.pattern for e in self.exprs]

    @property
    def flags(self):
        return [e.flags for e in self.exprs]

    def ids(self, shared: bool):
        return [0] * len(self.exprs) if shared else list(range(len(self.exprs)))

    @property
    def short(self):
        """The expression the geometry sweeps plant: the first with short matches."""
        return next(i for i, e in enumerate(self.exprs) if e.short and e.short[0])


ONE_SLAB = "the automata have one slab of 64 words"
NO_CTX = "no member with boundary conditions: the issue asks for them in reg2, reg4, lds_staged and lds_l2"
NOT_T0 = "a cell of the always-on tier"
NOT_T1 = "a cell of the literal-anchored tier"
FIVES = ("ae", "fj", "ko", "pt", "uy", "04", "59", "AE", "FJ", "KO", "PT")  # (narrower classes give the compiler a required literal)

CELLS = [
    # -- routine and size, under the always-on caller.  Each cell: a SINGLEMATCH walk, an all-matches dense member (the one the
    #    geometry sweeps plant), and from reg2 on three members with boundary conditions
    Cell("ao_reg1_64", 1, (walk("q", 2015, "X", "reg1", nw=64), dense("Q", 2030, "Z", "reg1", nw=64)), {"slab": ONE_SLAB, "ctx": NO_CTX, "confirm": NOT_T0}, floor=318),
    Cell("ao_reg2", 1, (walk("q", 2047, "X", "reg2", nw=65), dense("Q", 4090, "Z", "reg2", nw=128), ctx_bol_wb("K", 4093, "reg2", nw=128), ctx_nwb_eol("L", 2100, "reg2"),
                        ctx_wb_nwb("M", 2060, "reg2", nw=65)), {"confirm": NOT_T0}, floor=328),
    Cell("ao_reg4", 1, (walk("q", 4095, "X", "reg4", nw=129), dense("Q", 8186, "Z", "reg4", nw=256), ctx_bol_wb("K", 4200, "reg4"), ctx_nwb_eol("L", 4100, "reg4", nw=129),
                        ctx_wb_nwb("M", 6200, "reg4")), {"confirm": NOT_T0}, floor=330),
    Cell("ao_reg4_256", 1, (walk("q", 8190, "X", "reg4", nw=256), slabexc("J", 2100, 3, "Y", "reg4"), dense("Q", 4200, "Z", "reg4")), {"ctx": "the conditions of reg4 are in ao_reg4", "confirm": NOT_T0}, floor=332),
    Cell("ao_exc", 1, (optional(1500, "reg4"), loop(1500, "reg4"), allinit(1100, "reg1"), dense("Q", 2100, "Z", "reg2")),
         {"slab": "the slab cases are in ao_reg4_256", "ctx": "an exception cell: the conditions are in the routine cells", "confirm": NOT_T0}, floor=7832),
    Cell("ao_lds_staged", 1, (walk("q", 8191, "X", "lds_staged", nw=257), dense("Q", 8200, "Z", "lds_staged", nw=257), ctx_bol_wb("K", 8200, "lds_staged", nw=257),
                              ctx_nwb_eol("L", 8200, "lds_staged"), ctx_wb_nwb("M", 8250, "lds_staged")), {"confirm": NOT_T0}, floor=334),
    # the tables do not fit: boundary conditions and ten byte classes at 256 words; fourteen classes without conditions at 647
    # words (20 682 nodes: what it takes to outgrow the staging area without conditions); conditions at 313 words
    Cell("ao_lds_l2", 1, (classes_walk("J", ("af", "gm", "nz", "04", "59", "AF"), 1360, "K", "lds_l2", True, nw=256), classes_walk("V", FIVES, 1880, "W", "lds_l2", False, nw=647),
                          dense("Q", 9990, "Z", "lds_l2", ctx=True), ctx_nwb_eol("L", 9990, "lds_l2"), ctx_bol_wb("K", 9800, "lds_l2"), ctx_wb_nwb("M", 9700, "lds_l2")),
         {"slab": "huge_run has no slabs: a lane strides over the words", "confirm": NOT_T0}, floor=330),
    # -- restage: three always-on routines in one set (the always-on kernel restages for every piece), with the monster: S and T
    #    sit 12288 words apart
    Cell("ao_restage", 1, (dense("Q", 2030, "Z", "reg1", nw=64), walk("J", 8000, "Y", "reg4"), walk("q", 8300, "X", "lds_staged"), monster()),
         {"ctx": "a restage cell: the conditions are in the routine cells", "confirm": NOT_T0}, floor=336),
    # -- the same mixture literal-anchored: the confirm kernel restages on a change of expression
    Cell("cf_restage", 0, (dense("nenenenene", 2010, "end_r", "reg1", nw=64, lit=b"nenenenene"), walk("needle_rb_2", 8000, "Y", "reg4", lit=b"needle_rb_2"),
                           walk("needle_rc_3", 8300, "X", "lds_staged", lit=b"needle_rc_3"), alternation(700, "reg4")),
         {"ctx": "a restage cell: the conditions under the confirm caller are in confirm_cells (huge, huge_reg2, huge_reg4, huge_lds)", "always_on": NOT_T1}, floor=216),
]
BY_NAME = {c.name: c for c in CELLS}


@functools.lru_cache(maxsize=None)
def compiled(name: str) -> dict:
    import hugesim_py

    cell = BY_NAME[name]
    return hugesim_py.placement(cell.patterns, cell.flags, cell.ids(False))


def placement_errors(cell: Cell, pl: dict) -> list:
    """What hugesim_py's placement of the cell's expressions gets wrong; [] when it is right."""
    bad = []
    for i, e in enumerate(cell.exprs):
        p = pl["exprs"].get(i)
        if p is None:
            bad.append((e.pattern[:40], "not huge"))
            continue
        tier = 0 if e.shape == "idle" or e.lit or e.pattern.startswith("(abc|def)") else cell.tier
        if (p["tier"], p["mode"] if tier == 0 else 4) != (tier, 4):
            bad.append((e.pattern[:40], "tier/mode", p["tier"], p["mode"]))
        if p["routine"] != e.routine or p["ctxfree"] != e.ctxfree or (e.nw and p["nw"] != e.nw):
            bad.append((e.pattern[:40], "routine/ctxfree/nw", p["routine"], p["ctxfree"], p["nw"]))
        if p["single"] != bool(e.flags & 8):
            bad.append((e.pattern[:40], "single", p["single"]))
        need = {"lower": p["lower"], "crosses_slab": p["crosses_slab"], "sources": p["nsources"] > 0, "beyond": p["widest"] >= p["nw"] - 1}
        bad += [(e.pattern[:40], what) for what in e.needs if not need[what]]
        if e.shape == "init" and p["init_hi"] != p["nw"]:
            bad.append((e.pattern[:40], "init_hi", p["init_hi"]))
    return bad


# ------------------------------------------------------------------ texts
Text, Case = cc.Text, cc.Case


class _Builder(cc._Builder):  # pylint: disable=protected-access
    def room(self, n: int) -> bool:
        return len(self.buf) + n + 64 <= MAX_TEXT

    def text(self) -> Text:
        assert len(self.buf) <= MAX_TEXT, (self.label, len(self.buf))
        return Text(self.label, bytes(self.buf), self.sizes, self.cases)

    def plant64(self, tag, blob, expr, residue=None, newline=True, at=None, line_in=0):
        """The blob's first byte at the next offset with the given residue mod 64 (or at `at`)."""
        lo = len(self.buf) if at is None else at
        if residue is not None:
            lo += (residue - lo) % 64
        self.plant(tag, blob, 0, expr, fs_abs=lo, newline=newline, line_in=line_in)


def _sample_texts(cell: Cell) -> list:
    """Every sample of every expression on a line of its own, at changing residues mod 64; a text that is full is closed."""
    texts = []

    def builder():
        nb = _Builder(f"samples{len(texts)}", (DEFAULT_BS,))
        nb.buf += fill(30 + 7 * len(texts), 2) + b"\n"
        return nb

    b, k = builder(), 0
    last = None
    for ei, e in enumerate(cell.exprs):
        for tag, blob in e.samples:
            if tag == "ctx/^+\\b_before_newline":
                last = (tag, blob, ei)
            if not b.room(len(blob) + 160):
                texts.append(b.text())
                b = builder()
            b.plant64(tag, blob, ei, residue=(k * 23 + 5) % 64)
            k += 1
    # the end of the text without a newline: $ and \b at the end (the ctx members), else a sample of the first expression
    tag, blob, ei = last or (cell.exprs[0].samples[0][0], cell.exprs[0].samples[0][1], 0)
    eol = next(((t, s, i) for i, e in enumerate(cell.exprs) for t, s in e.samples if t.startswith("ctx/\\B_left+$")), None)
    if eol:
        tag, blob, ei = "ctx/$_at_the_end_without_newline", eol[1], eol[2]
    elif last:
        tag = "ctx/\\b_at_the_end_without_newline"
    if not b.room(len(blob) + 160):
        texts.append(b.text())
        b = builder()
    b.plant64(tag, blob, ei, residue=17, newline=False)
    texts.append(b.text())
    return texts


def _short(cell: Cell, gap: int, salt: int = 0) -> bytes:
    h, t = cell.exprs[cell.short].short
    return h + fill(gap, salt) + t


def _chunk_text(cell: Cell) -> Text:
    """Short pieces: the 64-byte text chunks of a run (lane l of the wave holds byte i0 + l)."""
    b = _Builder("chunk", (DEFAULT_BS,))
    ei = cell.short
    h, t = cell.exprs[ei].short
    n0 = len(h) + len(t)
    b.buf += fill(20, 1) + b"\n"
    k = 0
    for length in (1, 2, 63, 64, 65, 127, 128, 129):  # the scanned piece is the line and its newline: `length` bytes, and `length` + 1
        for line_len in (length - 1, length):
            if line_len >= n0:  # the match ends on the line's last byte
                b.plant64(f"chunk/piece_of_{length}_bytes", fill(line_len - n0, k) + h + t, ei, residue=(k * 11) % 64)
            elif line_len > 0:
                b.plant64(f"chunk/piece_of_{length}_bytes:miss", fill(line_len, k), ei, residue=(k * 11) % 64)
            else:
                b.plant64(f"chunk/piece_of_{length}_bytes:miss", b"", ei, residue=(k * 11) % 64)
            k += 1
    for end in (63, 64, 65, 127, 128, 129, 192):  # the match ends on byte `end` of the piece (1-based): the last of a chunk, the first of the next
        b.plant64(f"chunk/match_ends_on_byte_{end}", fill(end - n0, end) + h + t + fill(9, 1), ei, residue=(end * 7) % 64)
        b.plant64(f"chunk/tail_cut_at_byte_{end}:miss", fill(end - n0, end) + h + t[:-1], ei, residue=(end * 5) % 64)
    for length in (64, 128, 256):  # the match ends with the piece, whose length is a multiple of 64 (no newline inside: the next line's)
        b.plant64(f"chunk/ends_piece_of_{length}", fill(length - 1 - n0, 3) + h + t, ei, residue=length % 61)
    for r in range(0, 64, 3):  # piece starts at many residues of the buffer offset
        b.plant64(f"chunk/start_residue_{r}", _short(cell, 3 + r % 5, r) + fill(4), ei, residue=r)
    return b.text()


def _always_on_texts(cell: Cell) -> list:
    ei = cell.short
    h, t = cell.exprs[ei].short
    out = []
    b = _Builder("lines", (DEFAULT_BS,))
    for r in range(64):  # a line start at every residue mod 64
        b.plant64("always_on/line_start_residue", _short(cell, r % 7, r), ei, residue=r)
    for r in (0, 20, 50):  # several line starts and empty lines inside one 64-byte group
        b.plant64("always_on/starts_in_one_group", b"\n\n" + _short(cell, 1) + b"\n\n" + fill(2) + b"\n" + _short(cell, 0) + b"\n\n" + _short(cell, 2), ei, residue=r)
        b.plant64("always_on/starts_in_one_group:miss", b"\n" + h + b"\n" + t + b"\n\n" + fill(3), ei, residue=r + 7)
    # the NUL rules
    b.plant64("always_on/nul_leading", b"\0\0\0" + _short(cell, 4), ei, residue=9)
    b.plant64("always_on/nul_leading_70", b"\0" * 70 + _short(cell, 4), ei, residue=33)
    b.plant64("always_on/nul_ends_the_scanned_bytes:miss", h + fill(3) + b"\0" + t, ei, residue=13)
    b.plant64("always_on/nul_behind_the_match", _short(cell, 2) + b"\0" + fill(4), ei, residue=61)
    b.plant64("always_on/piece_of_nuls:miss", b"\0" * 66, ei, residue=63)
    b.plant64("always_on/nuls_then_newline:miss", b"\0\0\n" + h, ei, residue=62)
    b.plant64("always_on/nuls_then_newline_then_match", b"\0\0\n" + _short(cell, 1), ei, residue=1, line_in=3)
    # tile edges
    b.pad_to(TILE)
    b.plant64("always_on/line_at_first_byte_of_tile", _short(cell, 5) + fill(3), ei)
    b.plant64("always_on/carried_over_one_tile_edge", fill(TILE - 200, 1) + _short(cell, 6), ei, at=2 * TILE - 500)
    b.pad_to(3 * TILE)  # the '\n' of the last filler line is the last byte of tile 2
    b.plant64("always_on/newline_last_byte_of_tile", _short(cell, 2), ei)
    b.pad_to(4 * TILE - 30)
    b.buf += fill(30, 4) + b"\n"  # this '\n' is the first byte of tile 4
    b.plant64("always_on/newline_first_byte_of_tile", _short(cell, 3), ei)
    b.plant64("always_on/carried_over_two_tile_edges", fill(2 * TILE - 300, 2) + _short(cell, 7), ei, at=5 * TILE - 100)
    b.plant64("always_on/no_final_newline_last_tile_partial", fill(5) + _short(cell, 8), ei, newline=False)
    out.append(b.text())
    for label, data in (("one_byte", t[-1:] if len(t) == 1 else b"Q"), ("one_newline", b"\n"), ("one_nul", b"\0")):
        tb = _Builder(label, (DEFAULT_BS, 64))
        tag = "always_on/one_byte_text" + ("" if label == "one_byte" and cell.exprs[ei].short[0] == b"" else ":miss")
        tb.plant(tag, data, 0, ei, newline=False)
        out.append(tb.text())
    n0 = len(h) + len(t)
    for bs1 in BREAK_BS1:  # forced breaks: the line's pieces start every bs1 bytes
        made = []

        def line(tag, end, pieces=0, salt=0, bs1=bs1, made=made):
            """A line whose match ends `end` bytes behind the start of its piece number `pieces`; a text that is full is closed."""
            at = pieces * bs1 + end - n0
            if not made or not made[-1].room(at + n0 + 200):
                made.append(_Builder(f"break{bs1}_{len(made)}", (bs1 + 1,)))
                made[-1].buf += fill(min(30, bs1 - 1), 2) + b"\n"
            made[-1].plant64(tag, fill(at, salt) + h + t + fill(12, 1), ei, residue=(end + pieces) % 64)

        line("always_on/break_match_on_second_piece", min(40, bs1 - 2), 1, 1)
        line("always_on/break_match_on_third_piece", min(50, bs1 - 1), 2, 2)
        line("always_on/break_inside_match:miss", 1, 1, 3)
        line("always_on/break_one_byte_behind_match_end", bs1 - 1, 0, 4)  # the match's last byte is the piece's last but one
        line("always_on/break_at_match_end", bs1, 0, 5)  # ... is the piece's last
        line("always_on/break_one_byte_before_match_end:miss", bs1 + 1, 0, 6) if n0 > 1 else line("always_on/break_one_byte_before_match_end", bs1 + 1, 0, 6)
        out += [m.text() for m in made]
    return out


def _confirm_texts(cell: Cell) -> list:
    ei = cell.short
    e = cell.exprs[ei]
    h, t = e.short
    out = []
    b = _Builder("confirm", (DEFAULT_BS, 101))
    b.buf += fill(40, 1) + b"\n"
    for back in (1, 63, 64, 65, 200):  # the backward walk of wave_line_start
        for r in (0, 31, 63):
            b.plant64(f"confirm/literal_{back}_behind_line_start", fill(back, r) + _short(cell, 3), ei, residue=r)
    b.plant64("confirm/literal_several_times", h + fill(2) + h + fill(3) + t + fill(2) + h + t, ei, residue=5)
    b.plant64("confirm/literal_overlaps_itself", h[:2] * 5 + h + fill(2) + t + fill(1), ei, residue=40)
    b.plant64("confirm/literal_several_times:miss", h + fill(2) + h + fill(3) + t[:-1], ei, residue=50)
    b.plant64("confirm/piece_k_gt_0", fill(230, 3) + _short(cell, 4) + fill(10), ei, residue=9)
    b.plant64("confirm/line_from_previous_tile", fill(300, 1) + _short(cell, 5), ei, at=TILE - 150)
    b.plant64("confirm/line_from_two_tiles_back", fill(TILE + 500, 2) + _short(cell, 6), ei, at=3 * TILE - 300)
    b.plant64("confirm/line_at_tile_start", _short(cell, 2), ei, at=5 * TILE)
    b.plant64("confirm/match_ends_the_text", fill(6) + _short(cell, 3), ei, newline=False)  # accepted at the end of the unit
    out.append(b.text())
    return out


@functools.lru_cache(maxsize=None)
def cell_texts(name: str) -> tuple:
    cell = BY_NAME[name]
    texts = _sample_texts(cell) + [_chunk_text(cell)]
    texts += _always_on_texts(cell) if cell.tier == 1 else _confirm_texts(cell)
    assert all(len(t.data) <= MAX_TEXT for t in texts)
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def cell_blocks(name: str) -> tuple:
    """Block mode: (label, block).  A sample that reports and one that does not of every expression, the chunk text, and a
    block that ends with a match, as one unit each (newlines are ordinary bytes: ^ and $ with and without MULTILINE in mid-buffer), and for cf_restage a block from
    which one literal-anchored expression's literal is absent (it is skipped through pattern_flags)."""
    cell = BY_NAME[name]
    lines = []
    for e in cell.exprs:  # of every expression its first sample that must report and its first that must not
        lines += [next(s for t, s in e.samples if expectation(t) == want) for want in ("hit", "miss") if any(expectation(t) == want for t, _ in e.samples)]
    samples = b"\n".join(lines) + b"\n"
    blocks = [("samples", samples), ("chunk", next(t for t in cell_texts(name) if t.label == "chunk").data)]
    tail = (("literal_absent", None),) if cell.name == "cf_restage" else ()
    if cell.name == "cf_restage":
        lit = cell.exprs[2].lit
        assert lit and lit in samples
        blocks.append(("literal_absent", samples.replace(lit, b"#" * len(lit))))
    assert len(blocks) == 2 + len(tail)
    blocks.append(("match_ends_the_block", fill(7) + _short(cell, 3)))  # no byte behind the match: accepted at the end of the unit
    return tuple(blocks)


# ------------------------------------------------------------------ reference
_REF = {}


def cell_reference(name: str, text_index: int, buffer_size: int, shared: bool):
    """(sorted rows of (line, id, to, start, len), n_lines, the oracle's own rows), cached."""
    key = (name, text_index, buffer_size, shared)
    if key not in _REF:
        cell = BY_NAME[name]
        _REF[key] = reference(cell_texts(name)[text_index].data, cell.patterns, cell.flags, cell.ids(shared), buffer_size)
    return _REF[key]


_BLOCK_REF = {}


def block_reference(name: str):
    """The oracle's libhs on the cell's blocks, with the driver of the Face A tests: [[(id, to), ...] per block]."""
    if name not in _BLOCK_REF:
        import ctypes
        import os

        import oracle_py
        import test_gpu_parity as tg

        oracle_py.lib()  # (builds the oracle)
        cell = BY_NAME[name]
        oracle = ctypes.CDLL(os.path.join(oracle_py.ORACLE_DIR, "_build", "libhs.so.5"))
        _BLOCK_REF[name] = tg._hs_events(oracle, cell.patterns, cell.flags, cell.ids(False), [blk for _, blk in cell_blocks(name)])  # pylint: disable=protected-access
    return _BLOCK_REF[name]


def expectation(tag: str) -> str:
    return "miss" if tag.endswith(":miss") else "any" if tag.endswith(":any") else "hit"


def judged(cell: Cell, text: Text, want: np.ndarray) -> list:
    """[(case, expectation, reported)] of the text's cases against reference rows with distinct ids: a case is reported when a
    row of its expression starts inside its bytes."""
    out = []
    for c in text.cases:
        rows = want[(want[:, 1] == c.expr) & (want[:, 3] >= c.lo) & (want[:, 3] < max(c.hi, c.lo + 1))]
        out.append((c, expectation(c.tag), len(rows) > 0))
    return out
