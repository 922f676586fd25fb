"""The routines of the always-on tier as test cells (hypergrep_amd/csrc/hg_always_on.hip), the texts that drive each cell
through the segment, lead-in and break geometry of the segment-parallel kernel, and the reference.  Test infrastructure:
imported by test_always_on_cells.py, test_always_on_cells_gpu.py and gpu_cases.py.

A cell is a small set of expressions without a usable required literal that the compiler and always_on_stage must place in
one routine: always_on_word<CTX, NT> (lean steps, or ao_exact_dword wave-wide), a group (HgSlowGroup), always_on_word2,
always_on_segment<2, false>, or the scalar hg_always_on_kernel.  Cell.units says what aosim_py.placement must report.
Every cell's texts plant cases of these geometry classes (segment = a lane's 256 bytes [lo, lo + 256) of a 16 KiB tile):

    seg     the match end at every residue mod 64 and at the segment offsets 0..4 and 253..256, the match split across a lane
            boundary at every split, a match of the full max_len that starts at the lane's first lead-in byte, its near miss
    tile    the same splits across a tile edge, lines carried in from one and two tiles back, a line at the tile's first byte,
            newlines as first / last byte of a segment and of a tile, line starts at every residue mod 64 (unbounded units)
    edge    byte 0, no final newline, lengths that are no multiple of 16 and exact multiples of 256 and of 16384, short texts
    nul     the NUL rules: leading NULs, a NUL inside / behind a match, a NUL that blocks its line, NULs in the lead-in
    break   forced breaks of over-long lines at every buffer_size of BREAK_BS1
    single  two matches on one line: the same segment, adjacent segments, far apart, different tiles
    long    (unbounded units) lines of 700, 5000 and 40960 bytes with a match at their end, a long line from mid-tile
    dense   (group_cf) an all-matches member reporting on nearly every byte: the workgroup's note list overflows

Each planted case carries a tag "class/subcase".  Filler bytes come from FILLER: no word byte, no letter, no digit, so no
expression of a cell matches across them and a planted case is judged on its own.

The reference is the oracle's (line, id, to) with the (start, len) of invert_ref.pieces: five columns, as
Scanner.hits_array() gives them.  wave_is_careful() replicates the kernel's lean / exact decision per tile; it labels
reference hits for the floors and never takes part in computing expected hits."""
from __future__ import annotations

import bisect
import functools
from dataclasses import dataclass, field

import numpy as np

from confirm_cells import DEFAULT_BS, FILLER, MAX_TEXT, TILE, diff_report, diff_tags, fill, reference, sort_hits  # noqa: F401

SEG = 256
FAST_MAX_LEN = 64  # HG_ALWAYS_ON_FAST_MAX_LEN
CAREFUL_BS = 400  # a buffer_size whose bs1 (399) is below the 512 of the `careful` predicate: every wave takes the exact routine
BREAK_BS1 = (63, 100, 511, 512, 513, 1000, 4096, 16384, 20000)  # buffer_size - 1 of the forced-break texts
CLASSES = ("seg", "tile", "edge", "nul", "break", "single", "long", "dense")
LEAN_CLASSES = ("seg", "tile", "nul", "single")  # each reported in a lean and in a careful tile, where the cell has a lean path


@dataclass(frozen=True)
class Expr:
    pattern: str
    flags: int
    good: tuple  # byte strings that match as a whole between filler bytes (one ending in '\n': the newline is its last byte);
    #              good[0] has at least 7 bytes: it is the sample of the split sweeps
    bad: tuple  # near misses of its own kind: silent
    full: bytes = b""  # bounded: a match of exactly max_len bytes
    over: bytes = b""  # ... and the same one byte longer than max_len allows: silent
    bol: bool = False  # a match begins at the line / piece start only: nothing is put in front of a sample
    eol: bool = False  # a match ends at the line / piece end only: nothing is put behind a sample
    cut: int = 1  # a forced break this many bytes in front of the end of good[0] leaves no match on either side

    @property
    def plain(self):
        """The samples that do not end with the newline."""
        return tuple(g for g in self.good if not g.endswith(b"\n"))


@dataclass(frozen=True)
class Unit:
    """What aosim_py.placement must say of one unit, in kernel order.  None / (): not asserted."""
    kind: str  # "group", "single", "scalar"
    members: tuple  # expression indices
    ctx: bool | None = None
    nw: int | None = None
    nt: int | None = None
    shift_form: bool | None = None  # one word: the lean steps take the shift form (NT == 0)
    nexc: int | None = None  # exactly this many exception nodes
    min_nexc: int | None = None
    masks: tuple = ()  # M0..M3 that must be non-zero
    bounded: bool | None = None
    max_len: int | None = None
    nl_accepts: bool | None = None
    lean2: bool | None = None


@dataclass(frozen=True)
class Cell:
    name: str
    exprs: tuple
    units: tuple
    n_literal: int = 0  # literal-anchored expressions riding along (the mixed cell)
    max_nw: int | None = None  # info["max_state_words"]
    excluded: dict = field(default_factory=dict)  # class, tag or "lean" -> why it cannot apply to this cell

    @property
    def patterns(self):
        return [e.pattern for e in self.exprs]

    @property
    def flags(self):
        return [e.flags for e in self.exprs]

    def ids(self, shared: bool):
        return [0] * len(self.exprs) if shared else list(range(len(self.exprs)))

    @property
    def n_always_on(self):
        return len(self.exprs) - self.n_literal

    @property
    def has_scalar(self):
        return any(u.kind == "scalar" for u in self.units)

    @property
    def all_scalar(self):
        return all(u.kind == "scalar" for u in self.units)

    @property
    def main_sizes(self):
        """The buffer sizes of the seg, nul / single and tile texts.  CAREFUL_BS is there to send every wave of the fast kernel
        through its exact routine; the scalar kernel has no such choice (and takes a tenth of a second for a scan of short pieces),
        so a cell of scalar units alone takes a buffer size above a tile in its place.  Short pieces reach those cells in the
        forced-break texts."""
        return (DEFAULT_BS, 20001) if self.all_scalar else (DEFAULT_BS, CAREFUL_BS)


HEX = b"0123456789abcdef"


def hexs(n: int, salt: int = 0) -> bytes:
    return bytes(HEX[(i * 5 + salt + (i >> 2)) % 16] for i in range(n))


def af(n: int, salt: int = 0) -> bytes:
    return bytes(b"abcdef"[(i * 5 + salt + (i >> 2)) % 6] for i in range(n))


NO_FULL = {"seg/full_len_from_q": "no bound on the match length: the lead-in is the line", "seg/over_len": "no bound on the match length"}
NOT_UNBOUNDED = {"long": "every unit is bounded: the lead-in never reaches back to the line start", "tile/line_start_residues": "every unit is bounded"}
NOT_DENSE = {"dense": "planted in group_cf alone"}
BOUNDED = {**NOT_UNBOUNDED, **NOT_DENSE}
UNBOUNDED = {**NO_FULL, **NOT_DENSE}
NO_LEAN = "no lean path: every wave takes the exact routine"
NO_63 = "the samples are longer than a piece of 63 bytes"

# An alternation of four two-byte branches has an exception node per branch end but the last two (and the node in front of it
# is one): no shift form.  Classes of three bytes, so that no branch is a required literal.
ALT = "(?:[a-c][d-f]|[g-i][j-l]|[m-o][p-r]|[s-u][v-x])"
P_NT1 = "[a-c][d-f][0-9]{2,4}[g-i]"                 # 7 nodes
P_NT2 = f"[0-9]{ALT}[yz]{{1,3}}[0-9]"               # 13 nodes
P_NT3 = f"[0-9]{ALT}{ALT}[yz]{{1,3}}[0-9]"          # 21 nodes
P_NT4 = f"[0-9]{ALT}{ALT}{ALT}[yz]{{1,3}}[0-9]"     # 29 nodes
P_SH1 = "[a-c]+[d-f]?[g-i]?[j-l][a-c][d-f][g-i][j-l][0-9]{2}"  # 11 nodes, one exception node, M0..M3
P_W2_0 = "[a-f]{30}[g-i]?[j-l]?[a-f]{6}[0-9]"       # 39 nodes: the optional nodes 30 and 31 make M1, M2 and M3 carry into word 1

S_NT1 = dict(good=(b"be1234h", b"ad12g", b"cf987i"), bad=(b"ad1g", b"a12g", b"ad12"), full=b"be1234h", over=b"be12345h")
S_NT2 = dict(good=(b"1adyzy2", b"3gjz4", b"5svyy6"), bad=(b"1ad2", b"1ayz2", b"1adyzy"), full=b"1adyzy2", over=b"1adyzyz2")
S_NT3 = dict(good=(b"1adgjyzy2", b"3mpsvz4", b"5svadyy6"), bad=(b"1adg2", b"1adjgyz2", b"1adgjyzy"), full=b"1adgjyzy2", over=b"1adgjyzyz2")
S_NT4 = dict(good=(b"1adgjmpyzy2", b"3mpsvadz4", b"5svadgjyy6"), bad=(b"1adgjm2", b"1adgjpmyz2", b"1adgjmpyzy"), full=b"1adgjmpyzy2", over=b"1adgjmpyzyz2")
S_SH1 = dict(good=(b"aadgjbehk12", b"bjadgj34", b"abcabcfkcfil56", b"chkbehk78", b"abjcfil90"), bad=(b"adgjbeh12", b"adggjbehk12", b"jbehk12"))
S_NL = dict(good=(b"a12345 ", b"b7\n", b"c456\t", b"a99\n"), bad=(b"a#", b"12 ", b"a1x"))
S_W2_0 = dict(good=(af(30) + b"gj" + af(6, 1) + b"7", af(30, 2) + af(6, 3) + b"1", af(30, 4) + b"k" + af(6, 5) + b"3", af(30, 6) + b"h" + af(6, 7) + b"5"),
              bad=(af(29) + b"gj" + af(6, 1) + b"7", af(30) + b"gg" + af(6, 1) + b"7", af(30) + b"gj" + af(5, 1) + b"7"), full=af(30) + b"hl" + af(6, 1) + b"9", over=af(30) + b"hl" + af(7, 1) + b"9")
S_W2_1 = dict(good=(b"adefd" + b"jkl" * 10, b"bh" + b"lkj" * 10, b"cfeed" + b"kkl" * 10), bad=(b"adef" + b"jkl" * 10, b"bh" + b"jkl" * 9 + b"jk", b"bhh" + b"jkl" * 10), full=b"adefd" + b"jkl" * 10,
              over=b"adefdd" + b"jkl" * 10)
S_SC_B = dict(good=(hexs(70) + b"g", hexs(70, 3) + b"h", hexs(70, 7) + b"i"), bad=(hexs(69) + b"g", hexs(70), hexs(35) + b"g" + hexs(34) + b"g"), full=hexs(70, 5) + b"gh", over=hexs(35, 5) + b"x" + hexs(35, 5) + b"gh")


def _wb(s: dict) -> dict:
    """The samples of an expression between \\b ... \\b: a word byte on either side is one more near miss."""
    g = s["good"][0]
    return {**s, "bad": s["bad"] + (b"_" + g, g + b"_")}


# members of the groups: disjoint alphabets
G_A = Expr(P_NT1, 14, **S_NT1)                                                                                                                           # 7 nodes, SINGLEMATCH
G_B = Expr("[j-l][m-o]{1,3}[p-r]", 6, (b"jmnop", b"kmq", b"lnnr"), (b"jp", b"jmnomp", b"mmp"), full=b"jmnop", over=b"jmnomp")                              # 5 nodes, all matches
G_C = Expr("[s-u][v-x]{1,5}[yz]", 6, (b"svwxvwy", b"tvz", b"uxxy"), (b"sy", b"svwxvwxy", b"vwy"), full=b"svwxvwy", over=b"svwxvwxy")                     # 7 nodes, all matches
G_D = Expr("[A-C][D-F]{2}[G-I]?[J-L]", 14, (b"ADEGJ", b"BFFK", b"CDDHL"), (b"ADGJ", b"ADEGGJ", b"DEGJ"), full=b"ADEGJ", over=b"ADEEGJ")                   # 5 nodes, SINGLEMATCH
G_E = Expr("[M-O][P-R]{3}[S-U]", 6, (b"MPQRS", b"NRRRT", b"OPPPU"), (b"MPQS", b"MPQRRS", b"PQRS"), full=b"MPQRS", over=b"MPQRRS")                          # 5 nodes, all matches
G_F = Expr("[X-Z]{2,3}", 6, (b"XY", b"YZX", b"ZZ"), (b"X", b"Y#Z"), full=b"XYZ", over=b"X#YZ")                                                          # 3 nodes: the dense member
G_UNB = Expr("[j-l][m-o]+[p-r]", 6, (b"jmnomnp", b"kmq", b"l" + b"mno" * 30 + b"r"), (b"jp", b"jmnom", b"mmp"))                                            # no bound
G_BOL = Expr("^[j-l][m-o]{2,4}", 6, (b"jmnom", b"kmm", b"lnono"), (b"jm", b"mno", b"j#mn"), full=b"jmnom", bol=True)
G_EOL = Expr("[A-C][D-F]{2,4}$", 14, (b"ADEFD", b"BFF", b"CDDDD"), (b"AD", b"ADEFDE", b"DEF"), full=b"ADEFD", eol=True)
E_W2_1 = Expr("[a-c](?:[d-f]{4}|[g-i])[j-l]{30}", 6, **S_W2_1)   # 36 nodes, one exception node (0, below bit 32)
E_SC_B = Expr("[0-9a-f]{70}[g-i]{1,2}", 14, **S_SC_B)            # 72 nodes: three state words


def _one(kind="single", **kw):
    return (Unit(kind, (0,), **kw),)


CELLS = [
    # ---- always_on_word<false, 1..4>: one word, context-free, follow-union tables
    Cell("word_cf_nt1", (Expr(P_NT1, 14, **S_NT1),), _one(ctx=False, nw=1, nt=1, shift_form=False, bounded=True, max_len=7, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    Cell("word_cf_nt2", (Expr(P_NT2, 14, **S_NT2),), _one(ctx=False, nw=1, nt=2, shift_form=False, min_nexc=3, bounded=True, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    Cell("word_cf_nt3", (Expr(P_NT3, 6, **S_NT3),), _one(ctx=False, nw=1, nt=3, shift_form=False, min_nexc=3, bounded=True, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    Cell("word_cf_nt4", (Expr(P_NT4, 14, **S_NT4),), _one(ctx=False, nw=1, nt=4, shift_form=False, min_nexc=3, bounded=True, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    Cell("word_cf_nt2_unbounded", (Expr("(?:ab|cd|ef)+z", 14, (b"abcdefabz", b"efz", b"cdcdcdcdz"), (b"abcdea", b"abcz", b"acz")),),
         _one(ctx=False, nw=1, nt=2, shift_form=False, min_nexc=3, bounded=False, nl_accepts=False), max_nw=1, excluded=UNBOUNDED),
    # ---- always_on_word<false, 0>: the shift form with 0, 1 and 2 exception nodes; M2 and M3 in use
    Cell("word_cf_shift_nexc0", (Expr("[a-c][d-f]?[g-i][a-c][d-f]?[g-i][j-l][0-9]{2}", 14, (b"adgbehj12", b"agbhk34", b"cfibil56"), (b"adgbeh12", b"addgbehj12", b"adgbehj1"), full=b"adgbehj12",
                                      over=b"adgbehhj12"),), _one(ctx=False, nw=1, nt=2, shift_form=True, nexc=0, masks=(1, 2), bounded=True), max_nw=1, excluded=BOUNDED),
    Cell("word_cf_shift_nexc1", (Expr(P_SH1, 6, **S_SH1),), _one(ctx=False, nw=1, nt=2, shift_form=True, nexc=1, masks=(0, 1, 2, 3), bounded=False), max_nw=1, excluded=UNBOUNDED),
    Cell("word_cf_shift_nexc2", (Expr("[a-c](?:[d-f]{4}|[g-i]{4})[j-l][0-9]{2,4}[m-o]", 14, (b"adefdj12m", b"bghigk1234n", b"cffffl999o"), (b"adefj12m", b"adefdj1m", b"adefgj12m"), full=b"bghigk1234n",
                                      over=b"bghigk12345n"),), _one(ctx=False, nw=1, nt=2, shift_form=True, nexc=2, masks=(1, 2, 3), bounded=True), max_nw=1, excluded=BOUNDED),
    # ---- always_on_word<true, 0..4>: the same with boundary conditions
    Cell("word_ctx_nt1", (Expr(rf"\b{P_NT1}\b", 14, **_wb(S_NT1)),), _one(ctx=True, nw=1, nt=1, shift_form=False, bounded=True, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    Cell("word_ctx_nt2", (Expr(rf"\b{P_NT2}\b", 14, **_wb(S_NT2)),), _one(ctx=True, nw=1, nt=2, shift_form=False, min_nexc=3, bounded=True, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    Cell("word_ctx_nt3", (Expr(rf"\b{P_NT3}\b", 14, **_wb(S_NT3)),), _one(ctx=True, nw=1, nt=3, shift_form=False, min_nexc=3, bounded=True, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    Cell("word_ctx_nt4", (Expr(rf"\b{P_NT4}\b", 6, **_wb(S_NT4)),), _one(ctx=True, nw=1, nt=4, shift_form=False, min_nexc=3, bounded=True, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    Cell("word_ctx_shift", (Expr(rf"\b{P_SH1}\b", 14, **_wb(S_SH1)),), _one(ctx=True, nw=1, nt=2, shift_form=True, nexc=1, masks=(0, 1, 2, 3), bounded=False, nl_accepts=False), max_nw=1, excluded=UNBOUNDED),
    Cell("word_ctx_nomultiline", (Expr(f"[A-C][0-9]{{1,3}}{ALT}[yz]$", 10, (b"A123adz", b"B3gjy", b"C45svz"), (b"A123adz#", b"A12ad", b"A1ayz"), full=b"A123adz", over=b"A1234adz", eol=True),),
         _one(ctx=True, nw=1, nt=2, shift_form=False, min_nexc=3, bounded=True, nl_accepts=False), max_nw=1, excluded=BOUNDED),
    # ---- an accepting node that takes the newline
    Cell("word_cf_nl", (Expr(r"[a-c][0-9]+\s", 6, **S_NL),), _one(ctx=False, nw=1, nt=1, bounded=False, nl_accepts=True), max_nw=1, excluded=UNBOUNDED),
    Cell("word_ctx_nl", (Expr(r"\b[a-c][0-9]+\s", 6, S_NL["good"], S_NL["bad"] + (b"_a12 ",)),), _one(ctx=True, nw=1, nt=1, bounded=False, nl_accepts=True), max_nw=1,
         excluded={**UNBOUNDED, "lean": NO_LEAN + " (a unit with conditions whose match can include the newline)"}),
    # ---- groups
    Cell("group_cf", (G_A, G_B, G_C, G_D, G_E, G_F), (Unit("group", (0, 1, 2, 3, 4, 5), ctx=False, nw=1, nt=4, bounded=True, max_len=7, nl_accepts=False),), max_nw=1, excluded=NOT_UNBOUNDED),
    Cell("group_ctx_riders", (Expr(rf"\b{P_NT1}\b", 14, **_wb(S_NT1)), G_BOL, G_EOL, G_C, G_E), (Unit("group", (0, 1, 2, 3, 4), ctx=True, nw=1, nt=4, bounded=True, max_len=7),), max_nw=1,
         excluded=BOUNDED),
    Cell("group_unbounded", (G_A, G_UNB, G_C), (Unit("group", (0, 1, 2), ctx=False, nw=1, nt=3, bounded=False),), max_nw=1, excluded=NOT_DENSE),
    # two groups (13 + 15 and 21 + 11 nodes), a single of one word that fits in neither (29 nodes) and one of two words: the
    # tables are staged again for every unit and tile
    Cell("two_groups_and_singles", (Expr(P_NT2, 14, **S_NT2), Expr("[A-C](?:[D-F]{4}|[G-I]{4})[J-L][0-9]{2,4}[M-O]", 6, (b"ADEFDJ12M", b"BGHIGK1234N"), (b"ADEFJ12M", b"ADEFDJ1M"), full=b"BGHIGK1234N",
                                                                 over=b"BGHIGK12345N"),
                                    Expr(P_NT3.replace("[yz]", "[YZ]"), 6, (b"1adgjYZY2", b"3mpsvZ4"), (b"1adg2", b"1adgjYZY"), full=b"1adgjYZY2", over=b"1adgjYZYZ2"),
                                    Expr(P_SH1.upper(), 14, (b"AADGJBEHK12", b"BJADGJ34"), (b"ADGJBEH12", b"JBEHK12")),
                                    Expr(P_NT4.replace("[yz]", "[wW]"), 14, (b"1adgjmpwWw2", b"3mpsvadW4"), (b"1adgjm2", b"1adgjmpwWw"), full=b"1adgjmpwWw2", over=b"1adgjmpwWwW2"),
                                    Expr(P_W2_0, 14, **S_W2_0)),
         (Unit("group", (0, 1), ctx=False, nw=1), Unit("group", (2, 3), ctx=False, nw=1), Unit("single", (4,), ctx=False, nw=1, nt=4, shift_form=False), Unit("single", (5,), nw=2, lean2=True)),
         max_nw=2, excluded=NOT_DENSE),
    # ---- always_on_word2: two words, context-free, shift form
    Cell("word2_lean_nexc0", (Expr(P_W2_0, 14, **S_W2_0),), _one(ctx=False, nw=2, nexc=0, masks=(1, 2, 3), bounded=True, nl_accepts=False, lean2=True), max_nw=2, excluded=BOUNDED),
    Cell("word2_lean_nexc1", (E_W2_1,), _one(ctx=False, nw=2, nexc=1, masks=(1, 2), bounded=True, nl_accepts=False, lean2=True), max_nw=2, excluded=BOUNDED),
    # exception sources 29 (below bit 32: the head of the second branch) and 33 (above: the end of the first); each sample takes one
    Cell("word2_lean_nexc2_skip", (Expr("[a-f]{30}(?:[g-i]{4}|[j-l]{4})[m-o][0-9]", 14, (af(30) + b"ghigm7", af(30, 2) + b"jkljn1", af(30, 4) + b"iiiio3"),
                                        (af(29) + b"ghigm7", af(30) + b"ghim7", af(30) + b"ghijm7"), full=af(30, 1) + b"jjjjm9", over=af(30, 1) + b"jjjjjm9"),),
         _one(ctx=False, nw=2, nexc=2, bounded=True, max_len=36, nl_accepts=False, lean2=True), max_nw=2, excluded=BOUNDED),
    # one exception node, at bit 32: the head of the second branch.  ao_follow2 takes it from the high word (src0 >= 32)
    Cell("word2_lean_nexc1_high", (Expr("[a-f]{33}(?:[g-i]{4}|[j-l])[m-o][0-9]", 14, (af(33) + b"jm7", af(33, 2) + b"ghign1", af(33, 4) + b"lo3"),
                                        (af(32) + b"jm7", af(33) + b"jjm7", af(33) + b"ghim7"), full=af(33, 1) + b"ihgim9", over=af(33, 1) + b"ihgiim9"),),
         _one(ctx=False, nw=2, nexc=1, bounded=True, max_len=39, nl_accepts=False, lean2=True), max_nw=2, excluded=BOUNDED),
    # a way back from bit 34 to node 1 in word 0, which the start state does not open: a second round of the repeat needs it
    Cell("word2_lean_back_edge", (Expr("[x-z](?:[a-f]{33}[g-i])*[0-9]", 14, (b"x" + af(33) + b"g" + af(33, 2) + b"h7", b"y" + af(33, 3) + b"i1", b"z5", b"y" + (af(33, 1) + b"g") * 3 + b"3"),
                                       (b"x" + af(32) + b"g7", b"x" + af(33) + b"g" + af(32, 2) + b"h7", af(33) + b"g7")),),
         _one(ctx=False, nw=2, nexc=2, bounded=False, nl_accepts=False, lean2=True), max_nw=2, excluded=UNBOUNDED),
    # exception sources 31 and 36, the follow rest of each in both words ({0, 37} and {0, 32}).  (The way back to a branch head
    # is also open from the start state: of these exceptions only 31 -> 37, the digits behind the long branch, decides a report.)
    Cell("word2_lean_nexc2", (Expr("(?:[g-i][j-l]{31}|[m-o]{5})*[0-9]{2}", 14, (b"g" + b"jkl" * 10 + b"j77", b"mnomn12", b"mmmmmh" + b"lkj" * 10 + b"lnnnnn34", b"55", b"mnomnooooo56", b"h" + b"kl" * 15 + b"ki" + b"jl" * 15 + b"j78"),
                                   (b"g" + b"jkl" * 10 + b"#7"[:1], b"mnom", b"h" + b"jkl" * 10 + b"j")),), _one(ctx=False, nw=2, nexc=2, bounded=False, nl_accepts=False, lean2=True), max_nw=2, excluded=UNBOUNDED),
    # max_len exactly HG_ALWAYS_ON_FAST_MAX_LEN: the longest fixed lead-in (an expression of more than 64 nodes, so every bounded
    # one of more than 64 bytes, has three state words: test_always_on_cells.py::test_max_len_65_is_out_of_the_fast_kernel)
    Cell("word2_len64", (Expr("[0-9a-f]{63}[g-i]", 14, (hexs(63) + b"g", hexs(63, 3) + b"h", hexs(63, 7) + b"i"), (hexs(62) + b"g", hexs(63), hexs(31) + b"g" + hexs(31) + b"g"), full=hexs(63, 5) + b"g",
                              over=hexs(31, 5) + b"x" + hexs(32, 5) + b"g"),), _one(ctx=False, nw=2, nexc=0, bounded=True, max_len=64, lean2=True), max_nw=2, excluded={**BOUNDED, "break/63": NO_63}),
    # ---- always_on_segment<2, false>
    Cell("word2_ctx", (Expr(rf"\b{P_W2_0}\b", 14, **_wb(S_W2_0)),), _one(ctx=True, nw=2, bounded=True, lean2=False), max_nw=2, excluded={**BOUNDED, "lean": NO_LEAN}),
    Cell("word2_noshift", (Expr("[0-9](?:[a-c]{6}|[d-f]{6}|[g-i]{6}|[j-l]{6}|[m-o]{6}|[p-r]{6})[s-u]{1,3}", 6, (b"2defdeft", b"1abcabcstu", b"3prqprqss"), (b"1abcabs", b"1abcabcd", b"abcabcs"),
                                full=b"1abcabcstu", over=b"1abcabccstu"),), _one(ctx=False, nw=2, min_nexc=3, bounded=True, lean2=False), max_nw=2, excluded={**BOUNDED, "lean": NO_LEAN}),
    Cell("word2_nl", (Expr(r"[a-f]{34}[0-9]+\s", 6, (af(34) + b"12 ", af(34, 2) + b"7\n", af(34, 3) + b"456\t", af(34, 5) + b"99\n"), (af(33) + b"12 ", af(34) + b" ", af(34) + b"1x")),),
         _one(nw=2, bounded=False, nl_accepts=True, lean2=False), max_nw=2, excluded={**UNBOUNDED, "lean": NO_LEAN}),
    # ---- hg_always_on_kernel: more than two words
    Cell("scalar_bounded", (E_SC_B,), _one("scalar", nw=3, bounded=True), max_nw=3, excluded={**BOUNDED, "lean": NO_LEAN, "break/63": NO_63}),
    Cell("scalar_unbounded", (Expr("[0-9a-f]{70,}[g-i]", 14, (hexs(70) + b"g", hexs(90, 3) + b"h", hexs(75, 7) + b"i"), (hexs(69) + b"g", hexs(70), hexs(35) + b"g" + hexs(34) + b"g")),),
         _one("scalar", nw=3, bounded=False), max_nw=3, excluded={**UNBOUNDED, "lean": NO_LEAN, "break/63": NO_63}),
    # ---- everything at once, also on one id: a group, a single with conditions (29 nodes: too many to join it), a lean
    # two-word unit, a scalar one and one literal-anchored expression
    Cell("mixed_shared_ids", (G_A, G_C, Expr(rf"\b{P_NT4}\b".replace("[yz]", "[YZ]"), 14, (b"1adgjmpYZY2", b"3mpsvadZ4"), (b"1adgjm2", b"_1adgjmpYZY2", b"1adgjmpYZY2_"), full=b"1adgjmpYZY2", over=b"1adgjmpYZYZ2"),
                              E_W2_1, E_SC_B, Expr("needle_mx_1[0-9]{1,3}Q", 14, (b"needle_mx_15Q", b"needle_mx_1123Q"), (b"needle_mx_1Q", b"needle_mx_11234Q"))),
         (Unit("group", (0, 1), ctx=False, nw=1), Unit("single", (2,), ctx=True, nw=1, nt=4), Unit("single", (3,), nw=2, lean2=True), Unit("scalar", (4,), nw=3)), n_literal=1, max_nw=3,
         excluded=BOUNDED),
]
BY_NAME = {c.name: c for c in CELLS}

def placement_errors(cell: Cell, pl: dict) -> list:
    """What aosim_py.placement of the cell's set gets wrong against Cell.units; [] when every unit is placed as named."""
    bad = []
    n_ao = cell.n_always_on
    if pl["tiers"] != [1] * n_ao + [0] * cell.n_literal:
        bad.append(("tiers", pl["tiers"]))
    units = [u for u in pl["units"] if u["kind"] != "huge"]
    if len(units) != len(cell.units) or len(units) != len(pl["units"]):
        return bad + [("units", [(u["kind"], u["members"]) for u in pl["units"]])]
    for want, u in zip(cell.units, units):
        got = {"kind": u["kind"], "members": tuple(sorted(u["members"]))}
        exp = {"kind": want.kind, "members": tuple(sorted(want.members))}
        for key in ("ctx", "nw", "nt", "shift_form", "nexc", "max_len", "nl_accepts", "lean2"):
            if getattr(want, key) is not None:
                exp[key], got[key] = getattr(want, key), u[key]
        if want.min_nexc is not None:
            exp["min_nexc"], got["min_nexc"] = True, u["nexc"] >= want.min_nexc
        if want.masks:
            exp["masks"], got["masks"] = want.masks, tuple(k for k in u["masks"] if k in want.masks)
        if want.bounded is not None:
            exp["bounded"], got["bounded"] = want.bounded, 0 < u["max_len"] <= FAST_MAX_LEN if u["kind"] != "scalar" else u["max_len"] > 0
        if got != exp:
            bad.append((want.members, {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]}))
    return bad


# ------------------------------------------------------------------ texts
@dataclass(frozen=True)
class Case:
    tag: str
    lo: int  # the planted bytes [lo, hi)
    hi: int
    end: int  # where the sample ends (exclusive): the match end of a reported case
    expr: int
    k: int = 0  # split sweeps: bytes of the sample in front of the boundary


@dataclass
class Text:
    label: str
    data: bytes
    sizes: tuple  # the buffer_size values it is scanned with
    cases: list

    def tag_at(self, off: int) -> str:
        """The tag of the planted case that holds byte `off` ("filler" outside every case)."""
        if not hasattr(self, "_lo_cache"):
            self._lo_cache = [c.lo for c in self.cases]
        k = bisect.bisect_right(self._lo_cache, off) - 1
        if k >= 0 and off < self.cases[k].hi:
            c = self.cases[k]
            return f"{c.tag}[expr {c.expr}, sample ends at {c.end} = segment offset {c.end % SEG}, tile {c.end // TILE}, k {c.k}]"
        return "filler"


class _Builder:
    def __init__(self, label: str, sizes, limit: int = MAX_TEXT):
        self.label, self.sizes, self.limit = label, tuple(sizes), limit
        self.buf = bytearray()
        self.cases = []

    def pad_to(self, target: int) -> None:
        """Filler lines (each at most 90 bytes, '\\n' included) up to offset `target`."""
        gap = target - len(self.buf)
        assert gap >= 0, (self.label, target, len(self.buf), self.cases[-1:])
        while gap > 0:
            n = min(gap, 61 + len(self.buf) % 29)
            self.buf += fill(n - 1, len(self.buf)) + b"\n"
            gap -= n

    def plant(self, tag: str, blob: bytes, end_in: int, expr: int, end_abs: int | None = None, k: int = 0, newline: bool = True) -> None:
        """Put `blob` (one or more lines; a '\\n' is added unless newline is False) so that its offset end_in lands at end_abs
        (default: right here); filler lines make up the distance."""
        if end_abs is None:
            end_abs = len(self.buf) + end_in
        lo = end_abs - end_in
        self.pad_to(lo)
        self.buf += blob + (b"\n" if newline else b"")
        self.cases.append(Case(tag, lo, len(self.buf), end_abs, expr, k))

    @property
    def here(self) -> int:
        return len(self.buf)

    def next_lane(self, min_gap: int = 0, lanes: int = 1) -> int:
        """The first lane boundary at least min_gap bytes ahead (`lanes`: a multiple of that many lanes from the tile start)."""
        step = SEG * lanes
        return (len(self.buf) + min_gap + step - 1) // step * step

    def text(self) -> Text:
        assert 0 < len(self.buf) <= self.limit, (self.label, len(self.buf))
        return Text(self.label, bytes(self.buf), self.sizes, self.cases)


def _wrap(e: Expr, s: bytes, front: int = 3, back: int = 3, salt: int = 0):
    """(blob, offset of the sample's end in it, newline to be added): the sample with filler around it where the expression
    allows filler; a sample that ends with the newline brings its own."""
    f = b"" if e.bol else fill(front, salt)
    own_nl = s.endswith(b"\n")
    b = b"" if (e.eol or own_nl) else fill(back, salt + 1)
    return f + s + b, len(f) + len(s), not own_nl


def _tail_in_last_tile(b: _Builder, cell: Cell, what) -> None:
    """The text's last tile (the wave that meets the end of the text takes the exact routine at every buffer size): `what`
    plants a short version of the text's classes there."""
    b.pad_to((b.here + TILE - 1) // TILE * TILE + 40)
    what(b)


def _seg_text(cell: Cell) -> Text:
    b = _Builder("seg", cell.main_sizes)
    ex = cell.exprs[: cell.n_always_on]
    n = len(ex)
    b.buf += fill(40, 1) + b"\n"

    def at(tag, ei, s, end_abs, k=0, front=3, back=3):
        blob, end_in, nl = _wrap(cell.exprs[ei], s, front, back, salt=end_abs)
        b.plant(tag, blob, end_in, ei, end_abs=end_abs, k=k, newline=nl)

    def sweeps(b, short=False):
        # the match end at every residue mod 64 (segment offsets 64 + r and 128 + r in turn), every expression and sample in turn
        lane = b.next_lane(400)
        for r in (range(0, 64, 9) if short else range(64)):
            e = ex[r % n]
            at("seg/end_residue", r % n, e.good[(r // n) % len(e.good)], lane + 64 * (1 + r % 2) + r)
            lane += SEG
        # the match end at the first and last offsets of a segment: 0 and 256 are the boundary itself (the last byte is the
        # previous lane's), 1 has its last byte at the segment's first
        for ei, e in enumerate(ex[:3]):
            for j, o in enumerate((0, 1) if short else (0, 1, 2, 3, 4, 253, 254, 255, 256)):
                lane = b.next_lane(300)
                at("seg/end_offset", ei, e.plain[j % len(e.plain)], lane + o)
                if e.bad and j < 3:
                    lane = b.next_lane(300)
                    at("seg/miss", ei, e.bad[j % len(e.bad)], lane + o)
        # the sample across a lane boundary, every split: k bytes in front of it
        for ei, e in enumerate(ex[:3]):
            g = e.plain[0]
            ks = range(1, len(g)) if ei == 0 else (1, len(g) // 2, len(g) - 1)
            for k in ((1, len(g) - 1) if short else ks):
                lane = b.next_lane(len(g) + 100)
                at("seg/split", ei, g, lane - k + len(g), k=k)
                if ei == 0 and k % 5 == 1 and not short:  # the same split of a near miss
                    lane = b.next_lane(len(g) + 100)
                    m = e.bad[k % len(e.bad)]
                    at("seg/split:miss", ei, m, lane - min(k, len(m) - 1) + len(m), k=k)
        # a match of the full max_len whose last byte is the segment's first: it starts at the lane's first lead-in byte; one
        # byte more than max_len allows is silent
        for ei, e in enumerate(ex):
            if e.full and not short:
                for s, tag in ((e.full, "seg/full_len_from_q"), (e.over, "seg/over_len")):
                    if s:
                        lane = b.next_lane(len(s) + 100)
                        at(tag, ei, s, lane + 1, front=2)
        # the literal-anchored expressions that ride along (the mixed cell): their reports share lines and ids with the tier's
        for ei in range(cell.n_always_on, len(cell.exprs) if not short else 0):
            e = cell.exprs[ei]
            for j, s in enumerate(e.good + e.bad):
                lane = b.next_lane(300)
                at("seg/literal_anchored" if j < len(e.good) else "seg/literal_anchored:miss", ei, s, lane + (0, 1, 130)[j % 3])
        # newlines as the first and the last byte of a segment, a sample right behind
        e = ex[0]
        lane = b.next_lane(300)
        b.pad_to(lane - 30)
        b.buf += fill(30, 2)  # (a line that ends with the newline at the segment's first byte)
        blob, end_in, nl = _wrap(e, e.plain[0], 0, 3)
        b.plant("tile/newline_first_byte_of_segment", b"\n" + blob, 1 + end_in, 0, newline=nl)
        lane = b.next_lane(300)
        b.pad_to(lane - 31)
        b.buf += fill(30, 3) + b"\n"  # (the newline is the segment's last byte)
        assert b.here == lane
        b.plant("tile/newline_last_byte_of_segment", blob, end_in, 0, newline=nl)

    sweeps(b)
    _tail_in_last_tile(b, cell, lambda bb: sweeps(bb, short=True))
    return b.text()


def _nul_single_text(cell: Cell) -> Text:
    b = _Builder("nul_single", cell.main_sizes)
    ex = cell.exprs[: cell.n_always_on]
    b.buf += fill(33, 2) + b"\n"

    def body(b, short=False):
        for ei, e in enumerate(ex[: (1 if short else 3)]):
            g = e.plain[0]
            head = b"" if e.bol else fill(4, 7)
            tail = b"" if e.eol else fill(5, 3)
            for o in ((130,) if short else (130, 0)):  # the sample's end inside a segment, and on a lane boundary
                def put(tag, blob, end_in, newline=True):
                    lane = b.next_lane(len(blob) + 420)
                    b.plant(tag, blob, end_in, ei, end_abs=lane + o, newline=newline)

                put("nul/leading", b"\0\0\0" + head + g + tail, 3 + len(head) + len(g))
                put("nul/leading_only", b"\0\0\0" + g + tail, 3 + len(g))  # (a line start for ^ expressions: the first scanned byte)
                put("nul/inside", head + g[: len(g) // 2] + b"\0" + g[len(g) // 2:] + tail, len(head) + len(g) + 1)
                put("nul/blocked", b"#\0" + head + g + tail, 2 + len(head) + len(g))
                put("nul/blocked_far", b"#\0" + fill(300, 2) + g + tail, 302 + len(g))  # the NUL lies beyond a bounded lead-in: the line geometry blocks it
                put("nul/after_match", head + g + b"\0" + fill(5, 3), len(head) + len(g))  # END context behind the match
                put("nul/before_newline", head + g + b"\0", len(head) + len(g))
                put("nul/line_of_nuls_before", b"\0" * 7 + b"\n" + head + g + tail, 8 + len(head) + len(g))
                if len(g) >= 4:  # the lane boundary inside the sample: the NULs are in the next lane's lead-in
                    k = len(g) // 2
                    lane = b.next_lane(len(g) + 120)
                    b.plant("nul/in_leadin", b"\0\0" + g + tail, 2 + len(g), ei, end_abs=lane - k + len(g), k=k)
                    lane = b.next_lane(len(g) + 120)
                    b.plant("nul/in_leadin_blocked", b"%\0" + g + tail, 2 + len(g), ei, end_abs=lane - k + len(g), k=k)
        # two matches on one line
        for ei, e in enumerate(ex[: (1 if short else 3)]):
            p = e.plain
            g1, g2, gs = p[0], p[1 % len(p)], min(p, key=len)
            head = b"" if e.bol else fill(3, 1)
            tail = b"" if e.eol else fill(2, 5)
            lane = b.next_lane(100)
            blob = head + g1 + fill(4, 2) + g2 + tail
            b.plant("single/same_segment", blob, len(blob) - len(tail), ei, end_abs=lane + len(blob) + 8)
            # the first match ends one byte in front of a lane boundary, the second starts right behind it: a bounded lead-in
            # that holds the first match has seen it
            lane = b.next_lane(len(gs) + 120)
            blob = head + gs + fill(1, 2) + g2 + tail
            b.plant("single/adjacent_segments", blob, len(blob) - len(tail), ei, end_abs=lane + len(g2))
            lane = b.next_lane(200)
            blob = head + g1 + fill(310 - len(g1), 2) + g2 + tail  # more than 300 bytes apart: two lanes note a match, and no bounded lead-in sees the first
            b.plant("single/far_apart", blob, len(blob) - len(tail), ei, end_abs=lane + 400)
            if e.bad:
                lane = b.next_lane(100)
                blob = head + e.bad[0] + fill(4, 2) + e.bad[-1] + tail
                b.plant("single/both_miss", blob, len(blob) - len(tail), ei, end_abs=lane + len(blob) + 8)

    body(b)
    _tail_in_last_tile(b, cell, lambda bb: body(bb, short=True))
    return b.text()


def _tile_texts(cell: Cell) -> list:
    """One event per tile edge, six tiles per text."""
    ex = cell.exprs[: cell.n_always_on]
    n = len(ex)
    free = [i for i, e in enumerate(ex) if not e.bol] or [0]
    events = []  # (tag, expr, blob, end_in, end relative to the edge, k, edges used, newline)

    def ev(tag, ei, s, front, rel_end, back=5, edges=1, k=0):
        blob, end_in, nl = _wrap(ex[ei], s, front, back, salt=len(events))
        events.append((tag, ei, blob, end_in, rel_end, k, edges, nl))

    g = ex[0].plain[0]
    ks = sorted({1, 2, 3, len(g) // 2, len(g) - 3, len(g) - 2, len(g) - 1, (len(g) * 2) // 3} - {0})
    for k in ks:  # the sample across a tile edge: lane 63 and lane 0 of another wave
        ev("tile/split", 0, g, 9, len(g) - k, k=k)
    for ei in range(1, min(n, 3)):
        gg = ex[ei].plain[0]
        for k in (1, len(gg) - 1):
            ev("tile/split", ei, gg, 9, len(gg) - k, k=k)
    miss = ex[0].bad[0]
    ev("tile/split:miss", 0, miss, 9, len(miss) - min(2, len(miss) - 1), k=2)
    for j in range(2):  # a line that starts in the previous tile, the whole sample in this one
        ei = free[j % len(free)]
        s = ex[ei].plain[j % len(ex[ei].plain)]
        ev("tile/line_from_previous_tile", ei, s, 100 + 7 * j, len(s) + 3 + 5 * j)
    ei = free[0]
    ev("tile/line_from_two_tiles_back", ei, ex[ei].plain[0], 2000 + TILE + 2100, 2100 + len(ex[ei].plain[0]), edges=2)
    for j in range(2):
        ei = j % n
        s = ex[ei].plain[-1]
        ev("tile/line_at_tile_start", ei, s, 0, len(s))  # the previous line's newline is the last byte of the tile before
        ei = (j + 1) % n
        s = ex[ei].plain[0]
        ev("tile/newline_first_byte", ei, s, 0, 1 + len(s))
    for j in range(min(n, 2)):  # two matches on one line, one in either tile
        e = ex[j]
        p = e.plain
        line = (b"" if e.bol else fill(3, 1)) + p[0] + fill(40, 2) + p[1 % len(p)]
        events.append(("single/different_tiles", j, line + (b"" if e.eol else fill(2, 1)), len(line), 12 + len(p[1 % len(p)]), 0, 1, True))
    texts, b, edge = [], None, 0
    for tag, ei, blob, end_in, rel, k, edges, nl in events:
        if b is None or edge + edges > 5:
            if b is not None:
                texts.append(b.text())
            # (a cell with a scalar unit beside fast ones, the mixed cell, scans only its first tile text at CAREFUL_BS)
            b, edge = _Builder(f"tile{len(texts)}", (DEFAULT_BS,) if cell.has_scalar and texts else cell.main_sizes), 0
        edge += edges
        t = edge * TILE
        if tag == "tile/newline_first_byte":  # the previous line's '\n' is byte 0 of the tile
            b.pad_to(t - 40)
            b.buf += fill(40, 3) + b"\n"
            assert b.here == t + 1 and t + rel - end_in == t + 1
        if tag == "tile/line_at_tile_start":
            assert t + rel - end_in == t
        b.plant(tag, blob, end_in, ei, end_abs=t + rel, k=k, newline=nl)
    texts.append(b.text())
    return texts


# the cells whose text-edge texts also run on guarded buffers (gpu_cases.guarded_cases), and the texts taken in this order
GUARDED_CELLS = ("word_ctx_shift", "word2_lean_nexc1", "group_cf")
GUARDED_LABELS = ("edge_end0_0", "edge_end1_0", "edge_endmiss0_0", "edge_cut_0", "edge_onetile_0", "edge_end0_1", "edge_end1_1", "edge_endmiss1_0")


def guarded_edge_cases():
    """(name, text, patterns, flags, ids, buffer_size) of the text-edge class of three cells, four texts each, for buffers
    whose end is followed by unmapped memory.  Every length is no multiple of 16 (texts whose length is one are passed over):
    the always-on kernels may read up to the size rounded up to 16, their 16-byte loads being aligned, not a byte further."""
    for name in GUARDED_CELLS:
        cell = BY_NAME[name]
        texts = {t.label: t for t in edge_texts(cell)}
        labels = [x for x in GUARDED_LABELS if x in texts and len(texts[x].data) % 16][:4]
        for label in labels:
            yield (f"alwayson-{name}-{label}", texts[label].data, cell.patterns, cell.flags, cell.ids(False), DEFAULT_BS)


def edge_texts(cell: Cell) -> list:
    """Small texts of their own: what the start and the end of a text can meet."""
    out = []
    ex = cell.exprs[: cell.n_always_on]

    def one(label, tag, ei, blob, end_in, head=b"", newline=True, tail=b"", total=None, sizes=(DEFAULT_BS, 64)):
        b = _Builder(f"edge_{label}_{ei}", sizes)
        b.buf += head
        if total is not None:  # the text is `total` bytes long and ends with the blob
            b.plant(tag, blob, end_in, ei, end_abs=total - (len(blob) - end_in) - (1 if newline else 0), newline=newline)
            assert b.here == total, (label, b.here, total)
        else:
            b.plant(tag, blob, end_in, ei, newline=newline)
        b.buf += tail
        out.append(b.text())

    for ei, e in enumerate(ex[:2]):
        g = e.plain[0]
        one("byte0", "edge/match_at_byte_0", ei, g + (b"" if e.eol else fill(3, 1)), len(g), tail=fill(30, 1) + b"\n" + fill(11, 2) + b"\n")
        for k, lead_in in enumerate((fill(20, 4) + b"\n", fill(41 + ei, 4) + b"\n" + fill(3 + ei, 1) + b"\n")):
            # the match ends at the last byte of the text: END context; the lengths differ mod 16
            head = b"" if e.bol else fill(2 + k, 6)
            one(f"end{k}", "edge/match_ends_the_text", ei, head + g, len(head) + len(g), head=lead_in, newline=False)
            miss = e.bad[0]
            one(f"endmiss{k}", "edge/near_miss_ends_the_text", ei, head + miss, len(head) + len(miss), head=lead_in, newline=False)
        one("cut", "edge/match_cut_by_the_end", ei, g[:-1], len(g) - 1, head=fill(25 + ei, 2) + b"\n", newline=False)
        head = b"" if e.bol else fill(2, 6)
        one("len256", "edge/len_multiple_of_256", ei, head + g, len(head) + len(g), total=512, newline=False)
        one("len256nl", "edge/len_multiple_of_256", ei, head + g + (b"" if e.eol else fill(3, 1)), len(head) + len(g), total=768, newline=True)
        big = (DEFAULT_BS,) if cell.has_scalar else (DEFAULT_BS, 64)  # (the scalar kernel on tiles of 63-byte pieces: see Cell.main_sizes)
        one("len16384", "edge/len_multiple_of_16384", ei, head + g, len(head) + len(g), total=TILE, newline=False, sizes=big)
        one("len32768nl", "edge/len_multiple_of_16384", ei, head + g + (b"" if e.eol else fill(3, 1)), len(head) + len(g), total=2 * TILE, newline=True, sizes=big)
        one("short", "edge/short_text", ei, head + g, len(head) + len(g), head=fill(20, 4) + b"\n", newline=True)
        one("shortmiss", "edge/short_text:miss", ei, head + e.bad[-1], len(head) + len(e.bad[-1]), head=fill(20, 4) + b"\n", newline=True)
        b = _Builder(f"edge_onetile_{ei}", big)  # one tile, not full: samples at a few lanes, the last one ends the text
        for j, lane in enumerate((3, 17, 18, 35)):
            s = e.plain[j % len(e.plain)]
            blob, end_in, nl = _wrap(e, s, 3, 3, salt=j)
            b.plant("edge/one_tile", blob, end_in, ei, end_abs=lane * SEG + (0, 1, 77, 255)[j], newline=nl)
        b.plant("edge/one_tile", head + g, len(head) + len(g), ei, end_abs=37 * SEG + 5, newline=False)
        out.append(b.text())
    return out


def _break_texts(cell: Cell, bs1: int) -> list:
    """Lines longer than bs1 bytes: the line's pieces start every bs1 bytes from its start.  Events sit at the break
    B = line start + k * bs1.  Up to 4096 the first two expressions get every kind of event; above a tile, where one line
    fills a sixth of a text, every kind is planted once, for expressions that change with the kind and with bs1.  A text that
    is full is closed and the next one begun: no event is dropped."""
    texts = []
    ex = cell.exprs[: cell.n_always_on]
    k = 3 if bs1 < 100 else 2 if bs1 <= 1000 else 1
    tailroom = max(300 - k * bs1, bs1 // 3 if bs1 < 4096 else 0) + 40

    def builder():
        nb = _Builder(f"break{bs1}_{len(texts)}", (bs1 + 1,))
        nb.buf += fill(30, 2) + b"\n"
        return nb

    b = builder()

    def event(tag, ei, s, rel_end, nuls=0, kk=None, on_boundary=False):
        """Sample s ends at B + rel_end; nuls > 0: that many NULs at the start of piece kk; nuls < 0: one NUL between the start
        of the piece and the sample; on_boundary: B is a lane boundary."""
        nonlocal b
        e = ex[ei]
        kk = kk or k
        brk = kk * bs1
        start = brk + rel_end - len(s)  # the sample's offset in the line
        assert start >= 0
        body = bytearray(fill(start, ei + kk))
        for i in range(max(nuls, 0)):
            body[brk + i] = 0
        if nuls < 0:
            body[brk + 2] = 0
        body += s
        if not e.eol:
            body += fill(tailroom, 3)
        if b.here + len(body) + 500 > MAX_TEXT:
            texts.append(b.text())
            b = builder()
        line_at = b.here + 70
        if on_boundary:
            line_at += -(line_at + brk) % SEG
        b.pad_to(line_at)
        b.plant(tag, bytes(body), start + len(s), ei)
        assert b.cases[-1].lo == line_at and b.buf[line_at - 1] == 10

    events = []
    for ei, e in enumerate(ex[:2]):
        g = min(e.plain, key=len) if bs1 < 100 else e.plain[0]
        if len(g) + 4 > bs1:
            continue
        near = 3 if len(g) + 12 > bs1 else 12
        events.append(("break/inside_match", ei, g, e.cut, 0))  # silent: the break cuts the sample
        if not e.bol:
            events.append(("break/right_after_match", ei, g, 0, 0))  # $ and \b see the END context
            events.append(("break/on_segment_boundary", ei, g, 0, 0))
            events.append(("break/in_leadin", ei, g, len(g) + 3, 0))  # the break lies in the bytes in front of the sample
        events.append(("break/at_piece_start", ei, g, len(g), 0))  # ^ and \b see the START context
        events.append(("break/later_piece_leading_nuls", ei, g, len(g) + 3, 3))
        events.append(("break/later_piece_nul_blocks", ei, g, len(g) + near, -1))
        events.append(("break/later_piece:miss", ei, e.bad[0], len(e.bad[0]) if e.bol else len(e.bad[0]) + 3, 0))
        events.append(("break/third_piece", ei, g, len(g) + (0 if e.bol else near), 0))
    by_kind = {}
    for v in events:
        by_kind.setdefault(v[0], []).append(v)
    kinds = list(by_kind)
    if bs1 > 4096:
        for ki, kind in enumerate(kinds):
            lst = by_kind[kind]
            by_kind[kind] = [lst[(ki + BREAK_BS1.index(bs1)) % len(lst)]]
    turn = 0
    while any(by_kind.values()):  # the kinds in turn, so that neighbouring lines hold different kinds
        kind = kinds[turn % len(kinds)]
        turn += 1
        if by_kind[kind]:
            tag, ei, s, rel, nuls = by_kind[kind].pop(0)
            event(tag, ei, s, rel, nuls, kk=(k + 1 if bs1 <= 1000 else 2) if kind == "break/third_piece" else None, on_boundary=kind == "break/on_segment_boundary")
    texts.append(b.text())
    return texts


def _long_texts(cell: Cell) -> list:
    """Units without a bound on the match length start at the line's start: long lines with the match at their end, a long line
    that begins in the middle of a tile (the lanes of its waves have very different lead-ins), line starts at every residue
    mod 64 with a near match of the previous line directly in front of its newline (the bytes that a lead-in block rounded
    down to 64 drags in)."""
    ex = cell.exprs[: cell.n_always_on]
    free = [i for i, e in enumerate(ex) if not e.bol] or [0]
    b = _Builder("long0", (DEFAULT_BS, 20001))
    b.buf += fill(50, 1) + b"\n"
    for j, n in enumerate((700, 5000, 40960)):
        ei = free[j % len(free)]
        e = ex[ei]
        s = e.plain[j % len(e.plain)]
        b.plant(f"long/line_{n}", fill(n - 1 - len(s), j) + s, n - 1, ei)
        m = e.bad[j % len(e.bad)]
        if n < 6000:
            b.plant("long/miss", fill(n - 1 - len(m), j) + m, n - 1, ei)
    texts = [b.text()]
    b = _Builder("long1", (DEFAULT_BS, 20001))
    b.buf += fill(50, 1) + b"\n"
    ei = free[0]
    s = ex[ei].plain[0]
    b.pad_to(TILE + 8000)
    b.plant("long/line_from_mid_tile", fill(6000, 3) + s + fill(6000 - len(s), 4) + s, 12000 + len(s), ei)
    lane = b.next_lane(300, lanes=64)  # a fresh tile: 64 lanes, a line start per lane
    for r in range(64):
        ei = free[r % len(free)]
        e = ex[ei]
        g = e.plain[(r // len(free)) % len(e.plain)]
        start = lane + r * SEG + 64 + r  # the next line's start: every residue mod 64
        prev = fill(20, r) + g[:-1] + b"\n"
        blob = prev + g[-1:] + fill(3, r) + g + (b"" if e.eol else fill(2, r))
        b.plant("tile/line_start_residues", blob, len(prev) + 4 + len(g), ei, end_abs=start + 4 + len(g), k=r)
        assert b.buf[start - 1] == 10 and b.cases[-1].lo == start - len(prev)
    texts.append(b.text())
    return texts


def _dense_text(cell: Cell) -> Text:
    """Five tiles of lines on which the all-matches member [X-Z]{2,3} reports at nearly every byte."""
    b = _Builder("dense", (DEFAULT_BS,))
    ei = next(i for i, e in enumerate(cell.exprs) if e.pattern == "[X-Z]{2,3}")
    for j in range(5 * TILE // 2048):
        if j % 8 == 7:
            b.plant("dense/quiet", b"\n".join(b"X#Y%Z&" * 14 + b"X" for _ in range(24)), 0, ei)
        else:
            b.plant("dense/every_byte", b"\n".join(bytes(b"XYZ"[(i + l) % 3] for i in range(96 + l % 5)) for l in range(20)), 0, ei)
    return b.text()


@functools.lru_cache(maxsize=None)
def cell_texts(name: str) -> tuple:
    cell = BY_NAME[name]
    texts = [_seg_text(cell), _nul_single_text(cell)] + _tile_texts(cell) + edge_texts(cell)
    for bs1 in BREAK_BS1:
        if bs1 == 63 and "break/63" in cell.excluded:
            continue
        texts += _break_texts(cell, bs1)
    if "long" not in cell.excluded:
        texts += _long_texts(cell)
    if "dense" not in cell.excluded:
        texts.append(_dense_text(cell))
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def compiled(name: str) -> dict:
    """aosim_py.placement of the cell's set."""
    import aosim_py

    cell = BY_NAME[name]
    return aosim_py.placement(cell.patterns, cell.flags, cell.ids(False))


# ------------------------------------------------------------------ lean or careful
def wave_is_careful(unit: dict, data: bytes, buffer_size: int, tile: int) -> bool:
    """Whether the wave of `tile` takes the exact routine for this unit (a dict of aosim_py.placement): the `careful` predicates
    of always_on_word and always_on_word2 (hg_always_on.hip) with the walk geometry they are computed from.  True for a unit
    that has no lean path.  Used only to label reference hits in the floors."""
    if unit["kind"] != "group" and not (unit["kind"] == "single" and unit["nw"] <= 2):
        return True  # the scalar kernel
    if unit["nw"] == 2 and not unit["lean2"]:
        return True  # always_on_word2: nexc > 2 stands for "not lean-eligible"
    bs1 = buffer_size - 1
    bs1c = min(bs1, 0x7FFFFFFF)
    if bs1c <= 512 or (unit["nw"] == 1 and unit["ctx"] and unit["nl_accepts"]):
        return True
    nbytes = len(data)
    tile_start = tile * TILE
    nl = _newlines(data)
    bounded = 0 < unit["max_len"] <= FAST_MAX_LEN
    geo = []
    for lane in range(64):
        lo = min(tile_start + lane * SEG, nbytes)
        hi = min(lo + SEG, nbytes)
        i = bisect.bisect_left(nl, lo)  # newlines before lo
        line_start = nl[i - 1] + 1 if i else 0
        if bounded:
            q = max(lo - (unit["max_len"] - 1), 0)
        elif lo - line_start >= bs1:
            q = line_start + (lo - line_start) // bs1 * bs1
        else:
            q = line_start
        q64 = q & ~63
        geo.append((lo, hi, line_start, q64, lo - q64 if lo < hi else 0))
    own = max(g[4] for g in geo)
    for lo, hi, line_start, q64, _ in geo:
        base = lo - own
        stop = own + (hi - lo)
        if q64 >= line_start:
            d = q64 - line_start
            k = 1 if d <= bs1 else (d + bs1 - 1) // bs1
            at = line_start + k * bs1 - base
        else:
            at = line_start + bs1 - base
        nb_first = at if at < 0x7FFFFFFF else 0xFFFFFFFF
        if nb_first <= stop + 4 or hi >= nbytes:
            return True
    return False


_NL_CACHE: dict = {}


def _newlines(data: bytes):
    key = id(data)
    if key not in _NL_CACHE or _NL_CACHE[key][0] is not data:
        _NL_CACHE[key] = (data, np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10).tolist())
    return _NL_CACHE[key][1]


def unit_of(placement: dict, expr: int):
    return next((u for u in placement["units"] if expr in u["members"]), None)


# ------------------------------------------------------------------ reference
_REF = {}


def cell_reference(name: str, text_index: int, buffer_size: int, shared: bool):
    """(sorted uint64 [n, 5] of (line, id, to, start, len), n_lines, the oracle's own rows) of one text of the cell."""
    key = (name, text_index, buffer_size, shared)
    if key not in _REF:
        cell = BY_NAME[name]
        _REF[key] = reference(cell_texts(name)[text_index].data, cell.patterns, cell.flags, cell.ids(shared), buffer_size)
    return _REF[key]
