"""The confirm routines of the literal-anchored tier as test cells (hypergrep_amd/csrc/hg_confirm_dev.h, hg_kernels.hip,
hg_huge.hip), the texts that drive each cell through the window and piece geometry, and the reference.  The huge-automaton
kernel has four cells, one per routine of hg_huge.hip (huge: huge_run_reg<1>, huge_reg2, huge_reg4, huge_lds: huge_run on
staged tables and on tables in L2); the routines' own word, slab and exception geometry is in huge_cells.py.  Test infrastructure:
imported by test_confirm_cells.py, test_confirm_cells_gpu.py and gpu_cases.py.

A cell is a small set of expressions the compiler must place in one confirm routine (mode 0-4) with one class of lead (the
bound on how far a match may start before its required literal).  Every cell's texts plant cases of six geometry classes:

    align   the occurrence start fs, the window start q = fs - lead and the match end at every residue mod 16; near misses
    tile    line starts and tile edges: carry-in starts (rank 0), starts inside the tile, literal / lead across the edge
    edge    the ends of the text: byte 0, no final newline, a length that is no multiple of 16, texts of one chunk
    nul     the NUL rules: leading NULs, a NUL before / inside / after what a match needs, lines of NULs
    break   forced breaks of over-long lines at every buffer_size of BREAK_BS1
    multi   several occurrences on one line: a failing one before a matching one, overlaps, far starts, other expressions

Each planted case carries a tag "class/subcase".  Filler bytes come from FILLER: no word byte, no letter, no digit, so no
expression of a cell matches across them and a planted case is judged on its own.

The reference is the oracle's (line, id, to) with the (start, len) of invert_ref.pieces: five columns, as
Scanner.hits_array() gives them."""
from __future__ import annotations

import bisect
import functools
from dataclasses import dataclass, field

import numpy as np

import invert_ref
import oracle_py

TILE = 16384  # HG_TILE_BYTES
DEFAULT_BS = 262140
BREAK_BS1 = (63, 100, 1000, 4096, 16384, 20000)  # buffer_size - 1 of the forced-break texts
MAX_TEXT = 6 * TILE
FILLER = b"#%&~@:"
CLASSES = ("align", "tile", "edge", "nul", "break", "multi")
UNBOUNDED = 0xFFFFFFFF


def fill(n: int, salt: int = 0) -> bytes:
    """n filler bytes, deterministic."""
    return bytes(FILLER[(i * 7 + salt * 3 + (i >> 3)) % len(FILLER)] for i in range(n))


@dataclass(frozen=True)
class Expr:
    pattern: str
    flags: int
    lit: bytes  # the required literal as the texts hold it
    good: tuple  # (pre, post): pre + lit + post between filler bytes is a match
    bad: tuple = ()  # (pre, lit', post): a near miss of its own kind (a bound passed by one byte, an assertion vetoed by one byte)
    lead: str = "zero"  # what lit_lead must be: "zero", "lt16" (0 < lead < 16), "ge17" (17 <= lead, bounded), "unbounded"
    bol: bool = False  # a match begins at the line / piece start only: nothing is put in front of a sample
    eol: bool = False  # a match ends at the line / piece end only: nothing is put behind a sample

    def samples(self, good: bool):
        """(pre, lit, post) triples: the matching samples, or the near misses (the own ones, the literal broken, the literal
        cut short)."""
        if good:
            return [(p, self.lit, q) for p, q in self.good]
        p, q = self.good[0]
        broken = bytearray(self.lit)
        broken[len(broken) // 2] = ord("!")
        return list(self.bad) + [(p, bytes(broken), q), (p, self.lit[:-1], b"")]


@dataclass(frozen=True)
class Cell:
    name: str
    mode: int  # hg_confirm_mode of every expression (None: see modes)
    exprs: tuple
    nw: str = ""  # "1", "2", ">=3", "huge" or "" (not asserted)
    modes: tuple = ()  # mixed cells: the mode of each expression
    excluded: dict = field(default_factory=dict)  # tag or class -> why it cannot apply to this cell

    @property
    def patterns(self):
        return [e.pattern for e in self.exprs]

    @property
    def flags(self):
        return [e.flags for e in self.exprs]

    def ids(self, shared: bool):
        return [0] * len(self.exprs) if shared else list(range(len(self.exprs)))


AZ = b"abcdefghijklmnopqrstuvwxyz"
D9 = b"1234567890"
NO_LEAD = {"tile/lead_straddles": "no expression of the cell has bytes in front of its literal", "break/in_prefix": "no prefix to break",
           "nul/in_lead": "no lead window", "nul/leading_in_window": "no lead window"}
NO_Q = "the routine does not use match_window: the window start is not swept"

CELLS = [
    Cell("lit", 0, (
        Expr("needle_lit_01", 14, b"needle_lit_01", ((b"", b""),)),
        Expr("Needle_Lit_02", 15, b"nEEDLE_lit_02", ((b"", b""),)),
        Expr("needle_lit_twentyfour_03", 14, b"needle_lit_twentyfour_03", ((b"", b""),)),
    ), excluded={**NO_LEAD, "nul/in_tail": "a literal has no tail behind it", "multi/far_start": "no lead", "q_sweep": "no lead"}),
    Cell("simple_lead0", 1, (
        Expr("needle_sa_1[0-9]{1,3}x", 14, b"needle_sa_1", ((b"", b"5x"), (b"", b"123x"), (b"", b"07x")), ((b"", b"needle_sa_1", b"1234x"), (b"", b"needle_sa_1", b"x"))),
        Expr("needle_sq_2(?:ab|cd)+e", 14, b"needle_sq_2", ((b"", b"abe"), (b"", b"abcdabe")), ((b"", b"needle_sq_2", b"ae"),)),
        Expr("needle_sr_3z?y", 14, b"needle_sr_3", ((b"", b"y"), (b"", b"zy")), ((b"", b"needle_sr_3", b"zzy"),)),
        # its last position takes the newline: at the end of a line the match's last byte is the line's '\n' (len ends there)
        Expr("needle_sn_5[^a-z]", 14, b"needle_sn_5", ((b"", b"#"), (b"", b"")), ((b"", b"needle_sn_5", b"a"),), eol=True),
    ), nw="1", excluded={**NO_LEAD, "multi/far_start": "no lead", "q_sweep": "lead 0: q is fs"}),
    Cell("simple_bounded", 1, (
        Expr("[a-z]{0,3}needle_sb_2", 14, b"needle_sb_2", ((b"", b""), (b"a", b""), (b"abc", b""), (b"abcd", b"")), lead="lt16"),
        Expr("[a-z]{0,19}needle_sc_3!", 14, b"needle_sc_3", ((b"", b"!"), (AZ[:19], b"!"), (AZ[:25], b"!"), (b"ab", b"!")), ((AZ[:19], b"needle_sc_3", b"?"),), lead="ge17"),
        Expr("[a-z]{2,5}-needle_sf_4", 14, b"needle_sf_4", ((b"ab-", b""), (b"abcde-", b""), (b"abcdefg-", b"")), ((b"a-", b"needle_sf_4", b""), (b"ab", b"needle_sf_4", b"")), lead="lt16"),
    ), nw="1", excluded={"multi/far_start": "the lead is bounded"}),
    Cell("simple_unbounded", 1, (
        Expr("x+needle_sd_4+", 14, b"needle_sd_4", ((b"x", b""), (b"xxxxx", b"444"), (b"x" * 300, b"")), ((b"", b"needle_sd_4", b""), (b"xy", b"needle_sd_4", b"")), lead="unbounded"),
        Expr("(?:aa|b)+needle_se_5", 14, b"needle_se_5", ((b"aa", b""), (b"b", b""), (b"aabaa", b""), (b"aab" * 150, b"")), ((b"a", b"needle_se_5", b""), (b"ba", b"needle_se_5", b"")),
             lead="unbounded"),
    ), nw="1", excluded={"q_sweep": "no bound on the lead: q is the first scanned byte"}),
    Cell("ctx1", 2, (
        Expr(r"\b[0-9]{2,5}-needle_ca_6\b", 14, b"needle_ca_6", ((b"12-", b""), (b"12345-", b""), (b"007-", b"")),
             ((b"123456-", b"needle_ca_6", b""), (b"12-", b"needle_ca_6", b"x"), (b"x12-", b"needle_ca_6", b""), (b"1-", b"needle_ca_6", b"")), lead="lt16"),
        Expr("^.{0,6}needle_cb_7", 14, b"needle_cb_7", ((b"", b""), (b"abc", b""), (b"ab#def", b"")), ((b"abcdefg", b"needle_cb_7", b""),), lead="lt16", bol=True),
        Expr("[A-Z][a-z]+ needle_cc_8$", 14, b"needle_cc_8", ((b"Hi ", b""), (b"Hello ", b""), (b"H" + b"e" * 200 + b" ", b"")),
             ((b"Hi ", b"needle_cc_8", b" more"), (b"Hi ", b"needle_cc_8", b"x"), (b"hi ", b"needle_cc_8", b"")), lead="unbounded", eol=True),
        Expr(r"\Bneedle_cg_9\B", 14, b"needle_cg_9", ((b"q", b"z"), (b"_", b"0")), ((b"", b"needle_cg_9", b"z"), (b"q", b"needle_cg_9", b""), (b"-", b"needle_cg_9", b"z")), lead="zero"),
    ), nw="1"),
    Cell("ctx1_nomultiline", 2, (
        Expr("^.{0,6}needle_cd_9", 10, b"needle_cd_9", ((b"", b""), (b"abc", b""), (b"ab#def", b"")), ((b"abcdefg", b"needle_cd_9", b""),), lead="lt16", bol=True),
        Expr("needle_ce_10$", 10, b"needle_ce_10", ((b"", b""),), ((b"", b"needle_ce_10", b"x"), (b"", b"needle_ce_10", b"#")), lead="zero", eol=True),
        Expr(r"[a-z]{0,4}needle_ci_12\b", 10, b"needle_ci_12", ((b"", b""), (b"abcd", b""), (b"abcdef", b"")), ((b"ab", b"needle_ci_12", b"3"),), lead="lt16"),
        # consumes the newline at the end of a line: the match is accepted at the end of the scanned bytes, behind the '\n'
        Expr(r"\bneedle_cn_13[^a-z]", 10, b"needle_cn_13", ((b"", b"#"), (b"", b"")), ((b"", b"needle_cn_13", b"a"), (b"_", b"needle_cn_13", b"")), lead="zero", eol=True),
    ), nw="1", excluded={"multi/far_start": "the leads are bounded"}),
    Cell("ctx2", 2, (
        Expr(r"[a-z]{0,20}needle_cf_11[0-9]{1,20}\b", 14, b"needle_cf_11", ((b"", b"1"), (b"abc", b"12345"), (AZ[:20], D9 * 2), (AZ[:24], b"7")),
             ((b"ab", b"needle_cf_11", b"1x"), (b"ab", b"needle_cf_11", b""), (b"", b"needle_cf_11", D9 * 2 + b"1")), lead="ge17"),
        Expr("[a-z]{0,18}needle_cj_12[0-9]{2,18}z", 14, b"needle_cj_12", ((b"", b"12z"), (AZ[:18], D9 + b"12345678z"), (b"q", b"123z")),
             ((b"", b"needle_cj_12", b"1z"), (b"", b"needle_cj_12", D9 * 2 + b"z")), lead="ge17"),
        Expr("q?(?:needle_eta_77){1,3}z", 14, b"needle_eta_77", ((b"", b"z"), (b"q", b"z"), (b"needle_eta_77", b"z"), (b"qneedle_eta_77needle_eta_77", b"z")),
             ((b"", b"needle_eta_77", b"q"),), lead="lt16"),
    ), nw="2", excluded={"multi/far_start": "the leads are bounded"}),
    Cell("generic_all", 3, (
        Expr("needle_ga_12[0-9]*", 6, b"needle_ga_12", ((b"", b""), (b"", b"123"), (b"", D9)), lead="zero"),
        Expr("[a-z]{0,3}needle_gb_13x*", 6, b"needle_gb_13", ((b"", b""), (b"abc", b"xx"), (b"abcde", b"x")), lead="lt16"),
        Expr(r"\bneedle_gh_14[a-c]?\b", 6, b"needle_gh_14", ((b"", b""), (b"", b"a")), ((b"", b"needle_gh_14", b"ab"), (b"_", b"needle_gh_14", b"")), lead="zero"),
    ), excluded={"q_sweep": NO_Q, "multi/far_start": "the leads are bounded"}),
    Cell("generic_wide", 3, (
        Expr("[a-z]{0,40}needle_gc_14[0-9]{1,60}z", 14, b"needle_gc_14", ((b"", b"1z"), (AZ + AZ[:14], D9 * 6 + b"z"), (b"abc", b"123z")),
             ((b"", b"needle_gc_14", b"z"), (b"", b"needle_gc_14", D9 * 6 + b"1z")), lead="ge17"),
        Expr(r"[a-z]{0,35}needle_gd_15[0-9]{1,70}\b", 14, b"needle_gd_15", ((b"", b"1"), (AZ, D9 * 7), (b"xy", b"42")), ((b"", b"needle_gd_15", b"1x"), (b"", b"needle_gd_15", b"")),
             lead="ge17"),
    ), nw=">=3", excluded={"q_sweep": NO_Q, "multi/far_start": "the leads are bounded"}),
    Cell("huge", 4, (
        Expr("needle_ha_1.{0,1100}end_h", 14, b"needle_ha_1", ((b"", b"end_h"), (b"", b"abc end_h"), (b"", fill(1100, 3) + b"end_h")),
             ((b"", b"needle_ha_1", fill(1101, 3) + b"end_h"), (b"", b"needle_ha_1", b"abc end_")), lead="zero"),
        Expr(r"[0-9]{0,3}needle_hb_2.{0,1050}fin\b", 14, b"needle_hb_2", ((b"", b"fin"), (b"123", b" fin"), (b"7", fill(1050, 5) + b"fin")),
             ((b"", b"needle_hb_2", b"fine"), (b"", b"needle_hb_2", fill(1051, 5) + b"fin")), lead="lt16"),
    ), nw="huge", excluded={"q_sweep": NO_Q, "multi/far_start": "the leads are bounded"}),
    # the same shape with longer repeats: the other routines of hg_huge.hip under the confirm caller (the routine of each
    # expression is asserted through hugesim_py: HUGE_ROUTINES)
    Cell("huge_reg2", 4, (
        Expr("needle_hc_3.{0,2100}end_i", 14, b"needle_hc_3", ((b"", b"end_i"), (b"", b"abc end_i"), (b"", fill(2100, 3) + b"end_i")),
             ((b"", b"needle_hc_3", fill(2101, 3) + b"end_i"), (b"", b"needle_hc_3", b"abc end_")), lead="zero"),
        Expr(r"[0-9]{0,3}needle_hd_4.{0,2050}fim\b", 14, b"needle_hd_4", ((b"", b"fim"), (b"123", b" fim"), (b"7", fill(2050, 5) + b"fim")),
             ((b"", b"needle_hd_4", b"fime"), (b"", b"needle_hd_4", fill(2051, 5) + b"fim")), lead="lt16"),
    ), nw="huge", excluded={"q_sweep": NO_Q, "multi/far_start": "the leads are bounded"}),
    Cell("huge_reg4", 4, (
        Expr("needle_he_5.{0,4200}end_j", 14, b"needle_he_5", ((b"", b"end_j"), (b"", b"abc end_j"), (b"", fill(4200, 3) + b"end_j")),
             ((b"", b"needle_he_5", fill(4201, 3) + b"end_j"), (b"", b"needle_he_5", b"abc end_")), lead="zero"),
        Expr(r"[0-9]{0,3}needle_hf_6.{0,4150}fio\b", 14, b"needle_hf_6", ((b"", b"fio"), (b"123", b" fio"), (b"7", fill(4150, 5) + b"fio")),
             ((b"", b"needle_hf_6", b"fioe"), (b"", b"needle_hf_6", fill(61, 5) + b"fi")), lead="lt16"),
    ), nw="huge", excluded={"q_sweep": NO_Q, "multi/far_start": "the leads are bounded"}),
    # above 256 words: huge_run, on staged tables (the first) and on tables in L2 (the second: conditions and twelve byte classes
    # outgrow the staging area).  Only the first carries a sample as long as its repeat, the near miss one byte past the bound:
    # the text limit (huge_cells.py holds the repeat bounds of both routines from both sides)
    Cell("huge_lds", 4, (
        Expr("needle_hg_7.{0,8300}end_k", 14, b"needle_hg_7", ((b"", b"end_k"), (b"", b"abc end_k"), (b"", fill(1500, 3) + b"end_k")),
             ((b"", b"needle_hg_7", fill(8301, 3) + b"end_k"), (b"", b"needle_hg_7", b"abc end_")), lead="zero"),
        Expr(r"[0-9]{0,3}needle_hh_8.{0,8250}fiq\b", 14, b"needle_hh_8", ((b"", b"fiq"), (b"123", b" fiq"), (b"7", fill(50, 5) + b"fiq")),
             ((b"", b"needle_hh_8", b"fiqe"), (b"", b"needle_hh_8", fill(60, 5) + b"fi")), lead="lt16"),
    ), nw="huge", excluded={"q_sweep": NO_Q, "multi/far_start": "the leads are bounded"}),
    Cell("mixed_shared_ids", None, (
        Expr("needle_ma_1", 14, b"needle_ma_1", ((b"", b""),)),
        Expr("needle_mb_2[0-9]{1,3}x", 14, b"needle_mb_2", ((b"", b"5x"), (b"", b"123x")), ((b"", b"needle_mb_2", b"1234x"),)),
        Expr(r"\b[a-z]{0,4}needle_mc_3\b", 14, b"needle_mc_3", ((b"", b""), (b"abcd", b"")), ((b"abcde", b"needle_mc_3", b""), (b"ab", b"needle_mc_3", b"_")), lead="lt16"),
        Expr("[a-z]{0,40}needle_md_4[0-9]{1,60}z", 14, b"needle_md_4", ((b"", b"1z"), (AZ, D9 * 5 + b"z")), ((b"", b"needle_md_4", b"z"),), lead="ge17"),
    ), modes=(0, 1, 2, 3), excluded={"q_sweep": "covered by the cells of the single routines", "multi/far_start": "the leads are bounded"}),
]
BY_NAME = {c.name: c for c in CELLS}
# the huge cells: the routine of hg_huge.hip each expression runs in (hugesim_py.placement)
HUGE_ROUTINES = {"huge": ("reg1", "reg1"), "huge_reg2": ("reg2", "reg2"), "huge_reg4": ("reg4", "reg4"), "huge_lds": ("lds_staged", "lds_l2")}
# every cell plants each of these at least once, unless its `excluded` names the tag with the reason
REQUIRED_TAGS = (
    "align/hit", "align/miss",
    "tile/line_from_previous_tile", "tile/line_from_two_tiles_back", "tile/line_at_tile_start", "tile/newline_first_byte", "tile/literal_straddles",
    "tile/literal_straddles:miss", "tile/lead_straddles",
    "edge/line_at_byte_0", "edge/match_ends_the_text", "edge/near_miss_ends_the_text", "edge/literal_cut_by_the_end", "edge/one_chunk",
    "nul/leading", "nul/leading17", "nul/blocked", "nul/blocked_far", "nul/in_lead", "nul/leading_in_window", "nul/after_match", "nul/in_tail", "nul/before_newline",
    "nul/line_of_nuls_before",
    "break/later_piece", "break/later_piece_leading_nuls", "break/later_piece_nul_blocks", "break/inside_literal", "break/in_prefix", "break/right_after_match",
    "break/one_byte_before_match_end", "break/one_byte_after_match_end", "break/at_piece_start", "break/third_piece",
    "multi/fail_then_match", "multi/all_miss", "multi/overlap", "multi/twice", "multi/far_start", "multi/other_expression",
)


def placement_errors(cell: Cell, info: list) -> list:
    """What the compiler's placement of the cell's expressions (extsim_py.Db.pattern(i) dicts) gets wrong; [] when it is right."""
    bad = []
    for i, (e, p) in enumerate(zip(cell.exprs, info)):
        mode = cell.modes[i] if cell.modes else cell.mode
        if p["tier"] != 0 or p["mode"] != mode:
            bad.append((e.pattern, "tier/mode", p["tier"], p["mode"]))
        lead = p["lit_lead"]
        ok = {"zero": lead == 0, "lt16": 0 < lead < 16, "ge17": 17 <= lead < UNBOUNDED, "unbounded": lead == UNBOUNDED}[e.lead]
        if not ok:
            bad.append((e.pattern, "lit_lead", lead, e.lead))
        if not cell.modes:
            nw_ok = {"": True, "1": p["nw"] == 1, "2": p["nw"] == 2, ">=3": 3 <= p["nw"] <= 32, "huge": p["nw"] > 32}[cell.nw]
            if not nw_ok:
                bad.append((e.pattern, "nw", p["nw"], cell.nw))
        if mode == 0 and not (p["literal_only"] and p["single"]):
            bad.append((e.pattern, "literal_only/single"))
        if mode in (1, 2) and not p["single"]:
            bad.append((e.pattern, "single"))
    return bad


# ------------------------------------------------------------------ texts
@dataclass(frozen=True)
class Case:
    tag: str
    lo: int  # the planted bytes [lo, hi)
    hi: int
    fs: int  # where the sample's literal starts
    expr: int
    line: int  # where the sample's line starts


@dataclass
class Text:
    label: str
    data: bytes
    sizes: tuple  # the buffer_size values it is scanned with
    cases: list

    def tag_at(self, off: int) -> str:
        """The tag of the planted case that holds byte `off` ("filler" outside every case)."""
        k = bisect.bisect_right(self._los(), off) - 1
        if k >= 0 and off < self.cases[k].hi:
            c = self.cases[k]
            return f"{c.tag}[expr {c.expr}, fs {c.fs} = {c.fs % 16} mod 16, line at {c.line}]"
        return "filler"

    def _los(self):
        if not hasattr(self, "_lo_cache"):
            self._lo_cache = [c.lo for c in self.cases]
        return self._lo_cache


class _Builder:
    def __init__(self, label: str, sizes):
        self.label, self.sizes = label, tuple(sizes)
        self.buf = bytearray()
        self.cases = []

    def room(self, n: int) -> bool:
        return len(self.buf) + n + 64 <= MAX_TEXT

    def pad_to(self, target: int) -> None:
        """Filler lines (each at most 90 bytes, '\\n' included) up to offset `target`."""
        gap = target - len(self.buf)
        assert gap >= 0, (self.label, target, len(self.buf))
        while gap > 0:
            n = min(gap, 61 + len(self.buf) % 29)
            self.buf += fill(n - 1, len(self.buf)) + b"\n"
            gap -= n

    def plant(self, tag: str, blob: bytes, fs_in: int, expr: int, fs_abs: int | None = None, residue: int | None = None, newline: bool = True, line_in: int = 0) -> None:
        """Put `blob` (one or more lines; a '\\n' is added unless newline is False) so that its byte fs_in lands at fs_abs, or at
        the next offset with the given residue mod 16; filler lines make up the distance."""
        here = len(self.buf)
        if fs_abs is None:
            fs_abs = here + fs_in
            if residue is not None:
                fs_abs += (residue - fs_abs) % 16
        lo = fs_abs - fs_in
        self.pad_to(lo)
        self.buf += blob + (b"\n" if newline else b"")
        self.cases.append(Case(tag, lo, len(self.buf), fs_abs, expr, lo + line_in))

    def text(self) -> Text:
        assert len(self.buf) <= MAX_TEXT, (self.label, len(self.buf))
        return Text(self.label, bytes(self.buf), self.sizes, self.cases)


def _line(e: Expr, s, front: int = 0, back: int = 0, salt: int = 0):
    """(line bytes without the newline, offset of the literal in them) of a sample with filler around it, where the
    expression allows filler."""
    pre, lit, post = s
    f = b"" if e.bol else fill(front, salt)
    b = b"" if e.eol else fill(back, salt + 1)
    return f + pre + lit + post + b, len(f) + len(pre)


def _main_text(cell: Cell, leads) -> Text:
    b = _Builder("main", (DEFAULT_BS, 101))
    b.buf += fill(40, 1) + b"\n"
    # align: every sample with its literal at every residue; in front of it, more filler than the lead where the lead is
    # bounded (q = fs - lead inside the line) and none for every other sample
    for ei, e in enumerate(cell.exprs):
        lead = leads[ei]
        far = lead + 3 if 0 < lead < 64 else 5
        for good in (True, False):
            for si, s in enumerate(e.samples(good)):
                front = far if si % 2 == 0 else 0
                line, fs_in = _line(e, s, front, 4 + si, salt=si)
                sub = ("hit" if good else "miss") + (":far" if front and not e.bol and 0 < lead < 64 else "")
                for r in (range(16) if len(line) <= 120 else (0, 5, 10, 15)):
                    if b.room(len(line) + 16):
                        b.plant(f"align/{sub}", line, fs_in, ei, residue=r)
    # nul
    for ei, e in enumerate(cell.exprs):
        g = e.samples(True)[min(1, len(e.good) - 1)]
        longest = max(e.samples(True), key=lambda s: (len(s[0]) if len(s[0]) <= 40 else 0))
        for r in (3, 14):
            line, fs_in = _line(e, g, 6, 3)
            b.plant("nul/leading", b"\0\0\0" + line, fs_in + 3, ei, residue=r)
            b.plant("nul/leading17", b"\0" * 17 + line, fs_in + 17, ei, residue=r)
            b.plant("nul/blocked", b"#\0" + line, fs_in + 2, ei, residue=r)
            b.plant("nul/blocked_far", b"#\0" + fill(45, 2) + line, fs_in + 47, ei, residue=r)
            if len(longest[0]) >= 2:
                pre, lit, post = longest
                k = len(pre) // 2
                b.plant("nul/in_lead", b"#" + pre[:k] + b"\0" + pre[k:] + lit + post, len(pre) + 2, ei, residue=r)
                b.plant("nul/leading_in_window", b"\0" * 5 + pre[-1:] + lit + post, 6, ei, residue=r)
            sample = g[0] + g[1] + g[2]
            head = b"" if e.bol else fill(4, 7)
            b.plant("nul/after_match", head + sample + b"\0" + fill(5, 3), len(head) + len(g[0]), ei, residue=r)
            b.plant("nul/before_newline", head + sample + b"\0", len(head) + len(g[0]), ei, residue=r)
            with_tail = next((s for s in e.samples(True) if len(s[2]) >= 1), None)
            if with_tail:
                pre, lit, post = with_tail
                k = len(post) // 2
                b.plant("nul/in_tail", head + pre + lit + post[:k] + b"\0" + post[k:], len(head) + len(pre), ei, residue=r)
            b.plant("nul/line_of_nuls_before", b"\0" * 7 + b"\n" + line, fs_in + 8, ei, residue=r, line_in=8)
    # multi
    n = len(cell.exprs)
    for ei, e in enumerate(cell.exprs):
        g = e.samples(True)[0]
        for r in (1, 12):
            if not e.bol:
                for si, s in enumerate(e.samples(False)[:3]):
                    miss = s[0] + s[1] + s[2]
                    line = fill(3, si) + miss + fill(3 + si, 5) + g[0] + g[1] + g[2]
                    b.plant("multi/fail_then_match", line, 3 + len(s[0]), ei, residue=r)
            misses = e.samples(False)
            m0, m1 = misses[0], misses[-2]
            b.plant("multi/all_miss", m0[0] + m0[1] + m0[2] + fill(3, 4) + m1[0] + m1[1] + m1[2] + fill(2, 1) + e.lit[:-1], len(m0[0]), ei, residue=r)
            head = b"" if e.bol else fill(2, 9)
            b.plant("multi/overlap", head + g[0] + g[1] + g[0] + g[1] + g[2], len(head) + len(g[0]), ei, residue=r)
            b.plant("multi/twice", head + g[0] + g[1] + g[2] + fill(2, 1) + g[0] + g[1] + g[2], len(head) + len(g[0]), ei, residue=r)
            if e.lead == "unbounded":
                far_s = max(e.samples(True), key=lambda s: len(s[0]))
                b.plant("multi/far_start", head + far_s[0] + far_s[1] + far_s[2], len(head) + len(far_s[0]), ei, residue=r)
            # another expression's sample behind this one's, and a near miss of this one behind another's match
            o = cell.exprs[(ei + 1) % n]
            if n > 1 and not o.bol and not e.eol:
                og = o.samples(True)[0]
                line = head + g[0] + g[1] + g[2] + fill(3, 2) + og[0] + og[1] + og[2]
                b.plant("multi/other_expression", line, len(head) + len(g[0]), ei, residue=r)
    if cell.modes:  # needles of every routine on one line, in both orders, matching and not
        order = [i for i, e in enumerate(cell.exprs) if not e.bol and not e.eol]
        for r in range(16):
            for k, seq in enumerate((order, order[::-1], order[1:] + order[:1])):
                parts, fs_in = [fill(2, r)], None
                for j, ei in enumerate(seq):
                    e = cell.exprs[ei]
                    ss = e.samples((r + j + k) % 3 != 0)
                    s = ss[(r + j) % len(ss)]
                    if j == 0:
                        fs_in = 2 + len(s[0])
                    parts += [s[0] + s[1] + s[2], fill(1 + (r + j) % 3, j)]
                b.plant("multi/all_routines", b"".join(parts), fs_in, seq[0], residue=r)
    return b.text()


def _tile_texts(cell: Cell, leads) -> list:
    """One event per tile edge, six tiles per text."""
    events = []  # (tag, expr, blob, fs_in, fs relative to the edge, line_in, edges used)
    ex = cell.exprs
    n = len(ex)
    free = [i for i, e in enumerate(ex) if not e.bol] or list(range(n))

    def ev(tag, ei, s, front, rel, back=5, edges=1, prefix=b""):
        line, fs_in = _line(ex[ei], s, front, 0 if edges == 2 else back)
        events.append((tag, ei, prefix + line, len(prefix) + fs_in, rel, len(prefix), edges))

    for j in range(max(2, min(n, 3))):  # a line that starts in the previous tile, the whole sample in this one
        ei = free[j % len(free)]
        s = ex[ei].samples(True)[j % len(ex[ei].good)]
        ev("tile/line_from_previous_tile", ei, s, 100 + 7 * j, len(s[0]) + 3 + 5 * j)
    ei = free[0]
    ev("tile/line_from_two_tiles_back", ei, ex[ei].samples(True)[0], 2000 + TILE + 2100, 2100, edges=2)
    for j in range(2):
        ei = j % n
        s = ex[ei].samples(True)[-1 if len(ex[ei].good[-1][0]) < 64 else 0]
        ev("tile/line_at_tile_start", ei, s, 0, len(s[0]), prefix=b"")  # the line starts at the edge: filler in front is a line of its own
        ev("tile/newline_first_byte", (ei + 1) % n, ex[(ei + 1) % n].samples(True)[0], 0, 1 + len(ex[(ei + 1) % n].samples(True)[0][0]))
    for j, off in enumerate((1, 2, 3, 5, 7, 8, 10, 4, 6)):  # the literal across the edge; every third one a near miss
        ei = j % n
        e = ex[ei]
        good = j % 3 != 2
        s = e.samples(good)[0 if good else -2]  # (-2: the broken literal)
        off = min(off, len(s[1]) - 1)
        ev("tile/literal_straddles" + ("" if good else ":miss"), ei, s, 9, -off)
    for j in range(3):  # the lead across the edge, the literal behind it
        cand = [(ei, s) for ei, e in enumerate(ex) for s in e.samples(True) if 2 <= len(s[0]) <= 64]
        if not cand:
            break
        ei, s = cand[j % len(cand)]
        ev("tile/lead_straddles", ei, s, 4, 1 + (j * (len(s[0]) - 2)) // 2)
    texts, b, edge = [], None, 0
    for tag, ei, blob, fs_in, rel, line_in, edges in events:
        if b is None or edge + edges > 5:
            if b is not None:
                texts.append(b.text())
            b, edge = _Builder(f"tile{len(texts)}", (DEFAULT_BS, 20001, 4097)), 0
        edge += edges
        t = edge * TILE
        fs_abs = t + rel
        if tag == "tile/newline_first_byte":  # the previous line's '\n' is byte 0 of the tile
            b.pad_to(t - 40)
            b.buf += fill(40, 3) + b"\n"
            assert len(b.buf) == t + 1 and fs_abs - fs_in == t + 1
        if tag == "tile/line_at_tile_start":
            assert fs_abs - fs_in == t
        b.plant(tag, blob, fs_in, ei, fs_abs=fs_abs, line_in=line_in)
    texts.append(b.text())
    return texts


# the text-edge texts that also run on guarded buffers (gpu_cases.guarded_cases): cell -> labels
GUARDED_EDGES = {
    "lit": ("edge_end0_0", "edge_end1_2", "edge_cut_1", "edge_tiny_0"),
    "simple_bounded": ("edge_end0_1", "edge_end1_0", "edge_cut_2", "edge_tiny_0"),
    "ctx1": ("edge_end0_0", "edge_end1_2", "edge_endmiss1_2", "edge_cut_3", "edge_tiny_0"),
}


def guarded_edge_cases():
    """(name, text, patterns, flags, ids, buffer_size) of the text-edge class of three cells, for buffers whose end is
    followed by unmapped memory: the confirm walks may read up to the size rounded up to 16, not a byte further."""
    for name, labels in GUARDED_EDGES.items():
        cell = BY_NAME[name]
        texts = {t.label: t for t in edge_texts(cell)}
        for label in labels:
            yield (f"confirm-{name}-{label}", texts[label].data, cell.patterns, cell.flags, cell.ids(False), DEFAULT_BS)


def edge_texts(cell: Cell) -> list:
    """Small texts of their own: what the start and the end of a text can meet."""
    out = []
    n = len(cell.exprs)

    def one(label, tag, ei, blob, fs_in, head=b"", newline=True, tail=b""):
        b = _Builder(f"edge_{label}_{ei}", (DEFAULT_BS, 64))
        b.buf += head
        b.plant(tag, blob, fs_in, ei, newline=newline)
        b.buf += tail
        out.append(b.text())

    for ei, e in enumerate(cell.exprs):
        short = min(e.samples(True), key=lambda s: len(s[0] + s[1] + s[2]))
        g = [s for s in e.samples(True) if len(s[0]) <= 40 and len(s[2]) <= 40][-1]
        whole = short[0] + short[1] + short[2]
        one("byte0", "edge/line_at_byte_0", ei, g[0] + g[1] + g[2], len(g[0]), tail=fill(30, 1) + b"\n" + fill(11, 2) + b"\n")
        for k, lead_in in enumerate((fill(20, 4) + b"\n", fill(41 + ei, 4) + b"\n" + fill(3 + ei, 1) + b"\n")):
            # the match ends at the last byte of the text; the lengths differ mod 16
            head = b"" if e.bol else fill(2 + k, 6)
            one(f"end{k}", "edge/match_ends_the_text", ei, head + g[0] + g[1] + g[2], len(head) + len(g[0]), head=lead_in, newline=False)
            miss = e.samples(False)[0]
            one(f"endmiss{k}", "edge/near_miss_ends_the_text", ei, head + miss[0] + miss[1] + miss[2], len(head) + len(miss[0]), head=lead_in, newline=False)
        one("cut", "edge/literal_cut_by_the_end", ei, g[0] + g[1][:-2], len(g[0]), head=fill(25 + ei, 2) + b"\n", newline=False)
        tag = "edge/one_chunk" if len(whole) <= 16 else "edge/short_text"
        one("tiny", tag, ei, whole, len(short[0]), newline=False)
        one("tinynl", tag, ei, whole[:15], len(short[0]), newline=True)
        one("tinycut", "edge/one_chunk_cut", ei, (short[0] + short[1])[:-1], len(short[0]), newline=False)
    return out


def _break_texts(cell: Cell, bs1: int) -> list:
    """Lines longer than bs1 bytes: the line's pieces start every bs1 bytes from its start.  Events sit at the break
    B = line start + k * bs1.  Up to 4096 every expression gets every kind of event; above a tile, where one line fills a
    sixth of a text, every kind is planted once, for expressions that change with the kind and with bs1.  A text that is
    full is closed and the next one begun: no event is dropped."""
    texts = []
    ex = cell.exprs
    k = 3 if bs1 < 100 else 2 if bs1 < 1000 else 1
    tailroom = max(300 - k * bs1, bs1 // 3 if bs1 < 4096 else 0) + 40

    def builder():
        nb = _Builder(f"break{bs1}_{len(texts)}", (bs1 + 1,))
        nb.buf += fill(30, 2) + b"\n"
        return nb

    b = builder()

    def event(tag, ei, s, rel_fs, nuls=0, kk=None):
        """The literal of sample s starts at B + rel_fs; nuls > 0: that many NULs at the start of piece kk; nuls < 0: one NUL
        between the start of the piece and the occurrence."""
        nonlocal b
        e = ex[ei]
        kk = kk or k
        brk = kk * bs1
        pre, lit, post = s
        start = brk + rel_fs - len(pre)  # the sample's offset in the line
        body = bytearray(fill(start, ei + kk))
        for i in range(max(nuls, 0)):
            body[brk + i] = 0
        if nuls < 0:
            body[brk + 2] = 0
        body += pre + lit + post
        if not e.eol:
            body += fill(tailroom, 3)
        if not b.room(len(body) + 100):
            texts.append(b.text())
            b = builder()
        assert b.room(len(body) + 100), (cell.name, bs1, tag, len(body))
        b.plant(tag, bytes(body), start + len(pre), ei)

    events = []
    for ei, e in enumerate(ex):
        g = e.samples(True)[0]
        sample_len = len(g[0] + g[1] + g[2])
        with_pre = next((s for s in e.samples(True) if 2 <= len(s[0]) <= 40), None)
        events.append(("break/inside_literal", ei, g, -4, 0))
        if not e.bol:
            events.append(("break/right_after_match", ei, g, -(sample_len - len(g[0])), 0))
            events.append(("break/one_byte_before_match_end", ei, g, -(sample_len - len(g[0])) + 1, 0))
            events.append(("break/one_byte_after_match_end", ei, g, -(sample_len - len(g[0])) - 1, 0))
        events.append(("break/later_piece_leading_nuls", ei, g, (3 + len(g[0])) if e.bol else 10 + len(g[0]), 3))
        if with_pre:
            events.append(("break/in_prefix", ei, with_pre, 1, 0))
            events.append(("break/in_prefix", ei, with_pre, len(with_pre[0]) - 1, 0))
        events.append(("break/at_piece_start", ei, g, len(g[0]), 0))
        events.append(("break/later_piece", ei, g, len(g[0]) if e.bol else 12 + len(g[0]), 0))
        events.append(("break/later_piece_nul_blocks", ei, g, 12 + len(g[0]), -1))
        miss = e.samples(False)[0]
        events.append(("break/later_piece:miss", ei, miss, len(miss[0]) if e.bol else 12 + len(miss[0]), 0))
    by_kind = {}
    for v in events:
        by_kind.setdefault(v[0], []).append(v)
    kinds = list(by_kind)
    if bs1 > 4096:
        for ki, kind in enumerate(kinds):
            lst = by_kind[kind]
            if kind == "break/in_prefix":  # where the prefix may be empty, the rest of the sample still matches from the piece start
                lst = [v for v in lst if any(not pre for pre, _ in ex[v[1]].good)] or lst
            j = ki + BREAK_BS1.index(bs1)
            by_kind[kind] = [lst[(j + x) % len(lst)] for x in ((0, len(lst) // 2) if kind == "break/in_prefix" else (0,))]  # (in_prefix: two expressions, where two have a prefix)
    # the kinds in turn, so that neighbouring lines hold different kinds
    turn = 0
    while any(by_kind.values()):
        kind = kinds[turn % len(kinds)]
        turn += 1
        if by_kind[kind]:
            event(*by_kind[kind].pop((turn // len(kinds)) % len(by_kind[kind])))
    # an occurrence two breaks into the line (bs1 20000: a line of 40 KiB)
    ei = next((i for i, e in enumerate(ex) if not e.bol), 0)
    g = ex[ei].samples(True)[0]
    event("break/third_piece", ei, g, 25 + len(g[0]), kk=k + 1 if bs1 <= 1000 else 2)
    texts.append(b.text())
    return texts


@functools.lru_cache(maxsize=None)
def cell_texts(name: str, leads: tuple) -> tuple:
    """The texts of a cell.  leads: lit_lead of each expression as compiled (the filler in front of the ":far" samples
    exceeds it, so that the window starts inside the line)."""
    cell = BY_NAME[name]
    return tuple([_main_text(cell, leads)] + _tile_texts(cell, leads) + edge_texts(cell) + [t for bs1 in BREAK_BS1 for t in _break_texts(cell, bs1)])


@functools.lru_cache(maxsize=None)
def compiled(name: str) -> tuple:
    """The host compile's placement of the cell's expressions: extsim_py.Db.pattern(i) of each."""
    import extsim_py

    cell = BY_NAME[name]
    db = extsim_py.Db(cell.patterns, cell.flags, cell.ids(False), mode="plain")
    assert db.h, (name, db.error)
    return tuple(db.pattern(i) for i in range(len(cell.exprs)))


def compiled_leads(name: str) -> tuple:
    return tuple(p["lit_lead"] for p in compiled(name))


# ------------------------------------------------------------------ reference
def sort_hits(h) -> np.ndarray:
    h = np.asarray(h, dtype=np.uint64).reshape(-1, 5)
    return h[np.lexsort(tuple(h[:, c] for c in range(4, -1, -1)))]


def reference(data: bytes, patterns, flags, ids, buffer_size: int):
    """(sorted uint64 [n, 5] of (line, id, to, start, len), n_lines): the oracle's reports with the piece geometry of
    invert_ref.pieces; the oracle's own geometry columns are returned third, for the check that the two agree."""
    rc, hits, nlines = oracle_py.scan_buffer(data, patterns, flags=flags, ids=ids, buffer_size=buffer_size)
    assert rc == 0, rc
    pcs = invert_ref.pieces(data, buffer_size)
    assert len(pcs) == nlines, (len(pcs), nlines)
    rows = [(ln, rid, to, pcs[ln][0], len(pcs[ln][1])) for ln, rid, to, _, _ in hits]
    return sort_hits(rows), nlines, sort_hits(hits)


_REF = {}


def cell_reference(name: str, leads: tuple, text_index: int, buffer_size: int, shared: bool):
    key = (name, leads, text_index, buffer_size, shared)
    if key not in _REF:
        cell = BY_NAME[name]
        _REF[key] = reference(cell_texts(name, leads)[text_index].data, cell.patterns, cell.flags, cell.ids(shared), buffer_size)
    return _REF[key]


def diff_tags(text: Text, got: np.ndarray, want: np.ndarray) -> set:
    """"missing <tag>" / "extra <tag>" of every hit that one side lacks."""
    rows = lambda a: np.ascontiguousarray(a).view([("", np.uint64)] * 5).ravel()  # noqa: E731
    short = lambda h: text.tag_at(int(h[3])).split("[")[0]  # noqa: E731
    return {f"missing {short(h)}" for h in np.setdiff1d(rows(want), rows(got))} | {f"extra {short(h)}" for h in np.setdiff1d(rows(got), rows(want))}


def diff_report(text: Text, got: np.ndarray, want: np.ndarray, limit: int = 5) -> str:
    """The first missing and extra hits with the tags of the planted cases they lie in."""
    rows = lambda a: np.ascontiguousarray(a).view([("", np.uint64)] * 5).ravel()  # noqa: E731
    where = lambda h: f"{tuple(int(x) for x in h)} ends at {int(h[3]) + int(h[2])} (tile {(int(h[3]) + int(h[2])) // TILE}) in {text.tag_at(int(h[3]))}"  # noqa: E731
    missing, extra = np.setdiff1d(rows(want), rows(got))[:limit], np.setdiff1d(rows(got), rows(want))[:limit]
    return f"{len(got)} hits, want {len(want)}; missing {[where(h) for h in missing]}; extra {[where(h) for h in extra]}"
