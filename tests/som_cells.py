"""The cells of the backward walk (som_walk, hypergrep_amd/csrc/hg_som.hip) and of its two kernels, hg_som_kernel (`from` of a
delivered report) and hg_minlen_kernel (which raw reports survive min_length), shared by the host test (test_som_cells.py)
and the GPU test (test_som_cells_gpu.py).

A text is (database, buffer_size, cells).  A cell is a run of whole lines of its text: filler lines of `-` that move the cell's
line to the offset it wants, then the planted line.  The packer (Pack) knows the offset of every line, so a cell can ask for
`a mod 64` of its line (a: the piece's first scanned byte, relative to the text pointer) or for `top mod 64` of the match it
plants (top = a + to - 1; the kernel's chunks are top & ~15 downward).  The pieces a cell covers identify it: a report belongs
to the cell whose bytes hold the piece's first byte.

Expected reports come from Python `re` only: minlensim_py.expected_piece (somsim_py.start_by_brute_force over
regex_gen.ends_by_brute_force) on every piece of a text (reference()).  Nothing here calls the product or the host replay.

Tags say what a cell is FOR; test_som_cells.py proves each from the compiler's read-out and from the trace of the host
restatement of the walk (somsim_walk), so that a cell that stopped reaching its target is noticed:

  ("top", m)          a walk of the cell starts at top mod 64 == m
  ("exit", how, nw)   a start-of-match walk of an expression with nw state words ends that way (somsim_py.EXITS)
  ("mexit", how, nw)  the same for a match-length walk (the early mode, hg_minlen_kernel)
  ("at_lo", nw)       a match-length walk with to > max_len returns at its last position, q == lo
  ("rounds", n)       a walk of the cell takes n or more 64-byte rounds
  ("from", id, to, s) the reference's report (id, to) of the cell's planted line has from == s (stated by hand)
  ("absent", id)      the cell has no report of that id
  "empty"             the cell must have no report at all
No expression of any cell matches inside filler."""
from __future__ import annotations

from dataclasses import dataclass, field

import minlensim_py
import somsim_py

SOM = 256
A = 6  # DOTALL | MULTILINE
S = A | SOM
BIG = 262140
FILL = b"-"

SPANS = (2, 3, 15, 16, 17, 18, 47, 48, 49, 63, 64, 65, 66, 129)
SPANS_WIDE = SPANS + (257,)
TOPS_FEW = (0, 1, 15, 16, 17, 31, 32, 47, 48, 63)
STARTS_A = (0, 1, 15, 16, 17, 48, 63)  # a mod 64 of group B.2
TOPS_H = (0, 15, 16, 63)


@dataclass(frozen=True)
class Db:
    name: str
    pats: tuple
    flags: tuple
    ids: tuple
    need: tuple        # min_length per expression (None: no parameter)
    shape: tuple       # per expression the asserted read-out (nw, max_len, literal_only)

    @property
    def filtering(self) -> bool:
        return any(self.need)


def db(name, rows):
    """rows: (expression, flags, id, min_length, (nw, max_len, literal_only))"""
    return Db(name, tuple(r[0] for r in rows), tuple(r[1] for r in rows), tuple(r[2] for r in rows), tuple(r[3] for r in rows), tuple(r[4] for r in rows))


# ---- the expressions.  head + [a-p]{...} + z: every state class has a bounded and an unbounded one.  (nw, max_len, literal_only)
# are READ from the compiled database and asserted by the host test; they are stated here, never assumed by a cell's reference.
# The 32-word classes: `q[a-p]{0,1000}z` has about a thousand live nodes behind its q (measured in the parts stage at 1.7 ms
# per byte), so it keeps short spans; the long spans take 32-word expressions with few live nodes (`Y{990}|...`: the walked
# branch's nodes are the last three of 993).
B1, B2, B3, B32 = "q[a-p]{0,20}z", "q[a-p]{0,50}z", "q[a-p]{0,80}z", "q[a-p]{0,1000}z"
U1, U2, U3 = "q[a-p]*z", "q[a-p]*([r-s][t-u]){20}z", "q[a-p]*([r-s][t-u]){40}z"
U32 = "q[a-p]*([r-s][t-u]){500}z"
B32S, U32S = "S[A-P]{929}|q[a-p]{0,80}z", "Y{990}|q[a-p]*z"
WB1, WB2, WB3 = r"\bq[a-p]{0,20}z\b", r"\bq[a-p]{0,50}z\b", r"\bq[a-p]{0,80}z\b"
WB32S = r"\b(S[A-P]{929}|q[a-p]{0,80}z)\b"
RUN32 = b"S" + b"A" * 929  # the longest match of B32S: one live node per byte (a run of one letter under `Y{930}` keeps 930)
ML_FULL32 = "T[A-P]{929}|k[a-p]{0,80}z"  # group H's 32-word expression with min_length == max_len: its longest match is T and 929 letters


def head(expr: str, h: str) -> str:
    """The expression with another head letter (so that several classes live in one database without sharing matches)."""
    return expr.replace("q[", h + "[")


DBS = {d.name: d for d in (
    db("w1", [(B1, S, 0, None, (1, 22, 0)), (U1, S, 1, None, (1, 0, 0))]),
    db("w2", [(B2, S, 0, None, (2, 52, 0)), (U2, S, 1, None, (2, 0, 0))]),
    db("w3", [(B3, S, 0, None, (3, 82, 0)), (U3, S, 1, None, (3, 0, 0))]),
    db("w32", [(B32S, S, 0, None, (32, 930, 0)), (U32S, S, 1, None, (32, 0, 0))]),
    db("dense32", [(B32, S, 0, None, (32, 1002, 0))]),
    db("long32", [(U32, S, 0, None, (32, 0, 0))]),
    # B: how the walk ends
    db("start", [("^q[a-p]*z", S, 0, None, (1, 0, 0)), (WB3, S, 1, None, (3, 82, 0)), (".*z", S, 2, None, (1, 0, 0)), ("z", S, 3, None, (1, 1, 0)),
                 ("^q[a-p]*([r-s][t-u]){40}z", S, 4, None, (3, 0, 0)), ("^(Y{990}|q[a-p]*z)", S, 5, None, (32, 0, 0)), ("^q[a-p]{0,50}z", S, 6, None, (2, 52, 0))]),
    db("bound", [(B1, S, 0, None, (1, 22, 0)), (B2, S, 1, None, (2, 52, 0)), (B3, S, 2, None, (3, 82, 0)), (WB1, S, 3, None, (1, 22, 0)),
                 (WB2, S, 4, None, (2, 52, 0)), (WB3, S, 5, None, (3, 82, 0))]),
    db("bound32", [(B32S, S, 0, None, (32, 930, 0)), (WB32S, S, 1, None, (32, 930, 0))]),
    # C: piece starts that are not line starts
    db("piece", [(r"\bq[a-p]{0,20}z", S, 0, None, (1, 22, 0)), ("[a-c]+z", S, 1, None, (1, 0, 0)), (r"\bq[a-p]{0,80}z", S, 2, None, (3, 82, 0)),
                 ("^q[a-p]*z", S, 3, None, (1, 0, 0))]),
    # D: contexts at `to`
    db("ctx", [("q[a-p]*z$", S, 0, None, (1, 0, 0)), ("q[a-p]*z$", 2 | SOM, 1, None, (1, 0, 0)), (r"q[a-p]*z\b", S, 2, None, (1, 0, 0)),
               (r"q[a-p]*z\B", S, 3, None, (1, 0, 0)), ("q[a-p]{0,80}z$", S, 4, None, (3, 82, 0)), (r"q[a-p]{0,80}z\b", S, 5, None, (3, 82, 0)),
               (r"q[a-p]{0,80}z\B", S, 6, None, (3, 82, 0)),
               # a match that takes the piece's final newline in: the pending position's own byte is the last of the piece
               ("q[a-p]*z\\n", S, 7, None, (1, 0, 0)), ("q[a-p]{0,80}z\\n", S, 8, None, (3, 83, 0)),
               # the \b and \B tails without MULTILINE (ids 2 and 3 again: their reports must be the same)
               (r"q[a-p]*z\b", 2 | SOM, 9, None, (1, 0, 0)), (r"q[a-p]*z\B", 2 | SOM, 10, None, (1, 0, 0))]),
    # E: several starts
    db("multi", [("[a-c]+z", S, 0, None, (1, 0, 0)), ("a|aaa", S, 1, None, (1, 3, 0)), ("(ab|b)c", S, 2, None, (1, 3, 0)), ("q[a-q]*z", S, 3, None, (1, 0, 0)),
                 ("q[a-q]{0,80}z", S, 4, None, (3, 82, 0))]),
    # F: lanes and state homes
    db("lane3", [(B3, S, 0, None, (3, 82, 0))]),
    db("lane32", [(U32S, S, 0, None, (32, 0, 0))]),
    db("lane32d", [(B32, S, 0, None, (32, 1002, 0))]),
    db("mix", [(B1, S, 0, None, (1, 22, 0)), (head(B2, "r"), S, 1, None, (2, 52, 0)), (head(B3, "s"), S, 2, None, (3, 82, 0)),
               (head(U32S, "t"), S, 3, None, (32, 0, 0)), (head(B3, "u"), A, 4, None, (3, 82, 0))]),
    db("nolds", [(B1, S, 0, None, (1, 22, 0)), (head(B3, "u"), A, 1, None, (3, 82, 0))]),
    # G: shared ids.  id 1: one and three words; id 2: one, three and 32 words; id 3: a literal alone; id 4: a literal with a
    # regular expression; id 5: two literals
    db("share", [(B1, S, 1, None, (1, 22, 0)), ("x[a-q]{0,80}z", S, 1, None, (3, 82, 0)),
                 ("r[a-p]{0,20}z", S, 2, None, (1, 22, 0)), ("w[a-r]{0,80}z", S, 2, None, (3, 82, 0)), ("Y{990}|y[a-w]*z", S, 2, None, (32, 0, 0)),
                 ("needle", S, 3, None, (1, 6, 1)), ("hay-stack", S, 4, None, (1, 9, 1)), ("h[a-y-]{0,20}stack", S, 4, None, (1, 26, 0)),
                 ("abcde-f", S, 5, None, (1, 7, 1)), ("cde-f", S, 5, None, (1, 5, 1))]),
    # H: min_length without the flag (hg_minlen_kernel)
    db("ml", [(B1, A, 0, 10, (1, 22, 0)), (head(B2, "r"), A, 1, 10, (2, 52, 0)), (head(B3, "s"), A, 2, 10, (3, 82, 0)), (head(B32S, "t"), A, 3, 10, (32, 930, 0)),
              ("[a-c]+z", A, 4, 4, (1, 0, 0)), (head(U1, "u"), A, 5, None, (1, 0, 0)), (head(B1, "v"), A, 6, 22, (1, 22, 0)),
              (head(B2, "w"), A, 7, 52, (2, 52, 0)), (head(B3, "x"), A, 8, 82, (3, 82, 0)), (ML_FULL32, A, 9, 930, (32, 930, 0))]),
    db("compact", [(B1, A, 0, 10, (1, 22, 0))]),
    # I: both together
    db("share_ml", [(B1, S, 1, None, (1, 22, 0)), ("x[a-q]{0,80}z", S, 1, 8, (3, 82, 0)),
                    ("r[a-p]{0,20}z", S, 2, 4, (1, 22, 0)), ("w[a-r]{0,80}z", S, 2, 7, (3, 82, 0)), ("Y{990}|y[a-w]*z", S, 2, 12, (32, 0, 0)),
                    ("needle", S, 3, None, (1, 6, 1)), ("hay-stack", S, 4, None, (1, 9, 1)), ("h[a-y-]{0,20}stack", S, 4, 12, (1, 26, 0))]),
    db("bound_ml", [(B1, S, 0, 22, (1, 22, 0)), (B2, S, 1, 40, (2, 52, 0)), (B3, S, 2, 82, (3, 82, 0)), (WB1, S, 3, 21, (1, 22, 0)),
                    (WB2, S, 4, 52, (2, 52, 0)), (WB3, S, 5, 60, (3, 82, 0))]),
    db("bound32_ml", [(B32S, S, 0, 930, (32, 930, 0)), (WB32S, S, 1, 930, (32, 930, 0))]),
    db("start_ml", [("^q[a-p]*z", S, 0, 5, (1, 0, 0)), (WB3, S, 1, 5, (3, 82, 0)), (".*z", S, 2, 3, (1, 0, 0)), ("^q[a-p]{0,50}z", S, 3, 5, (2, 52, 0))]),
)}


@dataclass
class Cell:
    name: str
    group: str
    data: bytes              # filler lines, then the planted line
    planted: int             # offset of the planted line in `data`
    tags: tuple
    offset: int = 0          # of `data` in its text (set by the packer)


@dataclass
class Text:
    name: str
    db: str
    bs: int
    cells: list = field(default_factory=list)

    @property
    def data(self) -> bytes:
        return b"".join(c.data for c in self.cells)


class Pack:
    """Builds one text cell by cell and knows where the next line starts."""

    def __init__(self, name: str, dbname: str, bs: int = BIG):
        self.text = Text(name, dbname, bs)
        self.at = 0

    def cell(self, name, group, line: bytes, tags=(), a_mod=None, top_at=None):
        """line: the planted line (with its newline, unless it ends the text).  a_mod: the line starts at an offset of that
        residue mod 64.  top_at = (m, to): the byte to - 1 of the line lies at residue m instead."""
        if top_at is not None:
            a_mod = (top_at[0] - (top_at[1] - 1)) % 64
        filler = b""
        if a_mod is not None:
            k = (a_mod - self.at) % 64
            if k:
                filler = FILL * (k - 1) + b"\n"
        assert not self.text.cells or self.text.cells[-1].data.endswith(b"\n"), name
        c = Cell(f"{self.text.name}/{name}", group, filler + line, len(filler), tuple(tags), self.at)
        self.text.cells.append(c)
        self.at += len(c.data)
        assert a_mod is None or (c.offset + c.planted) % 64 == a_mod
        return c


def word(n: int, h: bytes = b"q", body: bytes = b"a") -> bytes:
    """A match of n >= 2 bytes of a head + [a-p]{..} + z expression."""
    return h + body * (n - 2) + b"z"


def tail20(n: int, pairs: int) -> bytes:
    """A match of n bytes of q[a-p]*([r-s][t-u]){pairs}z."""
    assert n >= 2 * pairs + 2
    return b"q" + b"a" * (n - 2 * pairs - 2) + b"rt" * pairs + b"z"


# ---- A: top and span grid.  One non-matching byte before each match: the state dies one byte left of the start.
def _grid(dbname, tops, spans, makers, more=None):
    """makers: [(id, longest span or 0, shortest span, maker(n))]; every (top, span) with the expressions that can hold it."""
    d = DBS[dbname]
    pk = Pack("A/" + dbname, dbname)
    for n in spans:
        for rid, longest, shortest, make in makers:
            if n < shortest or (longest and n > longest):
                continue
            for m in tops:
                nw = d.shape[d.ids.index(rid)][0]
                tags = (("top", m), ("exit", "lo" if n == d.shape[d.ids.index(rid)][1] else "died", nw), ("from", rid, 2 + n, 2))  # (span max_len: the walk ends at lo)
                pk.cell(f"id {rid} span {n} top {m}", "A", FILL * 2 + make(n) + b"\n", tags, top_at=(m, 2 + n))
    if more:
        more(pk)
    return pk.text


def _w32_max_len(pk):
    """The bounded 32-word expression's max_len is its other branch's: S and 929 letters, at every top of the grid."""
    for m in TOPS_FEW:
        pk.cell(f"id 0 span 930 top {m}", "A", FILL * 2 + RUN32 + b"\n", (("top", m), ("exit", "lo", 32), ("from", 0, 932, 2), ("rounds", 15)), top_at=(m, 932))


def _a():
    out = [_grid("w1", range(64), SPANS, [(0, 22, 2, word), (1, 0, 47, word)]),
           _grid("w2", TOPS_FEW, SPANS_WIDE + (52,), [(0, 52, 2, word), (1, 0, 63, lambda n: tail20(n, 20))]),
           _grid("w3", TOPS_FEW, SPANS_WIDE + (82,), [(0, 82, 2, word), (1, 0, 129, lambda n: tail20(n, 40))]),
           _grid("w32", TOPS_FEW, SPANS_WIDE + (82,), [(0, 82, 2, word), (1, 0, 129, word)], _w32_max_len),
           _grid("dense32", TOPS_H, (2, 3, 15, 16, 17, 18), [(0, 1002, 2, word)])]  # (about a thousand live nodes per byte: few and short)
    pk = Pack("A/long32", "long32")  # the 32-word expression of the issue's table: its shortest match has 1002 bytes
    for m, n in ((0, 1002), (17, 1002), (63, 1040)):
        pk.cell(f"span {n} top {m}", "A", FILL * 2 + tail20(n, 500) + b"\n", (("top", m), ("exit", "died", 32), ("from", 0, 2 + n, 2), ("rounds", 16)), top_at=(m, 2 + n))
    out.append(pk.text)
    return out


# ---- B: how the walk ends
def _b():
    out = []
    # B.2 the piece start is reached: finish(HG_PC_START).  Matches at byte 0 of the piece; a mod 64 by filler; a == 0 below.
    pk = Pack("B2/start", "start")
    bodies = [("short", word(5), ((0, 5, 0), (1, 5, 0), (2, 5, 0), (6, 5, 0))), ("span 66", word(66), ((0, 66, 0), (1, 66, 0), (2, 66, 0))),
              ("three words", tail20(90, 40), ((4, 90, 0), (2, 90, 0))), ("32 words", word(70), ((5, 70, 0), (0, 70, 0)))]
    for am in STARTS_A:
        for what, body, froms in bodies:
            tags = tuple(("from",) + f for f in froms) + (("exit", "start", 1), ("exit", "start", {"three words": 3, "32 words": 32}.get(what, 3)))
            pk.cell(f"{what} at a mod 64 = {am}", "B2", body + b"\n", tags, a_mod=am)
    pk.cell("two words, bounded, at the piece start", "B2", word(30) + b"\n", (("from", 6, 30, 0), ("exit", "start", 2)), a_mod=17)
    # alive to the piece start without a further start: `.*z` from a z far into the line; ^ and \b do not match there
    pk.cell("dot-star alive over 100 bytes", "B2", b"-" * 100 + b"z--\n", (("from", 2, 101, 0), ("exit", "start", 1), ("rounds", 2), ("absent", 0), ("absent", 1)), a_mod=48)
    pk.cell("caret expression off the piece start", "B2", b"-" + word(5) + b"\n", (("absent", 0), ("from", 1, 6, 1), ("from", 2, 6, 0)), a_mod=1)
    # B.5 to == 1
    pk.cell("to == 1", "B5", b"z\n", (("from", 2, 1, 0), ("from", 3, 1, 0), ("exit", "start", 1)), a_mod=16)
    pk.cell("to == 1 then more", "B5", b"z-qz\n", (("from", 2, 1, 0), ("from", 3, 1, 0), ("from", 3, 4, 3), ("from", 1, 4, 2), ("from", 2, 4, 0)), a_mod=63)
    out.append(pk.text)
    for which, body in (("first line, top in the first 64 bytes", word(20)), ("first line, top in a later 64-byte line", word(80))):
        pk = Pack("B2/" + which, "start")  # a == 0: the text's first line
        n = len(body)
        pk.cell("a == 0", "B2", body + b"\n", (("from", 0, n, 0), ("from", 1, n, 0), ("from", 2, n, 0), ("exit", "start", 1), ("exit", "start", 3), ("top", (n - 1) % 64)))
        pk.cell("behind it", "B2", b"-" + word(4) + b"\n", (("from", 1, 5, 1),))
        out.append(pk.text)
    # B.3 q == lo: a match of exactly max_len bytes with to > max_len; the byte before lo a word byte, then a non-word byte.
    # B.4 a match of max_len - 1 bytes beside a full one.
    pk = Pack("B3/bound", "bound")
    for k, (nw, ml) in enumerate(((1, 22), (2, 52), (3, 82))):
        for m in (0, 15, 16, 63):
            full = word(ml)
            pk.cell(f"{nw} words, word byte before lo, top {m}", "B3", b"-a" + full + b"\n",
                    (("from", k, 2 + ml, 2), ("absent", k + 3), ("exit", "lo", nw), ("top", m)), top_at=(m, 2 + ml))
            pk.cell(f"{nw} words, non-word byte before lo, top {m}", "B3", b"--" + full + b"\n",
                    (("from", k, 2 + ml, 2), ("from", k + 3, 2 + ml, 2), ("exit", "lo", nw), ("top", m)), top_at=(m, 2 + ml))
        pk.cell(f"{nw} words, max_len - 1 beside max_len", "B4", b"--" + word(ml - 1) + b"-" + word(ml) + b"\n",
                (("from", k, ml + 1, 2), ("from", k, 2 * ml + 2, ml + 2), ("from", k + 3, ml + 1, 2), ("exit", "died", nw), ("exit", "lo", nw)), a_mod=(5 + 20 * k) % 64)
        # a q exactly max_len + 1 bytes before the end: one byte too far left to be a start
        pk.cell(f"{nw} words, a head one byte beyond the bound", "B3", b"-q" + word(ml) + b"\n", (("from", k, 2 + ml, 2), ("absent", k + 3), ("exit", "lo", nw)), a_mod=31)
    out.append(pk.text)
    pk = Pack("B3/bound32", "bound32")
    full = RUN32
    pk.cell("32 words, word byte before lo", "B3", b"-a" + full + b"\n", (("from", 0, 932, 2), ("absent", 1), ("exit", "lo", 32), ("rounds", 15)), top_at=(15, 932))
    pk.cell("32 words, non-word byte before lo", "B3", b"--" + full + b"\n", (("from", 0, 932, 2), ("from", 1, 932, 2), ("exit", "lo", 32)), top_at=(16, 932))
    pk.cell("32 words, a shorter branch beside it", "B4", b"--" + word(81) + b"-" + word(82) + b"\n",
            (("from", 0, 83, 2), ("from", 0, 166, 84), ("from", 1, 83, 2), ("exit", "died", 32)), a_mod=40)
    out.append(pk.text)
    return out


# ---- C: piece starts that are not line starts
def _c():
    out = []
    pk = Pack("C/nuls", "piece")
    for k in (1, 15, 16, 17):
        for am in (0, 63):
            pk.cell(f"{k} leading NULs, line at {am}", "C", b"\0" * k + word(6) + b" abcz\n",
                    (("from", 0, 6, 0), ("from", 2, 6, 0), ("from", 3, 6, 0), ("from", 1, 11, 7), ("exit", "start", 1), ("exit", "start", 3), ("top", (am + k + 5) % 64)), a_mod=am)
        pk.cell(f"{k} leading NULs, every byte a start", "C", b"\0" * k + b"abcz\n", (("from", 1, 4, 0), ("exit", "start", 1)), a_mod=(64 - k) % 64)
    out.append(pk.text)
    for bs in (33, 40):
        cut = bs - 1
        pk = Pack(f"C/cut {bs}", "piece", bs)
        for am in (0, 17, 48):
            # \b at the first byte of a piece whose preceding text byte is a word byte: a start, the piece start is the context
            pk.cell(f"word byte before the cut, line at {am}", "C", b"-" * (cut - 1) + b"a" + word(6) + b"-\n",
                    (("from", 0, 6, 0), ("from", 2, 6, 0), ("from", 3, 6, 0), ("exit", "start", 1), ("exit", "start", 3)), a_mod=am)
            # alive at the piece start while the byte before the piece would extend the match: it must not extend
            pk.cell(f"the match would extend over the cut, line at {am}", "C", b"-" * (cut - 3) + b"abc" + b"bcz-\n",
                    (("from", 1, 3, 0), ("exit", "start", 1)), a_mod=am)
            # a match cut in two: the head's piece reports nothing, the tail's piece has no head
            pk.cell(f"a match across the cut, line at {am}", "C", b"-" * (cut - 3) + word(8, body=b"d") + b"\n", ("empty",), a_mod=am)
        pk.cell("three words across two cuts", "C", b"-" * (cut - 1) + b"a" + word(cut) + word(5) + b"\n", (("from", 0, 5, 0), ("from", 2, 5, 0), ("from", 3, 5, 0)), a_mod=15)
        out.append(pk.text)
    return out


# ---- D: contexts at `to`
def _d_tags(froms, absent):
    """The stated reports and silent ids; \\b and \\B without MULTILINE (ids 9, 10) must do what ids 2, 3 do."""
    same = {2: 9, 3: 10}
    froms = tuple(froms) + tuple((same[f[0]],) + f[1:] for f in froms if f[0] in same)
    absent = tuple(absent) + tuple(same[r] for r in absent if r in same)
    return tuple(("from",) + f for f in froms) + tuple(("absent", r) for r in absent)


def _d():
    out = []
    inner = [("before a word byte", b"-qaza-\n", ((3, 4, 1), (6, 4, 1)), (0, 1, 2, 4, 5)),
             ("before a non-word byte", b"-qaz-a\n", ((2, 4, 1), (5, 4, 1)), (0, 1, 3, 4, 6)),
             # (every line is a piece of its own, so its newline is the piece's final one: `$` without MULTILINE matches before it too)
             ("before a newline inside the text", b"-qaz\n", ((0, 4, 1), (1, 4, 1), (2, 4, 1), (4, 4, 1), (5, 4, 1), (7, 5, 1), (8, 5, 1)), (3, 6)),
             ("span 70 before a newline", b"-" + word(70) + b"\n", ((0, 71, 1), (1, 71, 1), (2, 71, 1), (4, 71, 1), (5, 71, 1), (7, 72, 1), (8, 72, 1)), (3, 6))]
    for ending, last, froms, absent in (("no final newline", b"-" + word(5), ((0, 6, 1), (1, 6, 1), (2, 6, 1), (4, 6, 1), (5, 6, 1)), (3, 6)),
                                        ("final newline", b"-" + word(5) + b"\n", ((0, 6, 1), (1, 6, 1), (2, 6, 1), (4, 6, 1), (5, 6, 1)), (3, 6)),
                                        ("long, no final newline", b"-" + word(75), ((0, 76, 1), (1, 76, 1), (2, 76, 1), (4, 76, 1), (5, 76, 1)), (3, 6)),
                                        ("long, final newline", b"-" + word(75) + b"\n", ((0, 76, 1), (1, 76, 1), (2, 76, 1), (4, 76, 1), (5, 76, 1)), (3, 6)),
                                        ("a word byte ends the text", b"-qaza", ((3, 4, 1), (6, 4, 1)), (0, 1, 2, 4, 5))):
        pk = Pack("D/" + ending, "ctx")
        for i, (what, line, fr, ab) in enumerate(inner):
            pk.cell(what, "D", line, _d_tags(fr, ab), a_mod=(15 + 17 * i) % 64)
        pk.cell("to at the end of the text", "D", last, _d_tags(froms, absent), a_mod=48)
        out.append(pk.text)
    return out


# ---- E: several starts
def _e():
    pk = Pack("E/multi", "multi")
    for m in (0, 16, 63):
        pk.cell(f"every position a start, top {m}", "E", b"--" + b"abc" * 7 + b"z\n", (("from", 0, 24, 2), ("top", m), ("exit", "died", 1)), top_at=(m, 24))
        pk.cell(f"every position a start, 90 bytes, top {m}", "E", b"-" + b"abc" * 30 + b"z\n", (("from", 0, 92, 1), ("top", m), ("rounds", 2)), top_at=(m, 92))
    pk.cell("a|aaa", "E", b"-aaaa-a\n", (("from", 1, 2, 1), ("from", 1, 3, 2), ("from", 1, 4, 1), ("from", 1, 5, 2), ("from", 1, 7, 6)), a_mod=62)
    pk.cell("(ab|b)c", "E", b"-abc-bc-xbc\n", (("from", 2, 4, 1), ("from", 2, 7, 5), ("from", 2, 11, 9)), a_mod=15)
    for m in (0, 17, 47):
        line = b"-q" + b"a" * 70 + b"q" + b"a" * 3 + b"z\n"
        pk.cell(f"a start, 70 live bytes without one, the leftmost start, top {m}", "E", line, (("from", 3, 77, 1), ("from", 4, 77, 1), ("top", m), ("rounds", 2)), top_at=(m, 77))
    pk.cell("the leftmost start lies beyond the bound", "E", b"-q" + b"a" * 90 + b"q" + b"a" * 3 + b"z\n", (("from", 3, 97, 1), ("from", 4, 97, 92)), a_mod=33)
    return [pk.text]


# ---- F: lanes and state homes.  Hits are ordered by line, so lane i of a wave holds hit i.
F_COUNTS = (1, 63, 64, 65, 129)
MIX_HEADS = (b"q", b"r", b"s", b"t", b"u")  # the 1-, 2-, 3- and 32-word expressions and the unflagged one of database `mix`


def _f():
    out = []
    for n in F_COUNTS:
        pk = Pack(f"F/{n} hits", "lane3")
        for i in range(n):
            pk.cell(f"hit {i}", "F", b"-" + word(2 + i % 7) + b"\n", (("from", 0, 3 + i % 7, 1),))
        out.append(pk.text)
    for dbname, span in (("lane3", lambda i: 2 + i), ("lane32", lambda i: 2 + i), ("lane32d", lambda i: 2 + i % 4)):
        pk = Pack(f"F/wave of {dbname}", dbname)
        for i in range(64):
            pk.cell(f"lane {i}", "F", b"-" + word(span(i)) + b"\n", (("from", 0, 1 + span(i), 1),))
        out.append(pk.text)
    pk = Pack("F/wave of every state home", "mix")
    for i in range(130):
        k = i % 5
        n = 2 + (i * 7) % 19
        pk.cell(f"lane {i % 64} of wave {i // 64}", "F", b"-" + word(n, MIX_HEADS[k]) + b"\n", (("from", k, 1 + n, 1 if k < 4 else 0),))
    out.append(pk.text)
    pk = Pack("F/no multi-word expression with the flag", "nolds")
    for i in range(70):
        k = i % 2
        pk.cell(f"hit {i}", "F", b"-" + word(3 + i % 11, (b"q", b"u")[k]) + b"\n", (("from", k, 4 + i % 11, 1 - k),))
    out.append(pk.text)
    return out


# ---- G: shared ids (and I: the same lines with min_length on members)
def _share_cells(pk, group, ml):
    """ml: the database gives x[a-q]{0,80}z min_length 8, r.. 4, w.. 7, y.. 12 and h[a-y-]{0,20}stack 12."""
    c = pk.cell
    c("two-cycle, the other member starts further left", group, b"-xaaaqaaz\n", (("from", 1, 9, 1),), a_mod=60)
    # under min_length 8 the three-word member's match [1, 8) has 7 bytes: its start does not count
    c("two-cycle, the further-left start is one byte too short", group, b"-xaaqaaz\n", (("from", 1, 8, 4 if ml else 1),), a_mod=15)
    c("two-cycle, only the one-word member matches", group, b"-qaaz\n", (("from", 1, 5, 1), ("absent", 2)), a_mod=16)
    c("two-cycle, only the three-word member matches", group, b"-" + word(70, b"x") + b"\n", (("from", 1, 71, 1),), a_mod=47)
    c("two-cycle, three-word member from far left", group, b"-x" + b"a" * 60 + b"qaaz\n", (("from", 1, 66, 1),), a_mod=1)
    # under min_length y's [1, 12) has 11 bytes (below 12) and w's [6, 12) has 6 (below 7): only r's [8, 12) counts
    c("three-cycle, 32 words leftmost", group, b"-yaaaawarabz\n", (("from", 2, 12, 8 if ml else 1),), a_mod=63)
    c("three-cycle, 32 words leftmost and long enough", group, b"-yaaaaawarabz\n", (("from", 2, 13, 1),), a_mod=14)
    # y's match [1, 12) has 11 bytes (below 12), w's [4, 12) has 8 (7 or more)
    c("three-cycle, 32-word start one byte too short", group, b"-yaawaaarabz\n", (("from", 2, 12, 4 if ml else 1),), a_mod=31)
    c("three-cycle, three words leftmost", group, b"-waaraabz\n", (("from", 2, 9, 1),), a_mod=32)
    c("three-cycle, only one word", group, b"-raaaz\n", (("from", 2, 6, 1), ("absent", 1)), a_mod=48)
    c("three-cycle, only 32 words", group, b"-y" + b"v" * 80 + b"z\n", (("from", 2, 83, 1), ("rounds", 2)), a_mod=17)
    if ml:
        c("three-cycle, the reporting member alone is long enough", group, b"-rabz\n", (("from", 2, 5, 1),), a_mod=5)
        c("three-cycle, every member too short", group, b"-raz-waaaaz-yaz\n", ("empty",), a_mod=6)
    c("a literal alone on its id", group, b"--needle needle\n", (("from", 3, 8, 2), ("from", 3, 15, 9)), a_mod=59)
    c("a literal at the piece start: to == max_len", group, b"needle-\n", (("from", 3, 6, 0),), a_mod=16)
    c("a literal with a regular expression: it walks", group, b"-haaa-hay-stack\n", (("from", 4, 15, 1),), a_mod=50)
    # under min_length 12 the regular expression's [1, 12) has 11 bytes: only the literal's start counts
    c("a literal with a regular expression, its further-left start too short", group, b"-hahay-stack\n", (("from", 4, 12, 3 if ml else 1),), a_mod=49)
    c("a literal with a regular expression, the literal alone", group, b"-zhay-stack\n", (("from", 4, 11, 2),), a_mod=0)
    c("a literal with a regular expression, long enough", group, b"-haa-hay-stack\n", (("from", 4, 14, 1),), a_mod=20)


def _g():
    pk = Pack("G/share", "share")
    _share_cells(pk, "G", False)
    pk.cell("two literals on one id", "G", b"-abcde-f cde-f\n", (("from", 5, 8, 1), ("from", 5, 14, 9)), a_mod=58)
    pk.cell("two literals on one id at the piece start", "G", b"abcde-f\n", (("from", 5, 7, 0),), a_mod=63)
    return [pk.text]


# ---- H: min_length without the flag, through hg_minlen_kernel
ML_CLASSES = ((0, b"q", 1, 10), (1, b"r", 2, 10), (2, b"s", 3, 10), (3, b"t", 32, 10))  # (id, head, nw, min_length)
ML_FULL = ((6, b"v", 1, 22), (7, b"w", 2, 52), (8, b"x", 3, 82))  # min_length == max_len


def _h():
    out = []
    wd = lambda n, h=b"q": word(n, h, b"d")  # (bodies of d: `[a-c]+z` matches nothing inside them)
    pk = Pack("H/ml", "ml")
    for rid, h, nw, need in ML_CLASSES:
        for m in TOPS_H:
            pk.cell(f"{nw} words, leftmost start exactly at to - need, top {m}", "H", b"--" + wd(need, h) + b"\n", (("from", rid, 2 + need, 0), ("top", m), ("mexit", "early", nw)), top_at=(m, 2 + need))
            pk.cell(f"{nw} words, leftmost start one byte right of it, top {m}", "H", b"--" + wd(need - 1, h) + b"\n", ("empty", ("top", m), ("mexit", "died", nw)), top_at=(m, 1 + need))
            pk.cell(f"{nw} words, longer than needed, top {m}", "H", b"-" + wd(need + 9, h) + b"\n", (("from", rid, 10 + need, 0), ("top", m)), top_at=(m, 10 + need))
        pk.cell(f"{nw} words, to < need", "H", wd(need - 1, h) + b"\n", ("empty",), a_mod=16)
        pk.cell(f"{nw} words, a kept report at the piece start", "H", wd(need, h) + b"\n", (("from", rid, need, 0), ("mexit", "early", nw)), a_mod=63)
    for m in TOPS_H:
        # [a-c]+z with min_length 4: the first starts met lie above the limit, a later one at it
        pk.cell(f"first start above the limit, a later one at it, top {m}", "H", b"-abcz\n", (("from", 4, 5, 0), ("top", m), ("mexit", "early", 1)), top_at=(m, 5))
        pk.cell(f"every start above the limit, top {m}", "H", b"-bcz\n", ("empty", ("top", m), ("mexit", "start", 1)), top_at=(m, 4))
        pk.cell(f"need 0 beside filtering expressions, top {m}", "H", b"-uz-" + wd(9) + b"-" + wd(10) + b"\n", (("from", 5, 3, 0), ("from", 0, 24, 0)), top_at=(m, 3))
    for rid, h, nw, need in ML_FULL:
        for m in TOPS_H:
            pk.cell(f"{nw} words, need == max_len, kept, top {m}", "H", b"-a" + wd(need, h) + b"\n", (("from", rid, 2 + need, 0), ("top", m), ("mexit", "early", nw), ("at_lo", nw)), top_at=(m, 2 + need))
            pk.cell(f"{nw} words, need == max_len, one byte short, top {m}", "H", b"--" + wd(need - 1, h) + b"\n", ("empty", ("top", m)), top_at=(m, 1 + need))
        # the bound cells of B.3: a head one byte beyond the bound is no start, and the walk ends at q == lo
        pk.cell(f"{nw} words, a head one byte beyond the bound", "H", b"-" + h + wd(need, h) + b"\n", (("from", rid, 2 + need, 0),), a_mod=31)
        pk.cell(f"{nw} words, max_len - 1 behind a head: the walk ends at lo without a start at the limit", "H", b"-" + h + h + wd(need - 1, h)[1:] + b"\n", ("empty",), a_mod=33)
    # 32 words: the longest match is T and 929 letters; the short branch gives raw reports deep in a long line
    run = b"T" + RUN32[1:]
    for m in TOPS_H:
        pk.cell(f"32 words, need == max_len, kept, top {m}", "H", b"-a" + run + b"\n", (("from", 9, 932, 0), ("top", m), ("mexit", "early", 32), ("at_lo", 32)), top_at=(m, 932))
        pk.cell(f"32 words, need == max_len, a short match at to >= need, top {m}", "H", b"-" * 930 + b"kdddz\n", ("empty", ("top", m), ("mexit", "died", 32)), top_at=(m, 935))
        pk.cell(f"32 words, a head one byte beyond the bound, top {m}", "H", b"-T" + run + b"\n", (("from", 9, 932, 0), ("top", m), ("at_lo", 32)), top_at=(m, 932))
    pk.cell("32 words, need == max_len, one byte short: no report to filter", "H", b"--" + run[:-1] + b"\n", ("empty",), a_mod=33)
    out.append(pk.text)
    return out


KEPT_LINE, DROPPED_LINE = b"-" + word(10) + b"\n", b"-" + word(9) + b"\n"
COMPACT_COUNTS = (1, 63, 64, 65, 128, 129)
COMPACT_SETS = {"none": lambda i, n: False, "all": lambda i, n: True, "every other": lambda i, n: i % 2 == 0, "first half": lambda i, n: i < n // 2}


def compact_text(name: str, keep) -> Text:
    """One raw report per line of the one filtering expression of database `compact`; keep[i]: line i's report survives."""
    pk = Pack(name, "compact")
    for i, k in enumerate(keep):
        pk.cell(f"raw report {i}", "H", KEPT_LINE if k else DROPPED_LINE, (("from", 0, 11, 0),) if k else ("empty",))
    return pk.text


def _compaction():
    out = []
    for n in COMPACT_COUNTS:
        for which, rule in COMPACT_SETS.items():
            out.append(compact_text(f"H/compaction {n} raw, {which} kept", [rule(i, n) for i in range(n)]))
    for k in range(65):
        out.append(compact_text(f"H/compaction 65 raw, only {k} kept", [i == k for i in range(65)]))
    return out


# ---- I: start of match and min_length together, over the lines of groups B and G
def _i():
    out = []
    pk = Pack("I/share_ml", "share_ml")
    _share_cells(pk, "I", True)
    out.append(pk.text)
    pk = Pack("I/bound_ml", "bound_ml")  # min_length: 22 (== max_len), 40, 82 (== max_len); \b forms 21, 52, 60
    for k, (nw, ml) in enumerate(((1, 22), (2, 52), (3, 82))):
        full = word(ml)
        pk.cell(f"{nw} words, word byte before lo", "I", b"-a" + full + b"\n", (("from", k, 2 + ml, 2), ("absent", k + 3), ("exit", "lo", nw)), top_at=(16 * k, 2 + ml))
        pk.cell(f"{nw} words, non-word byte before lo", "I", b"--" + full + b"\n", (("from", k, 2 + ml, 2), ("from", k + 3, 2 + ml, 2)), top_at=(63 - k, 2 + ml))
        pk.cell(f"{nw} words, max_len - 1 beside max_len", "I", b"-" + word(ml - 1) + b"-" + word(ml) + b"\n", (("from", k, 2 * ml + 1, ml + 1),), a_mod=(7 + 20 * k) % 64)
    pk.cell("short matches of every member are dropped", "I", b"-" + word(20) + b"\n", ("empty",), a_mod=15)
    out.append(pk.text)
    pk = Pack("I/bound32_ml", "bound32_ml")  # min_length 930 == max_len on both
    run = RUN32
    pk.cell("32 words, word byte before lo", "I", b"-a" + run + b"\n", (("from", 0, 932, 2), ("absent", 1), ("exit", "lo", 32), ("at_lo", 32)), top_at=(16, 932))
    pk.cell("32 words, non-word byte before lo", "I", b"--" + run + b"\n", (("from", 0, 932, 2), ("from", 1, 932, 2), ("at_lo", 32)), top_at=(63, 932))
    pk.cell("32 words, a head one byte beyond the bound", "I", b"-S" + run + b"\n", (("from", 0, 932, 2), ("absent", 1)), a_mod=31)
    pk.cell("32 words, the short branch is dropped", "I", b"-" * 930 + word(20) + b"\n", ("empty",), a_mod=15)
    out.append(pk.text)
    pk = Pack("I/start_ml", "start_ml")
    for am in STARTS_A:
        pk.cell(f"kept at the piece start, a mod 64 = {am}", "I", word(5) + b"\n", (("from", 0, 5, 0), ("from", 1, 5, 0), ("from", 2, 5, 0), ("from", 3, 5, 0)), a_mod=am)
        pk.cell(f"one byte short at the piece start, a mod 64 = {am}", "I", word(4) + b"\n", (("from", 2, 4, 0), ("absent", 0), ("absent", 1), ("absent", 3)), a_mod=am)
    pk.cell("to < need for every member", "I", b"qz\n", ("empty",), a_mod=16)
    out.append(pk.text)
    return out


GROUPS = {"A": _a(), "B": _b(), "C": _c(), "D": _d(), "E": _e(), "F": _f(), "G": _g(), "H": _h(), "Hc": _compaction(), "I": _i()}
TEXTS = [t for g in GROUPS.values() for t in g]
CELLS = [c for t in TEXTS for c in t.cells]
assert len({t.name for t in TEXTS}) == len(TEXTS)  # names are unique
assert len({c.name for c in CELLS}) == len(CELLS), [c.name for i, c in enumerate(CELLS) if c.name in {x.name for x in CELLS[:i]}][:5]
assert all(len(t.data) <= 400 << 10 for t in TEXTS)
FACE_A_STRIDE = 7  # hs_scan block mode runs every cell of group G and every seventh cell of group A

# ---- the reference: Python `re` only
_piece_cache: dict = {}
_reference: dict = {}


def piece_reports(d: Db, piece: bytes):
    key = (d.name, piece)
    if key not in _piece_cache:
        _piece_cache[key] = minlensim_py.expected_piece(d.pats, d.flags, d.ids, d.need, piece)
    return _piece_cache[key]


def raw_count(d: Db, piece: bytes) -> int:
    """Reports of the piece before min_length and before the report rules (one per expression and end)."""
    key = (d.name, piece, "raw")
    if key not in _piece_cache:
        _piece_cache[key] = sum(len(minlensim_py.spans(p, f, piece)) for p, f in zip(d.pats, d.flags))
    return _piece_cache[key]


def layout(text: Text):
    """[(piece index, offset of its first scanned byte, its bytes, cell)] for every non-empty piece of the text."""
    data = text.data
    bounds = [(c.offset, c.offset + len(c.data), c) for c in text.cells]
    out, k = [], 0
    for idx, a, piece in somsim_py.pieces(data, text.bs):
        if not piece:
            continue
        while not bounds[k][0] <= a < bounds[k][1]:
            k += 1
        out.append((idx, a, piece, bounds[k][2]))
    return out


def reference(text: Text):
    """({cell name: [(line, id, to, from)]}, the whole text's list in (line, id, to) order, raw report count); computed once."""
    if text.name not in _reference:
        d = DBS[text.db]
        per_cell = {c.name: [] for c in text.cells}
        whole, raw = [], 0
        for idx, _a, piece, c in layout(text):
            rows = [(idx, rid, to, frm) for rid, to, frm in piece_reports(d, piece)]
            per_cell[c.name] += rows
            whole += rows
            if d.filtering:
                raw += raw_count(d, piece)
        _reference[text.name] = (per_cell, whole, raw)
    return _reference[text.name]
