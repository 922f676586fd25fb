"""Cells for the stream-mode kernels (hg_flow_scan_kernel, hg_flow_som_kernel; hypergrep_amd/csrc/hg_flows.hip): write, piece,
slice, group and item geometry planted by hand, with a reference that knows only the definition.

A cell is an expression set and a list of runs.  A run is one stream: its bytes, its write boundaries, and how it ends
("close": a close after the last write, a zero-length item in a batch; "last": the last write carries the end of data).  The
reference (reference()) gives, for a run, every report with the window of calls in which it may arrive:

  * what an expression matches comes from Python's `re` over the concatenation (spans(): a lookahead at every start; the
    expressions here have one end per start) or, for `st.*us` (several ends per start), from the construction;
  * the stream rules of include/hypergrep_amd.h: an expression without assertions reports (id, to) in the call whose write
    holds byte to - 1; one with ^ $ \\Z \\b \\B (and a start-of-match expression that shares its id) no earlier than that and
    no later than the call that holds byte `to` (the byte behind it when byte `to` is a '\\n': a write's trailing newline may
    be held until the next byte shows whether it is the final one, rule 4), or the end of data; SINGLEMATCH once per id with the smallest `to`; an
    identical (id, to) once; `from` the smallest start; within a call (to, id) order.

Nothing in an expectation comes from the product.  The product's constants are restated below for the COVERAGE claims only:
each run records, as (text, bool) pairs computed from them, that it sits where it says (this needle straddles slice
boundary k with b bytes in front of it; this write has three pieces; this launch is above the HBM cut-off).  A claim that has
drifted is False and fails tests/test_flow_cells.py without a GPU.  Which groups are staged in LDS is claimed per cell
(Cell.staged) and checked there against the read-out of the kernel's formula (flowsim_group_span).
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field

import regex_gen

# ---- the product's constants, restated for the coverage claims (never used in an expectation)
PIECE = 4096          # HG_FLOW_PIECE
LANES = 256           # lanes of a workgroup of hg_flow_scan_kernel
MIN_SLICE = 8
PPW = 32              # HG_FLOW_PPW: expressions per workgroup
POOL = 10240          # HG_BLOCK_SMALL_POOL: words of tables a workgroup stages
HBM_MIN = 1 << 20     # HG_FLOW_HBM_MIN_DEFAULT: bytes x groups from which a launch's text is copied to HBM
FIRST_CAP = 4096      # reports the report array holds at a scratch's first launch

SINGLE, SOM, MULTILINE = 8, 256, 4
FILL = 0x2D  # '-': no expression of any cell matches inside a run of it


def most(npat: int) -> int:
    return LANES // npat


def slice_len(plen: int, npat: int) -> int:
    return max(MIN_SLICE, -(-plen // most(npat)))


def npieces(wlen: int) -> int:
    return -(-wlen // PIECE)


def locate(wpos: int, wlen: int, npat: int):
    """(piece, slice, offset in the slice, slice length, slices of the piece) of byte wpos of a write of wlen bytes."""
    q = wpos // PIECE
    plen = min(PIECE, wlen - q * PIECE)
    sl = slice_len(plen, npat)
    p = wpos - q * PIECE
    return q, p // sl, p % sl, sl, -(-plen // sl)


def rounded(n: int) -> int:
    return (n + 15) & ~15


def launch_in_hbm(lengths, ngroups: int, som: bool = False) -> bool:
    total = sum(rounded(n) for n in lengths)
    return total > 0 and (total * ngroups >= HBM_MIN or som)


# ---- cells
@dataclass
class Run:
    label: str
    data: bytes
    cuts: list          # ascending stream offsets between writes (equal cuts: empty writes); writes = len(cuts) + 1
    end: str = "close"  # "close" or "last"
    claims: list = field(default_factory=list)  # (text, bool)
    refs: dict = field(default_factory=dict, repr=False, compare=False)  # cell name -> its reference (computed once, left unchanged)

    def writes(self):
        edges = [0] + list(self.cuts) + [len(self.data)]
        return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]

    def ncalls(self) -> int:
        return len(self.cuts) + 1 + (self.end == "close")

    def claim(self, text: str, ok) -> None:
        self.claims.append((text, bool(ok)))


@dataclass
class Cell:
    name: str
    patterns: list
    flags: list
    ids: list
    runs: list
    horizon: str | None = None
    staged: dict = field(default_factory=dict)   # group -> the kernel stages its tables in LDS
    words: dict = field(default_factory=dict)    # expression -> (min, max) state words claimed
    claims: list = field(default_factory=list)   # (text, bool) about the cell as a whole (launch geometry)
    single_entry: int = 3                        # runs that also go through hs_scan_stream / close / reset

    def npat(self, group: int) -> int:
        return min(PPW, len(self.patterns) - group * PPW)

    def ngroups(self) -> int:
        return -(-len(self.patterns) // PPW)


# ---- the reference
def _strip_classes(pat: str) -> str:
    return re.sub(r"\[[^\]]*\]", "", pat)


def has_assertion(pat: str) -> bool:
    return bool(re.search(r"\\[bBAZz]|\^|\$", _strip_classes(pat)))


def is_literal(pat: str) -> bool:
    return re.fullmatch(r"[A-Za-z0-9_=\- ]+", pat) is not None


def _st_us(data: bytes) -> dict:
    """st.*us without DOTALL, from the construction: in each line, every `us` behind the line's first `st`."""
    out, base = {}, 0
    for line in data.split(b"\n"):
        first = line.find(b"st")
        j = line.find(b"us", first + 2) if first >= 0 else -1
        while j >= 0:
            out[base + j + 2] = base + first
            j = line.find(b"us", j + 1)
        base += len(line) + 1
    return out


MULTI_END = {"st.*us": _st_us}  # several ends per start: `re` finds one of them, the construction all
_RE_CACHE: dict = {}


def spans(pat: str, flags: int, data: bytes) -> dict:
    """{to: smallest from} of every match of pat in data."""
    if pat in MULTI_END:
        return MULTI_END[pat](data)
    out: dict = {}
    if is_literal(pat) and not flags & 1:
        lit = pat.encode()
        j = data.find(lit)
        while j >= 0:
            out[j + len(lit)] = j
            j = data.find(lit, j + 1)
        return out
    cre = _RE_CACHE.get((pat, flags))
    if cre is None:  # PCRE's \Z (the end, or in front of a final newline) is `$` without MULTILINE in Python
        cre = _RE_CACHE[(pat, flags)] = re.compile(b"(?=(" + pat.replace("\\Z", "(?=\\n?\\Z)").encode() + b"))", regex_gen.py_flags(flags))
    for m in cre.finditer(data):
        s, e = m.span(1)
        if e > s and s < out.get(e, e):
            out[e] = s
    return out


@dataclass(frozen=True)
class Want:
    lo: int     # first call that may deliver it
    hi: int     # last
    key: tuple  # (id, to), with a horizon (id, from, to)


def reference(cell: Cell, run: Run):
    """[Want] of a run, in (to, id) order (computed once per cell and run; callers leave it unchanged)."""
    if cell.name not in run.refs:
        run.refs[cell.name] = _reference(cell, run)
    return run.refs[cell.name]


def _reference(cell: Cell, run: Run):
    data, n = run.data, len(run.data)
    writes = run.writes()
    end_call = run.ncalls() - 1

    def call_of(byte: int) -> int:
        return next(c for c, (a, b) in enumerate(writes) if a <= byte < b)

    shared = {i for i in cell.ids if cell.ids.count(i) > 1}
    best: dict = {}  # (id, to) -> [lo, hi, from]
    for pat, fl, rid in zip(cell.patterns, cell.flags, cell.ids):
        late = has_assertion(pat) or (fl & SOM and rid in shared)
        for to, frm in spans(pat, fl, data).items():
            lo = call_of(to - 1)
            # (rule 3: at the latest the call that holds byte `to`; when that byte is a '\n', which an expression that tells a
            # final newline from another holds back, rule 4, the call that holds the byte behind it; else the end of data)
            nxt = to + 1 if to < n and data[to] == 10 else to
            hi = lo if not late else (call_of(nxt) if nxt < n else end_call)
            frm = frm if fl & SOM else 0
            cur = best.get((rid, to))
            best[(rid, to)] = [lo, hi, frm] if cur is None else [min(cur[0], lo), max(cur[1], hi), min(cur[2], frm)]
    single = {rid for fl, rid in zip(cell.flags, cell.ids) if fl & SINGLE}
    for rid in single:
        tos = sorted(t for (i, t) in best if i == rid)
        for t in tos[1:]:
            del best[(rid, t)]
    out = []
    for (rid, to), (lo, hi, frm) in sorted(best.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        out.append(Want(lo, hi, (rid, frm, to) if cell.horizon else (rid, to)))
    return out


def windowed_cap(cell: Cell, run: Run) -> int:
    """Reports of the run that belong to an expression with an assertion (or to a shared start-of-match id): only these may
    be compared by window."""
    shared = {i for i in cell.ids if cell.ids.count(i) > 1}
    ids = {rid for pat, fl, rid in zip(cell.patterns, cell.flags, cell.ids) if has_assertion(pat) or (fl & SOM and rid in shared)}
    return sum(w.key[0] in ids for w in reference(cell, run))


def compare(cell: Cell, run: Run, calls):
    """(errors, reports compared by window) of the calls' reports [[report] per call] against the reference."""
    want = reference(cell, run)
    errors = []
    if len(calls) != run.ncalls():
        return [f"{len(calls)} calls, {run.ncalls()} expected"], 0
    got = [(c, tuple(r)) for c, lst in enumerate(calls) for r in lst]
    if sorted(r for _, r in got) != sorted(w.key for w in want):
        miss = sorted(set(w.key for w in want) - set(r for _, r in got))
        extra = sorted(set(r for _, r in got) - set(w.key for w in want))
        count: dict = {}
        for _, r in got:
            count[r] = count.get(r, 0) + 1
        twice = sorted(r for r, k in count.items() if k > 1)
        errors.append(f"missing {miss[:6]} unexpected {extra[:6]} twice {twice[:6]} ({len(got)} reports, {len(want)} expected)")
    where = {r: c for c, r in got}
    for w in want:
        c = where.get(w.key)
        if c is not None and not w.lo <= c <= w.hi:
            errors.append(f"{w.key} in call {c}, expected in [{w.lo}, {w.hi}]")
    for c, lst in enumerate(calls):
        if list(lst) != sorted(lst, key=lambda r: (r[-1], r[0])):
            errors.append(f"call {c} is not in (to, id) order")
    return errors[:8], sum(w.lo < w.hi for w in want)


# ---- builders
def fill(n: int) -> bytearray:
    return bytearray([FILL]) * n


def plant(buf: bytearray, pos: int, what: bytes) -> None:
    assert 0 <= pos and pos + len(what) <= len(buf), (pos, len(what), len(buf))
    buf[pos:pos + len(what)] = what


def fillers(n: int, start: int = 0):
    return [f"zq{start + i:02d}x" for i in range(n)]


BIG = "zk[a-z]{900}q"  # about 29 state words: a group that holds it is over the pool, its tables stay in HBM; it occurs nowhere


def _set_with(npat: int, placed: dict, big: int | None = None):
    """npat expressions: `placed` {index: (pattern, flags)}, the rest literals that occur nowhere (at index `big`: BIG)."""
    pats, flags = [], []
    for i in range(npat):
        p, f = placed.get(i, (BIG if i == big else f"zq{i:02d}x", 0))
        pats.append(p)
        flags.append(f)
    return pats, flags, [100 + i for i in range(npat)]


CELLS: list = []


def _slice_sets(npat: int):
    prim = [("wxyz", 0), ("ab+c", 0), ("a+b", 0), ("st.*us", 0)]
    if npat == 1:
        return [{0: p} for p in prim]
    if npat in (2, 3):
        return [{0: prim[0], npat - 1: prim[1]}, {0: prim[2], npat - 1: prim[3]}]
    return [{0: prim[0], 1: prim[1], npat - 2: prim[2], npat - 1: prim[3]}]  # the first and the last indices of the group


def _slice_runs(npat: int, have):
    runs = []
    m = most(npat)
    for wlen in (8 * m - 8, 8 * m + 8, PIECE):
        sl, ns = slice_len(wlen, npat), -(-wlen // slice_len(wlen, npat))
        ks = sorted({1, ns // 2, ns - 1} - {0})
        mid = ns // 2 or 1

        def one(label, pos, what, k, b, extra=None):
            if pos < 0 or pos + len(what) > wlen:
                return
            buf = fill(wlen)
            plant(buf, pos, what)
            r = Run(f"{label}/w{wlen}/k{k}/b{b}", bytes(buf), [])
            q, kk, off, sl2, ns2 = locate(pos + b, wlen, npat)
            r.claim(f"byte {b} of the plant is the first byte of slice {k}", (q, kk, off, sl2) == (0, k, 0, sl) and 0 < k < ns2)
            r.claim("one piece", npieces(wlen) == 1)
            if extra:
                extra(r)
            runs.append(r)

        r0 = Run(f"geometry/w{wlen}", bytes(fill(wlen)), [])
        r0.claim("slice length on its side of 8 x most", (sl == 8) == (wlen <= 8 * m) and (wlen != 8 * m + 8 or sl == 9) and (wlen != PIECE or sl == -(-PIECE // m)))
        runs.append(r0)
        if "wxyz" in have:
            for k in ks:
                for b in range(5):  # b = 0: starts on a slice's first byte; 1: on the last byte of the slice in front; 4: ends with it
                    one("needle", k * sl - b, b"wxyz", k, b)
        if "ab+c" in have:
            for run_len in (1, sl, 2 * sl):
                what = b"a" + b"b" * run_len + b"c"
                for k in ks:
                    for b in (range(len(what) + 1) if k == mid else (0, 1, len(what) - 1, len(what))):
                        one(f"run{run_len}", k * sl - b, what, k, b)
        if "a+b" in have:
            for k in ks:
                for n_a, b in ((6, 3), (2 * sl + sl // 2, sl + 2), (sl, 0), (sl, sl)):
                    one(f"a{n_a}b", k * sl - b, b"a" * n_a + b"b", k, b)
        if "st.*us" in have:
            buf = fill(wlen)
            plant(buf, 1, b"st")
            plant(buf, wlen - 2, b"us")
            if wlen >= 64:
                plant(buf, wlen // 2, b"us")
            r = Run(f"never-dying/w{wlen}", bytes(buf), [])
            r.claim("starts in slice 0, ends on the last byte of the last slice", locate(1, wlen, npat)[1] == 0 and locate(wlen - 1, wlen, npat)[1] == ns - 1 and ns > 1)
            runs.append(r)
    return runs


def _build_slices():
    for npat in (1, 2, 3, 7, 8, 31, 32):
        for si, placed in enumerate(_slice_sets(npat)):
            pats, flags, ids = _set_with(npat, placed)
            runs = _slice_runs(npat, {p for p, _ in placed.values()})
            for big in (None, 3) if npat in (8, 32) else (None,):  # the same runs under a staged and an unstaged set
                pats, flags, ids = _set_with(npat, placed, big)
                cell = Cell(f"slices-n{npat}-s{si}" + ("-unstaged" if big else ""), pats, flags, ids, runs, staged={0: big is None})
                cell.claims.append(("idle lanes exactly at 3, 7 and 31", (LANES % npat != 0) == (npat in (3, 7, 31))))
                CELLS.append(cell)


def _build_contexts():
    pats = [r"\bfoo\b", "^x", "foo$", r"\Bab"]
    flags = [0, MULTILINE, 0, 0]
    runs = []
    sl = slice_len(PIECE, 4)
    for where in ("slice", "piece", "write"):
        for d in (b"a", b"-", b"\n"):
            for tok in (b"foo", b"x", b"ab"):
                if where == "slice":
                    wlen, pos, cuts = PIECE, 5 * sl, []
                elif where == "piece":
                    wlen, pos, cuts = 2 * PIECE, PIECE, []
                else:
                    wlen, pos, cuts = 200, 100, [100]
                buf = fill(wlen)
                plant(buf, pos - 1, d + tok)
                r = Run(f"left/{where}/{d!r}/{tok.decode()}", bytes(buf), cuts)
                wpos = pos - (cuts[0] if cuts else 0)
                q, k, off, _, _ = locate(wpos, wlen - (cuts[0] if cuts else 0), 4)
                r.claim("the deciding byte is the last of the slice, piece or write in front",
                        {"slice": q == 0 and k == 5 and off == 0, "piece": q == 1 and k == 0 and off == 0, "write": wpos == 0}[where])
                runs.append(r)
    for where in ("slice", "piece", "write"):  # foo$ / \bfoo\b: decided by the bytes BEHIND foo, the first of the next slice, piece or write
        for tail in (b"", b"\n", b"\n-", b"-", b"\n\n", b"a"):
            end = {"slice": 256, "piece": PIECE, "write": 100}[where]
            buf = fill(end) + bytearray(tail)
            plant(buf, end - 3, b"foo")
            cuts = [end] if where == "write" else []
            r = Run(f"right/{where}/{tail!r}", bytes(buf), cuts)
            if tail and where != "write":
                q, k, off, _, _ = locate(end, len(buf), 4)
                r.claim("foo ends on the last byte of a slice or piece", off == 0 and (k > 0 if where == "slice" else (q, k) == (1, 0)))
            runs.append(r)
    CELLS.append(Cell("contexts", pats, flags, [1, 2, 3, 4], runs, staged={0: True}, single_entry=8))


PIECE_SET = (["wxyz", "s[a-z]{40}t-*us", "k[a-z]{900}-*z", "ab+c"], [0, 0, 0, 0], [1, 2, 3, 4])
LETTERS = bytes(97 + i % 23 for i in range(900))  # a..w: no 'z', no "us"


def _build_pieces():
    pats, flags, ids = PIECE_SET
    runs = []
    for wlen in (4095, 4096, 4097, 8192, 8193, 12289):
        buf = fill(wlen)
        plant(buf, 0, b"wxyz")
        plant(buf, wlen - 4, b"wxyz")
        plant(buf, wlen // 2, b"abbc")
        r = Run(f"length/w{wlen}", bytes(buf), [])
        r.claim("pieces", npieces(wlen) == {4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, 12289: 4}[wlen])
        runs.append(r)
    wlen = 12289
    for edge in (PIECE, 2 * PIECE, 3 * PIECE):
        for b in range(5):
            if edge - b + 4 > wlen:
                continue
            buf = fill(wlen)
            plant(buf, edge - b, b"wxyz")
            r = Run(f"needle/edge{edge}/b{b}", bytes(buf), [])
            r.claim("byte b of the needle is a piece's first byte", locate(edge - b + b, wlen, 4)[1:3] == (0, 0) and edge % PIECE == 0)
            runs.append(r)
    for name, head, at, tail, end in (("2-words", b"s" + LETTERS[:40] + b"t", 4000, b"us", 8200), ("29-words", b"k" + LETTERS, 3500, b"z", 8300)):
        buf = fill(wlen)  # a multi-word expression alive across the piece edges at 4096 and 8192
        plant(buf, at, head)
        plant(buf, end, tail)
        r = Run(f"alive-across-two-edges/{name}", bytes(buf), [])
        r.claim("starts in piece 0, ends in piece 2", at // PIECE == 0 and end // PIECE == 2)
        runs.append(r)
    buf = fill(wlen)  # one expression ending at the same piece-relative offset in pieces 0, 1 and 2
    for q in range(3):
        plant(buf, q * PIECE + 100, b"wxyz")
        plant(buf, q * PIECE + 200, b"abc")
    r = Run("same-offset-in-three-pieces", bytes(buf), [])
    r.claim("piece-relative ends equal", len({(q * PIECE + 104) % PIECE for q in range(3)}) == 1)
    runs.append(r)
    for first in (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 2 * PIECE + 1, 3 * PIECE):  # the state a write of 1, 2, 3 (and 4) pieces hands on
        for name, plants in (("needle", ((first - 2, b"wxyz"),)), ("run", ((first - 300, b"a" + b"b" * 310 + b"c"),)), ("2-words", ((first - 30, b"s" + LETTERS[:40] + b"t"), (first + 100, b"us"))),
                             ("29-words", ((first - 500, b"k" + LETTERS), (first + 1000, b"z")))):
            buf = fill(first + 3000)
            for pos, what in plants:
                plant(buf, pos, what)
            r = Run(f"carried/w{first}/{name}", bytes(buf), [first])
            r.claim("pieces of the first write", npieces(first) == {PIECE - 1: 1, PIECE: 1, PIECE + 1: 2, 2 * PIECE: 2, 2 * PIECE + 1: 3, 3 * PIECE: 3}[first])
            runs.append(r)
    CELLS.append(Cell("pieces", pats, flags, ids, runs, staged={0: False}, words={1: (2, 2), 2: (28, 32)}, single_entry=6))
    # the same needle runs under a staged set (one-word expressions only)
    CELLS.append(Cell("pieces-staged", ["wxyz", "ab+c", "a+b"], [0, 0, 0], [1, 4, 5], [r for r in runs if r.label.startswith(("length", "needle", "same"))], staged={0: True}))


def _build_shared_ends():
    runs = []
    for wlen, cuts in ((40, []), (40, [18]), (40, [19]), (40, [20]), (PIECE + 40, []), (PIECE + 40, [PIECE + 18])):
        buf = fill(wlen)
        plant(buf, wlen - 23, b"foo")
        plant(buf, 7, b"foo")
        plant(buf, wlen - 3, b"foo")
        runs.append(Run(f"foo/w{wlen}/{cuts}", bytes(buf), cuts))
    same = [("every foo is an end of three expressions at once", all(r.data.count(b"foo") == 3 and r.data.count(b"o") == 6 for r in runs))]
    CELLS.append(Cell("shared-ends-3", ["foo", "oo", "o"], [0, 0, 0], [1, 2, 3], runs, staged={0: True}, claims=same))
    pats, flags, ids = _set_with(33, {0: ("foo", 0), 1: ("oo", 0), 31: ("o", 0), 32: ("o", 0)})
    CELLS.append(Cell("shared-ends-two-groups", pats, flags, ids, runs, staged={0: True, 1: True},
                      claims=same + [("the two `o` are the last expression of group 0 and the only one of group 1", (31 // PPW, 32 // PPW, len(pats)) == (0, 1, 33))]))


def _build_held():
    pats, flags, ids = ["foo$", r"foo\Z", "o\n", "foo"], [0, 0, 0, 0], [1, 2, 3, 4]
    runs = []

    def body(n, nl):
        buf = fill(n)
        if nl:
            buf[n - 1] = 10
        if n >= 4:
            plant(buf, n - 3 - nl, b"foo")
        return bytes(buf)

    for n in (1, PIECE, PIECE + 1):
        head = b"--foo" if n == 1 else b""
        first = head + body(n, True)
        f = len(first)
        pre = [len(head)] if head else []
        tails = [("byte", b"x", [f], "close"), ("newline", b"\n", [f], "close"), ("empty-item", b"", [f, f], "close"), ("close", b"", [], "close")]
        for m in (1, PIECE, PIECE + 1):
            for nl in (True, False):
                tails.append((f"last{m}{'nl' if nl else ''}", body(m, nl), [f], "last"))
        for label, tail, cuts, end in tails:
            r = Run(f"held/w{n}/{label}", first + tail, pre + cuts, end)
            a, b = r.writes()[len(pre)]
            r.claim("a write of n bytes ends in a newline; at 1 it is that byte alone, at 4097 its last piece is",
                    r.data[b - 1] == 10 and b - a == n and (n != PIECE + 1 or (npieces(n) == 2 and n - PIECE == 1)))
            runs.append(r)
    CELLS.append(Cell("held-newline", pats, flags, ids, runs, staged={0: True}, single_entry=12))


def _build_single():
    pats, flags, ids = ["wxyz", "pqrs", "o", "wxyz"], [SINGLE, SINGLE, SINGLE, 0], [1, 2, 3, 4]
    runs = []
    wlen = 12289
    buf = fill(wlen)
    plant(buf, 50, b"wxyz")
    plant(buf, 2 * PIECE + 50, b"pqrs")
    plant(buf, 2 * PIECE + 500, b"wxyz")
    r = Run("A-in-piece-0/B-in-piece-2", bytes(buf), [])
    r.claim("pieces", 50 // PIECE == 0 and (2 * PIECE + 50) // PIECE == 2)
    runs.append(r)
    buf = fill(300)
    plant(buf, 50, b"wxyz")
    plant(buf, 250, b"pqrs")
    runs.append(Run("A-in-write-0/B-in-write-2", bytes(buf), [100, 200]))
    for label, cuts in (("B-in-piece-0/A-in-piece-2", []), ("B-in-write-0/A-in-write-1", [PIECE])):  # the later expression of the group reports first
        buf = fill(wlen)
        plant(buf, 50, b"pqrs")
        plant(buf, 2 * PIECE + 50, b"wxyz")
        runs.append(Run(label, bytes(buf), cuts))
    sl = slice_len(PIECE, 4)
    buf = fill(wlen)
    for pos in (5 * sl + 3, 2 * sl + 3, 2 * PIECE + 7):
        plant(buf, pos, b"o")
    r = Run("slices-5-and-2/pieces-0-and-2", bytes(buf), [])
    r.claim("slices", locate(5 * sl + 3, wlen, 4)[:2] == (0, 5) and locate(2 * sl + 3, wlen, 4)[:2] == (0, 2) and locate(2 * PIECE + 7, wlen, 4)[0] == 2)
    runs.append(r)
    buf = fill(PIECE)
    plant(buf, 5 * sl + 3, b"o")
    runs.append(Run("slice-5-only", bytes(buf), []))
    CELLS.append(Cell("singlematch", pats, flags, ids, runs, staged={0: True}, single_entry=6))
    pats, flags, ids = _set_with(33, {0: ("wxyz", SINGLE), 32: ("pqrs", SINGLE)})
    ids[0] = ids[32] = 7
    runs = []
    for a, b in ((50, 20), (20, 50), (50, 150), (150, 50)):
        buf = fill(200)
        plant(buf, a, b"wxyz")
        plant(buf, b, b"pqrs")
        runs.append(Run(f"shared-id/{a}/{b}", bytes(buf), [100]))
    CELLS.append(Cell("singlematch-shared-id-two-groups", pats, flags, ids, runs, staged={0: True, 1: True},
                      claims=[("the id's two expressions are in different groups", 0 // PPW != 32 // PPW and ids[0] == ids[32])]))


LENS = (0, 1, 15, 16, 17, 4097)


def _group_set(n: int, big: int | None = None):
    """n expressions; the ones that can match sit on the first and the last index of every group."""
    hot = sorted({g * PPW for g in range(-(-n // PPW))} | {min(g * PPW + PPW, n) - 1 for g in range(-(-n // PPW))})
    pats = [f"m{i:02d}q" if i in hot else (BIG if i == big else f"zq{i:02d}x") for i in range(n)]
    return pats, [0] * n, [100 + i for i in range(n)], hot


def _item_run(i: int, needles) -> Run:
    """Stream i of a batch: three writes whose lengths differ from item to item; its needle begins two bytes in front of the
    first write's end where that fits."""
    lens = [LENS[(i + r * 5) % 6] for r in range(2)] + [17 + i % 3]
    total = sum(lens)
    buf = fill(total)
    needle = needles[i % len(needles)].encode()
    plant(buf, max(0, min(lens[0] - 2, total - len(needle))), needle)
    second = needles[(i // len(needles)) % len(needles)].encode()
    plant(buf, total - len(second), second)
    return Run(f"item{i}/{lens}", bytes(buf), [lens[0], lens[0] + lens[1]], "last" if i % 2 else "close")


def _build_groups():
    for n in (1, 32, 33, 64, 65):
        pats, flags, ids, hot = _group_set(n)
        runs = [_item_run(i, [pats[h] for h in hot]) for i in range(12)]
        cell = Cell(f"groups-{n}", pats, flags, ids, runs)
        cell.staged = {g: True for g in range(cell.ngroups())}
        cell.claims.append(("the last group of 33 and 65 has one expression", n not in (33, 65) or cell.npat(cell.ngroups() - 1) == 1))
        CELLS.append(cell)
    pats, flags, ids, hot = _group_set(65, big=40)  # groups 0 and 2 staged, group 1 not, in one launch
    runs = [_item_run(i, [pats[h] for h in hot]) for i in range(12)]
    CELLS.append(Cell("groups-65-middle-unstaged", pats, flags, ids, runs, staged={0: True, 1: False, 2: True}, claims=[("BIG is in group 1", 40 // PPW == 1)]))
    pats, flags, ids, hot = _group_set(33)
    for items in (1, 2, 63, 64, 65, 300):
        runs = [_item_run(i, [pats[h] for h in hot]) for i in range(items)]
        cell = Cell(f"items-{items}", pats, flags, ids, runs, staged={0: True, 1: True}, single_entry=2)
        lens0 = {len(r.data[:r.cuts[0]]) for r in runs}
        cell.claims.append(("write lengths 0, 1, 15, 16, 17 and 4097 in one launch", items < 6 or lens0 == set(LENS)))
        CELLS.append(cell)


def _build_hbm():
    pats, flags, ids, hot = _group_set(33)
    for items in (127, 128):
        runs = []
        for c in range(items):
            buf = fill(PIECE)
            plant(buf, c * 32 + 1, pats[hot[c % len(hot)]].encode())
            plant(buf, PIECE - 2, pats[hot[(c + 1) % len(hot)]].encode()[:2])
            runs.append(Run(f"sweep{c}", bytes(buf) + pats[hot[(c + 1) % len(hot)]].encode()[2:] + b"-", [PIECE]))
        cell = Cell(f"hbm-{'above' if items == 128 else 'below'}", pats, flags, ids, runs, staged={0: True, 1: True}, single_entry=1)
        cell.claims.append(("the first round's launch is on its side of the cut-off", launch_in_hbm([PIECE] * items, 2) == (items == 128)))
        cell.claims.append(("... and one item fewer or more would change sides", launch_in_hbm([PIECE] * 127, 2) is False and launch_in_hbm([PIECE] * 128, 2) is True))
        CELLS.append(cell)


def _build_overflow():
    for som in (False, True):
        pats = ["o", "[o]", "o{1}", "wxyz"]
        flags = [0, 0, 0, SOM if som else 0]
        w1, w2 = 2000, 5000
        data = b"o" * (w1 - 2) + b"wx" + b"yz" + b"o" * (w2 - 2)
        r = Run("two-overflows", data, [w1])
        n1 = 3 * (w1 - 2)
        n2 = 3 * (w2 - 2) + 1
        r.claim("the first write has more reports than a fresh report array holds", n1 > FIRST_CAP)
        r.claim("the second more than twice those", n2 > 2 * n1)
        r.claim("a match begun in the first write completes in the second", data[w1 - 2:w1 + 2] == b"wxyz")
        CELLS.append(Cell("overflow-som" if som else "overflow", pats, flags, [1, 2, 3, 4], [r], horizon="large" if som else None, staged={0: True}, single_entry=1))


SOM_SET = (["ab+c", "wxyz", "k[a-z]{20}z", "foo$", "st.*us", "pqrs", "fo+x", "o+x"], [SOM, 0, SOM, SOM, SOM, 0, SOM, SOM], [1, 2, 3, 4, 5, 6, 7, 7])


def _som_pool():
    runs = []
    # three start-of-match expressions alive at once with different starts (st.*us from 8, k[a-z]{20}z from 11, ab+c from 12):
    # the first runs of the pool, so that the smallest batches, whose lanes share one wavefront, hold them
    alive = b"st-k" + LETTERS[:20] + b"z-us"
    for c in range(0, len(alive) + 1, 2):
        buf = fill(48)
        plant(buf, 8, alive)
        r = Run(f"all-alive/cut{c}", bytes(buf), [8 + c])
        r.claim("ab+c matches inside k[a-z]{20}z inside st.*us", alive.find(b"abc") == 4 and alive.find(b"k") == 3 and alive.endswith(b"us"))
        runs.append(r)
    short = b"abbbc"
    for c in range(len(short) + 1):
        buf = fill(40) + bytearray(b"wxyz")
        plant(buf, 10, short)
        runs.append(Run(f"short/cut{c}", bytes(buf), [10 + c]))
    long = b"k" + LETTERS[:20] + b"z"
    for c1 in range(1, len(long)):
        for c2 in sorted({c1 + 1, len(long) - 1, len(long)}):
            if c1 < c2 <= len(long):
                buf = fill(60)
                plant(buf, 7, long)
                plant(buf, 40, b"ffoox-pqrs")
                runs.append(Run(f"three-writes/{c1}/{c2}", bytes(buf), [7 + c1, 7 + c2]))
    for tail, cuts, end in ((b"", [], "close"), (b"\n", [], "close"), (b"\n", [23], "close"), (b"\n-", [24], "close"), (b"\n", [24, 24], "close"), (b"\n", [10], "last"),
                            (b"\n\n", [24], "last")):
        buf = fill(20) + bytearray(b"foo" + tail)
        plant(buf, 3, b"st-us-us")
        runs.append(Run(f"held/{tail!r}/{cuts}/{end}", bytes(buf), cuts, end))
    for c in range(7):
        buf = fill(30)
        plant(buf, 10, b"ffooox")
        runs.append(Run(f"shared-id/cut{c}", bytes(buf), [10 + c]))
    buf = fill(3 * PIECE + 1)  # a long write: the SOM lane walks it serially (at most 16 KiB here)
    plant(buf, PIECE - 2, b"abbc")
    plant(buf, 100, b"st")
    plant(buf, 3 * PIECE - 1, b"us")
    runs.append(Run("long-write", bytes(buf), [3 * PIECE]))
    return runs


def _build_som():
    pats, flags, ids = SOM_SET
    pool = _som_pool()
    for horizon in ("small", "medium", "large"):
        CELLS.append(Cell(f"som-{horizon}", pats, flags, ids, pool, horizon=horizon, staged={0: True}, single_entry=6,
                          claims=[("writes at most 16 KiB", all(b - a <= 16384 for r in pool for a, b in r.writes()))]))
    for items in (1, 8, 63, 64, 65, 130):  # (8: every start-of-match lane of the launch in one wavefront, all of them alive at once)
        runs = [pool[i % len(pool)] for i in range(items)]
        CELLS.append(Cell(f"som-items-{items}", pats, flags, ids, runs, horizon="medium", staged={0: True}, single_entry=0,
                          claims=[("enough distinct runs", len(pool) >= 65)]))


_build_slices()
_build_contexts()
_build_pieces()
_build_shared_ends()
_build_held()
_build_single()
_build_groups()
_build_hbm()
_build_overflow()
_build_som()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)


def cell_lanes(cell: Cell):
    """{lanes per expression: [expressions]}: the slice count of each expression's group."""
    out: dict = {}
    for e in range(len(cell.patterns)):
        out.setdefault(most(cell.npat(e // PPW)), []).append(e)
    return out
