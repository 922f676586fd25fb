"""Pure-Python reference for approximate matching (hs_expr_ext_t edit_distance / hamming_distance), standard library only.

The contract (include/hypergrep_amd.h): an end t of a piece is reported iff data[s:t] is within distance k of some string
the expression matches, for some s <= t.  Edits are one-byte insertions, deletions and substitutions (Hamming:
substitutions only); an inserted or substituting byte is any byte `.` matches (every byte with DOTALL, all but '\\n'
without it); under CASELESS a case change is no edit.  A leading ^ / \\A holds at s, a trailing $ / \\z / \\Z at t.

The expression body is parsed with `sre_parse` into a byte-level Thompson NFA; one state set per error level runs over the
piece, with start states injected at every s where the leading anchor holds.  Anchors are only recognised at the ends of
the expression text; anything else that is an assertion raises Unsupported (the compiler rejects those).
"""
from __future__ import annotations

import sre_constants as C
import sre_parse

HS_FLAG_CASELESS, HS_FLAG_DOTALL, HS_FLAG_MULTILINE, HS_FLAG_SINGLEMATCH, HS_FLAG_SOM_LEFTMOST = 1, 2, 4, 8, 256


class Unsupported(ValueError):
    pass


_WORD = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_")
_DIGIT = frozenset(b"0123456789")
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_CATEGORY = {
    C.CATEGORY_DIGIT: _DIGIT, C.CATEGORY_NOT_DIGIT: _ALL - _DIGIT,
    C.CATEGORY_WORD: _WORD, C.CATEGORY_NOT_WORD: _ALL - _WORD,
    C.CATEGORY_SPACE: _SPACE, C.CATEGORY_NOT_SPACE: _ALL - _SPACE,
}


def _fold(s: frozenset) -> frozenset:
    out = set(s)
    for b in s:
        if 65 <= b <= 90 or 97 <= b <= 122:
            out.add(b ^ 0x20)
    return frozenset(out)


def split_anchors(expr: str):
    """(leading anchor or None, body, trailing anchor or None): anchors are `^` / `\\A` and `$` / `\\z` / `\\Z`."""
    lead = trail = None
    if expr.startswith("^"):
        lead, expr = "^", expr[1:]
    elif expr.startswith("\\A"):
        lead, expr = "\\A", expr[2:]
    for a in ("\\z", "\\Z", "$"):
        if expr.endswith(a) and not expr.endswith("\\" + a):
            trail, expr = a, expr[: -len(a)]
            break
    return lead, expr, trail


class Nfa:
    """Thompson NFA: states are ('char', byteset, next) / ('split', [next...]) / ('match',)."""

    def __init__(self, body: str, flags: int):
        self.caseless = bool(flags & HS_FLAG_CASELESS)
        self.dotall = bool(flags & HS_FLAG_DOTALL)
        self.states: list = [("match",)]
        self.start = self._build(sre_parse.parse(body), 0)
        self._closure: dict = {}

    def _new(self, st) -> int:
        self.states.append(st)
        return len(self.states) - 1

    def _set(self, op, av) -> frozenset:
        if op is C.LITERAL:
            s = frozenset([av])
        elif op is C.NOT_LITERAL:
            return _ALL - (_fold(frozenset([av])) if self.caseless else frozenset([av]))
        elif op is C.ANY:
            return _ALL if self.dotall else _ALL - {10}
        elif op is C.IN:
            s, neg = set(), False
            for o, a in av:
                if o is C.NEGATE:
                    neg = True
                elif o is C.LITERAL:
                    s.add(a)
                elif o is C.RANGE:
                    s.update(range(a[0], a[1] + 1))
                elif o is C.CATEGORY:
                    s.update(_CATEGORY[a])
                else:
                    raise Unsupported(str(o))
            s = _fold(frozenset(s)) if self.caseless else frozenset(s)
            return _ALL - s if neg else s
        else:
            raise Unsupported(str(op))
        return _fold(s) if self.caseless else s

    def _build(self, seq, nxt: int) -> int:
        """State that matches `seq` and continues at nxt."""
        for op, av in reversed(list(seq)):
            nxt = self._item(op, av, nxt)
        return nxt

    def _item(self, op, av, nxt: int) -> int:
        if op in (C.LITERAL, C.NOT_LITERAL, C.ANY, C.IN):
            return self._new(("char", self._set(op, av), nxt))
        if op is C.SUBPATTERN:
            return self._build(av[-1], nxt)
        if op is C.BRANCH:
            return self._new(("split", [self._build(b, nxt) for b in av[1]]))
        if op in (C.MAX_REPEAT, C.MIN_REPEAT):
            lo, hi, body = av
            unbounded = hi is C.MAXREPEAT
            if unbounded:
                loop = self._new(("split", []))
                first = self._build(body, loop)
                self.states[loop] = ("split", [first, nxt])
                cur = loop
            else:
                cur = nxt
                for _ in range(hi - lo):
                    cur = self._new(("split", [self._build(body, cur), nxt]))
                    nxt = cur
            for _ in range(lo):
                cur = self._build(body, cur)
            return cur
        raise Unsupported(str(op))

    def closure(self, s: int) -> frozenset:
        c = self._closure.get(s)
        if c is None:
            out, todo = set(), [s]
            while todo:
                x = todo.pop()
                if x in out:
                    continue
                out.add(x)
                if self.states[x][0] == "split":
                    todo.extend(self.states[x][1])
            c = self._closure[s] = frozenset(out)
        return c


def _lead_ok(lead, data: bytes, s: int, flags: int) -> bool:
    if lead is None:
        return True
    if lead == "^" and flags & HS_FLAG_MULTILINE:
        return s == 0 or data[s - 1] == 10
    return s == 0


def _trail_ok(trail, data: bytes, t: int, flags: int) -> bool:
    n = len(data)
    if trail is None:
        return True
    if trail == "\\z":
        return t == n
    if trail == "$" and flags & HS_FLAG_MULTILINE:
        return t == n or data[t] == 10
    return t == n or (t == n - 1 and data[t] == 10)


class Approx:
    """One expression with its flags and distance: ends(piece) -> sorted ends t, start(piece, t) -> smallest s."""

    def __init__(self, expr: str, flags: int, edit: int = 0, hamming: int = 0, min_offset: int = 0, max_offset: int | None = None):
        assert not (edit and hamming)
        self.flags = flags
        self.min_offset, self.max_offset = min_offset, max_offset
        self.k = edit or hamming
        self.edit = bool(edit)
        self.lead, body, self.trail = split_anchors(expr)
        self.nfa = Nfa(body, flags)
        self.edit_bytes = _ALL if flags & HS_FLAG_DOTALL else _ALL - {10}

    def _run(self, data: bytes, starts):
        """Per end t: the error levels' state sets evolve over data; `starts` yields whether a match may start at s."""
        nfa, k = self.nfa, self.k
        st = nfa.states
        levels = [set() for _ in range(k + 1)]
        ends = []
        for i in range(len(data) + 1):
            if starts(i):
                levels[0] |= nfa.closure(nfa.start)
            if self.edit:  # deletions: skip a pattern byte for one error, chained level by level
                for e in range(k):
                    for x in list(levels[e]):
                        if st[x][0] == "char":
                            levels[e + 1] |= nfa.closure(st[x][2])
            if any(0 in lv for lv in levels) and _trail_ok(self.trail, data, i, self.flags):
                ends.append(i)
            if i == len(data):
                break
            c = data[i]
            nxt = [set() for _ in range(k + 1)]
            for e in range(k + 1):
                for x in levels[e]:
                    if st[x][0] != "char":
                        continue
                    if c in st[x][1]:
                        nxt[e] |= nfa.closure(st[x][2])
                    if e < k and c in self.edit_bytes:
                        nxt[e + 1] |= nfa.closure(st[x][2])
                if self.edit and e < k and c in self.edit_bytes:
                    nxt[e + 1] |= levels[e]
            levels = nxt
        return ends

    def ends(self, data: bytes) -> list[int]:
        return self._run(data, lambda s: _lead_ok(self.lead, data, s, self.flags))

    def reports(self, data: bytes) -> list[int]:
        """The ends delivered for one piece: the offset bounds first, then SINGLEMATCH (the smallest end in bounds)."""
        ends = [t for t in self.ends(data) if t >= self.min_offset and (self.max_offset is None or t <= self.max_offset)]
        return ends[:1] if self.flags & HS_FLAG_SINGLEMATCH else ends

    def start(self, data: bytes, t: int):
        """Smallest s with a match spanning [s, t), or None."""
        for s in range(t + 1):
            if _lead_ok(self.lead, data, s, self.flags) and t in self._run(data, lambda i, s=s: i == s):
                return s
        return None


def piece_reports(exprs, data: bytes):
    """Reports of one piece under the report rules, for exprs = [(Approx, id)] with one expression per id: (id, to)
    sorted, every end of an expression within its offset bounds, the smallest of those only under SINGLEMATCH."""
    out = set()
    for ax, rid in exprs:
        out.update((rid, t) for t in ax.reports(data))
    return sorted(out)
