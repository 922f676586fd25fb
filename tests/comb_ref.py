"""Independent Python reference for logical combinations (HS_FLAG_COMBINATION, HS_FLAG_QUIET) — TEST INFRASTRUCTURE ONLY.

It shares no code with the product: its own formula parser and evaluator, applied per line piece to the reports of the
set with the combinations removed and QUIET cleared (the oracle's reports, or a list made up by a test), following the
contract in include/hypergrep_amd.h.
"""
from __future__ import annotations

COMBINATION, QUIET, SINGLE = 512, 1024, 8


class FormulaError(ValueError):
    pass


def parse(text: str):
    """Formula -> tree: ("id", n) | ("!", t) | ("&", a, b) | ("|", a, b).  `!` > `&` > `|`, whitespace ignored."""
    toks = []
    i = 0
    while i < len(text):
        c = text[i]
        if c.isspace():
            i += 1
        elif c in "!&|()":
            toks.append(c)
            i += 1
        elif "0" <= c <= "9":
            j = i
            while j < len(text) and "0" <= text[j] <= "9":
                j += 1
            v = int(text[i:j])
            if v > 0xFFFFFFFF:
                raise FormulaError("id too large")
            toks.append(v)
            i = j
        else:
            raise FormulaError(f"bad character {c!r}")
    pos = 0

    def peek():
        return toks[pos] if pos < len(toks) else None

    def take():
        nonlocal pos
        pos += 1
        return toks[pos - 1]

    def p_or():
        t = p_and()
        while peek() == "|":
            take()
            t = ("|", t, p_and())
        return t

    def p_and():
        t = p_not()
        while peek() == "&":
            take()
            t = ("&", t, p_not())
        return t

    def p_not():
        tok = peek()
        if tok == "!":
            take()
            return ("!", p_not())
        if tok == "(":
            take()
            t = p_or()
            if peek() != ")":
                raise FormulaError("unbalanced")
            take()
            return t
        if isinstance(tok, int):
            take()
            return ("id", tok)
        raise FormulaError(f"unexpected {tok!r}")

    if not toks:
        raise FormulaError("empty")
    tree = p_or()
    if pos != len(toks):
        raise FormulaError(f"trailing {toks[pos]!r}")
    return tree


def operands(tree) -> set:
    if tree[0] == "id":
        return {tree[1]}
    return set().union(*(operands(t) for t in tree[1:]))


def evaluate(tree, true_ids) -> bool:
    op = tree[0]
    if op == "id":
        return tree[1] in true_ids
    if op == "!":
        return not evaluate(tree[1], true_ids)
    if op == "&":
        return evaluate(tree[1], true_ids) and evaluate(tree[2], true_ids)
    return evaluate(tree[1], true_ids) or evaluate(tree[2], true_ids)


class CombSet:
    """The combinations and QUIET ids of a set of expressions."""

    def __init__(self, patterns, flags, ids):
        self.base = [i for i, f in enumerate(flags) if not f & COMBINATION]  # expressions the oracle scans
        self.quiet = {ids[i] for i in self.base if flags[i] & QUIET}
        self.combs = []  # (id, tree, single)
        for i, f in enumerate(flags):
            if f & COMBINATION and not f & QUIET:
                self.combs.append((ids[i], parse(patterns[i]), bool(f & SINGLE)))

    def oracle_inputs(self, patterns, flags, ids):
        """patterns, flags (QUIET cleared), ids of the set without its combinations"""
        return [patterns[i] for i in self.base], [flags[i] & ~QUIET for i in self.base], [ids[i] for i in self.base]

    def piece(self, reports):
        """reports: one piece's (id, to) after the report rules -> the delivered (id, to), in (id, to) order."""
        first = {}
        for rid, to in reports:
            first[rid] = min(to, first.get(rid, to))
        out = [(rid, to) for rid, to in reports if rid not in self.quiet]
        for cid, tree, single in self.combs:
            ops = operands(tree)
            events = sorted({to for rid, to in reports if rid in ops})
            for t in events:
                if evaluate(tree, {x for x in ops if x in first and first[x] <= t}):
                    out.append((cid, t))
                    if single:
                        break
        return sorted(set(out))


def apply_to_hits(cs: CombSet, hits):
    """hits: (line_number, id, to, line_off, line_len) of whole pieces, as oracle_py.scan_buffer gives them -> the delivered
    hits in the same form, ordered by (line, id, to)."""
    by_line = {}
    for h in hits:
        by_line.setdefault(h[0], []).append(h)
    out = []
    for line in sorted(by_line):
        hs = by_line[line]
        off, ln = hs[0][3], hs[0][4]
        for rid, to in cs.piece(sorted({(h[1], h[2]) for h in hs})):
            out.append((line, rid, to, off, ln))
    return out
