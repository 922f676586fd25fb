"""The cells of the parts stage (hg_parts.hip, and hg_segparts.hip as its second caller), shared by the host test
(test_parts_cells.py) and the GPU test (test_parts_cells_gpu.py).

A cell is (name, patterns, flags, text, buffer_size, claims).  Expected parts come from parts_ref only.  `claims` say what the
cell is FOR; the host test proves each of them from the compiler's read-out, from the grouped replay's trace or from the text,
so that a cell that stopped reaching its target is noticed:

  ("tier", j, T)   expression j walks as tier T (TIERS below)
  "edge"           a part ends exactly on its group's base + 64
  "jump"           a group ends with cursor > base + 64
  "unaligned"      a group's base is no multiple of 64
  "outrun"         a start inside an accepted part had a match that ends behind that part, and was dropped
  "rounds64"       a group with 64 ballot rounds
  ("words", n)     the database's expression count (the compiler's read-out) gives a first-byte bitmap of n words per byte
                   value, and an expression of the last of them wins a part
  ("wins", j)      expression j wins a part
  "higher_longer"  a part of an expression of index 32 or above, at whose start one below 32 matches exactly a shorter span
  "high_byte"      a part that starts on a byte of 0x80 or above
  ("caseless", j)  parts of expression j that start with the upper and with the lower case of one letter
  "tie"            a part whose end an expression of another bitmap word reaches too
  ("ctx", what)    a piece edge of class `what` (CTX below)

Groups: A1..A5 group-loop geometry, B1..B3 context at piece edges (the plain expressions, their three-word forms, one-byte and
newline parts), C expression selection.  Pieces stay below 1 100 bytes."""
from __future__ import annotations

import invert_ref

A = 6  # DOTALL | MULTILINE
CASELESS, DOTALL, MULTILINE = 1, 2, 4
BIG = 1 << 20
QUIET_LINE = b"nothing here\n"  # no k, q, z, f or w: no expression of the cells matches in it

# tier -> (expression, longest part, (nw, simple))
TIERS = {
    "S": ("k[a-z]{0,20}z", 22, (1, 1)),
    "C": (r"\bk[a-z]{0,20}z\b", 22, (1, 0)),
    "R2": ("k[a-z]{0,50}z", 52, (2, 0)),
    "L3": ("k[a-z]{0,70}z", 72, (3, 0)),
    "L32": ("k[a-z]{0,1000}z", 1002, (32, 0)),
    # 32 words with few live nodes (k, [a-z], z are nodes 990..992: state words 30 and 31): the long parts of the geometry
    # cells.  The compiler lets the k enter all thousand positions of {0,1000} at once, so about a thousand nodes are live
    # behind it; on an MI355X a walk of L32 measured 1.7 ms per byte in the parts stage and 2.2 ms per byte in the scan, so
    # L32 itself keeps the short parts, the saturated groups and the mixed database.
    "L32s": ("Q{990}|k[a-z]*z", 1002, (32, 0)),
}
ORDER = ("S", "C", "R2", "L3", "L32")
LONG_FROM = 9  # parts of L32 from this length on are walked by L32s


def tier_for(tier: str, n: int) -> str:
    return "L32s" if tier == "L32" and n >= LONG_FROM else tier


CTX =("after_word", "after_nonword", "ends_midline", "behind_nuls", "inner_nul", "one_byte", "dollar_nl", "dollar_end", "nl_in_part")


def word(n: int) -> bytes:
    """A part of n >= 2 bytes for every tier expression that reaches so far."""
    return b"k" + b"a" * (n - 2) + b"z"


def line(placed, length: int = 0) -> bytearray:
    """A line of dots with `placed` = [(offset, bytes)] written into it; no final newline."""
    need = max([at + len(b) for at, b in placed] + [length])
    out = bytearray(b"." * need)
    for at, b in placed:
        assert out[at:at + len(b)] == b"." * len(b), (at, b)  # (placements never overlap)
        out[at:at + len(b)] = b
    return out


def tier_db(t):
    """The tier's expression, and a literal that can stand right behind its parts (a second k...z there would be one longer part)."""
    return [TIERS[t][0], "XY"], [A, A], (("tier", 0, t),)


def q_db(t):
    """The tier's expression with a one-byte and a two-byte alternative (the walk is still the tier's), a part that takes the
    newline in, and the empty line."""
    return ["q|XY|" + TIERS[t][0], "q\\n", "^\\n"], [A, A, A], (("tier", 0, t),)


def _a1():
    out = []
    for edge in (64, 128):
        for f in (edge - 64, edge - 63, edge - 2, edge - 1):
            for t in (edge - 1, edge, edge + 1):
                for tier in ORDER:
                    n = t - f
                    if n < 2 or n > TIERS[tier][1]:
                        continue
                    tier = tier_for(tier, n)
                    # the part, a second one at the cursor (for C one byte behind: no \b between z and X), a third further on
                    gap = 1 if tier == "C" else 0
                    body = line([(f, word(n)), (t + gap, b"XY"), (t + gap + 5, b"kaz")])
                    pats, flags, claims = tier_db(tier)
                    if t == edge:
                        claims += ("edge",)
                    out.append((f"A1/{tier} [{f},{t})", pats, flags, QUIET_LINE + bytes(body) + b"\ntail\n", BIG, claims))
    for f in (0, 1, 62, 63):  # ... around 128 from the first group: a jump
        for t in (127, 128, 129):
            body = line([(f, word(t - f)), (t, b"XY"), (t + 63, b"kz"), (t + 65, b"kz")])
            pats, flags, claims = tier_db("L32s")
            out.append((f"A1/L32s [{f},{t})", pats, flags, QUIET_LINE + bytes(body) + b"\n", BIG, claims + ("jump",)))
    return out


def _a2():
    out = []
    for tier, again in (("L3", 66), ("L32s", 129)):
        for n in (66, 129, 200):
            if n > TIERS[tier][1]:
                continue
            for f in (0, 5, 63):
                for d in (0, 63, 64):
                    nb = f + n  # the base behind the jump
                    second = nb + d
                    third = second + 2 + 3
                    behind = third + again + 1
                    body = line([(f, word(n)), (second, b"XY"), (third, word(again)), (behind, b"kaz")])
                    pats, flags, claims = tier_db(tier)
                    claims += ("jump",) + (("unaligned",) if nb % 64 else ())
                    out.append((f"A2/{tier} {n} from {f}, second at +{d}", pats, flags, QUIET_LINE + bytes(body) + b"\n", BIG, claims))
    return out


def _a3():
    out = []
    # literals: ab{6} is accepted at p; bbbx starts inside it and ends one byte behind it (dropped); xq starts exactly at its
    # end (taken); the second bbbx lies in the same group behind the cursor (taken)
    for p in (10, 57, 60, 70):
        body = line([(p, b"abbbbbbxq bbbx")])
        claims = (("tier", 0, "S"), ("tier", 1, "S")) + (("outrun",) if p != 60 else ("jump",)) + (("edge",) if p == 57 else ())
        out.append((f"A3/S at {p}", ["ab{6}", "bbbx", "xq"], [A] * 3, QUIET_LINE + bytes(body) + b"\n", BIG, claims))
    # the same with walks of two and of three words: k...z accepted, m...zx from inside it ends one byte behind it
    for tier, g, h in (("R2", 20, 20), ("L3", 30, 35)):
        n = TIERS[tier][1] - 2
        pats = [TIERS[tier][0], "m[a-z]{0,%d}zx" % n, "xq"]
        for p in (3, 40):
            body = line([(p, b"k" + b"a" * g + b"m" + b"a" * h + b"zxq maazx")])
            same_group = (p + 1 + g) // 64 == p // 64
            claims = (("tier", 0, tier),) + (("outrun",) if same_group else ("jump",))
            out.append((f"A3/{tier} at {p}", pats, [A] * 3, QUIET_LINE + bytes(body) + b"\n", BIG, claims))
    # one word with conditions: the literals' geometry between non-word bytes
    for p in (10, 57, 70):
        body = line([(p, b"abbbbbb-q bbb-")])
        claims = (("tier", 0, "C"), "outrun") + (("edge",) if p == 57 else ())
        out.append((f"A3/C at {p}", [r"\bab{6}\b", "bbb-", "-q"], [A] * 3, QUIET_LINE + bytes(body) + b"\n", BIG, claims))
    # 32 words: L32 itself with a short accepted part, L32s with the long one of the three-word cells
    for p in (3, 57):
        body = line([(p, b"kamazxq maazx")])
        out.append((f"A3/L32 at {p}", [TIERS["L32"][0], "m[a-z]{0,5}zx", "xq"], [A] * 3, QUIET_LINE + bytes(body) + b"\n", BIG, (("tier", 0, "L32"), "outrun")))
    for p in (3, 40):
        body = line([(p, b"k" + b"a" * 30 + b"m" + b"a" * 35 + b"zxq maazx")])
        claims = (("tier", 0, "L32s"),) + (("outrun",) if p == 3 else ("jump",))
        out.append((f"A3/L32s at {p}", [TIERS["L32s"][0], "m[a-z]{0,70}zx", "xq"], [A] * 3, QUIET_LINE + bytes(body) + b"\n", BIG, claims))
    return out


def _a4():
    out = []
    for tier in ORDER:
        pats, flags, claims = q_db(tier)
        for name, body, extra in (("64 adjacent", b"q" * 64, ("rounds64",)), ("65 adjacent", b"q" * 65, ("rounds64",)), ("128 adjacent", b"q" * 128, ("rounds64",)),
                                  ("every second byte", b"q." * 64, ()), ("two-byte parts, seam on the edge", b"XY" * 40, ("edge",)),
                                  ("two-byte parts across the edge", b"." + b"XY" * 40, ()),
                                  ("neighbouring lanes walk at once", b"." * 58 + b"k" * 10 + b"az kkz", ())):
            out.append((f"A4/{tier} {name}", pats, flags, QUIET_LINE + body + b"\ntail\n", BIG, claims + extra))
    return out


def _a5():
    out = []
    turn = 0
    for tier in ORDER:
        pats, flags, claims = q_db(tier)
        for n in (1, 2, 63, 64, 65, 127, 128, 129):
            # with the final newline: the last part takes it in (q\n; the empty line for n = 1)
            body = b"\n" if n == 1 else b"." * (n - 2) + b"q\n"
            out.append((f"A5/{tier} {n} bytes, newline", pats, flags, QUIET_LINE + body, BIG, claims + (("edge",) if n == 64 else ())))
            # without: the last line of a text of 4k + 1, 2, 3 bytes
            body = b"." * (n - 1) + b"q"
            turn += 1
            lead = QUIET_LINE[:-1] + b" " * ((1 + turn % 3 - len(QUIET_LINE) - n) % 4) + b"\n"
            assert (len(lead) + n) % 4 == 1 + turn % 3
            out.append((f"A5/{tier} {n} bytes, unterminated", pats, flags, lead + body, BIG, claims))
        for n in (65, 129):  # a long part that ends with the text, and a walk that is still alive there without an end
            m = min(TIERS[tier][1], n - 2, 20 if tier == "L32" else n)
            out.append((f"A5/{tier} {n} bytes, part of {m} at the end", pats, flags, QUIET_LINE + b"." * (n - m) + word(m), BIG, claims))
            out.append((f"A5/{tier} {n} bytes, walk alive at the end", pats, flags, QUIET_LINE + b"q" + b"." * (n - m - 1) + word(m)[:-1], BIG, claims))
    return out


# --- B: context at piece edges ---------------------------------------------------------------------------------------------
B_TEXTS = [
    ("cut behind a word byte", b"abcdefgfoo foo\nfoo\n", 8, ("after_word", "ends_midline")),
    ("cut behind a non-word byte", b"abcdef foo xfoo\n", 8, ("after_nonword", "ends_midline")),
    ("piece ends before a word byte", b"xxx foobar foo\n", 8, ("ends_midline", "after_word")),
    ("piece ends before a space", b"xxx foo bar\n", 8, ("ends_midline", "after_word")),
    ("behind leading NULs", b"\0\0foo bar\nx\n\0\0\0foo\n\0f\n", BIG, ("behind_nuls", "dollar_nl")),
    ("cut by an inner NUL", b"a foo\0foo x\nfoo\0\nf\0f\n", BIG, ("inner_nul",)),
    ("one-byte last line", b"x\nf", BIG, ("one_byte", "dollar_end")),
    ("one-byte pieces", b"fff\nf\n", 2, ("one_byte", "after_word", "ends_midline")),
    ("dollar before the final newline", b"xfoo\nfoo\nf\n", BIG, ("dollar_nl",)),
    ("dollar at an unterminated end", b"x\nxfoo", BIG, ("dollar_end",)),
    ("long words", b"foo" + b"abc" * 20 + b" foo" + b"z" * 66 + b" zfoo" + b"a" * 75 + b" foo\n" + b"foo" + b"b" * 70, BIG, ("dollar_end",)),
    ("empty lines", b"x\n\n\nfoo\n\n", BIG, ("dollar_nl",)),
    ("long word cut mid-line", b"x" * 60 + b"foo" + b"a" * 77 + b" foo\n", 101, ("after_word", "ends_midline")),
]
B_EXPRESSIONS = [(r"\bfoo", A), (r"foo\b", A), (r"\Bfoo", A), ("^foo", A), ("^foo", DOTALL), ("foo$", A), ("foo$", DOTALL)]
B_LONG = {r"\bfoo": r"\bfoo[a-z]{0,70}", r"foo\b": r"foo[a-z]{0,70}\b", r"\Bfoo": r"\Bfoo[a-z]{0,70}", "^foo": "^foo[a-z]{0,70}", "foo$": "foo[a-z]{0,70}$"}
# one-byte parts (s + 1 == len at the walk's entry; `$\n` enters on the final newline itself), the `$` a DOTALL part runs on
# from, and a part that holds the newline
B_SHORT = [("^f$", A), (r"\bf\b", A), ("f$", DOTALL), ("f$", A), ("^f", DOTALL), (r"\Bf", A), ("foo$.", A), ("f$.?", A), ("foo.*", A), ("$\\n", A)]


def _b(which):
    out = []
    dbs = {"B1": [(e, f, ()) for e, f in B_EXPRESSIONS], "B2": [(B_LONG[e], f, (("tier", 0, "L3"),)) for e, f in B_EXPRESSIONS],
           "B3": [(e, f, ()) for e, f in B_SHORT]}[which]
    for expr, flag, tier in dbs:
        for name, text, bs, ctx in B_TEXTS:
            claims = tier + tuple(("ctx", c) for c in ctx)
            tails = [p[-4:] for _a, p in invert_ref.pieces(text, bs)]
            if expr in ("foo$.", "foo.*") and b"foo\n" in tails or expr == "$\\n" and any(t.endswith(b"\n") for t in tails) or expr == "f$.?" and any(t.endswith(b"f\n") for t in tails):
                claims += (("ctx", "nl_in_part"),)
            out.append((f"{which}/{expr} flags {flag}: {name}", [expr], [flag], text, bs, claims))
    return out


# --- C: expression selection ----------------------------------------------------------------------------------------------
def _c():
    out = []
    for n in (1, 31, 32, 33, 63, 64, 65, 97):
        words = [f"w{i:02d}x" for i in range(n)]
        winners = sorted({i for i in (0, 31, 32, 63, 64, n - 1) if i < n})
        text = QUIET_LINE + b" ".join(words[i].encode() for i in reversed(winners)) + b"\nw00 " + words[-1].encode() + b"x\n"
        claims = tuple(("tier", i, "S") for i in winners) + tuple(("wins", i) for i in winners) + (("words", (n + 31) // 32),)
        out.append((f"C/{n} literal words", words, [A] * n, text, BIG, claims))
    # 40 expressions, two bitmap words: 35 ties with 3 (the lower index wins), 36 is longer than 5 (the higher word wins),
    # 37 ties with 34 inside the second word
    pats = [f"w{i:02d}x" for i in range(35)] + ["w0[0-9]x", "w05x+", "w3[0-9]x"] + [f"v{i:02d}x" for i in range(2)]
    text = QUIET_LINE + b"w03x w05xx w05x w34x v01x w09x\n"
    out.append(("C/tie across bitmap words", pats, [A] * 40, text, BIG, (("words", 2), "tie", "higher_longer", ("wins", 3), ("wins", 36), ("wins", 34))))
    out.append(("C/high first bytes", ["\\xe9a", "\\xffb", "\\x80c", "a"], [A] * 4, QUIET_LINE + b"\xe9a \xffb\x80c \xe9\xff a\xe9a\n\xffb", BIG,
                ("high_byte", ("wins", 0), ("wins", 1), ("wins", 2), ("wins", 3))))
    out.append(("C/caseless first byte", ["hello", "World"], [A | CASELESS, A], QUIET_LINE + b"Hello hello HELLO world World\n", BIG,
                (("caseless", 0), ("wins", 1))))
    out.append(("C/class-led and dot-led", ["[a-f]x", ".oo"], [A, A], QUIET_LINE + b"cx foo gx fx\noo\n.oo ooo\n", BIG, (("wins", 0), ("wins", 1))))
    # the five tiers in one database (max_nw = 32: LDS is allocated, most winners walk in registers).  The languages are nested
    # and a tie goes to the lowest index, so each tier wins where the ones before it cannot match: C on a short word between
    # non-word bytes, S on one that leans on a word byte, R2, L3 and L32 by length.  No start can give C its own end (its \b
    # forbids the letter every longer match needs), so: one start where the four others match with four different ends
    # (z at 10, 40, 65 and 90 bytes), and one where all five match with the same end.
    pats = [TIERS[t][0] for t in ("C", "S", "R2", "L3", "L32")]
    claims = tuple(("tier", j, t) for j, t in enumerate(("C", "S", "R2", "L3", "L32"))) + tuple(("wins", j) for j in range(5))
    four = bytearray(b"k" + b"a" * 89 + b"z")
    for at in (10, 40, 65):
        four[at] = ord("z")
    text = QUIET_LINE + b"kaz 1kaaz " + word(40) + b" " + word(60) + b" " + word(80) + b" " + bytes(four) + b" kz\n" + word(30) + b"\n"
    out.append(("C/five tiers in one database", pats, [A] * 5, text, BIG, claims))
    return out


# The pipeline-chunk test's database (GPU only): the S and the L3 walk with different first bytes (a lane walks one of them) and
# the part that takes a newline in.  CHUNK_TIERS: what the host test reads out for it.
CHUNK_SET = (["q|XY|" + TIERS["S"][0], "m[a-z]{0,70}z", "q\\n"], [A, A, A])
CHUNK_TIERS = ("S", "L3", "S")

GROUPS = {"A1": _a1(), "A2": _a2(), "A3": _a3(), "A4": _a4(), "A5": _a5(), "B1": _b("B1"), "B2": _b("B2"), "B3": _b("B3"), "C": _c()}
CELLS = [c for g in GROUPS.values() for c in g]
assert len({c[0] for c in CELLS}) == len(CELLS)  # names are unique
