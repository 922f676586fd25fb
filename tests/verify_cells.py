"""Cells for the verify pass (hg_verify_kernel / hg_verify_lean_kernel) and the lists of verified occurrences behind it, and
an exact reference for them.

The verify pass takes the stream pass's candidates (a window value at a position) to the literals that hold the window: by
the direct window table, or by the discriminated buckets; it compares each (candidate, literal) pair with the text, and files
the verified occurrences in per-mode lists, the automaton modes 1 and 2 through a staging area in LDS.  Which of these paths
a candidate takes is a property of the compiled set, and a cell claims it: tests/test_verify_cells.py proves the claims from
the compiler's tables (hgsim_py.Db.windows(), selfcheck()) and from the engine's sizing rules restated here.

reference(): bytes.find of every expression's literal on every line piece, the expression's tail condition (none for a
literal, "any byte but '#', then three digits" or a word boundary for the automaton shapes used here), then the report rules of
hg_post.h as tests/finalize_cells.py states them.  Case-insensitive literals are found in the lower-cased text (ASCII letters
only change: '{' stays apart from '[').
"""
from __future__ import annotations

import bisect
import functools
import random
from dataclasses import dataclass, field

import finalize_cells as fc
from stream_cells import LOOKALIKE_PAIRS

TILE = 16384
CAND_CAP0 = 1 << 16  # candidate records of a fresh scanner for texts of up to 64 MiB (HgScanner::ensure)
DEFER_SHARDS = 64
STAGE_CAP = 768      # VERIFY_STAGE_CAP of hg_kernels.hip: flushed at half, filed directly when full
ESCAPE = set(b"\\.^$|?*+()[]{}")


@dataclass(frozen=True)
class Expr:
    lit: bytes
    id: int
    single: bool = True
    nocase: bool = False
    tail: object = None  # None: a literal; bytes of three digits: lit [^#] digits; "word": \\b lit \\b

    @property
    def pattern(self) -> str:
        body = "".join(("\\" + chr(c)) if c in ESCAPE else chr(c) for c in self.lit)
        if self.tail == "word":
            body = "\\b" + body + "\\b"
        elif self.tail is not None:
            body += "[^#]" + self.tail.decode()
        return ("(?i)" if self.nocase else "") + body

    @property
    def flags(self) -> int:
        return fc.FLAG_SINGLE if self.single else fc.FLAG_MULTI


def is_word(c: int) -> bool:
    return c == 95 or 48 <= c <= 57 or 65 <= c <= 90 or 97 <= c <= 122


# ---------------------------------------------------------------------------------------------------- the reference
def reference(text: bytes, exprs, buffer_size: int = 262140, line_base: int = 0):
    """(records [(line, id, to, start, len)] in delivery order, n_lines, verified): `verified` counts the literal occurrences
    that lie whole in a piece, whether or not the tail lets them report (what the verify pass files)."""
    assert b"\0" not in text
    starts, lens = fc.split_pieces(text, buffer_size)
    lowered = text.lower()
    ends = {}  # piece -> {(id, to): is a SINGLEMATCH report}
    verified = 0
    for e in exprs:
        hay, lit = (lowered, e.lit.lower()) if e.nocase else (text, e.lit)
        pos = hay.find(lit)
        while pos >= 0:
            k = bisect.bisect_right(starts, pos) - 1
            a, z = starts[k], starts[k] + lens[k]
            end = pos + len(lit)
            if end <= z:
                verified += 1
                ok = True
                if e.tail == "word":
                    ok = (pos == a or not is_word(text[pos - 1])) and (end == z or not is_word(text[end]))
                elif e.tail is not None:
                    ok = end + 4 <= z and text[end] != 35 and text[end + 1:end + 4] == e.tail
                    end += 4
                if ok:
                    ends.setdefault(k, []).append((e.id, end - a, e.single))
            pos = hay.find(lit, pos + 1)
    records = []
    for k in sorted(ends):
        first = {}
        for rid, to, single in ends[k]:
            if single:
                first[rid] = min(to, first.get(rid, to))
        kept = {(rid, to) for rid, to, single in ends[k] if not single or to == first[rid]}
        records += [(line_base + k, rid, to, starts[k], lens[k]) for rid, to in sorted(kept)]
    return records, len(starts), verified


# ---------------------------------------------------------------------------------------------------------- sets
def random_literals(n: int, length: int, seed: int):
    rng, out = random.Random(seed), set()
    while len(out) < n:
        out.add("".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(length)).encode())
    return sorted(out)


def literal_set(lits, nocase=False, single=True, first_id=0):
    return [Expr(lit, first_id + i, single, nocase) for i, lit in enumerate(lits)]


R40 = literal_set(random_literals(40, 12, 1))
STEMS30 = literal_set([b"shared_stem_%03d" % i for i in range(30)], first_id=100)
STEMS200 = literal_set([b"shared_stem_%03d" % i for i in range(200)])
BYTEWIN = literal_set([b"abc", b"xyz1", b"q=7"])
# byte-aligned windows, one per literal: the least shared window of these nine sits at literal offset 2, three literals hold each
# value, and what tells them apart is their first byte: a discriminator of delta -4 that selects bytes 2 and 3 of its dword.  A
# literal in the text's first two bytes is then looked up from an address below the text with its selected bytes inside it.
NEGATIVE = literal_set([b"xyz"] + [bytes([a]) + b"abcd" + bytes([z]) for a in b"123" for z in b"pqr"])
CI2 = literal_set([b"needle_{one}~ab", b"other`two|cd_ef"], nocase=True)
CI70 = literal_set(random_literals(68, 12, 2) + [b"needle_{one}~ab", b"other`two|cd_ef"], nocase=True)
# (letters behind the stem: the bytes that tell the literals apart, which the discriminator selects, fold)
CI_STEMS = literal_set([b"Shared_Stem_" + bytes([97 + i % 26, 97 + i // 26, 122 - i % 7]) for i in range(100)], nocase=True)
R3000 = literal_set(random_literals(3000, 12, 3))
ALPHABET = b"abcdefghijklmnopqrstuvwxyz0123456789ABCD"
LENGTHS = literal_set([(b"len%02d_" % n + ALPHABET)[:n] for n in range(7, 33)]
                      + [b"prefix_literal", b"prefix_literal_longer", b"shared_stem_000", b"hared_stem_0"])


def family(lit: bytes, n: int, first_id: int, tail_fmt=b"%03d"):
    return [Expr(lit, first_id + i, True, False, tail_fmt % i) for i in range(n)]


# expressions that share ONE required literal cannot be told apart by any discriminator: a bucket of as many windows
BUCKET_SIZES = (200, 65, 64, 63, 4, 2, 1)
BUCKETS = [e for k, n in enumerate(BUCKET_SIZES) for e in family(b"bucket_of_%03d_literal" % n, n, 1000 * k)]


# Candidates that belong to no literal.  The filter's second level knows the window values of a small set exactly, so what it
# lets through beside the literals are real windows in the wrong place: the stem of STEMS200 followed by three letters passes
# at its window "tem_" (offset 8), whose discriminator selects the three bytes behind the stem.  Other bytes there name another
# bucket: an empty one (zero pairs) or, for the words of NOISE_MISMATCH, a bucket that holds other windows (the value compare
# inside the bucket rejects).  tests/test_verify_cells.py proves both from the candidate read-out (hgsim_candidates).
NOISE_MISMATCH = (b"adp", b"cqa", b"dpz", b"duv", b"fcp", b"fjm", b"gsx", b"hik", b"hpx", b"hsz", b"jfv", b"joe")


def noise_words(n: int, seed: int):
    rng, out = random.Random(seed), []
    while len(out) < n:
        w = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(3))
        if w not in NOISE_MISMATCH and w not in out:
            out.append(w)
    return out


def noise_line(word: bytes, cur: int) -> bytes:
    """One line whose stem begins on a multiple of 4 (its window at offset 8 is then probed), when the line begins at `cur`."""
    return b"." * ((-cur) % 4) + b"shared_stem_" + word + b"\n"


STEMS1_200 = [Expr(b"shared_stem_%03d" % i, 9000 + i, True, False, b"123") for i in range(200)]  # mode 1, as BUCKETS


def spread_set(mode: int, n: int):
    """n expressions of one automaton mode, each with a literal of its own."""
    if mode == 1:
        return [Expr(b"spread_one_%03d_lit" % i, i, True, False, b"123") for i in range(n)]
    return [Expr(b"spread_two_%03d_lit" % i, i, True, False, "word") for i in range(n)]


MIXED = [Expr(b"mixed_literal_zero", 1), Expr(b"mixed_simple_one", 2, True, False, b"456"), Expr(b"mixed_context_two", 3, True, False, "word"),
         Expr(b"mixed_generic_three", 4, False)]
MIXED_HUGE = "mixed_huge_four.{0,1100}end_h"  # (mode 4; found by its own rule below)
OVERFLOW = spread_set(1, 64)


# ---------------------------------------------------------------------------------------------------------- texts
class Text:
    """Lines appended one after the other; at(lit, residue) puts a literal on a line of its own at a text offset with the
    given residue modulo 16."""

    def __init__(self):
        self.parts, self.cur = [], 0

    def add(self, data: bytes):
        self.parts.append(data)
        self.cur += len(data)
        return self

    def at(self, lit: bytes, residue: int, behind: bytes = b" .\n"):
        pad = (residue - self.cur) % 16
        return self.add(b"." * pad + lit + behind)

    def bytes(self) -> bytes:
        return b"".join(self.parts)


def case_variant(lit: bytes, k: int) -> bytes:
    return bytes(c ^ 0x20 if (65 <= c <= 90 or 97 <= c <= 122) and (i + k) % 2 else c for i, c in enumerate(lit))


def _alignments(exprs, nocase=False):
    """Every literal at every text offset modulo 16, the literals taking turns (lengths 16 and 17 meet in one wave)."""
    def make():
        t = Text()
        for r in range(16):
            for i, e in enumerate(exprs):
                t.at(case_variant(e.lit, r + i) if nocase else e.lit, r)
        return t.bytes()
    return make


def _near_misses():
    """The 32-byte literal with one byte changed, at every byte; every literal followed by bytes that its record does not
    hold (the compare mask's tail); a literal that ends on the line's newline."""
    t = Text()
    long = LENGTHS[32 - 7].lit
    assert len(long) == 32
    for j in range(32):
        for r in (0, 5):
            t.at(long[:j] + bytes([long[j] ^ 1]) + long[j + 1:], r)
    for e in LENGTHS:
        for behind in (b"\xff\xff\xff\xff\n", b"z\n", b"\n"):
            t.at(e.lit, 3, behind)
        t.at(e.lit[:-1] + bytes([e.lit[-1] ^ 2]), 7)
    return t.bytes()


def _case_and_lookalikes(exprs):
    def make():
        t = Text()
        for e in exprs[-2:] + exprs[:6]:
            for k in range(4):
                t.at(case_variant(e.lit, k), k * 5)
            for j, c in enumerate(e.lit):  # a byte that differs from the literal's in bit 5 alone and is no letter
                pair = {**LOOKALIKE_PAIRS, **{v: k for k, v in LOOKALIKE_PAIRS.items()}}
                if c in pair:
                    t.at(e.lit[:j] + bytes([pair[c]]) + e.lit[j + 1:], j)
                elif not (65 <= c <= 90 or 97 <= c <= 122):
                    t.at(e.lit[:j] + bytes([c ^ 0x20]) + e.lit[j + 1:], j)  # '_' against 0x7f, a digit against a control byte
        return t.bytes().replace(b"\0", b"?")
    return make


def _ends(exprs):
    """Texts that end with a literal, at every length modulo 16 (no newline behind it), and texts that begin inside one."""
    out = []
    for e in exprs:
        for r in range(16):
            head = b"." * 40 + b"\n"
            lit = case_variant(e.lit, r) if e.nocase else e.lit  # (the byte compare at the buffer's end under the case bits)
            out.append((f"end-{len(e.lit)}-{r}", head + b"." * ((r - len(head) - len(e.lit)) % 16) + lit))
        for cut in range(1, len(e.lit) - 3):
            out.append((f"begin-{len(e.lit)}-{cut}", e.lit[cut:] + b" .\n" + e.lit + b"\n"))
    return out


def _random_words(seed: int, nbytes: int, alphabet=b"abcdefghijklmnopqrstuvwxyz0123456789"):
    """Text over the literals' alphabet: nearly every window the filter lets through belongs to no literal."""
    def make():
        rng = random.Random(seed)
        out = bytearray()
        while len(out) < nbytes:
            out += bytes(rng.choice(alphabet) for _ in range(rng.randint(20, 90))) + b"\n"
        return bytes(out)
    return make


def _plant_all(exprs, seed: int, noise=None):
    def make():
        rng = random.Random(seed)
        t = Text()
        for e in exprs:
            t.at(e.lit, rng.randrange(16))
        return t.bytes() + (noise() if noise else b"")
    return make


def hit(e: Expr, good: bool = True) -> bytes:
    """The bytes of one occurrence of the expression that reports (or, with good=False, that verifies and does not report)."""
    if e.tail == "word":
        return b" " + e.lit + (b" " if good else b"x")
    if e.tail is not None:
        return e.lit + b"x" + (e.tail if good else b"xyz")
    return e.lit


def _bucket_text(counts: dict, gap: int = 40, noise: bytes = b""):
    """counts: {bucket size: candidates}: so many occurrences of that family's literal, one per line, the k-th followed by the
    digits of the family's member k (one report each); `noise` between them."""
    def make():
        t = Text()
        for size, n in counts.items():
            fam = [e for e in BUCKETS if e.lit == b"bucket_of_%03d_literal" % size]
            for k in range(n):
                t.add(noise + b"." * (gap - 25) + hit(fam[k % size]) + b"\n")
        return t.bytes()
    return make


def _text_starts(exprs):
    """Texts that begin with a literal, one and two bytes into the text as well, and further in."""
    return [(f"start-{e.lit.decode()}-{k}", b"." * k + e.lit + b" .\n" + b"." * 30 + e.lit + b"\n") for e in exprs for k in (0, 1, 2, 5)]


def _stems_with_noise():
    """Every literal of STEMS200 once, 300 zero-pair candidates and the value-mismatch words between them."""
    rng = random.Random(9)
    t = Text()
    words = noise_words(300, 10) + list(NOISE_MISMATCH) * 2
    rng.shuffle(words)
    for i, e in enumerate(STEMS200):
        t.at(e.lit, rng.randrange(16))
        for w in words[i::len(STEMS200)]:
            t.add(noise_line(w, t.cur))
    return t.bytes()


def _stem_cuts():
    """Texts of 1024 bytes that end inside a stem literal, its window on the last dword of the 1 KiB row (where the filter
    cannot see the dword behind the window and lets it pass): the discriminator's selected bytes lie at or behind the text's end."""
    out = []
    for k in range(3):  # the window at literal offset 8 + k stands at byte 1020
        start = 1020 - 8 - k
        head = (b"." * 99 + b"\n") * 10
        out.append((f"cut-{k}", head + b"." * (start - len(head)) + b"shared_stem_007"[:12 + k]))
    return out


def _interleaved(order):
    """Candidates in the order given: a number is an occurrence of that family's literal (so many pairs), "z" a zero-pair
    candidate, "m" a candidate whose bucket holds other windows only."""
    def make():
        t = Text()
        zero, mism = noise_words(64, 21), list(NOISE_MISMATCH)
        for k, what in enumerate(order):
            if what == "z":
                t.add(noise_line(zero[k % len(zero)], t.cur))
            elif what == "m":
                t.add(noise_line(mism[k % len(mism)], t.cur))
            else:
                fam = [e for e in BUCKETS if e.lit == b"bucket_of_%03d_literal" % what]
                t.add(b"." * 15 + hit(fam[k % what]) + b"\n")
        return t.bytes()
    return make


ZERO_MIXED = [200, "z", "z", 200, "z", 1, 200, "m", "z", "z", "z", 65, 200, "z", 200, 2, "z", 200, "z", "z", 63, 200, "m", 200, "z", 64, 200, "z", "z", 4, "z"]
ZERO_EDGES = ["z"] + [200, 65] * 10 + ["z"] * 42 + ["z"]  # the wave's first and last lane hold no pair, equal prefixes run over 43 lanes


def _dense_buckets():
    """16 tiles and more, a candidate every 64 bytes, four verified pairs each (the family of four): a round of a block stages
    4 waves * 64 candidates * 4 pairs = 1024 > 768 occurrences."""
    fam = [e for e in BUCKETS if e.lit == b"bucket_of_004_literal"]
    line = lambda k: (b"." * 38 + hit(fam[k % 4]) + b"\n")
    assert len(line(0)) == 64
    return b"".join(line(k) for k in range(17 * TILE // 64))


def _spread_text(exprs, repeat: int = 3):
    def make():
        t = Text()
        for k in range(repeat):
            for i, e in enumerate(exprs):
                t.at(hit(e, good=(i + k) % 3 != 0), (i + k) % 16, b"\n")
        return t.bytes()
    return make


def _overflow_text():
    """One expression of a mode with 64 expressions owns nearly every occurrence: 3000 of them against a list of
    overflow_capacity() records."""
    e0 = OVERFLOW[0]
    rest = b"".join(hit(e) + b"\n" for e in OVERFLOW[1:])
    return rest + b"".join(b"." * (k % 7) + hit(e0, good=k % 5 != 0) + b"\n" for k in range(3000))


def overflow_capacity() -> int:
    """Records of one list of verified occurrences on a fresh scanner: defer_shard_cap = cand_cap_ / HG_DEFER_SHARDS
    (HgScanner::plan_pass), cand_cap_ = 2^16 for a text of up to 64 MiB (HgScanner::ensure).  A mode with 64 expressions or more
    has list_spread 1: every occurrence of an expression goes to ONE list."""
    return CAND_CAP0 // DEFER_SHARDS


def _joiner_text():
    """2050 tiles of filler lines, the shared-stem set's literals around the two pipeline cuts and sprinkled between."""
    rng = random.Random(77)
    t = Text()
    exprs = R40 + STEMS30
    fill = b"." * 199 + b"\n"
    for at in sorted([1024 * TILE - 4000, 2048 * TILE - 4000] + [rng.randrange(0, 2049 * TILE) for _ in range(300)]):
        if at < t.cur:
            continue
        t.add(fill * ((at - t.cur) // 200))
        for e in rng.sample(exprs, 25):
            t.at(e.lit, rng.randrange(16))
        if at in (1024 * TILE - 4000, 2048 * TILE - 4000):  # lines up to and across the cut
            while t.cur < at + 8000:
                t.at(rng.choice(exprs).lit, rng.randrange(16), b" " + b"." * rng.randrange(300) + b"\n")
    t.add(fill * ((2050 * TILE - t.cur) // 200))
    return t.bytes()


# ---------------------------------------------------------------------------------------------------------- cells
@dataclass
class Cell:
    name: str
    exprs: list
    texts: list            # [(name, () -> bytes or bytes)]
    tags: tuple
    claim: dict = field(default_factory=dict)
    # claim: table_first, shared_windows, byte_windows, fold_mask (selfcheck / info); modes {mode: expressions} (the compiler);
    #   windows_per_literal; buckets (sizes that must occur in the read-out); ways / probes (table classes that must occur);
    #   kernel "staged" | "lean"; candidates {text: n} (the host mirror's filter, equal on the GPU); false_positives_min {text: n};
    #   verified / verified_min {text: n} (from the reference); final_flush_only (texts); zero_pair_candidates / mismatch_candidates {text: n},
    #   value_mismatch_min, zero_pairs_min, table_ends_min, negative_at_min (the candidate read-out, hgsim_candidates); reruns_min, second_reruns; joiner_launches_min; stream_launches_min
    env: dict = field(default_factory=dict)
    buffer_size: int = 262140
    extra_patterns: tuple = ()  # expressions beside exprs that the reference does not model (they match nowhere in the texts)


@functools.lru_cache(maxsize=None)
def _made(fn):
    return fn()


def text_bytes(t) -> bytes:
    return t if isinstance(t, bytes) else _made(t)


def cell_patterns(cell: Cell):
    n = len(cell.extra_patterns)
    return ([e.pattern for e in cell.exprs] + list(cell.extra_patterns), [e.flags for e in cell.exprs] + [fc.FLAG_SINGLE] * n,
            [e.id for e in cell.exprs] + [900000 + i for i in range(n)])


@functools.lru_cache(maxsize=256)
def _ref(exprs, data, buffer_size):
    return reference(data, exprs, buffer_size)


def cell_reference(cell: Cell, which: int):
    return _ref(tuple(cell.exprs), text_bytes(cell.texts[which][1]), cell.buffer_size)


def spread_of(n_in_mode: int) -> int:
    """list_spread of a mode with so many expressions (HgScanner::plan_pass, no boost)."""
    return min(DEFER_SHARDS, max(1, DEFER_SHARDS // max(1, n_in_mode)))


def cells():
    out = [
        Cell("direct-r40", R40, [("align", _alignments(R40)), ("noise", _plant_all(R40, 5, _random_words(6, 40000)))], ("table/direct", "kernel/lean"),
             claim={"table_first": 1, "shared_windows": 0, "windows_per_literal": 4, "kernel": "lean"}),
        Cell("direct-and-shared", R40 + STEMS30, [("align", _alignments(R40 + STEMS30)), ("noise", _plant_all(R40 + STEMS30, 7, _random_words(8, 40000)))],
             ("table/direct", "table/shared", "bucket/aligned-dword"), claim={"table_first": 1, "shared_windows": 5, "windows_per_literal": 4, "kernel": "lean"}),
        Cell("buckets-only", STEMS200, [("align", _alignments(STEMS200)), ("dense", _stems_with_noise)] + _stem_cuts(),
             ("table/none", "bucket/value-mismatch", "bucket/zero-pairs", "bucket/select-behind-text", "bucket/aligned-dword"),
             claim={"table_first": 0, "shared_windows": 23, "windows_per_literal": 4, "kernel": "lean", "value_mismatch_min": 24, "zero_pairs_min": 290,
                    "false_positives_min": {"dense": 320}, "candidates": {"cut-0": 1, "cut-1": 1, "cut-2": 1}}),
        Cell("byte-windows", BYTEWIN, [("align", _alignments(BYTEWIN)), ("noise", _random_words(11, 20000, b"abcxyz1q=7 "))] + _ends(BYTEWIN), ("bucket/byte-loads", "window/byte-aligned"),
             claim={"byte_windows": 1, "kernel": "lean"}),
        Cell("negative-address", NEGATIVE, [("align", _alignments(NEGATIVE))] + _text_starts(NEGATIVE[1:]), ("bucket/negative-address", "bucket/byte-loads", "window/byte-aligned"),
             claim={"byte_windows": 1, "kernel": "lean", "negative_at_min": 18}),
        Cell("casebits", CI2, [("align", _alignments(CI2, nocase=True)), ("variants", _case_and_lookalikes(CI2))] + _ends(CI2), ("compare/casebits", "compare/lookalikes"),
             claim={"fold_mask": 0, "kernel": "lean"}),
        Cell("folded", CI70, [("align", _alignments(CI70, nocase=True)), ("variants", _case_and_lookalikes(CI70))], ("compare/fold", "compare/lookalikes"),
             claim={"fold_mask": 0x20202020, "windows_per_literal": 4, "kernel": "lean"}),
        # folded windows in the discriminated buckets: the discriminator's text bytes are folded as the windows are
        Cell("folded-buckets", CI_STEMS, [("align", _alignments(CI_STEMS, nocase=True)), ("variants", _case_and_lookalikes(CI_STEMS))] + _ends(CI_STEMS[:2]),
             ("compare/fold", "table/none", "bucket/aligned-dword"), claim={"fold_mask": 0x20202020, "table_first": 0, "windows_per_literal": 4, "kernel": "lean"}),
        Cell("lengths", LENGTHS, [("align", _alignments(LENGTHS)), ("near", _near_misses)] + _ends(LENGTHS),
             ("compare/len-7..32", "compare/alignment-16", "compare/each-window", "compare/16-17", "compare/prefix", "compare/overlap", "compare/near-miss-each-byte", "compare/mask-tail",
              "end/literal-ends-text", "end/byte-compare-tail", "end/text-begins-inside-literal", "bucket/negative-delta", "bucket/select-before-text"),
             claim={"windows_per_literal": 4, "kernel": "lean"}),
        Cell("table-ways", R3000, [("all", _plant_all(R3000, 12)), ("noise", _random_words(13, 300000))] + _ends(R3000[:3]),
             ("table/way-1..4", "table/overflow-bucket", "filter/false-positives", "bucket/negative-delta"),
             claim={"table_first": 1, "ways": (0, 1, 2, 3), "probes_min": 1, "windows_per_literal": 4, "kernel": "lean", "false_positives_min": {"noise": 400},
                    "table_ends_min": 5}),
        # one stream workgroup, one candidate segment, one verify wave: the candidates of the text are the wave's
        Cell("flatten", BUCKETS, [("none", b"." * 3000 + b"\n"), ("one", _bucket_text({1: 1})), ("two", _bucket_text({2: 1})), ("63", _bucket_text({63: 1})), ("64", _bucket_text({64: 1})),
                                  ("65", _bucket_text({65: 1})), ("200", _bucket_text({200: 1})), ("5000", _bucket_text({200: 25})),
                                  ("mixed", _bucket_text({200: 9, 1: 7, 65: 5}, noise=b"bucket_of_zzz_ literal_of ")), ("lane63", _bucket_text({1: 64})), ("lane0", _bucket_text({2: 65}))],
             ("flatten/bucket-1-2-63-64-65-200", "flatten/pairs-0-1-63-64-65-4096", "flatten/lane-0-63", "stage/final-flush-only", "kernel/staged"),
             claim={"table_first": 0, "kernel": "staged", "buckets": BUCKET_SIZES, "modes": {1: len(BUCKETS)},
                    "candidates": {"none": 0, "one": 1, "two": 1, "63": 1, "64": 1, "65": 1, "200": 1, "5000": 25, "mixed": 21, "lane63": 64, "lane0": 65},
                    "verified": {"one": 1, "two": 2, "63": 63, "64": 64, "65": 65, "200": 200, "5000": 5000, "lane63": 64, "lane0": 130},
                    "final_flush_only": ("none", "one", "two", "63", "64", "65", "200", "lane63", "lane0")}),
        # zero-pair candidates between candidates with large buckets in ONE wave (at most 64 candidates in a text of one tile): the
        # owner search runs over equal exclusive prefixes
        Cell("flatten-zero-pairs", BUCKETS + STEMS1_200, [("mixed", _interleaved(ZERO_MIXED)), ("edges", _interleaved(ZERO_EDGES))], ("flatten/zero-pairs-interleaved",),
             claim={"table_first": 0, "kernel": "staged", "buckets": BUCKET_SIZES, "modes": {1: len(BUCKETS) + 200},
                    "candidates": {"mixed": len(ZERO_MIXED), "edges": len(ZERO_EDGES)},
                    "zero_pair_candidates": {"mixed": ZERO_MIXED.count("z"), "edges": ZERO_EDGES.count("z")}, "mismatch_candidates": {"mixed": 2, "edges": 0}}),
        Cell("stage-mid-flush", BUCKETS, [("one-pair", _bucket_text({1: 6000}))], ("stage/mid-loop-flush",), claim={"kernel": "staged", "verified_min": {"one-pair": 6000}}),
        Cell("stage-direct-filing", BUCKETS, [("dense", _dense_buckets)], ("stage/direct-filing",),
             claim={"kernel": "staged", "pairs_per_candidate": 4, "candidate_every": 64, "tiles_min": 16}),
        *[Cell(f"spread-mode{m}-{n}", spread_set(m, n), [("text", _spread_text(spread_set(m, n)))], (f"spread/mode{m}-{n}",), claim={"kernel": "staged", "modes": {m: n}, "list_spread": spread})
          for m in (1, 2) for n, spread in ((1, 64), (2, 32), (63, 1), (64, 1), (65, 1), (200, 1))],
        Cell("spread-mixed", MIXED, [("text", _spread_text(MIXED, 40))], ("spread/modes-0-1-2-3-huge",), claim={"kernel": "staged", "modes": {0: 1, 1: 1, 2: 1, 3: 1, 4: 1}},
             extra_patterns=(MIXED_HUGE,)),
        Cell("list-overflow", OVERFLOW, [("text", _overflow_text), ("text", _overflow_text)], ("list/overflow-rerun",),
             claim={"kernel": "staged", "modes": {1: 64}, "list_spread": 1, "reruns_min": 1, "second_reruns": 0}),
        Cell("joiner-segments", R40 + STEMS30, [("text", _joiner_text)], ("joiner/segments",),
             # (HG_JOINER=1: the engine decides about a joiner from the last pass's timing; the knob takes the decision, as in finalize_cells.py)
             env={"HG_JOINER_AHEAD": "1", "HG_JOINER": "1", "HG_CHUNK_TILES": "1024"},
             claim={"table_first": 1, "shared_windows": 5, "kernel": "lean", "joiner_launches_min": 1, "stream_launches_min": 3}),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


CELLS = cells()
# the classes the suite is written for; tests/test_verify_cells.py asserts that each is some cell's tag and proves the tags
REQUIRED_TAGS = (
    "table/direct", "table/shared", "table/none", "table/way-1..4", "table/overflow-bucket", "filter/false-positives",
    "bucket/aligned-dword", "bucket/byte-loads", "bucket/negative-delta", "bucket/negative-address", "bucket/select-before-text", "bucket/select-behind-text", "bucket/value-mismatch",
    "bucket/zero-pairs", "window/byte-aligned",
    "compare/len-7..32", "compare/alignment-16", "compare/each-window", "compare/16-17", "compare/prefix", "compare/overlap", "compare/near-miss-each-byte", "compare/mask-tail",
    "compare/casebits", "compare/fold", "compare/lookalikes", "end/literal-ends-text", "end/byte-compare-tail", "end/text-begins-inside-literal",
    "flatten/bucket-1-2-63-64-65-200", "flatten/pairs-0-1-63-64-65-4096", "flatten/lane-0-63", "flatten/zero-pairs-interleaved",
    "stage/final-flush-only", "stage/mid-loop-flush", "stage/direct-filing", "kernel/lean", "kernel/staged",
    *[f"spread/mode{m}-{n}" for m in (1, 2) for n in (1, 2, 63, 64, 65, 200)], "spread/modes-0-1-2-3-huge", "list/overflow-rerun", "joiner/segments",
)
