"""The cells of the value table stages (hg_count_values, hg_rank_values and the value store: hg_values.hip, hg_values_dev.h,
hg_rank.hip, hg_valstore.hip), shared by the host test (test_value_cells.py) and the GPU test (test_value_cells_gpu.py).
Nothing here calls the product or needs a GPU.

A cell is a dict:
  name       "<group>/<what>"
  pset       a key of PSETS
  text       the bytes of a one-buffer cell          (kind "text")
  files      the files of a many-file cell           (kind "files")
  buffers    the buffers of a store cell, in order   (kind "store")
  settings   the hash_bits / table_log2 keywords to run it with; "tight" stands for the smallest legal table, 2^k > n_parts
  by_pattern the values of by_pattern to run it with
  seg        also run as ONE file through rank_values(per_segment=True): the SEG instantiations of the three shared bodies
  claims     what the cell is FOR, each proved by the host test from the replay's read-outs (valuesim.cpp, Trace) or from the
             parts alone, so that a cell that stopped reaching its target is noticed.  A claim is (what, keywords of the
             replay it holds under, argument):
    ("path", kw, (wave, path, leader))   wave `wave` of the insert pass took path 1 (one add by the leader) or 2 (lane by lane),
                                         its first counted lane `leader`
    ("first_in_wave", kw, (value, wave)) the smallest part index of `value` lies in wave `wave`
    ("n_long", kw, n)                    n parts are a wave's
    ("long_iterations", kw, n)           the busiest wave of the long kernel's grid runs n iterations
    ("wrapped", kw, (tier, n))           at least n parts of the tier (1 lane, 2 wave) probed past the last slot
    ("homes", kw, {value: home})         the values' home slots
    ("last_slot", kw, (last, slot0))     the last slot and slot 0 occupied (1) or empty (0); None: not claimed
    ("n_values", kw, n)                  n occupied slots
    ("free_slots", kw, n)                n slots stay empty
    ("slots", kw, n)                     the table has n slots
    ("chain_tags", kw, None)             some part passed an occupied slot with its own tag (another value) and one with another tag
    ("no_tag", kw, None)                 every tag is 0
    ("passes", kw, (value, other))       the first part of `value` probed the slot `other` lies in before its own
    ("shared_chain", kw, None)           some part passed an occupied slot of another value (the bytes, the length or the key decide)
    ("sort_bits", kw, (bits, first))     the sort's key width, the least that holds `first`, the largest first of the cell
    ("two_expressions", None, None)      equal bytes under two expression indices
    ("alignments", None, pairs)          long values that are equal stand at these (earlier, later) start alignments
Expected results come from values_ref, rank_ref and valstore_ref only (a dict, a sort, a slice)."""
from __future__ import annotations

import re

A = 14  # DOTALL | MULTILINE | SINGLEMATCH
LANE_MAX = 256
PSETS = {
    "X": (["x[a-w]*"], [A]),
    "KV": (["[a-z]+=[0-9]+", "ERR[0-9]+"], [A, A]),
    # equal bytes at different spans of a line can only come from different expressions: in `xab xab\n` the first from `^...`
    "PAIR": (["^x[a-w]*", "x[a-w]*$"], [A, A]),
}
_RE = {"X": re.compile(rb"(x[a-w]*)"), "KV": re.compile(rb"([a-z]+=[0-9]+)|(ERR[0-9]+)")}
STD = ({}, {"hash_bits": 1}, {"table_log2": "tight"})
CHAIN = ({}, {"hash_bits": 1, "table_log2": "tight"})
BOTH = (False, True)


def letters(i: int) -> bytes:
    """i in base 23 as letters a .. w, least digit last, at least one digit."""
    out = bytearray()
    while True:
        out.insert(0, 97 + i % 23)
        i //= 23
        if not i:
            return bytes(out)


def cand(i: int, length: int = 0) -> bytes:
    """Candidate value i: `x` and the letters of i; with a length, filled up to it with a fixed run of letters behind a `w`."""
    v = b"x" + letters(i)
    if length:
        v += b"w"
        v += bytes(97 + (k * 5 + 3) % 22 for k in range(length - len(v)))
        assert len(v) == length
    return v


def long_value(n: int, salt: int = 0) -> bytes:
    return b"x" + bytes(97 + (n * 7 + k + salt) % 23 for k in range(n - 1))


def lines_of(values, sep=b"\n") -> bytes:
    return b"".join(v + sep for v in values)


def aligned(rows) -> bytes:
    """rows of (alignment, value): every value on a line of its own, behind as many dots as put its first byte at that offset mod 4."""
    out = b""
    for al, v in rows:
        out += b"." * ((al - len(out)) % 4) + v + b"\n"
    return out


# ---------------------------------------------------------------- parts by Python's re (no product call)
def re_parts(pset: str, text: bytes):
    """(records, parts) of a text scanned in whole lines: records (line, start, len, 0) of the lines with a part, parts
    (line, from, to, pattern, 0).  X and KV by re.finditer over the line; PAIR by parts_ref's definition."""
    records, parts = [], []
    at = 0
    for no, line in enumerate(text.splitlines(keepends=True)):
        if pset in _RE:
            spans = [(m.start(), m.end(), 0 if m.group(1) is not None else 1) for m in _RE[pset].finditer(line)]
        else:
            import parts_ref

            spans = parts_ref.piece_parts(PSETS[pset][0], PSETS[pset][1], line)
        if spans:
            records.append((no, at, len(line), 0))
        parts += [(no, f, t, p, 0) for f, t, p in spans]
        at += len(line)
    return records, parts


def re_files(pset: str, files):
    """(text, records, parts, seg_start) of the files packed one behind the other; lines and starts are the file's own."""
    text, records, parts, seg_start = b"", [], [], []
    for seg, data in enumerate(files):
        seg_start.append(len(text))
        recs, rows = re_parts(pset, data)
        records += [(r[0], r[1], r[2], seg) for r in recs]
        parts += [(p[0], p[1], p[2], p[3], seg) for p in rows]
        text += data
    return text, records, parts, seg_start


def tight(n_parts: int) -> int:
    return max(1, n_parts.bit_length())


def resolve(kw: dict, n_parts: int) -> dict:
    """The cell's keywords with "tight" made a number."""
    return {k: (tight(n_parts) if v == "tight" else v) for k, v in kw.items()}


# ---------------------------------------------------------------- aimed values: found by search(), recorded here
# The indices i of cand(i) (cand(i, 257) for the long ones) by home slot in a table of 2^10 under the full hash; the tag bits 40
# and 41 for CHAIN_TAGS.  test_value_cells.py::test_recorded_values_are_what_the_search_finds runs the searches again.
HOME_LAST = (1159, 3149, 3476)    # home 1023
HOME_BEFORE_LAST = (426, 1073)    # home 1022
HOME_LAST_LONG = 1733             # cand(i, 257) with home 1023
HOME_ZERO = (3924,)               # home 0
HOME_LAST_4TH = 4035              # a fourth with home 1023
HOME_LAST_LONGS = (1733, 1845, 2502, 2867)  # cand(i, 257) with home 1023
HOME_2047 = (1159, 3476, 4035)    # home 2047 in a table of 2^11: they share a chain there whenever they are stored
CHAIN_TAGS = (0, 723, 2156, 605)  # one home; bits (40, 41) of the first two equal, the third differs in bit 40, the fourth in bit 41


def search(want, length: int = 0, limit: int = 200000):
    """The first candidates, counted upwards, for which want(hash) is true; want returns a key or None, and the search ends when
    every key of want.keys has as many candidates as it asks for.  Deterministic and bounded."""
    import valuesim_py

    found = {k: [] for k in want.keys}
    for i in range(limit):
        v = cand(i, length)
        k = want(valuesim_py.hash_of(v, 0, len(v), which=0))
        if k in found and len(found[k]) < want.keys[k]:
            found[k].append(i)
            if all(len(found[k]) == n for k, n in want.keys.items()):
                return found
    raise AssertionError("the search ran out")


def home_search(homes: dict, length: int = 0):
    def want(h):
        return h & 1023

    want.keys = homes
    return search(want, length)


def chain_tag_search():
    """Four values of one home (mod 2^10): tags (bits 40, 41) t, t, t ^ 1, t ^ 2.  The first candidate fixes home and t."""
    import valuesim_py

    hashes = [valuesim_py.hash_of(cand(i), 0, len(cand(i)), which=0) for i in range(6000)]
    for i0, h0 in enumerate(hashes):
        same = [i for i, h in enumerate(hashes) if i > i0 and h & 1023 == h0 & 1023]
        tag = lambda h: (h >> 40) & 3  # noqa: E731
        picks = [next((i for i in same if tag(hashes[i]) == tag(h0) ^ d), None) for d in (0, 1, 2)]
        if None not in picks:
            return (i0,) + tuple(picks)
    raise AssertionError("the search ran out")


# ---------------------------------------------------------------- the cells
def cell(name, pset, text=None, files=None, buffers=None, settings=STD, by_pattern=BOTH, seg=True, claims=(), **more):
    c = {"name": name, "pset": pset, "settings": tuple(settings), "by_pattern": tuple(by_pattern), "seg": seg and text is not None, "claims": tuple(claims)}
    if text is not None:
        c["text"] = text
    if files is not None:
        c["files"] = files
    if buffers is not None:
        c["buffers"] = buffers
    c.update(more)
    return c


LONG = [long_value(257, s) for s in range(64)]  # 257 bytes each, all different


def _group_a():
    out = []
    for leader in (1, 31, 32, 63):  # wave 0: 64 x xb; wave 1: `leader` long values, then xa to the wave's end
        vals = [b"xb"] * 64 + LONG[:leader] + [b"xa"] * (64 - leader)
        out.append(cell(f"A/leader {leader}", "X", lines_of(vals), claims=[("path", {}, (0, 1, 0)), ("path", {}, (1, 1, leader)), ("first_in_wave", {}, (b"xa", 1)), ("n_long", {}, leader)]))
    for tail, leader in ((1, 0), (33, 31), (63, 1)):  # the uniform wave is the last, partial one
        vals = [b"xb"] * 64 + LONG[:leader] + [b"xa"] * (tail - leader)
        out.append(cell(f"A/tail {tail}, leader {leader}", "X", lines_of(vals), claims=[("path", {}, (1, 1, leader)), ("first_in_wave", {}, (b"xa", 1))]))
    for odd in (0, 32, 63):  # wave 1 has one other value, which first occurs there, as xa does
        vals = [b"xb"] * 64 + [b"xc" if k == odd else b"xa" for k in range(64)] + [b"xa"] * 64
        out.append(cell(f"A/odd lane {odd}", "X", lines_of(vals), claims=[("path", {}, (1, 2, 0)), ("path", {}, (2, 1, 0)), ("first_in_wave", {}, (b"xc", 1)), ("first_in_wave", {}, (b"xa", 1))]))
    # chosen winner: xa first occurs in lane 5 of a mixed wave of workgroup 0, its full waves lie in workgroup 1; and the reverse:
    # xd has a full wave in workgroup 0 and single lanes in workgroup 1
    vals = [b"xb"] * 64 + [b"xa" if k == 5 else b"xc" for k in range(64)] + [b"xd"] * 64 + [b"xb"] * 64 + [b"xa"] * 128 + [b"xd" if k % 7 == 0 else b"xe" for k in range(64)] + [b"xa"] * 40
    out.append(cell("A/winner across workgroups", "X", lines_of(vals),
                    claims=[("path", {}, (1, 2, 0)), ("path", {}, (2, 1, 0)), ("path", {}, (4, 1, 0)), ("path", {}, (5, 1, 0)), ("path", {}, (6, 2, 0)), ("path", {}, (7, 1, 0)),
                            ("first_in_wave", {}, (b"xa", 1)), ("first_in_wave", {}, (b"xd", 2))]))
    # one value in 5 waves, of which waves 1 and 3 are uniform
    vals = [b"xa" if k % 3 else b"xf" for k in range(64)] + [b"xa"] * 64 + [b"xg"] * 10 + [b"xa"] * 54 + LONG[:7] + [b"xa"] * 57 + [b"xa", b"xh"] * 20
    out.append(cell("A/five waves, two uniform", "X", lines_of(vals),
                    claims=[("path", {}, (0, 2, 0)), ("path", {}, (1, 1, 0)), ("path", {}, (2, 2, 0)), ("path", {}, (3, 1, 7)), ("path", {}, (4, 2, 0)), ("first_in_wave", {}, (b"xa", 0))]))
    for n in (255, 256, 257, 513):  # the value changes exactly where a workgroup ends
        vals = ([b"xa"] * 256 + [b"xb"] * 256 + [b"xa"])[:n]
        out.append(cell(f"A/workgroup edge {n}", "X", lines_of(vals), claims=[("path", {}, (3, 1, 0))] + ([("path", {}, (4, 1, 0)), ("first_in_wave", {}, (b"xb", 4))] if n > 256 else [])))
    return out


GRID_LENGTHS = (257, 258, 259, 260, 511, 512, 513, 767, 768, 1023, 1024, 1025, 1279)
GRID_PAIRS = [(a, b) for a in range(4) for b in range(4) if a != b] + [(a, a) for a in range(4)]  # 12 of unlike alignment first


def kv_long(n: int, eq: int) -> bytearray:
    """A value of [a-z]+=[0-9]+ of n bytes with its `=` at eq: any byte but that one can change within its class."""
    return bytearray(bytes(97 + (k * 3) % 26 for k in range(eq)) + b"=" + bytes(48 + (k * 7) % 10 for k in range(n - eq - 1)))


def diff_positions(n: int):
    whole = n // 256 * 256
    return sorted({0, 253, 255, 256, whole - 1, whole} | set(range(n - n % 4, n)))


def _group_b():
    out = []
    rows, pairs = [], []
    for k, (a, b) in enumerate(GRID_PAIRS):  # 13 lengths, the first three once more for the like alignments
        n = GRID_LENGTHS[k % len(GRID_LENGTHS)]
        rows += [(a, long_value(n, k // len(GRID_LENGTHS))), (b, long_value(n, k // len(GRID_LENGTHS)))]  # (the second round: other values of these lengths)
        pairs.append((a, b))
    text = aligned(rows)
    assert sorted(set(pairs)) == [(a, b) for a in range(4) for b in range(4)]
    out.append(cell("B/length grid", "X", text, settings=STD + ({"hash_bits": 1, "table_log2": "tight"},),
                    claims=[("alignments", None, tuple(pairs)), ("n_long", {}, 2 * len(GRID_PAIRS)), ("n_values", {}, len(GRID_PAIRS))]))
    for n, eq in ((1027, 600), (770, 500)):
        base = kv_long(n, eq)
        rows = [(1, bytes(base))]
        for k, pos in enumerate(diff_positions(n)):
            v = bytearray(base)
            v[pos] = (v[pos] - 97 + 1) % 26 + 97 if pos < eq else (v[pos] - 48 + 1) % 10 + 48
            rows.append((k % 4, bytes(v)))
        rows.append((2, bytes(base)))
        out.append(cell(f"B/one byte differs, {n} bytes", "KV", aligned(rows), settings=STD + ({"hash_bits": 1, "table_log2": "tight"},),
                        claims=[("n_values", {}, len(rows) - 1), ("n_long", {}, len(rows)), ("shared_chain", {"hash_bits": 1, "table_log2": "tight"}, None)]))
    short = long_value(256)
    longer, longest = short + b"abc" * 15, short + b"abc" * 115
    for name, order in (("short first", (short, longer, longest)), ("long first", (longest, longer, short))):
        rows = [(k + 1, v) for k, v in enumerate(order)] + [(3 - k, v) for k, v in enumerate(order)]
        out.append(cell(f"B/prefixes, {name}", "X", aligned(rows), settings=STD + ({"hash_bits": 1, "table_log2": "tight"},), claims=[("n_values", {}, 3), ("n_long", {}, 4)]))
    many = long_value(300)
    others = [many[:-1] + b"a", many[:150] + b"a" + many[151:], b"xa" + many[2:]]
    assert len(set(others + [many])) == 4 and all(len(o) == 300 for o in others)
    vals = [many] * 50 + others[:1] + [many] * 70 + others[1:2] + [many] * 80 + others[2:]
    out.append(cell("B/races, 200 equal long values", "X", aligned([(k % 4, v) for k, v in enumerate(vals)]), settings=STD + ({"hash_bits": 1, "table_log2": "tight"},),
                    claims=[("n_values", {}, 4), ("n_long", {}, 203), ("shared_chain", {"hash_bits": 1, "table_log2": "tight"}, None)]))
    vals = [cand(i % 2100, 260) for i in range(4200)]  # 2100 values, each twice, 2100 parts apart
    out.append(cell("B/stride, 4200 long parts", "X", lines_of(vals), settings=({}, {"hash_bits": 1}),
                    claims=[("n_long", {}, 4200), ("long_iterations", {}, 2), ("n_values", {}, 2100)]))
    for cut in (1, 2, 3):  # the long value ends the text, which has 4k + cut bytes
        v = long_value(258 + cut)
        text = b"xab\n" + v + b"\n.." + v
        text = b"." * ((12 + cut - len(text)) % 16) + text  # 16k + 12 + cut bytes: the dword that holds its last byte is the last before the guard
        assert len(text) % 4 == cut and (len(text) + 3) // 4 * 4 % 16 == 0
        out.append(cell(f"B/long value ends a text of 4k + {cut}", "X", text, claims=[("n_long", {}, 2), ("n_values", {}, 2)]))
    return out


def _group_c():
    out = []
    last, before = [cand(i) for i in HOME_LAST], [cand(i) for i in HOME_BEFORE_LAST]
    vals = before + last
    homes = {v: 1022 for v in before}
    homes.update({v: 1023 for v in last})
    out.append(cell("C/wrap, five values at the table's end", "X", lines_of(vals + vals[::-1]), settings=({},), seg=False,
                    claims=[("homes", {}, homes), ("wrapped", {}, (1, 3)), ("last_slot", {}, (1, 1)), ("n_values", {}, 5), ("slots", {}, 1024)]))
    lv = cand(HOME_LAST_LONG, 257)
    vals = before + last[:2] + [lv]
    homes = {v: 1022 for v in before}
    homes.update({v: 1023 for v in last[:2] + [lv]})
    out.append(cell("C/wrap, a long value among them", "X", lines_of(vals + vals[::-1]), settings=({},), seg=False,
                    claims=[("homes", {}, homes), ("wrapped", {}, (2, 1)), ("last_slot", {}, (1, 1)), ("n_values", {}, 5), ("slots", {}, 1024)]))
    fill = [cand(i) for i in range(20)]
    out.append(cell("C/last slot occupied, slot 0 empty", "X", lines_of(fill + last[:1] + fill[:3]), settings=({},), seg=False,
                    claims=[("homes", {}, {last[0]: 1023}), ("last_slot", {}, (1, 0)), ("n_values", {}, 21)]))
    out.append(cell("C/last slot empty", "X", lines_of(fill + [cand(HOME_ZERO[0])] + fill[:3]), settings=({},), seg=False,
                    claims=[("homes", {}, {cand(HOME_ZERO[0]): 0}), ("last_slot", {}, (0, 1)), ("n_values", {}, 21)]))
    out.append(cell("C/only the last slot occupied", "X", lines_of(last[:1] * 3), settings=({},), seg=False, claims=[("homes", {}, {last[0]: 1023}), ("last_slot", {}, (1, 0)), ("n_values", {}, 1)]))
    for k in (6, 8, 10):  # one free slot
        n = (1 << k) - 1
        sets = [{"table_log2": "tight"}] + ([{"hash_bits": 1, "table_log2": "tight"}] if k < 10 else [])
        out.append(cell(f"C/one free slot of 2^{k}", "X", lines_of(cand(i) for i in range(n)), settings=sets, seg=k < 10,
                        claims=[("free_slots", kw, 1) for kw in sets] + [("slots", sets[0], 1 << k), ("shared_chain", sets[0], None)]))
    for k in range(1, 9):  # tables below and of a workgroup's size
        n = (1 << k) - 1
        distinct = max(1, 1 << (k - 1))
        out.append(cell(f"C/table of 2^{k}", "X", lines_of(cand(i % distinct) for i in range(n)), settings=({"table_log2": k}, {"table_log2": k, "hash_bits": 1}),
                        claims=[("slots", {"table_log2": k}, 1 << k), ("n_values", {"table_log2": k}, min(n, distinct))]))
    chain = [cand(i) for i in CHAIN_TAGS]
    others = [v for v in (cand(i) for i in range(100, 160)) if v not in chain][:36]
    vals = [(chain[:1] + others[:12] + chain[2:3] + others[12:24] + chain[1:2] + chain[3:] + others[24:])[k % 40] for k in range(300)]
    widths = (40, 41, 42, 44, 63, 64, 32, 33)
    out.append(cell("C/tag widths", "X", lines_of(vals), settings=[{"hash_bits": b} for b in widths], seg=False,
                    claims=[("chain_tags", {"hash_bits": 41}, None), ("chain_tags", {"hash_bits": 42}, None), ("no_tag", {"hash_bits": 40}, None), ("no_tag", {"hash_bits": 32}, None),
                            ("n_values", {"hash_bits": 41}, 40), ("slots", {"hash_bits": 41}, 1024)]))
    return out


def _group_d():
    out = []
    for a, b in ((b"xab", b"xabc"), (b"xabc", b"xab"), (b"xabc", b"xabd"), (b"xabd", b"xabc")):
        # (xabcd has xabc's home under one hash bit and xab and xabd the next slot: behind it the three share a probe chain)
        out.append(cell(f"D/{a.decode()} before {b.decode()}", "X", b"xabcd\n" + a + b" " + b + b"\n" + b + b"\n.." + a + b" " + a + b"\n", settings=STD + CHAIN[1:],
                        claims=[("n_values", {}, 3), ("shared_chain", {"hash_bits": 1}, None), ("passes", {"hash_bits": 1}, (b, a))]))
    # equal bytes under two expressions: `^x..` takes the part at a line's start, `x..$` the one at its end
    text = b"xab xab\nxcd .. xab\n.. xcd\nxab\n.. xab\n"
    out.append(cell("D/two expressions, short values", "PAIR", text, settings=STD + CHAIN[1:], claims=[("two_expressions", None, None), ("n_values", {}, 2)]))
    v = long_value(300)
    text = v + b" " + v + b"\nxcd . " + v + b"\n. xcd\n" + v + b"\n.. " + v + b"\n"
    out.append(cell("D/two expressions, long values", "PAIR", text, settings=STD + CHAIN[1:], claims=[("two_expressions", None, None), ("n_values", {}, 2), ("n_long", {}, 5)]))
    return out


def _group_e():
    out = []
    for k in (6, 8, 10):  # n_parts 2^k + 1: the last part is a new value, first 2^k
        n = (1 << k) + 1
        out.append(cell(f"E/sort width, {n} parts", "X", lines_of([b"xa"] * (n - 1) + [b"xb"]), claims=[("sort_bits", {}, (k + 1, 1 << k)), ("n_values", {}, 2)]))
    return out


# many-file cells (rank_values, every mode): files, the cuts to try and what the cell is for
def _group_f():
    out = []
    # counts: xe 3, xa 2, xb 2, xc 2, xd 1; the tie at the cuts 2 and 3 goes to the smaller first, and xa, which sorts first by
    # its bytes, occurs last of the three
    tie = b"xc xb\nxe xe xa\nxd xc xb\nxa xe\n"
    out.append(cell("F/cuts and ties", "X", files=[tie], tops=(0, 1, 2, 3, 4, 5, 6, 1 << 40), note="seg_distinct 5: top 4, 5, 6 are below, at and above it"))
    out.append(cell("F/cuts and ties, three files", "X", files=[b"xq xq xr\n", tie, b"xa\n"], tops=(0, 1, 2, 3, 4, 5, 6, 1 << 40)))
    out.append(cell("F/empty files", "X", files=[b"", b"none\n", b"xa xb xa\n", b"", b"\n", b"xb\nxc xb\n", b"nothing\n", b"xa\n", b""], tops=(0, 1, 2)))
    for n_seg in (1, 2, 255, 256, 257):
        files = [lines_of([cand(s % 7), cand(s % 5 + 2)][:1 + s % 2]) + (b"xa xa\n" if s % 3 == 0 else b"") for s in range(n_seg)]
        out.append(cell(f"F/{n_seg} files", "X", files=files, tops=(0, 1)))
    for k in (6, 8):  # two values make up all parts, counts 2^k and 2^k - 1; the rarer one occurs first
        n = 1 << k
        body = lines_of([b"xr"] + [b"xf", b"xr"] * (n - 2) + [b"xf", b"xf"])
        assert body.count(b"xf") == n and body.count(b"xr") == n - 1
        out.append(cell(f"F/count width 2^{k}", "X", files=[body], tops=(0, 1)))
        out.append(cell(f"F/count width 2^{k}, the middle file of three", "X", files=[b"xf\n", body, b"xr xr\n"], tops=(0, 1)))
    out.append(cell("F/the same value in three files", "X", files=[b"xab\n", b". xab xab\n", b"xq xab\n"], tops=(0, 1)))
    out.append(cell("F/crossed key words", "PAIR", files=[b". xab\n", b"xab .\n"], tops=(0,), claims=[("two_expressions", None, None)]))
    v = long_value(300)
    out.append(cell("F/crossed key words, long values", "PAIR", files=[b". " + v + b"\n", v + b" .\n"], tops=(0,), claims=[("two_expressions", None, None)]))
    return out


# store cells: buffers accumulated in order, and the rankings to compare behind the calls
def _group_g():
    out = []
    stored = [b"k=%d" % i for i in range(0, 64, 2)]
    mixed = [b"k=%d" % i for i in range(64)]  # found, new, found, new, ...
    out.append(cell("G/found and new alternate", "KV", buffers=[lines_of(stored), lines_of(mixed), lines_of(mixed[::-1])]))
    longs = [cand(i, 300) for i in range(64)]
    out.append(cell("G/found and new alternate, long values", "X", buffers=[lines_of(longs[::2]), aligned([(k % 4, v) for k, v in enumerate(longs)]), lines_of(longs[::-1], b" ")]))
    out.append(cell("G/one free slot in a fixed table", "X", buffers=[lines_of(cand(i) for i in range(40)), lines_of(cand(i) for i in range(20, 63)), lines_of(cand(i) for i in range(63))],
                    store_log2=6, refused=lines_of([cand(5), cand(63)])))
    vals = [cand(i, 260) for i in range(4200)]
    out.append(cell("G/long-kernel stride", "X", buffers=[lines_of(vals), lines_of(vals)], tops=((0, True),), n_added=(4200, 0)))
    for total in (15, 16, 17, 0):  # the new bytes of the second call
        new = [b"xbcde", b"xfghi", b"x" + letters(7) * (total - 11)] if total else []
        assert sum(len(v) for v in new) == total
        out.append(cell(f"G/arena packing, {total} new bytes", "X", buffers=[b"xa xq\n", lines_of([b"xa"] + new), lines_of(new + [b"xq", b"xww"])]))
    for n in (258, 259, 513):  # the long value at every text alignment against every arena alignment
        for pad in (b"x", b"xa", b"xab", b"xabc"):
            v = long_value(n)
            out.append(cell(f"G/alignments, {n} bytes behind {len(pad)}", "X", buffers=[pad + b"\n" + v + b"\n"] + [b"." * al + v + b" " + pad + b"\n" for al in range(4)]))
    # ranking: counts 2^k and 2^k - 1 summed over three calls, a tie at the cut (xt before xs, which sorts first), order_first
    k = 6
    bufs = [lines_of([b"xr"] * 20 + [b"xf"] * 30 + [b"xt", b"xs"]), lines_of([b"xf"] * 14 + [b"xr"] * 23 + [b"xs", b"xt"]), lines_of([b"xr"] * 20 + [b"xf"] * 20 + [b"xu"])]
    tops = ((0, False), (1, False), (2, False), (3, False), (4, False), (5, False), (6, False), (0, True), (3, True))
    out.append(cell("G/ranking", "X", buffers=bufs, tops=tops, counts={b"xf": 1 << k, b"xr": (1 << k) - 1}))
    # ... and the two alone: 2^(k + 1) - 1 parts, so the larger count needs every bit of the count sort's key
    bufs = [lines_of([b"xr"] * 20 + [b"xf"] * 30), lines_of([b"xf"] * 14 + [b"xr"] * 23), lines_of([b"xr"] * 20 + [b"xf"] * 20)]
    out.append(cell("G/count width", "X", buffers=bufs, tops=((0, False), (1, False), (0, True)), counts={b"xf": 1 << k, b"xr": (1 << k) - 1}, sort_bits=k + 1))
    out.append(cell("G/growth over three calls", "X", buffers=[lines_of(cand(i) for i in range(600)), lines_of(cand(i) for i in range(300, 1500)), lines_of(cand(i) for i in range(0, 1500, 3))]))
    out.append(cell("G/reset behind a large store", "X", buffers=[lines_of(cand(i) for i in range(3000))], then_reset=[b"xa xb\nxa\n"]))
    return out


def _aimed_store():
    """Store cells whose claims the host test proves from valstoresim's read-outs:
      ("store_chain", call, (found, new))  in call `call` the group of `found` is found and that of `new` is not, both behind a
                                           probe that went past the table's last slot
      ("rehash", None, None)               the calls grow the table 2^10, 2^11, 2^12; at either growth some stored values keep their
                                           home and some move up by the old size; HOME_2047's values have one home in 2^11 slots;
                                           the last call finds every value"""
    out = []
    fill = [cand(i) for i in range(20)]
    for name, chain in (("short", [cand(i) for i in HOME_LAST + (HOME_LAST_4TH,)]), ("long", [cand(i, 257) for i in HOME_LAST_LONGS])):
        out.append(cell(f"G/aimed chain, {name} values", "X", buffers=[lines_of(chain[:3] + fill), lines_of(fill[:2] + chain[2:] + fill[5:7]), lines_of(chain)],
                        claims=[("store_chain", 1, (chain[2], chain[3]))]))
    fillers = [cand(i) for i in range(100000, 101497)]
    late = [cand(i) for i in HOME_2047]
    everything = fillers + late
    out.append(cell("G/rehash, 2^10 to 2^12", "X", buffers=[lines_of(fillers[:400]), lines_of(fillers[400:600] + late + fillers[600:897]), lines_of(fillers[897:]), lines_of(everything[::-1])],
                    tops=((0, False), (0, True), (5, False)), claims=[("rehash", None, None)]))
    return out


def _one_hash_bit_store():
    """Store cells under hash_bits 1: every tag is 0 and the stored values lie in one run of slots from slot 0 or 1, so a lookup
    that does not find its value passes every stored value (but one at slot 0, if its home is 1) and only the length, the
    expression and the bytes tell them apart.
      ("pattern_decides", 1, value)   by (expression, bytes), call 1 looks `value` up under expression 1, does not find it, and
                                      passes the slot of the same bytes stored under expression 0"""
    out = []
    v = long_value(300)
    for name, value in (("short", b"xab"), ("long", v)):
        out.append(cell(f"G/one hash bit, two expressions, {name} values", "PAIR", buffers=[b"xa .\nxq .\nxabe .\n" + value + b" .\n", b". " + value + b"\n" + value + b" .\n. xq\n"], hash_bits=1,
                        claims=[("two_expressions", None, None), ("pattern_decides", 1, value)]))
    for n, eq in ((1027, 600), (770, 500)):  # B's values that differ in one byte: the base alone, then its neighbours, then all again
        base = kv_long(n, eq)
        rows = []
        for k, pos in enumerate(diff_positions(n)):
            w = bytearray(base)
            w[pos] = (w[pos] - 97 + 1) % 26 + 97 if pos < eq else (w[pos] - 48 + 1) % 10 + 48
            rows.append((k % 4, bytes(w)))
        out.append(cell(f"G/one hash bit, one byte differs, {n} bytes", "KV", buffers=[aligned([(1, bytes(base))]), aligned(rows), aligned([(3, bytes(base))] + [((a + 1) % 4, w) for a, w in rows])],
                        hash_bits=1, n_added=(1, len(rows), 0)))
    return out


def _two_expression_buffers():
    v = long_value(300)
    # buffer 1 has the value under expression 0 only; in buffer 2 its first part is expression 1's
    return [cell("G/two expressions, short values", "PAIR", buffers=[b"xab .\n. xq\n", b". xab\nxab .\nxq\n"], claims=[("two_expressions", None, None)]),
            cell("G/two expressions, long values", "PAIR", buffers=[v + b" .\n. xq\n", b". " + v + b"\n" + v + b" .\n"], claims=[("two_expressions", None, None)])]


# E, stale buffers: one scanner, these calls one after the other, each behind a scan of its text
STALE = (("count", lines_of(b"k=%d" % i for i in range(5000)), {}),
         ("count", b"a=1 b=2\nc=3 a=1\n", {}),
         ("count", b"nothing\nhere\n", {}),
         ("count", lines_of([b"k=%d" % (i % 35), b"ERR%d" % (i % 35)][i % 2] for i in range(140)), {"by_pattern": True}),
         ("rank", lines_of(b"k=%d" % (i * i % 50) for i in range(300)), {"top": 7}),
         ("count", lines_of(b"k=%d" % (i % 9) for i in range(20)), {}))

GROUPS = {"A": _group_a(), "B": _group_b(), "C": _group_c(), "D": _group_d(), "E": _group_e(), "F": _group_f(), "G": _group_g() + _aimed_store() + _two_expression_buffers() + _one_hash_bit_store()}
TEXT_GROUPS = ("A", "B", "C", "D", "E")
for _g, _cells in GROUPS.items():
    assert len({c["name"] for c in _cells}) == len(_cells) and all(c["name"].startswith(_g + "/") for c in _cells)
