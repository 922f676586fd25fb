"""CPU checks of the stream-pass cell table (stream_cells.py): each cell's literal set selects its instantiation, the numpy
reference equals the oracle, and the host replay of the device logic (hgsim_py) equals the reference on every cell's text."""
from __future__ import annotations

import random
import re

import numpy as np
import pytest

import hgsim_py
import oracle_py
import stream_cells as sc


def _db(cell):
    lits, caseless = sc.literal_set(cell)
    db = hgsim_py.Db(sc.patterns_of(lits), flags=sc.flags_of(caseless), ids=list(range(len(lits))))
    assert db.ok(), db.error
    return db, lits, caseless


@pytest.mark.parametrize("cell", sc.CELLS, ids=lambda c: c.name)
def test_cell_selects_its_instantiation(cell):
    db, lits, _ = _db(cell)
    check, info = db.selfcheck(), db.info()
    assert check["violations"] == 0
    got = (check["filter_log2"], bool(check["wide"]), check["byte_windows"], info["fold_mask"] != 0, check["window_bytes"])
    assert got == (cell.log2, cell.wide, cell.dense, cell.fold, cell.window_bytes)
    assert info["nslow"] == 0 and info["npatterns"] == len(lits)  # every literal in the stream pass's tier


def test_table_covers_every_variant_once():
    names = [c.name for c in sc.CELLS]
    assert len(names) == len(set(names))
    stream_keys = [c.instantiation for c in sc.STREAM_CELLS]
    assert len(set(stream_keys)) == 23 and len(set(c.instantiation for c in sc.JOIN_CELLS)) == 12
    # the runtime variants share an instantiation with another cell but take another path through it
    assert any(c.window_bytes == 3 for c in sc.STREAM_CELLS)
    assert any(c.caseless and not c.fold and not c.dense for c in sc.STREAM_CELLS)
    assert any(c.fold and c.dense for c in sc.STREAM_CELLS)
    # every fold cell carries the literal of spaces (zeros past the end of the text fold onto it)
    for c in sc.CELLS:
        assert (sc.SPACES.encode() in sc.literal_set(c)[0]) == c.fold, c.name


def test_residues_meet_every_mode():
    met = {}
    for c in sc.STREAM_CELLS:
        for mode in c.modes:
            met.setdefault(mode, set()).update(sc.residues(c))
    assert set(met) == {"dword", "dense1", "dense2", "wide", "fold"}
    for mode, res in met.items():
        assert res == set(sc.RESIDUES), (mode, sorted(set(sc.RESIDUES) - res))


def test_launcher_switches_name_every_cell():
    """hg_launch_stream / hg_launch_stream_join dispatch exactly the table's (filter, mode) pairs: a case deleted from a switch
    (its kernel may still be instantiated by hg_stream_blocks_per_cu) fails here."""
    src = open(sc.STREAM_SOURCE, encoding="utf-8").read()
    layout = ("hg_stream.hip's launchers are read as laid out now: `bool hg_launch_stream(const HgStreamArgs` with the wide "
              "switch, then `if (a.dense == 1)`, `if (a.dense == 2)` (each switch followed by `return true;` and `  }`), then "
              "the dword switch; `bool hg_launch_stream_join(const HgStreamArgs` with `case L * 4 + D: launch_join<L, D>`; "
              "each function ends at a `}` in column 0.  A reformat of them needs this test changed with it")

    def split(text, sep):
        assert sep in text, f"{sep!r} not found. {layout}"
        return text.split(sep, 1)

    def body(sig):
        rest = split(src, sig)[1]
        return split(rest, "\n}\n")[0]

    stream = body("bool hg_launch_stream(const HgStreamArgs")
    wide_part, rest = split(stream, "if (a.dense == 1)")
    dense1, rest = split(rest, "if (a.dense == 2)")
    dense2, dword = split(rest, "return true;\n  }")
    got = set()
    for part, wide, dense in ((wide_part, "true", 0), (dense1, "false", 1), (dense2, "false", 2), (dword, "false", 0)):
        for case, l2, w, b in re.findall(r"case (\d+): launch_one<(\d+), (\w+), (\d)>", part):
            assert case == l2 and w == wide and int(b) == dense, (case, l2, w, b)
            got.add((int(l2), w == "true", dense))
    assert got == {(c.log2, c.wide, c.dense) for c in sc.STREAM_CELLS}
    join = body("bool hg_launch_stream_join(const HgStreamArgs")
    got = set()
    for l2a, da, l2, b in re.findall(r"case (\d+) \* 4 \+ (\d): launch_join<(\d+), (\d)>", join):
        assert (l2a, da) == (l2, b)
        got.add((int(l2), int(b)))
    assert got == {(c.log2, c.dense) for c in sc.JOIN_CELLS}


# ------------------------------------------------------------------ the reference against the oracle
def _oracle(text, lits, caseless, ids):
    rc, hits, nlines = oracle_py.scan_buffer(text, sc.patterns_of(lits), flags=sc.flags_of(caseless), ids=ids)
    assert rc == 0
    return sc.sort_hits(np.array(hits, dtype=np.uint64)), nlines


def _small_cases():
    cases = [
        ("overlaps", b"aaaa\nabababab\n\naaaaaaaaaaaaaaaaaaa\nabaaba", [b"aa", b"aaa", b"abab", b"aba", b"ba"], [False] * 5),
        ("caseless", b"FooBAR foobar FOOBAR\nfOObArfoobar\nbar\n", [b"foobar", b"bar", b"OBA"], [True, False, True]),
        ("caseless_shared_prefix", b"ABCDEFGHIJ abcdefghij AbCdEfGhIjK\n", [b"abcdefghij", b"abcdefghijk", b"ABCDEFGH"], [True, False, True]),
        ("fold_lookalikes", b"q@z[w\\x] q`z{w|x} Q`Z{W|X}\nk^m@p[r\\ K~M`P{R|\n^~@`[{\\|]}\n", [l.encode() for l in sc.LOOKALIKE_LITS] + [b"^~", b"[{"], [True] * 3 + [True, False]),
        ("spaces", b"        x         \n \n" + b" " * 40, [sc.SPACES.encode(), b"  x  "], [True, False]),
        ("empty_lines", b"\n\n\nabc\n\n\nabc\n\n", [b"abc", b"bc"], [False, False]),
        ("no_final_newline", b"first abc\nlast line abc", [b"abc"], [False]),
        ("single_line_no_newline", b"abcabcabc", [b"abc", b"cab"], [False, True]),
        ("empty_text", b"", [b"abc"], [False]),
        ("only_newlines", b"\n" * 100, [b"abc"], [False]),
        ("long_literals", b"xx" + b"0123456789abcdefghij" * 3 + b"\n0123456789abcdefghiJ\n", [b"0123456789abcdefghij", b"0123456789abcdefghij0", b"9abcdefghij"], [False, False, True]),
        ("duplicate_prefixes", b"abcdefgh1 abcdefgh2 abcdefgh3\n", [b"abcdefgh1", b"abcdefgh2", b"abcdefgh"], [False] * 3),
    ]
    # cell texts cut to at most 64 KiB (the literal sets of the smaller cells: the oracle compiles them fast)
    for name in ("dword11", "dword12", "dword11_fold", "dense1_11", "dense2_11", "dense1_12_w3", "dword_expand", "dense2_12_fold"):
        cell = sc.BY_NAME[name]
        lits, caseless = sc.literal_set(cell)
        text = sc.cell_text(cell, lits, caseless, 1 << 20, seed=3)
        rng = random.Random(name)
        at = rng.choice([0, 16 * sc.TILE, 24 * sc.TILE])  # the queue / geometry, alignment or near-miss sections
        cases.append(("cell_" + name, sc.truncated(text[at:], lits, 60000 + rng.randrange(4096), rng), lits, caseless))
    return cases


SMALL = _small_cases()


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c[0])
def test_reference_equals_oracle(case):
    _, text, lits, caseless = case
    assert len(text) <= 64 * 1024
    ids = list(range(len(lits)))
    want, nlines = _oracle(text, lits, caseless, ids)
    got = sc.reference_hits(text, lits, caseless, ids)
    assert got.tolist() == want.tolist()
    assert sc.line_table(text)[1] == nlines


def test_reference_small_cases_are_many_and_not_empty():
    assert len(SMALL) >= 20
    assert sum(len(sc.reference_hits(t, l, c, list(range(len(l))))) > 0 for _, t, l, c in SMALL) >= 18


# ------------------------------------------------------------------ the host replay against the reference
@pytest.mark.parametrize("cell", sc.STREAM_CELLS, ids=lambda c: c.name)
def test_hostsim_equals_reference(cell):
    db, lits, caseless = _db(cell)
    text = sc.cell_text(cell, lits, caseless, 1 << 20, seed=1)
    assert len(text) <= 1 << 20
    want = sc.reference_hits(text, lits, caseless, list(range(len(lits))))
    hits, _ = db.scan(text)
    got = sc.sort_hits(np.array(hits, dtype=np.uint64))
    assert got.tolist() == want.tolist()
    assert len(want) >= 10000
