"""Start of match (HS_FLAG_SOM_LEFTMOST) on the host: the compiler's acceptance rules and the reverse walk of hg_som.h
(replayed through tests/native/somsim.cpp) against a Python `re` brute force.  No GPU needed."""
from __future__ import annotations

import random

import pytest

import accept_rules
import regex_gen
import somsim_py
from somsim_py import SOM, start_by_brute_force

DOTALL, MULTILINE, CASELESS, SINGLE = 2, 4, 1, 8


def check_text(pats, flags, data, buffer_size=1 << 20, ids=None, want_reports=True):
    """Every report of every piece gets the brute-force start of its expression(s); the reports themselves equal those of
    the same set without the flag.  Returns the number of reports checked."""
    ids = ids or list(range(len(pats)))
    db = somsim_py.Db(pats, flags, ids)
    assert db.ok(), db.error
    plain = somsim_py.Db(pats, [f & ~SOM for f in flags], ids)
    assert plain.ok(), plain.error
    checked = 0
    for _, _, line in somsim_py.pieces(data, buffer_size):
        got = db.piece(line)
        assert [(r[0], r[1]) for r in got] == [(r[0], r[1]) for r in plain.piece(line)], (pats, line)
        for rid, to, frm, _ in got:
            members = [i for i, p in enumerate(pats) if ids[i] == rid]
            if not flags[members[0]] & SOM:
                assert frm == 0
                continue
            starts = [start_by_brute_force(pats[i], flags[i], line, to) for i in members]
            want = min(s for s in starts if s is not None)
            assert frm == want, (pats, flags, line, rid, to, frm, want)
            checked += 1
    if want_reports:
        assert checked, (pats, data)
    return checked


# ---- acceptance rules

@pytest.mark.parametrize("extra", [0, 1, 2, 4, 7])
def test_som_flag_is_accepted(extra):
    db = somsim_py.Db(["foo[0-9]+bar"], [SOM | extra])
    assert db.ok(), db.error
    assert db.info()["nsom"] == 1


def test_som_with_singlematch_is_rejected():
    db = somsim_py.Db(["foobar"], [SOM | SINGLE])
    assert not db.ok()
    assert "SINGLEMATCH" in db.error and db.error.startswith("0:")


def test_shared_id_with_mixed_som_is_rejected():
    assert not somsim_py.Db(["foo", "bar"], [SOM, 0], [5, 5]).ok()
    assert not somsim_py.Db(["foo", "bar"], [0, SOM | 4], [5, 5]).ok()
    db = somsim_py.Db(["foo", "bar", "baz"], [SOM, SOM, 0], [5, 5, 6])
    assert db.ok(), db.error


def test_som_on_huge_automaton_is_rejected_with_the_limit():
    assert somsim_py.Db(["foo.{0,3000}bar"], [6]).ok()  # without the flag it compiles (sparse tables)
    db = somsim_py.Db(["foo.{0,3000}bar"], [SOM | 6])
    assert not db.ok()
    assert "1024" in db.error and "HG_MAX_NODES" in db.error, db.error


def test_databases_without_som_are_unchanged():
    pats = ["foo[0-9]+bar", r"\bx+y", "literal"]
    a = somsim_py.Db(pats, [6, 6, 6]).info()
    b = somsim_py.Db(pats, [6 | SOM, 6, 6]).info()
    assert a["nsom"] == 0 and b["nsom"] == 1
    assert b["pool_words"] > a["pool_words"]  # the transposed follow table, only for the SOM expression


# ---- random expressions against Python `re`

def _compile_one_som(pat, flags):
    db = somsim_py.Db([pat], [flags | SOM])
    return db.ok(), db.error


@pytest.mark.parametrize("seed", range(20))
def test_starts_against_python_re(seed):
    total = 0
    for pat, flags, data, _ in regex_gen.end_offset_cases(seed, accepts=accept_rules.Tally().accepts(_compile_one_som, features=True)):
        total += check_text([pat], [flags | SOM], data, want_reports=False)
    assert total > 0


# ---- fixed cases: assertions at both ends, overlapping starts, pieces

@pytest.mark.parametrize("pat,flags,data", [
    (r"\bfoo", 6, b"foo xfoo foofoo _foo -foo\n"),
    (r"\Bbar\b", 6, b"bar xbar xbarx bar_ zbar.\n"),
    (r"^ab+", 6, b"abbb ab\nabab\n ab\n"),
    (r"a+$", 6 | MULTILINE, b"baaa\naa a\nxa"),
    (r"a+$", 2, b"baaa\naa a\nxa"),
    ("hello", 6 | CASELESS, b"HeLLo hello hELLO\n"),
    (".*x", 6, b"abcxdefx\nnox here x\n"),
    ("a|aaa", 6, b"aaaa baaab\n"),
    ("(ab|b)c", 6, b"abc bc xabcabc\n"),
    (r"x\d{2,5}y", 6, b"x12y x123456y xx99yy\n"),
    (r"\b\w+@\w+\.com\b", 6, b"mail a@b.com and bob@site.com.\n"),
    ("[a-c]+", 6, b"zzabcabc cab\n"),
])
def test_fixed_cases(pat, flags, data):
    check_text([pat], [flags | SOM], data)


def test_leading_nuls_and_split_pieces():
    data = b"\0\0foo123bar\nxx\0foo1bar\n" + b"zfoo12bar" * 20 + b"\n\0\0\0foo9bar foo8bar\n"
    for bs in (7, 12, 16, 33, 1 << 20):
        check_text(["foo[0-9]+bar", r"\bfoo\d"], [6 | SOM, 6 | SOM], data, buffer_size=bs, want_reports=bs > 12)


def test_shared_id_takes_the_smallest_start():
    # two SOM expressions on one id end at the same offsets: the single report carries the smaller start
    pats = ["cd", "abcd", "bc"]
    check_text(pats, [6 | SOM, 6 | SOM, 6 | SOM], b"abcd xcd abcdabcd\n", ids=[1, 1, 1])
    db = somsim_py.Db(pats, [6 | SOM] * 3, [1, 1, 1])
    assert [(r[1], r[2]) for r in db.piece(b"abcd\n")] == [(3, 1), (4, 0)]


def test_mixed_som_and_plain_ids():
    pats = ["foo[0-9]+", "bar", "x+y"]
    check_text(pats, [6 | SOM, 6, 6 | SOM], b"foo123 bar xxy barfoo9\n", ids=[3, 4, 5])
    db = somsim_py.Db(pats, [6 | SOM, 6, 6 | SOM], [3, 4, 5])
    for rid, _, frm, _ in db.piece(b"bar bar\n"):
        assert rid == 4 and frm == 0


def test_literal_only_needs_no_walk():
    # a literal-only expression (fast tier) alone on its id: from = to - len
    db = somsim_py.Db(["needle-in-hay"], [6 | SOM])
    info = db.info()
    assert info["tier0"] == 0 and info["literal_only0"] == 1
    line = b"xx needle-in-hay needle-in-hayneedle-in-hay\n"
    got = db.piece(line)
    assert [(r[1], r[2]) for r in got] == [(16, 3), (30, 17), (43, 30)]
    check_text(["needle-in-hay"], [6 | SOM], line)


def test_random_multi_expression_sets():
    rng = random.Random(11)
    tally = accept_rules.Tally()
    for _ in range(30):
        pats, flags = [], []
        while len(pats) < 4:
            p = regex_gen.random_pattern(rng)
            f = rng.choice([6, 7, 2, 4]) | SOM
            one = somsim_py.Db([p], [f])
            if tally.decide([p], [f], one.ok(), one.error, features=True):
                pats.append(p)
                flags.append(f)
        ids = [rng.randrange(3) for _ in pats]
        data = regex_gen.random_text(rng, 10, maxlen=16)
        check_text(pats, flags, data, ids=ids, want_reports=False)
