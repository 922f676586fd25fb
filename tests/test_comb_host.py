"""Logical combinations (HS_FLAG_COMBINATION, HS_FLAG_QUIET) on the host: the compiler's acceptance and rejection rules
through every compile entry point, and the scalar routines of the combination pass (hg_comb.h, replayed through
tests/native/combsim.cpp) against the independent reference tests/comb_ref.py.  No GPU needed."""
from __future__ import annotations

import ctypes
import itertools
import random

import pytest

import comb_ref
import combsim_py

COMB, QUIET, SINGLE, SOM = 512, 1024, 8, 256
BASE = [r"ERROR", r"disk", r"timeout", r"retry", r"[0-9]+x"]
BASE_IDS = [101, 102, 103, 104, 105]


def hg_compile(pats, flags, ids):
    """(rc, message) of hg_db_compile"""
    from hypergrep_amd import device

    n = len(pats)
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    rc = device.lib().hg_db_compile((ctypes.c_char_p * n)(*[p.encode() for p in pats]), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*ids), n,
                                    ctypes.byref(h), err, 512)
    if rc == 0:
        device.lib().hg_db_release(h)
    return rc, err.value.decode()


def hs_compile(pats, flags, ids):
    """(rc, message) of Face A's hs_compile_multi"""
    from hypergrep_amd import utils

    lib = ctypes.CDLL(utils._get_hyperscanner_lib()._name)  # pylint: disable=protected-access
    lib.hs_compile_multi.restype = ctypes.c_int
    n = len(pats)
    db, err = ctypes.c_void_p(), ctypes.c_void_p()
    rc = lib.hs_compile_multi((ctypes.c_char_p * n)(*[p.encode() for p in pats]), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*ids), n, 1, None,
                              ctypes.byref(db), ctypes.byref(err))
    msg = ""
    if rc == 0:
        lib.hs_free_database(db)
    else:
        msg = ctypes.cast(ctypes.cast(err, ctypes.POINTER(ctypes.c_void_p))[0], ctypes.c_char_p).value.decode()
        lib.hs_free_compile_error(err)
    return rc, msg


def check_all(pats, flags, ids):
    """rc of check_patterns (Face B), hg_db_compile, hs_compile_multi and the harness's message"""
    from hypergrep_amd import utils

    rc_b = utils.check_compatibility(pats, flags=flags, ids=ids)
    rc_c, msg_c = hg_compile(pats, flags, ids)
    rc_a, msg_a = hs_compile(pats, flags, ids)
    db = combsim_py.Db(pats, flags, ids)
    return rc_b, rc_c, rc_a, msg_c, msg_a, db


# ---- acceptance

@pytest.mark.parametrize("formula", ["101 & 102", "101&!102", "(101)&!(102)", "101 | 102 & 103", " ( ( 101 ) ) ", "101", "101 & !(102 | 103)",
                                     "101\t&\n102", "(101 | 102) & !103 & !104"])
@pytest.mark.parametrize("extra", [0, SINGLE, QUIET, SOM, SINGLE | SOM | 2 | 4 | 1])
def test_combinations_are_accepted(formula, extra):
    pats = BASE + [formula]
    flags = [6] * len(BASE) + [COMB | extra]
    ids = BASE_IDS + [7]
    rc_b, rc_c, rc_a, msg_c, msg_a, db = check_all(pats, flags, ids)
    assert (rc_b, rc_c, rc_a) == (0, 0, 0), (msg_c, msg_a)
    assert db.ok(), db.error
    info = db.info()
    assert info["ncomb"] == 1
    assert info["records"] == (0 if extra & QUIET else 1)  # a QUIET combination reports nothing: no record
    assert db.tier(len(BASE)) == 2


def test_quiet_expressions_are_accepted():
    flags = [6 | QUIET, 6 | QUIET, 6, 6, 6]
    rc_b, rc_c, rc_a, msg_c, msg_a, db = check_all(BASE, flags, BASE_IDS)
    assert (rc_b, rc_c, rc_a) == (0, 0, 0), (msg_c, msg_a)
    assert db.info()["nquiet"] == 2 and db.info()["ncomb"] == 0
    # QUIET on every expression that shares an id
    assert combsim_py.Db(["foo", "bar"], [QUIET, QUIET], [5, 5]).ok()


def test_flag_512_is_no_longer_unsupported():
    from hypergrep_amd import utils

    assert utils.check_compatibility(["foo", "bar", "1 & 2"], flags=[6, 6, COMB], ids=[1, 2, 3]) == 0
    assert utils.check_compatibility(["foo"], flags=[QUIET | 6]) == 0
    assert utils.check_compatibility(["foo"], flags=[2048]) == 4  # (still: bits outside the supported set)


REJECTIONS = [
    # (formula, comb id, fragment)
    ("   ", 7, "empty formula"),
    ("(101 & 102", 7, "unbalanced parentheses"),
    ("101 & 102)", 7, "unbalanced parentheses"),
    ("101 &", 7, "dangling operator"),
    ("& 101", 7, "dangling operator"),
    ("101 & | 102", 7, "dangling operator"),
    ("101 !102", 7, "missing operator"),
    ("101 102", 7, "two operands"),
    ("()", 7, "empty parentheses"),
    ("101 & abc", 7, "unexpected character"),
    ("101 & -102", 7, "unexpected character"),
    ("101 & 4294967296", 7, "UINT32_MAX"),
    ("101 & 999", 7, "999, which no expression in the set has"),
    ("101 & 7", 7, "its own report id 7"),
    ("101 & 102", 101, "is shared with another expression"),
    ("!101", 7, "true when none of its operands has matched"),
    ("101 | !102", 7, "true when none of its operands has matched"),
    ("!(101 & 102)", 7, "true when none of its operands has matched"),
    ("!101 & !102", 7, "true when none of its operands has matched"),
]


@pytest.mark.parametrize("formula,cid,fragment", REJECTIONS)
def test_rejections_name_the_rule(formula, cid, fragment):
    pats = BASE + [formula]
    flags = [6] * len(BASE) + [COMB]
    ids = BASE_IDS + [cid]
    rc_b, rc_c, rc_a, msg_c, msg_a, db = check_all(pats, flags, ids)
    assert (rc_b, rc_c, rc_a) == (4, -4, -4)
    assert fragment in msg_c and msg_c.startswith(f"{len(BASE)}:"), msg_c
    assert fragment in msg_a, msg_a
    assert not db.ok() and fragment in db.error


def test_nested_combinations_are_rejected():
    pats = BASE + ["101 & 102", "7 | 103"]
    flags = [6] * len(BASE) + [COMB, COMB]
    rc_b, rc_c, rc_a, msg_c, _, _ = check_all(pats, flags, BASE_IDS + [7, 8])
    assert (rc_b, rc_c, rc_a) == (4, -4, -4)
    assert "nested combinations are not supported" in msg_c and msg_c.startswith("6:")


def test_two_combinations_with_one_id_are_rejected():
    rc_b, rc_c, _, msg_c, _, _ = check_all(BASE + ["101 & 102", "103 & 104"], [6] * len(BASE) + [COMB, COMB], BASE_IDS + [7, 7])
    assert (rc_b, rc_c) == (4, -4) and "must be unique" in msg_c


def test_operand_limit_is_named():
    n = 65
    pats = [f"lit{i}x" for i in range(n)]
    ids = list(range(1, n + 1))
    ok = combsim_py.Db(pats + [" | ".join(str(i) for i in ids[:64])], [6] * n + [COMB], ids + [1000])
    assert ok.ok(), ok.error
    rc_b, rc_c, rc_a, msg_c, _, _ = check_all(pats + [" | ".join(str(i) for i in ids)], [6] * n + [COMB], ids + [1000])
    assert (rc_b, rc_c, rc_a) == (4, -4, -4)
    assert "64" in msg_c and "distinct operands" in msg_c
    # repeating an operand does not count twice
    assert combsim_py.Db(pats[:2] + ["1 & (1 | 2) & 1 & 1"], [6, 6, COMB], [1, 2, 9]).ok()


def test_deep_nesting_is_bounded():
    deep = "101 & (" * 80 + "102" + ")" * 80  # right-nested: every level keeps one more value on the stack
    rc_b, rc_c, _, msg_c, _, _ = check_all(BASE + [deep], [6] * len(BASE) + [COMB], BASE_IDS + [7])
    assert (rc_b, rc_c) == (4, -4) and "evaluation stack" in msg_c
    # long flat formulas are fine: the program keeps two values on the stack
    flat = " & ".join(["101"] * 5000)
    assert combsim_py.Db(BASE + [flat], [6] * len(BASE) + [COMB], BASE_IDS + [7]).ok()


def test_quiet_and_loud_share_no_id():
    rc_b, rc_c, rc_a, msg_c, _, _ = check_all(["foo", "bar"], [6 | QUIET, 6], [5, 5])
    assert (rc_b, rc_c, rc_a) == (4, -4, -4)
    assert "HS_FLAG_QUIET" in msg_c and msg_c.startswith("1:")


# ---- formulas: precedence, whitespace, evaluation

@pytest.mark.parametrize("formula", ["1&2|3", "1|2&3", "1&!2", "(1)&!(2)", "1 & ( 2|3 )", "!1&2|3&!4", "1|!2&3", "!!1&2", "(1|2)&(3|4)&!(1&4)",
                                     "1 & !(2 | !3)"])
def test_truth_tables_match_the_reference(formula):
    ids = [1, 2, 3, 4]
    tree = comb_ref.parse(formula)
    if comb_ref.evaluate(tree, set()):
        assert not combsim_py.Db(["a1", "b2", "c3", "d4", formula], [6] * 4 + [COMB], ids + [9]).ok()
        return
    db = combsim_py.Db(["a1", "b2", "c3", "d4", formula], [6] * 4 + [COMB], ids + [9])
    assert db.ok(), db.error
    slots, pattern = db.operands(0)
    assert pattern == 4
    for true_ids in itertools.chain.from_iterable(itertools.combinations(ids, k) for k in range(5)):
        status = sum(1 << s for s, x in enumerate(slots) if x in true_ids)
        assert db.eval(0, status) == comb_ref.evaluate(tree, set(true_ids)), (formula, true_ids)


def test_precedence_examples():
    t = set()
    ev = lambda f, on: comb_ref.evaluate(comb_ref.parse(f), set(on))  # noqa: E731
    assert ev("1&2|3", [3]) and not ev("1&2|3", [1])
    assert ev("1|2&3", [1]) and not ev("1|2&3", [2])
    assert ev("1 & ( 2|3 )", [1, 3]) and not ev("1 & ( 2|3 )", [2, 3])
    assert not ev("1&!2", t)


def make_piece(rng, ids, single_ids, pattern_of):
    """random reports of one piece after the report rules: [(id, to, pattern)] in (id, to) order"""
    reps = set()
    for _ in range(rng.randint(0, 12)):
        reps.add((rng.choice(ids), rng.randint(1, 30)))
    out = []
    for rid in sorted({r[0] for r in reps}):
        tos = sorted(to for x, to in reps if x == rid)
        if rid in single_ids:
            tos = tos[:1]
        out.extend((rid, to, pattern_of[rid]) for to in tos)
    return out


def test_same_offset_tie():
    pats = ["timeout", "retry", "101 & !102", "101 & 102"]
    db = combsim_py.Db(pats, [6, 6, COMB, COMB], [101, 102, 7, 8])
    assert db.ok(), db.error
    # both end at 10: `101 & !102` does not report, `101 & 102` does
    assert db.piece([(101, 10, 0), (102, 10, 1)]) == [(8, 10, 3), (101, 10, 0), (102, 10, 1)]
    # 101 first: `101 & !102` reports at 5 only
    assert db.piece([(101, 5, 0), (102, 10, 1)]) == [(7, 5, 2), (8, 10, 3), (101, 5, 0), (102, 10, 1)]


def random_formula(rng, ids, depth=0):
    r = rng.random()
    if depth > 3 or r < 0.35:
        return str(rng.choice(ids))
    if r < 0.5:
        return "!" + random_formula(rng, ids, depth + 1)
    op = rng.choice(["&", "|", " & ", " | "])
    f = random_formula(rng, ids, depth + 1) + op + random_formula(rng, ids, depth + 1)
    return f"({f})" if rng.random() < 0.5 else f


@pytest.mark.parametrize("seed", range(6))
def test_random_formulas_and_reports_against_the_reference(seed):
    rng = random.Random(seed)
    checked = 0
    for _ in range(60):
        nops = rng.randint(1, 6)
        ids = [10 + i for i in range(nops)]
        pats = [f"w{i}x" for i in range(nops)]
        flags = [6 | (SINGLE if rng.random() < 0.3 else 0) | (QUIET if rng.random() < 0.4 else 0) for _ in ids]
        combs = []
        while len(combs) < rng.randint(1, 4):
            f = random_formula(rng, ids)
            if not comb_ref.evaluate(comb_ref.parse(f), set()):
                combs.append(f)
        cflags = [COMB | (SINGLE if rng.random() < 0.4 else 0) | (QUIET if rng.random() < 0.15 else 0) for _ in combs]
        all_pats, all_flags, all_ids = pats + combs, flags + cflags, ids + [100 + k for k in range(len(combs))]
        db = combsim_py.Db(all_pats, all_flags, all_ids)
        assert db.ok(), (all_pats, db.error)
        ref = comb_ref.CombSet(all_pats, all_flags, all_ids)
        single_ids = {ids[i] for i in range(nops) if flags[i] & SINGLE}
        pattern_of = {rid: i for i, rid in enumerate(ids)}
        for _ in range(50):
            piece = make_piece(rng, ids, single_ids, pattern_of)
            got = db.piece(piece)
            want = ref.piece([(r[0], r[1]) for r in piece])
            assert [(g[0], g[1]) for g in got] == want, (all_pats, all_flags, piece, got, want)
            for rid, _, pattern in got:  # every record names the expression it belongs to
                assert all_ids[pattern] == rid
            checked += len(want)
    assert checked > 500


def test_hit_heavy_piece():
    # an operand with a report on every byte: every report evaluates its combinations with binary searches only
    pats = ["[a-z]", "zz", "(1 & !2)", "1 & 2"]
    db = combsim_py.Db(pats, [6 | QUIET, 6, COMB, COMB | SINGLE], [1, 2, 3, 4])
    assert db.ok(), db.error
    piece = [(1, to, 0) for to in range(1, 5001)] + [(2, 2500, 1)]
    got = db.piece(piece)
    want = comb_ref.CombSet(pats, [6 | QUIET, 6, COMB, COMB | SINGLE], [1, 2, 3, 4]).piece([(r[0], r[1]) for r in piece])
    assert [(g[0], g[1]) for g in got] == want
    assert sum(1 for g in got if g[0] == 3) == 2499 and [g[1] for g in got if g[0] == 4] == [2500]


# ---- databases

@pytest.mark.parametrize("base", [BASE, ["foo[0-9]+bar", r"\bword\b", "([a-f][0-9]){17}", "needle-in-hay", "x.{0,2000}y"], ["abc", "[0-9]+x"]])
def test_adding_combinations_leaves_the_other_expressions_unchanged(base):
    ids = list(range(1, len(base) + 1))
    alone = combsim_py.Db(base, [6] * len(base), ids)
    assert alone.ok(), alone.error
    combs = ["1 & 2", "1 & !2", "(1 | 2) & 1"]
    both = combsim_py.Db(base + combs, [6] * len(base) + [COMB, COMB | SINGLE, COMB | QUIET], ids + [50, 51, 52])
    assert both.ok(), both.error
    assert alone.digest(len(base)) == both.digest(len(base))
    assert both.info() == {"ncomb": 3, "nquiet": 0, "records": 2, "feed": 4}


def test_db_info_counts_combinations_as_neither_tier():
    from hypergrep_amd import device

    info = device.Database(BASE + ["101 & 102"], flags=[6] * len(BASE) + [COMB], ids=BASE_IDS + [7]).info()
    plain = device.Database(BASE, flags=[6] * len(BASE), ids=BASE_IDS).info()
    assert info["n_patterns"] == plain["n_patterns"] + 1
    assert (info["n_literal_anchored"], info["n_always_on"], info["table_bytes"]) == (plain["n_literal_anchored"], plain["n_always_on"], plain["table_bytes"])
