"""Extended parameters (hs_expr_ext_t) without a GPU: every rejection rule through the three compile entry points, byte-for-byte
identical databases for sets without parameters, the host replay of approximate expressions (hg_core.h routines through
tests/native/extsim.cpp) against tests/approx_ref.py, and the tiers the pigeonhole cover gives."""
from __future__ import annotations

import ctypes
import random

import pytest

import accept_rules
import approx_ref
import extsim_py
import regex_gen
import somsim_py
from extsim_py import ExprExt, ext
from hypergrep_amd import benchspec

SOM, SINGLE = 256, 8

# (expression, flags, ext, the rule's words in the message)
REJECTIONS = [
    ("foobar", 0, ext(flags=32), "unknown HS_EXT_FLAG"),
    ("foobar", 0, ext(edit=1, hamming=1), "cannot both be set"),
    ("foobar", 0, ext(min_offset=5, max_offset=4), "min_offset is larger than max_offset"),
    ("foobar", 0, ext(min_length=5, max_offset=4), "min_length is larger than max_offset"),
    ("0 & 1", 512, ext(edit=1), "HS_FLAG_COMBINATION"),
    ("a" * 40, 0, ext(edit=17), "above 16"),
    ("a" * 40, 0, ext(hamming=17), "above 16"),
    ("abc", 0, ext(edit=3), "minimum match width 3"),
    ("ab?", 0, ext(hamming=1), "minimum match width 1"),
    ("foo\\bbar", 0, ext(edit=1), "no assertion but a leading"),
    ("\\bfoobar", 0, ext(edit=1), "no assertion but a leading"),
    ("foobar\\B", 0, ext(edit=1), "no assertion but a leading"),
    ("foo$|bar", 0, ext(edit=1), "no assertion but a leading"),
    ("foo(?m:^)bar", 0, ext(edit=1), "no assertion but a leading"),
    ("foobar", 0, ext(min_length=7), "min_length 7 could remove reports"),
    ("foobar", 0, ext(edit=1, min_length=6), "min_length 6 could remove reports"),
    ("[a-z]{20000}", 0, ext(edit=16), "pattern too large"),
    ("(a|b|c|d|e){40}", SOM, ext(edit=3), "HS_FLAG_SOM_LEFTMOST needs an automaton"),
]


def _hg_compile_ext(pats, flags, exts):
    from hypergrep_amd import device

    try:
        device.Database(pats, flags=flags, ids=list(range(len(pats))), ext=exts)
    except device.CompileError as e:
        return str(e)
    return None


def _hs_compile_ext(pats, flags, exts):
    from hypergrep_amd import utils

    lib = ctypes.CDLL(utils._get_hyperscanner_lib()._name)  # pylint: disable=protected-access
    n = len(pats)
    db, err = ctypes.c_void_p(), ctypes.POINTER(ctypes.c_void_p)()

    class CompileError(ctypes.Structure):
        _fields_ = [("message", ctypes.c_char_p), ("expression", ctypes.c_int)]

    errp = ctypes.POINTER(CompileError)()
    ea = utils.ext_array(exts, n)
    rc = lib.hs_compile_ext_multi((ctypes.c_char_p * n)(*[p.encode() for p in pats]), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*range(n)), ea,
                                  n, 1, None, ctypes.byref(db), ctypes.byref(errp))
    if rc == 0:
        lib.hs_free_database(db)
        return None
    assert rc == -4  # HS_COMPILER_ERROR
    out = f"{errp.contents.expression}: {errp.contents.message.decode()}"
    lib.hs_free_compile_error(errp)
    return out


@pytest.mark.parametrize("expr,flags,x,words", REJECTIONS, ids=[r[3] + f"-{i}" for i, r in enumerate(REJECTIONS)])
def test_rejections_name_the_expression_and_the_rule(expr, flags, x, words):
    import hypergrep_amd

    pats = ["hello", "0" if flags & 512 else "world", expr]  # the bad expression is index 2
    fl = [0, 0, flags]
    exts = [None, ext(edit=1) if not flags & 512 else None, x]
    for compile_ in (_hg_compile_ext, _hs_compile_ext):
        msg = compile_(pats, fl, exts)
        assert msg is not None and msg.startswith("2: ") and words in msg, (compile_.__name__, msg)
    assert hypergrep_amd.check_compatibility(pats, flags=fl, ids=[0, 1, 2], ext=exts) == 4
    # the same expressions without parameters compile (where the rule is the parameters')
    if flags != 512 and "assertion" not in words and "too large" not in words:
        assert hypergrep_amd.check_compatibility(pats, flags=fl, ids=[0, 1, 2]) == 0


def test_parameters_that_cannot_remove_a_report_are_accepted():
    import hypergrep_amd

    pats = ["foobar", "foo[0-9]+bar", "foobar"]
    exts = [ext(min_length=6, min_offset=6), ext(edit=2, min_length=5), ext(hamming=2, min_length=6, min_offset=3)]
    assert hypergrep_amd.check_compatibility(pats, flags=[0, 0, 0], ext=exts) == 0
    assert hypergrep_amd.check_compatibility(pats, flags=[0, 0, 0], ext=[None, ExprExt(), None]) == 0


def test_offset_bounds_are_compiled():
    pats = ["ERR_DISK_FULL_[0-9]{3}", "abcde", "abcde", "foobar", "x[0-9]+"]
    exts = [ext(edit=1, min_offset=30), ext(min_offset=10, max_offset=40), ext(min_offset=5), ext(max_offset=2**40), None]
    flags = [SINGLE, SINGLE, SINGLE, 0, SINGLE]
    db = extsim_py.Db(pats, flags, exts=exts)
    assert db.h, db.error
    p = [db.pattern(i) for i in range(len(pats))]
    # a SINGLEMATCH expression with a min_offset emits every end (the report rules keep the smallest in bounds)
    none, rule = 0x7FFFFFFF, 0  # no upper bound
    assert (p[0]["single"], p[0]["lo"], p[0]["hi"]) == (0, 30, none | rule)
    assert (p[1]["single"], p[1]["lo"], p[1]["hi"], p[1]["mode"]) == (0, 10, 40 | rule, 3)
    assert (p[2]["single"], p[2]["lo"], p[2]["hi"]) == (1, 0, none)  # min_offset 5 <= the match length: removes nothing, dropped
    assert (p[3]["lo"], p[3]["hi"]) == (0, none)
    assert (p[4]["single"], p[4]["lo"], p[4]["hi"]) == (1, 0, none)
    # bounds that can remove nothing leave the database as it is without them
    plain = extsim_py.Db(["abcde", "foobar"], [SINGLE, 0], mode="plain").digest()
    assert extsim_py.Db(["abcde", "foobar"], [SINGLE, 0], exts=[ext(min_offset=5), ext(min_length=6, max_offset=0xFFFFFFFF)]).digest() == plain


def test_offset_bounds_host_replay():
    """Per piece: the expanded automaton's ends (every end: emission-time suppression is off) under the bounds and the report
    rules, against the reference."""
    rng = random.Random(15)
    for _ in range(300):
        case = _approx_case(rng)
        if case is None:
            continue
        pat, flags, k, edit, _db, _ref = case
        lo, hi = rng.randint(0, 12), rng.choice([None, rng.randint(4, 20)])
        x = ext(edit=k, min_offset=lo, max_offset=hi) if edit else ext(hamming=k, min_offset=lo, max_offset=hi)
        if hi is not None and lo > hi:
            continue
        db = extsim_py.Db([pat], [flags], exts=[x])
        assert db.h, db.error
        ref = approx_ref.Approx(pat, flags, edit=k if edit else 0, hamming=0 if edit else k, min_offset=lo, max_offset=hi)
        info = db.pattern(0)
        for _ in range(4):
            line = _line(rng)
            ends = [t for t, _ in db.nfa(0, line) if info["lo"] <= t <= info["hi"]]
            assert (ends[:1] if flags & SINGLE else ends) == ref.reports(line), (pat, flags, k, edit, lo, hi, line)


def _sets():
    rng = random.Random(5)
    yield "c1", benchspec.c1_spec()
    yield "c2", benchspec.c2_spec()
    yield "c3", benchspec.c3_spec()
    yield "c5", benchspec.c5_spec()
    for i in range(12):
        yield f"gen{i}", [regex_gen.random_pattern(rng) for _ in range(rng.randint(1, 24))]


@pytest.mark.parametrize("name,spec", list(_sets()), ids=[n for n, _ in _sets()])
def test_sets_without_parameters_compile_byte_identical(name, spec):
    pats = spec[0] if isinstance(spec, tuple) else spec
    pats = [p.decode() if isinstance(p, bytes) else p for p in pats]
    rng = random.Random(name)
    flags = [rng.choice([0, 2, 6, 8, 14, 1]) for _ in pats]
    plain = extsim_py.Db(pats, flags, mode="plain")
    if not plain.h:
        for mode, exts in (("null", None), ("ext", [None] * len(pats)), ("ext", [ExprExt() for _ in pats])):
            other = extsim_py.Db(pats, flags, exts=exts, mode=mode)
            assert not other.h and other.error == plain.error and other.bad == plain.bad
        return
    want = plain.digest()
    for mode, exts in (("null", None), ("ext", [None] * len(pats)), ("ext", [ExprExt() for _ in pats])):
        assert extsim_py.Db(pats, flags, exts=exts, mode=mode).digest() == want, mode


def _approx_case(rng):
    """A random approximate expression the compiler and the reference both take, or None."""
    pat = regex_gen.random_pattern(rng)
    if rng.random() < 0.15:
        pat = "\\A" + pat.lstrip("^") if rng.random() < 0.5 else pat.rstrip("$") + rng.choice(["\\z", "\\Z", "$"])
    k = rng.randint(1, 3)
    edit = rng.random() < 0.6
    flags = rng.choice([0, 1, 2, 4, 6, 8, 9, 14, 5])
    x = ext(edit=k) if edit else ext(hamming=k)
    db = extsim_py.Db([pat], [flags], exts=[x])
    if not db.h:
        # refused by the oracle too (as an exact expression), or by a documented rule of approximate matching / a capacity limit
        assert (not accept_rules.oracle_accepts([pat], [flags]) or "_distance " in db.error
                or "approximate matching supports no assertion" in db.error or accept_rules.explained_rejection(db.error)), (pat, flags, k, db.error)
        return None
    assert accept_rules.oracle_accepts([pat], [flags]), (pat, flags)
    try:
        ref = approx_ref.Approx(pat, flags, edit=k if edit else 0, hamming=0 if edit else k)
    except approx_ref.Unsupported:
        return None  # (assertions the automaton does not keep, e.g. inside a group that is stripped of its empty match)
    return pat, flags, k, edit, db, ref


def _line(rng):
    base = regex_gen.random_line(rng, 18)
    extra = rng.choice([b"", b"\n", b"\0z", b"\nab", b"\t\xff"])
    return base + extra


def test_host_replay_of_random_expressions_matches_the_reference():
    rng = random.Random(11)
    tested = 0
    for _ in range(500):
        case = _approx_case(rng)
        if case is None:
            continue
        pat, flags, k, edit, db, ref = case
        tested += 1
        for _ in range(6):
            line = _line(rng)
            want = ref.ends(line)
            if flags & SINGLE:
                want = want[:1]
            got = [t for t, _ in db.nfa(0, line)]
            assert got == want, (pat, flags, k, edit, line)
    assert tested > 120


def test_host_pipeline_replay_with_pieces_and_tiers():
    """The whole pipeline (stream filter, confirm windows, always-on, report rules) of sets that mix tiers, lines with '\\n'
    and NULs, split into pieces."""
    rng = random.Random(12)
    sets = [
        (["ERR_DISK_FULL_[0-9]{3}", "connection reset by peer", "[a-c]+x[0-9]"], [ext(edit=1), ext(edit=2), ext(hamming=1)]),
        (["user=[a-z]{4} status=5[0-9]{2}", "timeout", "^abc"], [ext(edit=1), ext(hamming=2), ext(edit=1)]),
        (["needle-in-hay", "other-literal-text", "foo[0-9]+bar$"], [None, ext(edit=3), ext(edit=1)]),
    ]
    frags = [b"ERR_DISK_FULL_123", b"ERR_DISC_FULL_12", b"ERRDISK_FULL_999", b"connection reste by peer", b"conection reset by per",
             b"abx1", b"ccx", b"user=abcd status=503", b"usr=abcd status=50x", b"timeo", b"tmeout", b"xabc", b"abc", b"needle-in-hay",
             b"other-litral-txt", b"foo12bar", b"fo12bar", b"\0", b"  ", b"zz"]
    for pats, exts in sets:
        for flags in ([0] * 3, [SINGLE] * 3, [1 | SINGLE, 2, 4]):
            db = extsim_py.Db(pats, flags, exts=exts)
            assert db.h, db.error
            refs = [approx_ref.Approx(p, f, edit=(x.edit_distance if x else 0), hamming=(x.hamming_distance if x else 0))
                    for p, f, x in zip(pats, flags, exts)]
            lines = [b" ".join(rng.choice(frags) for _ in range(rng.randint(0, 5))) for _ in range(80)]
            text = b"\n".join(lines) + b"\n"
            for bs in (262140, 17):
                want = []
                for idx, _a, piece in somsim_py.pieces(text, bs):
                    if piece:
                        want.extend((idx, rid, to) for rid, to in approx_ref.piece_reports(list(zip(refs, range(3))), piece))
                assert db.scan(text, buffer_size=bs) == sorted(want), (pats, flags, bs)


def test_start_of_match_is_the_smallest_start():
    rng = random.Random(13)
    for pat, x in (("abcdef", ext(edit=2)), ("^foo[0-9]+", ext(edit=1)), ("[a-c]+xyz", ext(hamming=1)), ("hello_world$", ext(edit=1))):
        db = extsim_py.Db([pat], [SOM], exts=[x])
        assert db.h, db.error
        ref = approx_ref.Approx(pat, SOM, edit=x.edit_distance, hamming=x.hamming_distance)
        for _ in range(40):
            line = bytes(rng.choice(b"abcdefxyz0123 _hellowrd") for _ in range(rng.randint(0, 16))) + rng.choice([b"", b"\n"])
            got = db.nfa(0, line)
            assert [t for t, _ in got] == ref.ends(line)
            assert [s for _, s in got] == [ref.start(line, t) for t, _ in got], (pat, line)


def test_tiers_of_approximate_expressions():
    from hypergrep_amd import device

    long_lit = device.Database(["ERR_DISK_FULL_[0-9]{3}"], flags=[0], ext=[ext(edit=1)]).info()
    assert long_lit["n_literal_anchored"] == 1 and long_lit["n_always_on"] == 0
    two = device.Database(["connection reset by peer"], flags=[0], ext=[ext(edit=2)]).info()
    assert two["n_literal_anchored"] == 1
    short = device.Database(["abcde"], flags=[0], ext=[ext(edit=1)]).info()  # pieces of 2 and 3 bytes: always-on
    assert short["n_always_on"] == 1 and short["n_literal_anchored"] == 0
    db = extsim_py.Db(["ERR_DISK_FULL_[0-9]{3}", "foobar", "[a-z]{3000}q"], [0, 0, 0], exts=[ext(edit=1), ext(hamming=2), ext(edit=1)])
    p0, p1, p2 = db.pattern(0), db.pattern(1), db.pattern(2)
    assert p0["tier"] == 0 and p0["lit_lead"] == 0xFFFFFFFF and p0["literal_only"] == 0 and p0["max_len"] == 17 + 1
    assert p1["tier"] == 1 and p1["max_len"] == 6
    assert p2["nw"] > 32  # huge tables


def test_reference_agrees_with_the_regex_module():
    regex = pytest.importorskip("regex")
    rng = random.Random(14)
    tested = 0
    for _ in range(300):
        pat = regex_gen.random_pattern(rng).lstrip("^").rstrip("$")
        k = rng.randint(1, 2)
        edit = rng.random() < 0.6
        try:
            ref = approx_ref.Approx(pat, 0, edit=k if edit else 0, hamming=0 if edit else k)
            rx = regex.compile(("(?:%s){e<=%d}" if edit else "(?:%s){s<=%d}") % (pat, k), regex.V0)
        except (approx_ref.Unsupported, regex.error):
            continue
        if approx_ref.Approx(pat, 0).ends(b"") or "\\b" in pat or "\\B" in pat:
            continue
        tested += 1
        for _ in range(3):
            line = regex_gen.random_line(rng, 10)
            s_line = line.decode()
            want = sorted({t for t in range(len(line) + 1) for s in range(t + 1) if rx.fullmatch(s_line, s, t)})
            assert ref.ends(line) == want, (pat, k, edit, line)
    assert tested > 60
