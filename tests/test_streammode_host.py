"""Stream mode on the host (no GPU): the compile rules of HS_MODE_STREAM through hs_compile_ext_multi, block-mode databases
unchanged, and a replay of the flow routines (tests/native/flowsim.cpp: hg_flow_scan_slice / hg_flow_unhold /
hg_flow_finish driven as hg_flow_scan_kernel drives them) over random splits against hg_nfa_scan on the concatenation and
against Python `re`."""
from __future__ import annotations

import bisect
import hashlib
import json
import os
import random

import pytest

import accept_rules
import extsim_py
import flowsim_py
import regex_gen
from hypergrep_amd import device

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSERTION_CHARS = ("^", "$", "\\b", "\\B", "\\A", "\\z", "\\Z")


# ---- compile rules (rule 7) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, word", [(256, "SOM_LEFTMOST"), (512 | 8, "COMBINATION"), (1024, "QUIET")])
def test_stream_mode_rejects_flags(flags, word):
    h, err = device.hs_compile(["abc", "1"] if flags & 512 else ["xyz", "abc"], flags=[0, flags], ids=[1, 2], mode=device.HS_MODE_STREAM)
    assert h is None and err[1] == 1 and "expression 1" in err[0] and word in err[0] and "stream mode" in err[0]
    # ... and block mode still takes them
    h, err = device.hs_compile(["abc", "1"] if flags & 512 else ["xyz", "abc"], flags=[0, flags], ids=[1, 2], mode=device.HS_MODE_BLOCK)
    assert err is None


def test_stream_mode_rejects_huge_automata():
    h, err = device.hs_compile(["abc", "foo.{0,3000}bar"], flags=[0, 0], mode=device.HS_MODE_STREAM)
    assert h is None and err[1] == 1 and "too large for stream mode" in err[0]
    # after ext expansion too
    h, err = device.hs_compile(["abc", "[a-z]{300}x"], flags=[0, 0], ext=[None, extsim_py.ext(edit=4)], mode=device.HS_MODE_STREAM)
    assert h is None and err[1] == 1 and "too large for stream mode" in err[0]
    assert device.hs_compile(["abc", "foo.{0,3000}bar"], flags=[0, 0], mode=device.HS_MODE_BLOCK)[1] is None


def test_stream_mode_accepts_what_block_mode_accepts():
    pats = ["foobar", r"\bab+c\b", "^x.*y$", "(?:ab|cd){12}e", r"baz\Z", "a[a-z]{40}b", "hello"]
    flags = [8, 0, 4, 1 | 2, 0, 0, 8]
    ext = [None, None, None, extsim_py.ext(edit=1), extsim_py.ext(min_offset=2, max_offset=90), extsim_py.ext(hamming=2), extsim_py.ext(min_offset=5)]
    h, err = device.hs_compile(pats, flags=flags, ids=list(range(len(pats))), ext=ext, mode=device.HS_MODE_STREAM)
    assert err is None and h


@pytest.mark.parametrize("mode", [0, 3, 4, 6, 1 | (1 << 24), 2 | (1 << 24), 2 | (1 << 25), 2 | (1 << 26), 8])
def test_bad_modes_rejected(mode):
    h, err = device.hs_compile(["abc"], flags=[0], mode=mode)
    assert h is None and err is not None


def test_block_mode_databases_unchanged():
    table = json.load(open(os.path.join(REPO, "tests", "golden", "block_db_digests.json"), encoding="utf-8"))
    for name, case in table.items():
        exts = None
        if "ext" in case:
            exts = [extsim_py.ext(**e) for e in case["ext"]]
        db = extsim_py.Db(case["patterns"], case["flags"], ids=case["ids"], exts=exts, mode="ext" if exts else "plain")
        assert db.h, (name, db.error)
        assert hashlib.sha256(db.digest()).hexdigest() == case["sha256"], name


# ---- flow replay --------------------------------------------------------------------------------------------------------
def _write_of(cuts, n, byte):
    """Index of the write holding stream byte `byte` (len(cuts) + 1: past the data, i.e. the close)."""
    if byte < 0:
        return 0
    if byte >= n:
        return len(cuts) + 1
    return bisect.bisect_right(cuts, byte)


def _check(db, pats, data, cuts, piece=4096, lanes=8):
    got = db.run(data, cuts, piece=piece, lanes=lanes)
    want = db.block(data)
    single = [db_single for db_single in getattr(db, "single", [False] * db.n)]
    for e in range(db.n):
        g = sorted(t for _, x, t in got if x == e)
        w = sorted(t for x, t in want if x == e)
        if single[e]:
            assert (g[:1] == w[:1]), (pats[e], data, cuts, g, w)
        else:
            assert g == w, (pats[e], data, cuts, g, w)
    # latency (rule 3) and order (rule 2) per expression
    n = len(data)
    for call, e, t in got:
        assert call >= _write_of(cuts, n, t - 1) or t == 0, ("delivered before its data", pats[e], data, cuts, call, t)
        assert call <= _write_of(cuts, n, t + 1), ("late", pats[e], data, cuts, call, t)
        if not any(a in pats[e] for a in ASSERTION_CHARS):
            assert not db.hold(e)
            assert call <= _write_of(cuts, n, t - 1), ("context-free report late", pats[e], data, cuts, call, t)
    for e in range(db.n):
        last = -1
        for call in range(len(cuts) + 2):
            ts = sorted(t for c, x, t in got if x == e and c == call)
            if ts:
                assert ts[0] >= last - 1, (pats[e], data, cuts, call, ts, last)
                last = max(last, ts[-1])


def _random_cuts(rng, n):
    k = rng.randint(0, min(n, 8))
    cuts = sorted(rng.randint(0, n) for _ in range(k))
    if rng.random() < 0.3:
        cuts += [c for c in cuts if rng.random() < 0.5]  # empty writes
        cuts.sort()
    return cuts


def test_flow_replay_matches_block_scan_random():
    rng = random.Random(2024)
    tally = accept_rules.Tally()
    done = 0
    for _ in range(600):
        pats = [regex_gen.random_pattern(rng) for _ in range(3)]
        flags = [rng.choice([0, 2, 4, 6, 1, 5]) for _ in pats]
        db = flowsim_py.Db(pats, flags)
        if not tally.decide(pats, flags, bool(db.h), db.error, features=True):
            continue  # both compilers refuse the set, or a documented limit / rule of the feature does (asserted)
        text = regex_gen.random_text(rng, rng.randint(1, 6), maxlen=12, final_newline=rng.random() < 0.5)
        for _ in range(4):
            _check(db, pats, text, _random_cuts(rng, len(text)), piece=rng.choice([1, 3, 7, 4096]), lanes=rng.choice([1, 2, 5, 32]))
        # every cut position once, 1-byte writes
        _check(db, pats, text, list(range(1, len(text))), piece=4096, lanes=4)
        done += 1
    assert done >= 300, tally.report()


def test_flow_replay_matches_python_re_small():
    rng = random.Random(99)
    tally = accept_rules.Tally()
    done = 0
    for _ in range(300):
        pat = regex_gen.random_pattern(rng)
        flags = rng.choice([0, 2, 4, 6])
        db = flowsim_py.Db([pat], [flags])
        if not tally.decide([pat], [flags], bool(db.h), db.error, features=True):
            continue  # both compilers refuse the set, or a documented limit / rule of the feature does (asserted)
        text = regex_gen.random_text(rng, rng.randint(1, 3), maxlen=8, final_newline=rng.random() < 0.5)
        want = regex_gen.ends_by_brute_force(pat, flags, text)
        got = sorted(t for _, _, t in db.run(text, _random_cuts(rng, len(text)), lanes=3))
        assert got == want, (pat, flags, text, got, want)
        done += 1
    assert done >= 100, tally.report()


@pytest.mark.parametrize("pat, flags", [("foo$", 0), (r"foo\Z", 0), ("foo$", 4), ("^x$", 0), ("^x$", 4), (r"\bab\b", 0), (r"ab\B", 0),
                                        ("foo", 0), ("o\n", 0), ("x\n$", 0)])
def test_boundary_cases_every_split(pat, flags):
    db = flowsim_py.Db([pat], [flags])
    assert db.h, db.error
    texts = [b"foo\n", b"foo\n\n", b"foo\nx", b"x\n", b"x\nx\n", b"\nx\n", b"ab ab", b"abab\n", b"ab\n", b"x\n\n", b"o\n\n"]
    for text in texts:
        n = len(text)
        splits = [[c] for c in range(n + 1)] + [list(range(1, n)), [0, 0, n, n]]
        for cuts in splits:
            for lanes in (1, 4):
                _check(db, [pat], text, cuts, piece=rng_piece(n), lanes=lanes)
                _check(db, [pat], text, cuts, piece=1, lanes=lanes)


def rng_piece(n):
    return max(1, n // 2)


def test_hold_decision():
    db = flowsim_py.Db(["foo$", r"foo\Z", "foo$", "foo", r"\bfoo\b", "^foo", r"foo\z"], [0, 0, 4, 0, 0, 0, 0])
    assert [db.hold(i) for i in range(7)] == [True, True, False, False, False, False, False]


def test_held_newline_reported_at_close():
    db = flowsim_py.Db(["foo$"], [0])
    assert db.run(b"foo\n", [4]) == [(2, 0, 3)]            # held by write 0, the close decides: final '\n'
    assert db.run(b"foo\nx", [4]) == []                     # ... a later byte: not final
    assert db.run(b"foo\n\n", [4]) == []
    db = flowsim_py.Db(["foo"], [0])
    assert db.run(b"xfoo", [4]) == [(0, 0, 4)]              # context-free: the write that ends the match reports it


def _block_reports(raw, ids, single, bounds):
    """hs_scan's report rules (hgface small path) restated: offset bounds, one SINGLEMATCH report per id (the smallest
    `to`), an identical (id, to) once; delivery order (to, id)."""
    reps = sorted((ids[e], t, single[e]) for e, t in raw if bounds[e][0] <= t <= bounds[e][1])
    out, seen_single = [], set()
    for k, (i, t, sg) in enumerate(reps):
        dup = k > 0 and reps[k - 1][:2] == (i, t)
        if not dup and not (sg and i in seen_single):
            out.append((i, t))
        if sg:
            seen_single.add(i)
    return sorted(out, key=lambda r: (r[1], r[0]))


def _check_delivered(db, data, cuts, ids, single, bounds, lanes=3):
    raw = db.run(data, cuts, lanes=lanes)
    got = db.deliver(data, cuts, raw)
    want = _block_reports(db.block(data), ids, single, bounds)
    assert sorted((i, t) for _, i, t in got) == sorted(want), (data, cuts, got, want)
    last = -1
    for call in range(len(cuts) + 2):
        mine = [(t, i) for c, i, t in got if c == call]
        assert mine == sorted(mine)  # rule 2: (to, id) within a call
        if mine:
            assert mine[0][0] >= last - 1, (data, cuts, call, mine, last)
            last = max(last, mine[-1][0])


def test_singlematch_and_offset_bounds_across_writes():
    """Face A's report rules (hg_flow_rules.h) over the replayed raw ends equal hs_scan's rules over the block scan:
    SINGLEMATCH once per stream, min_offset / max_offset on stream offsets, ids shared between expressions."""
    rng = random.Random(5)
    tally = accept_rules.Tally()
    done = 0
    for _ in range(400):
        pats = [regex_gen.random_pattern(rng) for _ in range(3)]
        flags = [rng.choice([0, 2, 4, 6]) | (8 if rng.random() < 0.5 else 0) for _ in pats]
        ids = [rng.choice([1, 1, 2, 3]) for _ in pats]
        bounds, exts = [], []
        for _p in pats:
            lo = rng.choice([None, None, 2, 7, 15])
            hi = rng.choice([None, None, 20, 40])
            if lo is not None and hi is not None and lo > hi:
                lo = None
            exts.append(extsim_py.ext(min_offset=lo, max_offset=hi) if (lo is not None or hi is not None) else None)
            bounds.append((lo or 0, hi if hi is not None else 1 << 62))
        db = flowsim_py.Db(pats, flags, ids=ids, exts=exts)
        if not tally.decide(pats, flags, bool(db.h), db.error, features=True):
            continue  # both compilers refuse the set, or a documented limit / rule of the feature does (asserted)
        single = [bool(f & 8) for f in flags]
        text = regex_gen.random_text(rng, rng.randint(2, 6), maxlen=12, final_newline=rng.random() < 0.5)
        for _ in range(3):
            _check_delivered(db, text, _random_cuts(rng, len(text)), ids, single, bounds, lanes=rng.choice([1, 3]))
        _check_delivered(db, text, list(range(1, len(text))), ids, single, bounds)
        done += 1
    assert done >= 150, tally.report()


def test_shared_singlematch_id_holds_together():
    """foo$ (holds a trailing newline) and o\n (does not) share a SINGLEMATCH id: both hold, so the smallest end wins."""
    db = flowsim_py.Db(["foo$", "o\n"], [8, 8], ids=[7, 7])
    assert db.hold(0) and db.hold(1)
    for cuts in ([4], [3], [2, 4], []):
        _check_delivered(db, b"foo\n", cuts, [7, 7], [True, True], [(0, 1 << 62)] * 2)


def test_stream_api_without_gpu():
    """open / copy / reset and close without a callback, and the mode errors, need no GPU."""
    import ctypes

    l = device.face_a()
    h, err = device.hs_compile(["foo", "bar$"], flags=[0, 0], ids=[1, 2], mode=device.HS_MODE_STREAM)
    assert err is None
    size = ctypes.c_size_t()
    assert l.hs_stream_size(h, ctypes.byref(size)) == 0 and size.value > 0
    s, t = ctypes.c_void_p(), ctypes.c_void_p()
    assert l.hs_open_stream(h, 0, ctypes.byref(s)) == 0
    assert l.hs_copy_stream(ctypes.byref(t), s) == 0 and t.value != s.value
    assert l.hs_reset_stream(s, 0, None, device.MATCH_EVENT(), None) == 0
    assert l.hs_close_stream(s, None, device.MATCH_EVENT(), None) == 0
    assert l.hs_close_stream(t, None, device.MATCH_EVENT(), None) == 0
    b, err = device.hs_compile(["foo"], flags=[0], mode=device.HS_MODE_BLOCK)
    assert err is None
    assert l.hs_open_stream(b, 0, ctypes.byref(s)) == device.HS_DB_MODE_ERROR
    assert l.hs_stream_size(b, ctypes.byref(size)) == device.HS_DB_MODE_ERROR
    l.hs_free_database(h)
    l.hs_free_database(b)
