"""Start of match in stream mode on the host (no GPU): the HS_MODE_SOM_HORIZON_* compile rules and stream sizes through
hs_compile_ext_multi, and a replay of the SOM flow routines (tests/native/flowsomsim.cpp: hg_flow_som_write with the
starts stored and reloaded at every write, the report rules of hg_flow_rules.h) over random splits against the block-mode
start of match (hg_hit_som) on the concatenation and against Python `re`."""
from __future__ import annotations

import ctypes
import random

import pytest

import accept_rules
import extsim_py
import flowsomsim_py
import regex_gen
from hypergrep_amd import device
from somsim_py import start_by_brute_force

SOM, SINGLE, MULTILINE = 256, 8, 4
STREAM = device.HS_MODE_STREAM
HORIZON = {"large": device.HS_MODE_SOM_HORIZON_LARGE, "medium": device.HS_MODE_SOM_HORIZON_MEDIUM, "small": device.HS_MODE_SOM_HORIZON_SMALL}
LATE, HOLD = 64, 32


def _compile(pats, flags, ids=None, ext=None, mode=STREAM):
    h, err = device.hs_compile(pats, flags, ids or list(range(len(pats))), ext, mode)
    return h, err


def _size(h) -> int:
    n = ctypes.c_size_t()
    assert device.face_a().hs_stream_size(h, ctypes.byref(n)) == device.HS_SUCCESS
    return n.value


# ---- compile rules (stream mode rule 7) -----------------------------------------------------------------------------------
def test_constants():
    assert (device.HS_MODE_SOM_HORIZON_LARGE, device.HS_MODE_SOM_HORIZON_MEDIUM, device.HS_MODE_SOM_HORIZON_SMALL) == (1 << 24, 1 << 25, 1 << 26)
    assert device.HS_OFFSET_PAST_HORIZON == 2**64 - 1


@pytest.mark.parametrize("hz", sorted(HORIZON))
def test_horizon_accepted_with_a_som_expression(hz):
    h, err = _compile(["foo[0-9]+bar", "xyz", r"\bab+c$"], [SOM, 0, SOM | MULTILINE], [1, 2, 3], mode=STREAM | HORIZON[hz])
    assert err is None and h
    device.face_a().hs_free_database(h)


@pytest.mark.parametrize("hz", sorted(HORIZON))
def test_horizon_rejections(hz):
    # on a set without SOM expressions
    h, err = _compile(["abc", "foo"], [0, 0], mode=STREAM | HORIZON[hz])
    assert h is None and err is not None and "HORIZON" in err[0]
    # with block mode
    h, err = _compile(["abc"], [SOM], mode=device.HS_MODE_BLOCK | HORIZON[hz])
    assert h is None and err is not None
    # two horizon bits
    other = HORIZON["small"] if hz != "small" else HORIZON["large"]
    h, err = _compile(["abc"], [SOM], mode=STREAM | HORIZON[hz] | other)
    assert h is None and err is not None


def test_som_without_horizon_names_expression_and_horizon():
    h, err = _compile(["xyz", "abc"], [0, SOM], [1, 2])
    assert h is None and err[1] == 1
    assert "expression 1" in err[0] and "SOM_LEFTMOST" in err[0] and "stream mode" in err[0] and "HORIZON" in err[0]


def test_block_som_rules_apply_in_stream_mode():
    mode = STREAM | HORIZON["large"]
    h, err = _compile(["foobar"], [SOM | SINGLE], mode=mode)
    assert h is None and "SINGLEMATCH" in err[0]
    h, err = _compile(["foo", "bar"], [SOM, 0], [5, 5], mode=mode)
    assert h is None and err is not None
    h, err = _compile(["foo", "bar", "baz"], [SOM, SOM, 0], [5, 5, 6], mode=mode)
    assert err is None
    device.face_a().hs_free_database(h)


def test_som_position_limit():
    mode = STREAM | HORIZON["small"]
    h, err = _compile(["abc", "x[a-z]{300}y"], [SOM, SOM], mode=mode)
    assert h is None and err[1] == 1 and "too large for start of match in stream mode" in err[0] and "256" in err[0]
    # after ext expansion too
    h, err = _compile(["abc", "x[a-z]{100}y"], [SOM, SOM], ext=[None, extsim_py.ext(edit=2)], mode=mode)
    assert h is None and err[1] == 1 and "too large for start of match in stream mode" in err[0]
    # a SOM expression below the limit, and a non-SOM expression above it (the 1024 limit holds for those)
    h, err = _compile(["x[a-z]{200}y", "q[a-z]{300}r"], [SOM, 0], mode=mode)
    assert err is None
    device.face_a().hs_free_database(h)


# ---- stream sizes --------------------------------------------------------------------------------------------------------
def test_stream_size_grows_with_the_horizon():
    sizes = {}
    for hz in HORIZON:
        h, err = _compile(["foo[0-9]+bar", "xyz", "a[^z]*b"], [SOM, 0, SOM], mode=STREAM | HORIZON[hz])
        assert err is None
        sizes[hz] = _size(h)
        device.face_a().hs_free_database(h)
    assert sizes["small"] < sizes["medium"] < sizes["large"], sizes
    h, _ = _compile(["foo[0-9]+bar", "xyz", "a[^z]*b"], [0, 0, 0])
    assert _size(h) < sizes["small"]
    device.face_a().hs_free_database(h)


# the sets of tests/test_streammode_gpu.py, sizes as the parent commit computed them
PLAIN_SETS = {
    "one_word": ((["foo", r"\bbar\b", "ba+z$", "qu[xy]", r"o\n", r"^x"], [0, 0, 0, 1, 0, 4], None), 168),
    "multi_word": ((["a[a-f]{40}b", "(ab|cd){12}e", "x[a-z ]{900}y", r"\bfo[a-z]{50}\b"], [0, 2, 2, 0], None), 276),
    "literal": ((["hello world", "status=5[0-9][0-9]", "foobar", "xyzzy"], [8, 0, 1 | 8, 0], None), 152),
    "caseless_ext": ((["foobar", "abcdef", "zebra"], [1, 0, 1 | 8], [extsim_py.ext(edit=1), extsim_py.ext(min_offset=10, max_offset=5000), extsim_py.ext(hamming=1)]), 144),
}


@pytest.mark.parametrize("name", sorted(PLAIN_SETS))
def test_stream_sizes_without_som_unchanged(name):
    (pats, flags, ext), want = PLAIN_SETS[name]
    h, err = _compile(pats, flags, ext=ext)
    assert err is None
    assert _size(h) == want
    device.face_a().hs_free_database(h)


# ---- replay --------------------------------------------------------------------------------------------------------------
def _check(db, pats, flags, ids, data, cuts, horizon="large", brute=True):
    got = db.run(data, cuts, horizon)
    want = db.block(data, horizon)
    flat = [(i, f, t) for _, i, f, t in got]
    assert sorted(flat) == sorted(want), (pats, flags, ids, data, cuts, got, want)
    assert len({(i, t) for i, _, t in flat}) == len(flat)  # an (id, to) once: every report of it in one call
    for call in {c for c, *_ in got}:
        order = [(t, i) for c, i, _, t in got if c == call]
        assert order == sorted(order)
    if brute:
        for i, f, t in want:
            members = [k for k in range(len(pats)) if ids[k] == i]
            if not flags[members[0]] & SOM:
                assert f == 0
                continue
            starts = [s for s in (start_by_brute_force(pats[k], flags[k], data, t) for k in members) if s is not None]
            assert f == min(starts), (pats, data, i, t, f, starts)
    return len(want)


def _random_cuts(rng, n):
    k = rng.randint(0, min(n, 8))
    cuts = sorted(rng.randint(0, n) for _ in range(k))
    if rng.random() < 0.3:
        cuts += [c for c in cuts if rng.random() < 0.5]  # empty writes
        cuts.sort()
    return cuts


def _around_newlines(data):
    return sorted({c for i, b in enumerate(data) if b == 10 for c in (i, i + 1) if 0 <= c <= len(data)})


def test_replay_random_sets_against_block_and_re():
    rng = random.Random(7)
    tally = accept_rules.Tally()
    done = reports = 0
    for _ in range(400):
        n = rng.randint(1, 3)
        pats = [regex_gen.random_pattern(rng) for _ in range(n)]
        flags = [rng.choice([0, 2, 4, 6, 1, 5]) | SOM for _ in pats]
        ids = list(range(n))
        db = flowsomsim_py.Db(pats, flags, ids)
        if not tally.decide(pats, flags, bool(db.h), db.error, features=True):
            continue  # both compilers refuse the set, or a documented limit / rule of the feature does (asserted)
        text = regex_gen.random_text(rng, rng.randint(1, 5), maxlen=12, final_newline=rng.random() < 0.5)
        for _ in range(3):
            reports += _check(db, pats, flags, ids, text, _random_cuts(rng, len(text)))
        reports += _check(db, pats, flags, ids, text, list(range(1, len(text))))  # 1-byte writes
        reports += _check(db, pats, flags, ids, text, _around_newlines(text))
        done += 1
    assert done >= 200 and reports > 500, tally.report()


def test_replay_shared_ids_take_the_smallest_start():
    rng = random.Random(8)
    tally = accept_rules.Tally()
    checked = 0
    for _ in range(250):
        n = rng.randint(2, 4)
        pats = [regex_gen.random_pattern(rng) for _ in range(n)]
        flags = [rng.choice([0, 2, 4, 6]) | SOM for _ in pats]
        ids = [rng.choice([1, 2]) for _ in pats]
        db = flowsomsim_py.Db(pats, flags, ids)
        if not tally.decide(pats, flags, bool(db.h), db.error, features=True):
            continue  # both compilers refuse the set, or a documented limit / rule of the feature does (asserted)
        for k in range(n):
            shared = ids.count(ids[k]) > 1
            assert bool(db.header(k) & LATE) == shared
        text = regex_gen.random_text(rng, rng.randint(1, 5), maxlen=12, final_newline=rng.random() < 0.5)
        for cuts in (_random_cuts(rng, len(text)), list(range(1, len(text))), _around_newlines(text)):
            checked += _check(db, pats, flags, ids, text, cuts)
    assert checked > 200, tally.report()
    # fixed: both expressions end at the same `to`, the longer one wins, whatever the split
    pats, flags, ids = ["ab+c", "b+c", "xa"], [SOM, SOM, SOM], [1, 1, 2]
    db = flowsomsim_py.Db(pats, flags, ids)
    data = b"zabbbc bc xa abc\n"
    for c in range(len(data) + 1):
        _check(db, pats, flags, ids, data, [c])


@pytest.mark.parametrize("pat,flags,data", [
    (r"\bfoo\b", 6, b"foo xfoo foo_ foo\n-foo"),
    (r"\Bbar", 6, b"bar xbar xbarx\nbar"),
    (r"^ab+", 2, b"abbb ab\nabab\n"),
    (r"^ab+", 6, b"abbb ab\nabab\n ab\n"),
    (r"a+$", 6 | MULTILINE, b"baaa\naa a\nxa"),
    (r"a+$", 2, b"baaa\naa a\nxaa\n"),
    (r"x+\Z", 2, b"xx\nxxx\n"),
    (r"[a-c]+\b", 6, b"zzabc abcab\ncab"),
])
def test_replay_boundary_assertions_at_every_split(pat, flags, data):
    db = flowsomsim_py.Db([pat], [flags | SOM], [1])
    assert db.h, db.error
    brute = "\\Z" not in pat  # (Python's \Z is Hyperscan's \z: the block reference alone checks those)
    for c in range(len(data) + 1):
        _check(db, [pat], [flags | SOM], [1], data, [c], brute=brute)
    _check(db, [pat], [flags | SOM], [1], data, list(range(1, len(data))), brute=brute)
    _check(db, [pat], [flags | SOM], [1], data, [0, 0, len(data), len(data)], brute=brute)


def test_replay_mixed_som_and_plain_expressions():
    rng = random.Random(9)
    pats = ["foo[0-9]*bar", r"\bba+z", "qu[xy]+", "o\n", r"ab+$"]
    flags = [SOM, 0, SOM | 2, 0, SOM]
    ids = [1, 2, 3, 4, 5]
    db = flowsomsim_py.Db(pats, flags, ids)
    assert db.h, db.error
    needles = [b"foo12bar", b"baaz", b"quxy", b"o\n", b"abb\n", b"foobar"]
    for _ in range(60):
        data = b"".join(rng.choice(needles) if rng.random() < 0.4 else bytes(rng.choice(b"abfoqxz \n") for _ in range(rng.randint(0, 6))) for _ in range(8))
        _check(db, pats, flags, ids, data, _random_cuts(rng, len(data)))
        _check(db, pats, flags, ids, data, list(range(1, len(data))))


def test_replay_edit_distance():
    rng = random.Random(10)
    pats = ["foobar", "abc[0-9]"]
    flags = [SOM, SOM | 1]
    exts = [extsim_py.ext(edit=1), extsim_py.ext(hamming=1)]
    db = flowsomsim_py.Db(pats, flags, [1, 2], exts)
    assert db.h, db.error
    needles = [b"foobar", b"fobar", b"fooxbar", b"foobaz", b"ABC7", b"abd7", b"abc"]
    total = 0
    for _ in range(80):
        data = b"".join(rng.choice(needles) if rng.random() < 0.5 else bytes(rng.choice(b"abfor \n") for _ in range(rng.randint(0, 5))) for _ in range(6))
        for cuts in (_random_cuts(rng, len(data)), list(range(1, len(data)))):
            total += _check(db, pats, flags, [1, 2], data, cuts, brute=False)
    assert total > 50


@pytest.mark.parametrize("hz", ["small", "medium", "large"])
def test_replay_horizon(hz):
    db = flowsomsim_py.Db(["a[^z]*b"], [SOM], [1])
    for k in (65533, 65534, 70000):  # spans 65535, 65536, 70002
        data = b"a" + b"x" * k + b"b"
        got = db.run(data, [1, 30000, k + 1], hz)
        span = k + 2
        want_from = flowsomsim_py.PAST if (hz == "small" and span >= 1 << 16) else 0
        assert [(i, f, t) for _, i, f, t in got] == [(1, want_from, span)], (hz, k, got)
        assert [(i, f, t) for _, i, f, t in got] == db.block(data, hz)
