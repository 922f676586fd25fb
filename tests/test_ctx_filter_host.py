"""CPU checks of the stream pass's first level with one byte of context (HgDb::filter_ctx, hg_db.h hg_slot_match_ctx)
through its host mirror tests/native/ctxsim.cpp: it never rejects what the first + second level behind it pass, and on the
headline workload's text it lets through what the design says it does."""
from __future__ import annotations

import random

import numpy as np
import pytest

import ctxsim_py
import regex_gen
import stream_cells as sc

MIB = 1 << 20
# the single-probe cells of dword-aligned windows: five filter sizes with nothing folded, five with the text folded, and the
# caseless set whose windows are stored in every case variant (nothing folded)
DWORD_CELLS = [c for c in sc.STREAM_CELLS if not c.wide and c.dense == 0]


def _cell_db(cell):
    lits, caseless = sc.literal_set(cell)
    db = ctxsim_py.Db(sc.patterns_of(lits), flags=sc.flags_of(caseless), ids=list(range(len(lits))))
    assert db.ok(), db.error
    info = db.info()
    assert (info["filter_log2"], info["wide"], info["dense"], info["fold_mask"] != 0) == (cell.log2, 0, 0, cell.fold), info
    assert info["has_ctx"] == 1, info
    return db, lits, caseless


def _c3_text(at: int, n: int, which: str = "c3") -> bytes:
    """Bytes [at, at + n) of a benchmark workload's text (bench.py; config 3 is the headline)."""
    from hypergrep_amd import benchspec, device

    _patterns, needles, hpm = {"c3": benchspec.c3_spec, "c1": benchspec.c1_spec}[which]()
    first = at // device.SYNTH_BLOCK
    skip = at - first * device.SYNTH_BLOCK
    return device.synth_host(n + skip, benchspec.SEED_BASE + int(which[1]), needles, hpm, first_block=first)[skip:skip + n]


@pytest.fixture(scope="module")
def c3_tuned():
    """Config 3's database with its windows tuned as bench.py tunes them: four pieces of 256 KiB spread over the first 256 MiB."""
    from hypergrep_amd import benchspec

    patterns, _needles, _hpm = benchspec.c3_spec()
    db = ctxsim_py.Db(patterns, ids=list(range(len(patterns))))
    assert db.ok(), db.error
    sample = b"".join(_c3_text(((256 * MIB) // 4 * i) & ~15, 256 << 10) for i in range(4))
    assert db.tune(sample) == 0
    assert db.info()["has_ctx"] == 1, db.info()
    return db


@pytest.mark.parametrize("cell", DWORD_CELLS, ids=lambda c: c.name)
def test_every_window_of_a_cell_passes(cell):
    db, _lits, _caseless = _cell_db(cell)
    bad, checks = db.windows()
    info = db.info()
    assert bad == 0 and checks >= 7 * info["windows"] > 0, (bad, checks, info)
    # the literals are 8 bytes: the windows at offsets 0-3 have a context byte, so most slots must care about it.  (Not where
    # caseless windows are stored in every case variant: a caseless letter after a window is no condition when nothing is
    # folded, and two thirds of ALNUM are letters.)
    if cell.fold or not cell.caseless:
        assert info["ctx_slots"] * 2 >= info["used_slots"], info
    else:
        assert info["ctx_slots"] > 0, info


def test_every_window_of_config3_passes(c3_tuned):
    from hypergrep_amd import benchspec

    patterns, _needles, _hpm = benchspec.c3_spec()
    static = ctxsim_py.Db(patterns, ids=list(range(len(patterns))))
    for db in (static, c3_tuned):
        bad, checks = db.windows()
        info = db.info()
        assert info["has_ctx"] == 1 and bad == 0 and checks >= 7 * info["windows"] > 0, (bad, checks, info)


def test_every_window_of_random_sets_passes():
    rng = random.Random(20260)
    with_ctx = 0
    for i in range(400):
        k = rng.randint(1, 6)
        pats = [regex_gen.random_pattern(rng) for _ in range(k)]
        if i % 2:  # (the generator's literals are short: most sets get byte-aligned windows.  A literal stem in front of each
            # expression gives them dword-aligned ones, whose neighbours are the expression's own first bytes)
            pats = ["".join(rng.choice(sc.ALNUM + "_= ") for _ in range(rng.randint(7, 14))) + p for p in pats]
        flags = [rng.choice([14, 14, 15, 10, 6, 12]) for _ in range(k)]
        db = ctxsim_py.Db(pats, flags)
        if not db.ok():
            continue
        info = db.info()
        if info["wide"] or info["dense"]:
            assert info["has_ctx"] == 0, (pats, info)  # (those layouts keep their first level)
            continue
        assert info["has_ctx"] == 1, (pats, info)
        bad, checks = db.windows()
        assert bad == 0, (pats, flags, bad, checks)
        with_ctx += 1 if info["windows"] else 0
    assert with_ctx >= 50, with_ctx


def _lookalike_text(lits, caseless, nbytes: int, seed: int) -> bytes:
    """Seeded random text over the literals' alphabet with planted literals, case variants and look-alikes: a literal cut
    after 4-8 bytes and continued with another byte, at every alignment."""
    rng = random.Random(seed)
    nprng = np.random.default_rng(seed)
    buf = nprng.choice(sc.FILLER, size=nbytes)
    buf[nprng.random(nbytes) < 1 / 70] = 10
    t = bytearray(buf.tobytes())
    real = [(l, c) for l, c in zip(lits, caseless) if l != sc.SPACES.encode()]
    at = 0
    while at < nbytes - 64:
        lit, cl = rng.choice(real)
        if cl and rng.random() < 0.5:
            lit = sc.case_variant(lit, rng)
        r = rng.random()
        if r < 0.6:  # equal through 4-8 bytes, then something else
            cut = rng.randint(4, len(lit))
            lit = lit[:cut] + bytes([rng.choice(b"!#%xyz059 AQ")])
        t[at:at + len(lit)] = lit
        at += len(lit) + rng.randint(0, 40)
    return bytes(t)


def test_never_rejects_what_both_old_levels_pass(c3_tuned):
    """{dwords passing the new first level} contains {dwords passing the old first level and the second level}, and the
    candidates are the same set, on more than 1e7 dwords of random text with planted look-alikes."""
    total = 0
    for name in ("dword11", "dword12", "dword13", "dword12_fold", "dword13_fold", "dword_expand"):
        db, lits, caseless = _cell_db(sc.BY_NAME[name])
        r = db.scan(_lookalike_text(lits, caseless, 7 * MIB, seed=len(name) + lits[0][0]))
        assert r["violations"] == 0 and r["cands_new"] == r["cands_old"] > 1000, (name, r)
        assert r["dropped"] > 1000, (name, r)  # (the look-alikes are what it is for)
        total += r["dwords"]
    r = c3_tuned.scan(_c3_text(48 * MIB, 4 * MIB))
    assert r["violations"] == 0 and r["cands_new"] == r["cands_old"] > 0, r
    total += r["dwords"]
    assert total >= 10_000_000, total


def test_config3_floors(c3_tuned):
    """16 MiB of config 3's text, tuned windows.  Measured with the context byte on top of all 16 bits of hash C: 0.14 % of the
    dwords, 30 % of the 1 KiB wave-iterations; the bounds leave room for the four fingerprint bits given up to it.  The old
    first level, measured on the same text, must still show the workload these figures are about (1.26 %, 85 %)."""
    r = c3_tuned.scan(_c3_text(0, 16 * MIB))
    print({k: r[k] for k in ctxsim_py.SCAN_FIELDS},
          "old %.3f %% of dwords, %.1f %% of rows; new %.3f %%, %.1f %%" % (100 * r["l1_old"] / r["dwords"], 100 * r["rows_old"] / r["rows"],
                                                                          100 * r["l1_new"] / r["dwords"], 100 * r["rows_new"] / r["rows"]))
    assert r["violations"] == 0 and r["cands_new"] == r["cands_old"], r
    assert r["l1_old"] >= 0.010 * r["dwords"] and r["rows_old"] >= 0.80 * r["rows"], r
    assert r["l1_new"] <= 0.0025 * r["dwords"], r
    assert r["rows_new"] <= 0.40 * r["rows"], r


def test_tune_keeps_the_context_byte_only_where_it_pays(c3_tuned):
    """hgc_tune runs the kernels with the context byte when it spares at least one 1 KiB wave-iteration in four of the sample
    (the reasoning is at the decision, hg_compile.cpp): config 3 keeps it (85 % -> 36 %), config 1 — one rare literal, next to
    nothing passes its first level — does not and runs the kernels without it; an untuned database keeps it."""
    from hypergrep_amd import benchspec

    assert c3_tuned.info()["use_ctx"] == 1, c3_tuned.info()
    patterns, _needles, _hpm = benchspec.c1_spec()
    c1 = ctxsim_py.Db(patterns, ids=[0])
    assert c1.ok() and c1.info()["has_ctx"] == 1 and c1.info()["use_ctx"] == 1, c1.info()
    sample = b"".join(_c3_text(((256 * MIB) // 4 * i) & ~15, 256 << 10, "c1") for i in range(4))
    assert c1.tune(sample) == 0
    info = c1.info()
    assert info["has_ctx"] == 1 and info["use_ctx"] == 0, info
    r = c1.scan(_c3_text(0, MIB, "c1"))
    assert r["violations"] == 0 and r["rows_old"] * 4 < r["rows"], r
