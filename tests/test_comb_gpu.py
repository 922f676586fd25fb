"""Logical combinations (HS_FLAG_COMBINATION, HS_FLAG_QUIET) on the MI355X: the combination pass (hg_comb.hip) against the
independent reference tests/comb_ref.py, applied to the oracle's reports of the same set without its combinations and with
QUIET cleared.  Every tier as operands, SINGLEMATCH and all-matches expressions, quiet and shared ids, SOM expressions,
several pipeline chunks, segmented scans, hit-heavy long lines, Face B and Face A.  Texts sit at the end of guarded buffers:
a read past them faults."""
from __future__ import annotations

import ctypes
import os
import random
import tempfile

import numpy as np
import pytest

import chunk_texts
import comb_ref
import oracle_py

pytestmark = pytest.mark.gpu

COMB, QUIET, SINGLE, SOM = 512, 1024, 8, 256

# operand sets, one per tier: literal-anchored confirm, byte-window short literals, always-on one word / two words, huge,
# literal-only
TIER_SETS = {
    "anchored": [r"user=[a-z0-9_]{4,12} status=5[0-9]{2}", r"ERROR [0-9]+ failed", r"\bconnection reset\b", r"timeout=\d+ms"],
    "byte_windows": [r"abc[0-9]+", r"\bxyz\d", r"qr[st]{1,3}u", r"abc"],
    "always_on_1w": [r"[0-9]+x", r"a.b", r"^[a-c]+", r"[d-f]_"],
    "always_on_2w": [r"([a-f][0-9]){17}", r"[a-f]([0-9][a-f]|_){16}z", r"[0-9]x", r"a-b"],
    "huge": [r"e[0-9a-f_]{0,1500}z", r"needle-in-hay", r"qrstu", r"12x"],
    "literal_only": [r"needle-in-hay", r"other-literal-text", r"ERROR", r"timeout"],
}
FRAGMENTS = [b"user=abcd_12 status=503", b"ERROR 42 failed", b"connection reset", b"timeout=120ms", b"abc123", b"xyz9", b"qrstu", b"qrsu",
             b"12x", b"a-b", b"aab", b"cab", b"a1b2c3d4e5f6" * 8 + b"x", b"e5_f6" * 7 + b"z", b"needle-in-hay", b"other-literal-text", b"ERROR",
             b"timeout", b"d_", b"0", b"\t", b"  ", b"\0", b"zz"]
FORMULAS = ["{0} & {1}", "{0} & !{1}", "({0} | {2}) & !{3}", "{1} | {2} & {3}", "{0}", "{3} & !({0} | {1})", "{0}&{1}&{2}&{3}", "!{1} & {2}"]


def make_text(rng: random.Random, nlines: int) -> bytes:
    lines = []
    for _ in range(nlines):
        parts = [rng.choice(FRAGMENTS) if rng.random() < 0.6 else bytes(rng.choice(b"abcdef0123456789 _-x") for _ in range(rng.randint(0, 12)))
                 for _ in range(rng.randint(0, 6))]
        lines.append(rng.choice([b" ", b"", b"; "]).join(parts))
    return b"\n".join(lines) + (b"\n" if rng.random() < 0.8 else b"")


def with_combinations(pats, ids, rng, quiet_mask, single_mask, comb_single_mask=0, comb_quiet_mask=0):
    """pats (flags 6, QUIET / SINGLEMATCH per mask) + one combination per FORMULAS entry over the distinct ids"""
    uniq = sorted(set(ids))
    flags = [6 | (QUIET if quiet_mask >> ids[i] & 1 else 0) | (SINGLE if single_mask >> ids[i] & 1 else 0) for i in range(len(pats))]
    combs, cflags = [], []
    for k, f in enumerate(FORMULAS):
        ops = [uniq[j % len(uniq)] for j in rng.sample(range(len(uniq)), len(uniq))] + uniq
        combs.append(f.format(*[100 + o for o in ops]))
        cflags.append(COMB | (SINGLE if comb_single_mask >> k & 1 else 0) | (QUIET if comb_quiet_mask >> k & 1 else 0))
    all_ids = [100 + i for i in ids] + [500 + k for k in range(len(combs))]
    return pats + combs, flags + cflags, all_ids


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(4 << 20)
    yield a
    a.free()


def gpu_scan(arena, text, pats, flags, ids, bs):
    """[(line, id, to, start, len)] and the expression index of each hit, and the hit starts"""
    from hypergrep_amd import device

    sc = device.Scanner(device.Database(pats, flags=flags, ids=ids), 0)
    st = sc.scan(arena.place(text), len(text), buffer_size=bs)
    n = st.n_hits
    hits = np.zeros(n, dtype=[("line_number", "<u8"), ("id", "<u4"), ("to", "<u4")])
    aux = np.zeros(n, dtype=[("start", "<u8"), ("len", "<u4"), ("pattern", "<u4")])
    if n:
        assert device.lib().hg_copy_hits(sc._h, hits.ctypes.data_as(ctypes.POINTER(device.HgHit)), aux.ctypes.data_as(ctypes.POINTER(device.HgHitAux)), n) == 0  # pylint: disable=protected-access
    rows = list(zip(hits["line_number"].tolist(), hits["id"].tolist(), hits["to"].tolist(), aux["start"].tolist(), aux["len"].tolist()))
    return rows, aux["pattern"].tolist(), sc.hit_starts(), st


def reference(text, pats, flags, ids, bs):
    cs = comb_ref.CombSet(pats, flags, ids)
    bp, bf, bi = cs.oracle_inputs(pats, flags, ids)
    rc, hits, _ = oracle_py.scan_buffer(text, bp, [f & ~SOM for f in bf], bi, buffer_size=bs)
    assert rc == 0
    return comb_ref.apply_to_hits(cs, hits)


def reference_by_distinct_lines(text, pats, flags, ids, bs):
    """The same reference with the oracle run once per DISTINCT line (texts of chunk_texts: every line shorter than the scan
    buffer, long runs of repeated lines)."""
    mini, which, starts = chunk_texts.distinct(text)
    return chunk_texts.expand(reference(mini, pats, flags, ids, bs), mini, which, starts)


def check(arena, text, pats, flags, ids, bs=262140, min_launches=0, ref=reference):
    got, patterns, _, st = gpu_scan(arena, text, pats, flags, ids, bs)
    assert st.stream_launches >= min_launches
    want = ref(text, pats, flags, ids, bs)
    assert got == want, next(((g, w) for g, w in zip(got, want) if g != w), (len(got), len(want)))
    for (_, rid, _, _, _), p in zip(got, patterns):  # each hit names an expression with its id
        assert ids[p] == rid
    ncomb = sum(1 for r in got if r[1] >= 500)
    return len(got), ncomb


@pytest.mark.parametrize("tier", sorted(TIER_SETS))
def test_every_tier_as_operands(arena, tier):
    rng = random.Random(sum(tier.encode()))
    base = TIER_SETS[tier]
    total = combs = 0
    for quiet_mask, single_mask, bs in ((0b0101, 0, 262140), (0, 0b0011, 40), (0b1111, 0b1010, 262140)):
        pats, flags, ids = with_combinations(base, list(range(len(base))), rng, quiet_mask, single_mask, comb_single_mask=0b10101010)
        n, c = check(arena, make_text(rng, 500), pats, flags, ids, bs)
        total += n
        combs += c
    assert combs > 20, (total, combs)


def test_shared_ids_quiet_and_singlematch_combinations(arena):
    rng = random.Random(4)
    base = TIER_SETS["anchored"] + TIER_SETS["always_on_1w"] + TIER_SETS["literal_only"]
    ids = [0, 1, 1, 2, 3, 3, 4, 5, 5, 6, 6, 2]
    for quiet_mask, single_mask, cs, cq in ((0b0100110, 0b0000101, 0b00001111, 0b01000000), (0b1111111, 0, 0b11110000, 0), (0, 0b1111111, 0, 0b1)):
        pats, flags, all_ids = with_combinations(base, ids, rng, quiet_mask, single_mask, cs, cq)
        n, c = check(arena, make_text(rng, 800), pats, flags, all_ids)
        assert c > 20, (n, c)


def test_quiet_only_database_delivers_nothing_quiet(arena):
    rng = random.Random(9)
    base = TIER_SETS["anchored"]
    flags = [6 | QUIET, 6, 6 | QUIET, 6]
    ids = [1, 2, 3, 4]
    text = make_text(rng, 500)
    n, _ = check(arena, text, base, flags, ids)
    assert n > 10
    got, _, _, _ = gpu_scan(arena, text, base, [6] * 4, ids, 262140)
    assert any(r[1] in (1, 3) for r in got)  # (the quiet expressions do match this text)


def test_combinations_with_som_expressions(arena):
    rng = random.Random(12)
    base = TIER_SETS["anchored"] + TIER_SETS["byte_windows"]
    ids = list(range(len(base)))
    pats, flags, all_ids = with_combinations(base, ids, rng, 0b00010001, 0)
    flags = [f | SOM if i < len(base) and not f & QUIET else f | (SOM if i >= len(base) else 0) for i, f in enumerate(flags)]
    text = make_text(rng, 800)
    check(arena, text, pats, flags, all_ids)
    got, _, starts, _ = gpu_scan(arena, text, pats, flags, all_ids, 262140)
    plain_rows, _, plain_starts, _ = gpu_scan(arena, text, base, [f for f in flags[:len(base)]], all_ids[:len(base)], 262140)
    start_of = {(r[0], r[1], r[2]): s for r, s in zip(plain_rows, plain_starts.tolist())}
    n_comb = 0
    for r, s in zip(got, starts.tolist()):
        if r[1] >= 500:
            assert s == 0  # combinations report from = 0
            n_comb += 1
        else:
            assert s == start_of[(r[0], r[1], r[2])], r
    assert n_comb > 20


def test_several_pipeline_chunks_and_segments(arena, monkeypatch):
    from hypergrep_amd import device

    rng = random.Random(8)
    text = make_text(rng, 30000)
    assert len(text) > (1 << 19)
    base = TIER_SETS["anchored"] + TIER_SETS["always_on_2w"]
    pats, flags, ids = with_combinations(base, list(range(len(base))), rng, 0b00110011, 0b01000100, comb_single_mask=0b0110)
    sc = device.Scanner(device.Database(pats, flags=flags, ids=ids), 0)
    raw = sc.scan(arena.place(text), len(text), buffer_size=1000).n_raw_hits
    assert raw > 4000
    for env in ({"HG_HIT_LIMIT": str(raw * 3 // 4)}, {"HG_HIT_LIMIT": str(raw // 2)}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            n, c = check(arena, text, pats, flags, ids, 1000)
            assert c > 1000, (env, n, c)
    # three pipeline chunks of 1024 tiles (the engine honours no smaller one) on more than 2048 tiles: lines of make_text around
    # the two cuts, a few repeated lines between them; the oracle runs once per distinct line
    parts = [[ln + b"\n" for ln in make_text(rng, 1200).rstrip(b"\n").split(b"\n")] for _ in range(4)]
    parts[2].append(b"user=abcd_12 status=503 " + b"q" * 300 + b" ERROR 42 failed; timeout=120ms\n")  # the line across the second cut
    every = b"user=abcd_12 status=503; ERROR 42 failed; connection reset; timeout=120ms " + b"q " * 200
    fillers = [b"lorem ipsum dolor " * 45 + b"\n", every + b"\n", b"0 " * 400 + b"\n", b"ERROR 42 failed " + b"q " * 300 + b"a1b2c3d4e5f6" * 8 + b"x\n",
               b"connection reset; " + b"- " * 200 + b"timeout=120ms\n"]
    big_text = chunk_texts.build(parts, fillers)
    big = device.GuardedArena(chunk_texts.SIZE + 64)
    try:
        with monkeypatch.context() as m:
            for k, v in chunk_texts.CHUNK_ENV.items():
                m.setenv(k, v)
            n, c = check(big, big_text, pats, flags, ids, 1000, min_launches=2, ref=reference_by_distinct_lines)
            assert c > 1000, (n, c)
    finally:
        big.free()


def test_hit_heavy_long_lines(arena):
    # an always-on QUIET operand reports on every byte of lines of up to 120 KiB
    rng = random.Random(17)
    lines = [bytes(rng.choice(b"abcdefgh") for _ in range(rng.choice([5, 1000, 120000]))) + (b" zz" if rng.random() < 0.5 else b"") for _ in range(6)]
    text = b"\n".join(lines) + b"\n"
    pats = [r"[a-h]", r"zz", r"h", "100 & !101", "100 & 101", "102 & !101"]
    flags = [6 | QUIET, 6, 6 | QUIET, COMB, COMB | SINGLE, COMB]
    ids = [100, 101, 102, 500, 501, 502]
    n, c = check(arena, text, pats, flags, ids)
    assert c > 100000, (n, c)


def test_face_b_scan_and_max_match_count():
    import hypergrep_amd

    rng = random.Random(21)
    base = TIER_SETS["anchored"] + TIER_SETS["byte_windows"]
    pats, flags, ids = with_combinations(base, list(range(len(base))), rng, 0b10011001, 0b00100010, comb_single_mask=0b1100)
    text = make_text(rng, 3000)
    want_hits = reference(text, pats, flags, ids, 262140)
    lines = {}
    for line, rid, to, off, ln in want_hits:
        lines.setdefault(line, []).append((to, rid, text[off:off + ln]))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "f.log")
        with open(path, "wb") as f:
            f.write(text)
        for max_count in (0, 1, 7, 150):
            want = []
            for line in sorted(lines):
                want.extend((line, rid, body) for _, rid, body in sorted(lines[line], key=lambda r: (r[0], r[1])))
                if max_count and len(want) >= max_count:
                    break
            rows = []

            def on_match(matches, n, rows=rows):
                rows.extend((matches[k].line_number, matches[k].id, matches[k].line) for k in range(n))

            assert hypergrep_amd.scan(path, pats, on_match, flags=flags, ids=ids, max_match_count=max_count) == 0
            assert [(r[0], r[1]) for r in rows] == [(w[0], w[1]) for w in want], max_count
            assert any(r[1] >= 500 for r in rows)
        assert hypergrep_amd.check_compatibility(pats, flags=flags, ids=ids) == 0


MATCH_EVENT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_void_p)


def face_a(pats, flags, ids, data):
    from hypergrep_amd import utils

    lib = ctypes.CDLL(utils._get_hyperscanner_lib()._name)  # pylint: disable=protected-access
    n = len(pats)
    db, err = ctypes.c_void_p(), ctypes.c_void_p()
    rc = lib.hs_compile_multi((ctypes.c_char_p * n)(*[p.encode() for p in pats]), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*ids), n, 1, None,
                              ctypes.byref(db), ctypes.byref(err))
    assert rc == 0
    scratch = ctypes.c_void_p()
    assert lib.hs_alloc_scratch(db, ctypes.byref(scratch)) == 0
    out = []

    @MATCH_EVENT
    def on_match(rid, frm, to, _flags, _ctx):
        out.append((rid, frm, to))
        return 0

    rc = lib.hs_scan(db, data, len(data), 0, scratch, on_match, None)
    lib.hs_free_scratch(scratch)
    lib.hs_free_database(db)
    return rc, out


@pytest.mark.parametrize("length", [60, 3000, 20000])
def test_face_a_block_callbacks(length):
    rng = random.Random(length)
    base = TIER_SETS["anchored"] + TIER_SETS["always_on_1w"]
    pats, flags, ids = with_combinations(base, list(range(len(base))), rng, 0b00100101, 0b00010000, comb_single_mask=0b0101)
    seen_comb = False
    for _ in range(4):
        data = make_text(rng, length // 8 + 1).replace(b"\n", b" ").replace(b"\0", b" ")[:length]
        rc, got = face_a(pats, flags, ids, data)
        assert rc == 0
        want_hits = reference(data, pats, flags, ids, len(data) + 2)
        want = sorted(((rid, 0, to) for _, rid, to, _, _ in want_hits), key=lambda r: (r[2], r[0]))
        assert got == want
        seen_comb = seen_comb or any(r[0] >= 500 for r in got)
    assert seen_comb
