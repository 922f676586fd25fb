"""Start of match (HS_FLAG_SOM_LEFTMOST) on the MI355X: the GPU pass (hg_som.hip) against the host reference routine
(hg_som.h through tests/native/somsim.cpp) and a Python `re` brute force, on every tier, through the hg_* API, Face A and
Face B.  Texts sit at the end of guarded buffers: a read past them faults."""
from __future__ import annotations

import ctypes
import os
import random
import tempfile

import numpy as np
import pytest

import chunk_texts
import somsim_py
from somsim_py import SOM, start_by_brute_force

pytestmark = pytest.mark.gpu

# one set per tier: literal-anchored confirm, byte-window short literals, always-on one word / two words / LDS state words,
# literal-only
TIER_SETS = {
    "anchored": [r"user=[a-z0-9_]{4,12} status=5[0-9]{2}", r"ERROR [0-9]+ failed", r"\bconnection reset\b", r"timeout=\d+ms$"],
    "byte_windows": [r"abc[0-9]+", r"\bxyz\d", r"qr[st]{1,3}u"],
    "always_on_1w": [r"[0-9]+x", r"a.b", r"^[a-c]+"],
    "always_on_2w": [r"([a-f][0-9]){17}", r"[a-f]([0-9][a-f]|_){16}z"],
    "always_on_lds": [r"([a-f][0-9]){40}x"],
    "literal_only": [r"needle-in-hay", r"other-literal-text"],
}
FRAGMENTS = [b"user=abcd_12 status=503", b"ERROR 42 failed", b"connection reset", b"connection resetx", b"timeout=120ms", b"abc123",
             b"xyz9", b"qrstu", b"qrsu", b"12x", b"a-b", b"aab", b"cab", b"a1b2c3d4e5f6" * 8 + b"x", b"e5_f6" * 7 + b"z", b"needle-in-hay",
             b"other-literal-text", b"needle-in-hayneedle-in-hay", b"0", b"\t", b"  ", b"\0", b"zz"]


def make_text(rng: random.Random, nlines: int) -> bytes:
    lines = []
    for _ in range(nlines):
        parts = [rng.choice(FRAGMENTS) if rng.random() < 0.6 else bytes(rng.choice(b"abcdef0123456789 _-x") for _ in range(rng.randint(0, 12)))
                 for _ in range(rng.randint(0, 6))]
        sep = rng.choice([b" ", b"", b"; "])
        lines.append(sep.join(parts))
    return b"\n".join(lines) + (b"\n" if rng.random() < 0.8 else b"")


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(4 << 20)
    yield a
    a.free()


def scan_with_starts(arena, text, pats, flags, ids, bs):
    from hypergrep_amd import device

    db = device.Database(pats, flags=flags, ids=ids)
    sc = device.Scanner(db, 0)
    stats = sc.scan(arena.place(text), len(text), buffer_size=bs)
    return sc.hits_array(), sc.hit_starts(), stats


def check_set(arena, text, pats, flags, ids, bs, brute=True, min_launches=0):
    got, starts, stats = scan_with_starts(arena, text, pats, flags, ids, bs)
    plain, plain_starts, plain_stats = scan_with_starts(arena, text, pats, [f & ~SOM for f in flags], ids, bs)
    assert stats.stream_launches >= min_launches and plain_stats.stream_launches >= min_launches
    assert np.array_equal(got, plain), "the flag changed the reports"
    assert not plain_starts.any(), "a database without SOM reports from = 0"
    assert len(starts) == len(got)
    host = somsim_py.Db(pats, flags, ids)
    assert host.ok(), host.error
    som_ids = {ids[i] for i, f in enumerate(flags) if f & SOM}
    checked = 0
    piece_cache = {}
    for (line_no, rid, to, start, ln), frm in zip(got.tolist(), starts.tolist()):
        line = text[start:start + ln]
        if rid not in som_ids:
            assert frm == 0
            continue
        key = line  # (each distinct piece goes through the host routine once)
        if key not in piece_cache:
            piece_cache[key] = {(r[0], r[1]): r[2] for r in host.piece(line)}
        assert frm == piece_cache[key][(rid, to)], (line, rid, to, frm)
        if brute:
            members = [i for i in range(len(pats)) if ids[i] == rid]
            want = min(s for s in (start_by_brute_force(pats[i], flags[i], line, to) for i in members) if s is not None)
            assert frm == want, (line, rid, to, frm, want)
        checked += 1
    return checked


@pytest.mark.parametrize("tier", sorted(TIER_SETS))
def test_every_tier(arena, tier):
    rng = random.Random(sum(tier.encode()))
    pats = TIER_SETS[tier]
    flags = [6 | SOM] * len(pats)
    ids = list(range(len(pats)))
    total = 0
    for bs in (262140, 40):
        total += check_set(arena, make_text(rng, 400), pats, flags, ids, bs)
    assert total > 20, total


def test_shared_ids_and_mixed_som(arena):
    rng = random.Random(5)
    pats = TIER_SETS["anchored"] + TIER_SETS["always_on_1w"] + TIER_SETS["literal_only"]
    ids = [0, 1, 1, 2, 3, 3, 4, 5, 5]
    flags = [6 | SOM, 6, 6, 6 | SOM, 6 | SOM, 6 | SOM, 6, 6 | SOM, 6 | SOM]
    assert check_set(arena, make_text(rng, 600), pats, flags, ids, 262140) > 20


def test_several_pipeline_chunks_and_segments(arena, monkeypatch):
    # a report limit below the text's reports (the scan is split into segments whose hits, and starts, are put one after the
    # other), and three pipeline chunks (several stream launches)
    from hypergrep_amd import device

    rng = random.Random(8)
    text = make_text(rng, 30000)
    assert len(text) > (1 << 19)
    pats = TIER_SETS["anchored"] + TIER_SETS["always_on_2w"]
    flags = [6 | SOM] * len(pats)
    ids = list(range(len(pats)))
    sc = device.Scanner(device.Database(pats, flags=flags, ids=ids), 0)
    raw = sc.scan(arena.place(text), len(text), buffer_size=1000).n_raw_hits
    assert raw > 4000
    with monkeypatch.context() as m:
        m.setenv("HG_HIT_LIMIT", str(raw * 3 // 4))
        assert check_set(arena, text, pats, flags, ids, 1000, brute=False) > 4000
    # chunks of 1024 tiles (the engine honours no smaller one) on more than 2048 tiles: lines of make_text around the two cuts,
    # a few repeated lines between them
    parts = [[ln + b"\n" for ln in make_text(rng, 1200).rstrip(b"\n").split(b"\n")] for _ in range(4)]
    parts[2].append(b"user=abcd_12 status=503 " + b"q" * 300 + b" ERROR 42 failed; timeout=120ms\n")  # the line across the second cut
    fillers = [b"lorem ipsum dolor " * 45 + b"\n", b"zz user=abcd_12 status=503 " + b"- " * 200 + b"ERROR 42 failed\n", b"0 " * 400 + b"\n",
               b"connection reset " + b"a1b2c3d4e5f6" * 8 + b"x " + b"q " * 250 + b"timeout=120ms\n"]
    big_text = chunk_texts.build(parts, fillers)
    big = device.GuardedArena(chunk_texts.SIZE + 64)
    try:
        with monkeypatch.context() as m:
            for k, v in chunk_texts.CHUNK_ENV.items():
                m.setenv(k, v)
            assert check_set(big, big_text, pats, flags, ids, 1000, brute=False, min_launches=2) > 4000
    finally:
        big.free()


def test_large_synthetic_buffer_sampled(arena):
    import torch

    from hypergrep_amd import benchspec, device

    patterns, needles, hpm = benchspec.c3_spec()
    nbytes = 256 << 20
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    device.synth_device(text.data_ptr(), nbytes, seed=11, needles=needles, hit_per_million=hpm * 20)
    torch.cuda.synchronize()
    flags = [6 | SOM] * len(patterns)
    ids = list(range(len(patterns)))
    db = device.Database(patterns, flags=flags, ids=ids)
    sc = device.Scanner(db, 0)
    sc.scan(text.data_ptr(), nbytes)
    got, starts = sc.hits_array(), sc.hit_starts()
    assert len(got) > 1000
    plain = device.Scanner(device.Database(patterns, flags=[6] * len(patterns), ids=ids), 0)
    plain.scan(text.data_ptr(), nbytes)
    assert np.array_equal(plain.hits_array(), got)
    rng = random.Random(3)
    for k in rng.sample(range(len(got)), 300):
        _, rid, to, start, ln = (int(v) for v in got[k])
        line = bytes(text[start:start + ln].cpu().numpy())
        assert int(starts[k]) == start_by_brute_force(patterns[rid], flags[rid], line, to), (line, patterns[rid], to)
    del text
    torch.cuda.empty_cache()


MATCH_EVENT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_void_p)


def face_a(pats, flags, data):
    from hypergrep_amd import utils

    # a handle of our own: other tests declare argtypes on the shared one
    lib = ctypes.CDLL(utils._get_hyperscanner_lib()._name)  # pylint: disable=protected-access
    n = len(pats)
    db, err = ctypes.c_void_p(), ctypes.c_void_p()
    rc = lib.hs_compile_multi((ctypes.c_char_p * n)(*[p.encode() for p in pats]), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*range(n)), n, 1, None,
                              ctypes.byref(db), ctypes.byref(err))
    if rc != 0:
        lib.hs_free_compile_error(err)
        return rc, None
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


def test_face_a_block_mode():
    pats = [r"\bfoo[0-9]+", r"b+ar", r"needle-in-hay", r"([a-f][0-9]){17}"]
    flags = [6 | SOM, 6 | SOM, 2 | SOM, 6]
    for data in (b"xfoo12 foo3 bbbar bar needle-in-hay\nfoo9", b"a1b2c3d4e5f6" * 4 + b"\0 bbar foo1"):
        rc, got = face_a(pats, flags, data)
        assert rc == 0
        want = []
        for rid, pat in enumerate(pats):
            for to in range(1, len(data) + 1):
                s = start_by_brute_force(pat, flags[rid], data, to)
                if s is not None:
                    want.append((rid, s if flags[rid] & SOM else 0, to))
        assert sorted(got, key=lambda r: (r[2], r[0])) == sorted(want, key=lambda r: (r[2], r[0]))
        assert [r[2] for r in got] == sorted(r[2] for r in got)  # delivered by ascending end offset
    assert face_a(["foobar"], [SOM | 8], b"foobar")[0] == -4  # HS_COMPILER_ERROR


def test_face_b_results_are_unchanged_by_the_flag():
    import hypergrep_amd

    rng = random.Random(21)
    pats = TIER_SETS["anchored"] + TIER_SETS["byte_windows"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "f.log")
        with open(path, "wb") as f:
            f.write(make_text(rng, 3000))
        runs = []
        for flags in ([6] * len(pats), [6 | SOM] * len(pats)):
            rows = []

            def on_match(matches, n, rows=rows):
                rows.extend((matches[k].line_number, matches[k].id, matches[k].line) for k in range(n))

            assert hypergrep_amd.scan(path, pats, on_match, flags=flags, ids=list(range(len(pats)))) == 0
            runs.append(rows)
        assert runs[0] == runs[1] and len(runs[0]) > 100
