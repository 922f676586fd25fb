"""Approximate matching (hs_expr_ext_t edit_distance / hamming_distance) on the MI355X: every tier, SINGLEMATCH, pieces,
start of match, Face A and Face B, against the pure-Python reference tests/approx_ref.py.  Texts sit at the end of guarded
buffers: a read past them faults."""
from __future__ import annotations

import ctypes
import os
import random
import tempfile

import pytest

import approx_ref
import somsim_py
from extsim_py import ext

pytestmark = pytest.mark.gpu

SOM, SINGLE = 256, 8

# one set per tier: pigeonhole-anchored, byte windows, always-on one word / two words / LDS state words, huge tables
TIER_SETS = {
    "anchored": (["ERR_DISK_FULL_[0-9]{3}", "connection reset by peer", "user=[a-z]{4} status=5[0-9]{2}"], [ext(edit=1), ext(edit=2), ext(hamming=1)]),
    "byte_windows": (["timeout=[0-9]+", "abcdefgh"], [ext(edit=1), ext(hamming=1)]),
    "always_on_1w": (["abcde", "^xyz1"], [ext(edit=1), ext(edit=1)]),
    "always_on_2w": (["[a-f]{4}x[0-9]{4}"], [ext(edit=1)]),
    "always_on_lds": (["([a-f][0-9]){12}"], [ext(edit=2)]),
    "huge": (["[a-f0-9]{400}z"], [ext(edit=1)]),
}
FRAGMENTS = [b"ERR_DISK_FULL_123", b"ERR_DISC_FULL_12", b"ERRDISK_FULL_999", b"connection reste by peer", b"conection reset by per",
             b"user=abcd status=503", b"usr=abcd status=50x", b"timeout=120", b"timout=9", b"abcdefgh", b"abcxefgh", b"abde", b"abxde",
             b"xyz1", b"xy1", b"abcdx1234", b"abcx12345", b"a1b2c3d4e5f6a1b2c3d4e5f6", b"a1b2c3d4e5f6a1b2c3dd4e5f6", b"\0", b"  ", b"zz", b"\t"]


def make_text(rng: random.Random, nlines: int, huge: bool = False) -> bytes:
    lines = []
    for _ in range(nlines):
        parts = [rng.choice(FRAGMENTS) if rng.random() < 0.6 else bytes(rng.choice(b"abcdef0123456789 _-x") for _ in range(rng.randint(0, 12)))
                 for _ in range(rng.randint(0, 6))]
        if huge and rng.random() < 0.3:
            body = bytearray(rng.choice(b"abcdef0123456789") for _ in range(400))
            if rng.random() < 0.5:
                body[rng.randrange(400)] = ord("-")
            parts.append(bytes(body) + b"z")
        lines.append(rng.choice([b" ", b"", b"; "]).join(parts))
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


def refs_of(pats, flags, exts):
    def one(p, f, x):
        if x is None:
            return approx_ref.Approx(p, f)
        return approx_ref.Approx(p, f, edit=x.edit_distance, hamming=x.hamming_distance, min_offset=x.min_offset if x.flags & 1 else 0,
                                 max_offset=x.max_offset if x.flags & 2 else None)

    return [one(p, f, x) for p, f, x in zip(pats, flags, exts)]


def expected(text, pats, flags, exts, bs, starts=False):
    refs = refs_of(pats, flags, exts)
    out = []
    for idx, _a, piece in somsim_py.pieces(text, bs):
        if not piece:
            continue
        for rid, to in approx_ref.piece_reports(list(zip(refs, range(len(pats)))), piece):
            out.append((idx, rid, to, refs[rid].start(piece, to) if starts and flags[rid] & SOM else 0))
    return sorted(out)


def gpu_hits(arena, text, pats, flags, exts, bs, starts=False):
    from hypergrep_amd import device

    db = device.Database(pats, flags=flags, ids=list(range(len(pats))), ext=exts)
    sc = device.Scanner(db, 0)
    sc.scan(arena.place(text), len(text), buffer_size=bs)
    hits = sc.hits()
    froms = list(sc.hit_starts()) if starts else [0] * len(hits)
    return sorted((h[0], h[1], h[2], int(f)) for h, f in zip(hits, froms)), db.info()


@pytest.mark.parametrize("tier", list(TIER_SETS))
def test_every_tier(arena, tier):
    pats, exts = TIER_SETS[tier]
    rng = random.Random(tier)
    text = make_text(rng, 80 if tier == "huge" else 1500, huge=tier == "huge")
    for flags in ([0] * len(pats), [SINGLE] * len(pats), [1 | 2] * len(pats)):
        got, info = gpu_hits(arena, text, pats, flags, exts, 262140)
        assert got == expected(text, pats, flags, exts, 262140), (tier, flags)
        assert len(got) > 10
        if tier == "anchored":
            assert info["n_literal_anchored"] == len(pats)
        elif tier == "byte_windows":  # 4-byte pieces: the stream pass probes a window at every byte offset
            assert info["n_literal_anchored"] == len(pats) and info["byte_windows"] == 1
        elif tier.startswith("always_on") or tier == "huge":
            assert info["n_always_on"] == len(pats)


def test_pieces_and_mixed_sets(arena):
    rng = random.Random(3)
    pats = TIER_SETS["anchored"][0] + TIER_SETS["always_on_1w"][0] + ["needle-in-hay", "xyz1"]
    exts = TIER_SETS["anchored"][1] + TIER_SETS["always_on_1w"][1] + [None, None]
    text = make_text(rng, 1200)
    for bs in (17, 100):
        flags = [rng.choice([0, SINGLE, 4]) for _ in pats]
        got, _ = gpu_hits(arena, text, pats, flags, exts, bs)
        assert got == expected(text, pats, flags, exts, bs), bs


# offset bounds on every tier: a SINGLEMATCH expression's first end below min_offset must not hide a later end that qualifies
BOUNDED = (["ERR_DISK_FULL_[0-9]{3}", "abcde", "abcde", "[0-9]+x", "([a-f][0-9]){12}", "timeout=[0-9]+", "needle-in-hay"],
           [ext(edit=1, min_offset=25), ext(min_offset=12, max_offset=60), ext(edit=1, min_offset=9), ext(min_offset=6, max_offset=40),
            ext(edit=2, min_offset=30), ext(max_offset=14), ext(max_offset=30)])


def test_offset_bounds_every_tier(arena):
    rng = random.Random(7)
    pats, exts = BOUNDED
    text = make_text(rng, 1500)
    for flags in ([SINGLE] * len(pats), [0] * len(pats), [SINGLE | 1 | 2] * len(pats)):
        got, info = gpu_hits(arena, text, pats, flags, exts, 262140)
        want = expected(text, pats, flags, exts, 262140)
        assert got == want, flags
        assert len(want) > 50 and info["n_literal_anchored"] >= 3 and info["n_always_on"] >= 2
    # the first end of many lines is out of bounds: SINGLEMATCH delivers a later one there
    refs = refs_of(pats, [SINGLE] * len(pats), exts)
    later = sum(1 for _i, _a, piece in somsim_py.pieces(text, 262140) for r in refs if r.ends(piece) and r.reports(piece)[:1] != r.ends(piece)[:1])
    assert later > 20


def test_offset_bounds_huge(arena):
    rng = random.Random(8)
    pats, exts = ["[a-f0-9]{400}z", "[a-f0-9]{400}z"], [ext(edit=1, min_offset=420), ext(max_offset=405)]
    text = make_text(rng, 80, huge=True)
    for flags in ([SINGLE, SINGLE], [0, 0]):
        got, _ = gpu_hits(arena, text, pats, flags, exts, 262140)
        assert got == expected(text, pats, flags, exts, 262140)


def test_max_offset_on_split_lines(arena):
    rng = random.Random(9)
    pats, exts = BOUNDED
    text = make_text(rng, 1000)
    for bs in (17, 40):
        flags = [rng.choice([0, SINGLE, 4]) for _ in pats]
        got, _ = gpu_hits(arena, text, pats, flags, exts, bs)
        assert got == expected(text, pats, flags, exts, bs), bs


def test_start_of_match(arena):
    rng = random.Random(4)
    pats = ["ERR_DISK_FULL_[0-9]{3}", "abcde", "^xyz1", "timeout=[0-9]+"]
    exts = [ext(edit=2), ext(edit=1), ext(edit=1), ext(hamming=1)]
    flags = [SOM] * 4
    text = make_text(rng, 800)
    got, _ = gpu_hits(arena, text, pats, flags, exts, 262140, starts=True)
    assert got == expected(text, pats, flags, exts, 262140, starts=True)
    assert any(f for *_, f in got)


MATCH_EVENT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_void_p)


def face_a(pats, flags, exts, data):
    from hypergrep_amd import utils

    lib = ctypes.CDLL(utils._get_hyperscanner_lib()._name)  # pylint: disable=protected-access
    n = len(pats)
    db, err = ctypes.c_void_p(), ctypes.c_void_p()
    rc = lib.hs_compile_ext_multi((ctypes.c_char_p * n)(*[p.encode() for p in pats]), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*range(n)),
                                  utils.ext_array(exts, n), n, 1, None, ctypes.byref(db), ctypes.byref(err))
    assert rc == 0
    scratch = ctypes.c_void_p()
    assert lib.hs_alloc_scratch(db, ctypes.byref(scratch)) == 0
    out = []

    @MATCH_EVENT
    def on_match(rid, frm, to, _flags, _ctx):
        out.append((rid, to))
        return 0

    rc = lib.hs_scan(db, data, len(data), 0, scratch, on_match, None)
    lib.hs_free_scratch(scratch)
    lib.hs_free_database(db)
    assert rc == 0
    return sorted(out)


def test_face_a_small_block_and_general_path():
    rng = random.Random(5)
    pats, exts = ["ERR_DISK_FULL_[0-9]{3}", "abcde", "[a-f]{4}x[0-9]{4}"], [ext(edit=1), ext(edit=1), ext(hamming=2)]
    flags = [0, 0, 0]
    refs = refs_of(pats, flags, exts)
    for nbytes in (200, 3000, 200000):  # a small block and larger ones
        data = make_text(rng, nbytes // 20)[:nbytes].replace(b"\0", b"-")
        want = sorted((rid, t) for rid, r in enumerate(refs) for t in r.ends(data))
        assert face_a(pats, flags, exts, data) == want, nbytes
    # offset bounds (such databases take the general path for every block size)
    pats, exts = BOUNDED
    flags = [SINGLE, 0, SINGLE, 0, SINGLE, 0, SINGLE]
    refs = refs_of(pats, flags, exts)
    for nbytes in (200, 3000):
        data = make_text(rng, nbytes // 20)[:nbytes].replace(b"\0", b"-")
        want = sorted((rid, t) for rid, r in enumerate(refs) for t in r.reports(data))
        assert face_a(pats, flags, exts, data) == want, nbytes


def test_face_b_scan_with_and_without_ext():
    import hypergrep_amd

    rng = random.Random(6)
    pats = ["ERR_DISK_FULL_[0-9]{3}", "abcde"]
    exts = [hypergrep_amd.ExprExt(flags=hypergrep_amd.HS_EXT_FLAG_EDIT_DISTANCE, edit_distance=1), None]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "f.log")
        text = make_text(rng, 3000)
        with open(path, "wb") as f:
            f.write(text)
        runs = []
        for e in (exts, None, exts):
            rows = []

            def on_match(matches, n, rows=rows):
                rows.extend((matches[k].line_number, matches[k].id) for k in range(n))

            assert hypergrep_amd.scan(path, pats, on_match, flags=[6, 6], ids=[0, 1], ext=e) == 0
            runs.append(sorted(set(rows)))
    for e, rows in zip((exts, None, exts), runs):
        want = set()
        for idx, _a, piece in somsim_py.pieces(text, 262140):
            for rid, to in approx_ref.piece_reports(list(zip(refs_of(pats, [6, 6], e or [None, None]), range(2))), piece):
                want.add((idx, rid))
        assert rows == sorted(want)
    assert runs[0] == runs[2] and runs[0] != runs[1]  # the cached database of one set is not used for the other
