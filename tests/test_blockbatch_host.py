"""The batched block scan on the host (no GPU): hg_scan_blocks is declared and exported, device.BlockDatabase compiles what
block mode compiles, and a replay of hg_batch.h (tests/native/batchsim.cpp: the packing, the shard / round / team / slice walk
of hg_block_batch_kernel, the per-item report rules) over random shard and lane counts equals hg_nfa_scan on every item
alone and, on assertion-free expressions, the ends Python `re` finds in that item's bytes."""
from __future__ import annotations

import ctypes
import os
import random
import re

import pytest

import accept_rules
import batchsim_py
import regex_gen
from hypergrep_amd import device

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSERTION_CHARS = ("^", "$", "\\b", "\\B", "\\A", "\\z", "\\Z")
# the four sets of tests/test_streammode_gpu.py's SETS (the replay compiles no extended parameters: the fourth without them)
SETS = {
    "one_word": (["foo", r"\bbar\b", "ba+z$", "qu[xy]", r"o\n", r"^x"], [0, 0, 0, 1, 0, 4]),
    "multi_word": (["a[a-f]{40}b", "(ab|cd){12}e", "x[a-z ]{900}y", r"\bfo[a-z]{50}\b"], [0, 2, 2, 0]),
    "literal": (["hello world", "status=5[0-9][0-9]", "foobar", "xyzzy"], [8, 0, 1 | 8, 0]),
    "caseless": (["foobar", "abcdef", "zebra"], [1, 0, 1 | 8]),
}
FIXED_LENGTHS = [0, 1, 15, 16, 17, 2047, 2048, 8191, 8192]
NEEDLES = [b"foo", b"bar", b"baz\n", b"baz", b"qux", b"hello world", b"status=512", b"FooBar", b"xyzzy", b"zebra", b"abcdef", b"abab" * 6 + b"e", b"o\n", b"\nx"]


def test_header_declares_and_library_exports_hg_scan_blocks():
    text = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^int\s+hg_scan_blocks\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    assert hasattr(lib, "hg_scan_blocks")
    assert device.face_a().hg_scan_blocks.argtypes is not None


def test_n_zero_and_argument_errors_need_no_gpu():
    l = device.face_a()
    assert l.hg_scan_blocks(None, None, None, 0, None, device.STREAM_EVENT(), None) == device.HS_SUCCESS
    h, err = device.hs_compile(["foo"], flags=[0], mode=device.HS_MODE_BLOCK)
    assert err is None
    lengths = (ctypes.c_uint * 1)(3)
    datas = (ctypes.c_char_p * 1)(b"foo")
    assert l.hg_scan_blocks(h, datas, lengths, 1, None, device.STREAM_EVENT(), None) == device.HS_INVALID
    assert l.hg_scan_blocks(None, datas, lengths, 1, None, device.STREAM_EVENT(), None) == device.HS_INVALID
    l.hs_free_database(h)


def test_block_database_class_rejects_what_block_mode_rejects():
    assert hasattr(device, "BlockDatabase")
    with pytest.raises(device.CompileError):
        device.BlockDatabase(["(?<!foo)bar"], [0], [1])  # lookbehind: unsupported
    with pytest.raises(device.CompileError):
        device.BlockDatabase(["a*"], [0], [1])  # matches the empty buffer
    with pytest.raises(device.CompileError):
        device.BlockDatabase(["foo"], [device.HS_FLAG_SOM_LEFTMOST | 8], [1])  # SOM with SINGLEMATCH
    with pytest.raises(ValueError):
        device.BlockDatabase(["foo", "bar"], [0], [1, 2])  # one flag for two expressions


def _rules(raw, ids, single):
    """hs_scan's report rules restated: one SINGLEMATCH report per id (the smallest `to`), an identical (id, to) once;
    delivery order (to, id)."""
    reps = sorted((ids[e], t, single[e]) for e, t in raw)
    out, seen_single = [], set()
    for k, (i, t, sg) in enumerate(reps):
        dup = k > 0 and reps[k - 1][:2] == (i, t)
        if not dup and not (sg and i in seen_single):
            out.append((i, t))
        if sg:
            seen_single.add(i)
    return sorted(out, key=lambda r: (r[1], r[0]))


def _text(rng, n, alphabet=b"abcdefoxyz \n\0"):
    parts, size = [], 0
    while size < n:
        p = bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 40))) if rng.random() < 0.7 else rng.choice(NEEDLES)
        parts.append(p)
        size += len(p)
    return b"".join(parts)[:n]


def _items(rng, lengths):
    items = []
    for n in lengths:
        d = _text(rng, n)
        if n and rng.random() < 0.3:
            d = d[:-1] + b"\n"  # '\n' as the last byte
        if n > 4 and rng.random() < 0.3:
            d = d[:n // 2] + b"\0\n" + d[n // 2 + 2:]  # NUL and '\n' inside
        items.append(d)
        if rng.random() < 0.2:
            items.append(d)  # identical neighbours
    return items


def _check(db, items, ids, single, lanes, ppw, nshards):
    got = db.run(items, lanes=lanes, ppw=ppw, nshards=nshards)
    assert len(got) == len(items)
    for i, d in enumerate(items):
        want = _rules(db.block(d), ids, single) if d else []
        assert got[i] == want, (i, len(d), lanes, ppw, nshards, got[i][:8], want[:8])


@pytest.mark.parametrize("name", sorted(SETS))
def test_replay_fixed_sets_and_lengths(name):
    pats, flags = SETS[name]
    ids = [10 + i for i in range(len(pats))]
    db = batchsim_py.Db(pats, flags, ids)
    assert db.h, db.error
    single = [bool(f & 8) for f in flags]
    rng = random.Random(len(name) * 977)
    ran = 0
    for lanes, ppw, nshards in [(256, 32, 1), (256, 32, 7), (64, 2, 3), (16, 32, 2), (128, 1, 40)]:
        lengths = FIXED_LENGTHS + [rng.randint(1, 300) for _ in range(12)] + [rng.randint(1, 8192) for _ in range(3)]
        rng.shuffle(lengths)
        _check(db, _items(rng, lengths), ids, single, lanes, ppw, nshards)
        ran += 1
    assert ran == 5


def _compiled_random_set(rng, k):
    """k generated expressions that compile; a rejected one is replaced by the next generated one."""
    pats, flags = [], []
    while len(pats) < k:
        p, f = regex_gen.random_pattern(rng), rng.choice([0, 2, 4, 6, 1, 5]) | (8 if rng.random() < 0.3 else 0)
        one = batchsim_py.Db([p], [f])
        if accept_rules.Tally().decide([p], [f], bool(one.h), one.error, features=True):
            pats.append(p)
            flags.append(f)
    return pats, flags


def test_replay_random_sets_match_block_scan():
    rng = random.Random(4242)
    cases, ran = 120, 0
    for _ in range(cases):
        pats, flags = _compiled_random_set(rng, rng.choice([1, 3, 4, 9, 40]))
        ids = [rng.choice([1, 1, 2, 3, 4]) for _ in pats]
        db = batchsim_py.Db(pats, flags, ids)
        assert db.h, (pats, db.error)
        single = [bool(f & 8) for f in flags]
        lengths = [rng.choice(FIXED_LENGTHS[:5]) for _ in range(4)] + [rng.randint(1, 200) for _ in range(20)]
        if rng.random() < 0.15:
            lengths += [rng.choice(FIXED_LENGTHS[5:])]
        rng.shuffle(lengths)
        items = [regex_gen.random_text(rng, max(1, n // 10), maxlen=12, final_newline=rng.random() < 0.5)[:n] if n else b"" for n in lengths]
        items += items[:2]
        _check(db, items, ids, single, lanes=rng.choice([16, 32, 64, 256]), ppw=rng.choice([1, 2, 5, 32]), nshards=rng.randint(1, 12))
        ran += 1
    assert ran == cases


def test_replay_groups_of_256_expressions():
    """The grouping of sets above 2048 expressions: up to 256 expressions per workgroup, an item's expressions in passes."""
    rng = random.Random(31)
    words = ["k%03dz" % i for i in range(296)]
    pats = words + ["foo", r"\bbar\b", "ba+z$", r"o\n"]
    flags = [0] * 296 + [0, 0, 0, 8]
    ids = list(range(len(pats)))
    db = batchsim_py.Db(pats, flags, ids)
    assert db.h, db.error
    single = [bool(f & 8) for f in flags]
    ran = 0
    for nshards in (1, 3, 17):
        items = []
        for n in FIXED_LENGTHS + [rng.randint(1, 300) for _ in range(20)]:
            d = bytearray(_text(rng, n))
            for _ in range(n // 40):
                w = rng.choice(words).encode()
                at = rng.randint(0, n - len(w))
                d[at:at + len(w)] = w
            items.append(bytes(d))
        rng.shuffle(items)
        _check(db, items, ids, single, lanes=256, ppw=256, nshards=nshards)
        ran += 1
    assert ran == 3


def test_replay_matches_python_re_on_assertion_free_expressions():
    rng = random.Random(77)
    tally = accept_rules.Tally()
    cases, ran = 60, 0
    while ran < cases:
        pat = regex_gen.random_pattern(rng)
        flags = rng.choice([0, 2, 4, 6])
        if any(a in pat for a in ASSERTION_CHARS):
            continue  # (not a case: the subset is the assertion-free expressions; replaced by the next one)
        db = batchsim_py.Db([pat], [flags])
        if not tally.decide([pat], [flags], bool(db.h), db.error, features=True):
            continue  # (rejected by both compilers, or by a documented limit: replaced by the next generated expression)
        items = [regex_gen.random_text(rng, rng.randint(1, 3), maxlen=8, final_newline=rng.random() < 0.5) for _ in range(rng.randint(1, 3))]
        items.insert(rng.randint(0, len(items)), b"")
        got = db.run(items, lanes=rng.choice([16, 64, 256]), ppw=32, nshards=rng.randint(1, 5))
        for d, g in zip(items, got):
            want = regex_gen.ends_by_brute_force(pat, flags, d) if d else []
            assert [t for _, t in g] == want, (pat, flags, d, g, want)
        ran += 1
    assert ran == cases


def test_geometry_fills_lanes_for_few_expressions_and_short_items():
    """Four expressions on 64-byte items: eight items per round, every lane of the workgroup with a slice of its own."""
    import subprocess
    import sys
    code = r'''
#include "hypergrep_amd/csrc/hg_batch.h"
#include <cstdio>
int main() {
  uint32_t lens[16]; for (auto &l : lens) l = 64;
  uint32_t ts; const uint32_t taken = hg_batch_round(lens, 16, 4, 256, &ts);
  const HgBatchGeom g = hg_batch_geom(4, 64, ts, 256 / ts);
  const HgBatchGeom big = hg_batch_geom(32, 8192, 256, 1);
  std::printf("%u %u %u %u %u %u %u %u\n", ts, taken, g.epp, g.nslices, g.passes, big.epp, big.passes, big.nslices);
}
'''
    exe = os.path.join(REPO, "tests", "native", f"batchgeom.{os.getpid()}.tmp")
    try:
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", REPO, "-x", "c++", "-", "-o", exe], input=code, text=True, check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    assert [int(x) for x in out] == [32, 8, 4, 8, 1, 16, 2, 16], out
