"""min_length (hs_expr_ext_t) on the MI355X: the match-length pass (hg_minlen_kernel, hg_som.hip) on every tier that can
hold a variable-width expression, through the hg_* API, Face A and Face B.  Every expectation is a Python `re` brute force
(minlensim_py.expected_piece): an end t stays iff a start s with t - s >= min_length exists, then the report rules.  Texts
sit at the end of guarded buffers: a read past them faults."""
from __future__ import annotations

import os
import random
import subprocess
import sys
import tempfile

import pytest

import chunk_texts
import somsim_py
from minlensim_py import COMBINATION, QUIET, SINGLE, SOM, expected_piece, exts_for

pytestmark = pytest.mark.gpu

# one set per tier that can hold a variable-width expression: (expression, min_length) pairs.  Every min_length lies above the
# shortest and at most at the longest match, so it removes some reports and keeps others.
TIER_SETS = {
    "anchored": [(r"user=[a-z0-9_]{4,12} status=5[0-9]{2}", 24), (r"ERROR [0-9]+ failed", 17), (r"timeout=\d+ms$", 13)],
    "byte_windows": [(r"abc[0-9]+", 6), (r"qrs[tu]{1,3}v", 6), (r"\bxyz\d+", 6)],
    "always_on_1w": [(r"[0-9]+x", 4), (r"^[a-c]+", 3), (r"a.?b", 3)],
    "always_on_2w": [(r"([a-f][0-9]){17,20}", 38)],
    "always_on_lds": [(r"([a-f][0-9]){40,44}x", 85)],
}
UNFILTERED = ["needle-in-hay", r"zz+"]  # mixed into every set, without parameters
TIER_FRAGMENTS = {
    "anchored": [b"user=abcd status=503", b"user=abcdefgh_12 status=599", b"user=abcdefgh status=500", b"ERROR 4 failed", b"ERROR 123456 failed",
                 b"ERROR 1234 failed", b"timeout=5ms", b"timeout=12345ms", b"timeout=123ms"],
    "byte_windows": [b"abc1", b"abc12345", b"abc123", b"qrstv", b"qrstuv", b"qrstutv", b"xyz1", b"xyz12345", b"_xyz123456", b"xyz123"],
    "always_on_1w": [b"1x", b"12345x", b"123x", b"ab", b"abcab", b"cab", b"axb", b"a-b", b"bca"],
    "always_on_2w": [b"a1" * 17, b"a1b2" * 10, b"c3" * 19, b"e5f6" * 9, b"d4" * 25],
    "always_on_lds": [b"a1" * 40 + b"x", b"e5" * 44 + b"x", b"a1b2" * 21 + b"x", b"c3" * 43 + b"x", b"f0" * 50 + b"x"],
}
COMMON = [b"needle-in-hay", b"zz", b"zzzz", b"\0", b"  ", b"-", b"0", b"q", b"\t"]


def line_pool(rng: random.Random, tiers, n: int = 40):
    frags = [f for t in tiers for f in TIER_FRAGMENTS[t]]
    pool = []
    for _ in range(n):
        parts = [rng.choice(frags) if rng.random() < 0.65 else rng.choice(COMMON) for _ in range(rng.randint(0, 4))]
        pool.append(rng.choice([b" ", b"", b"; "]).join(parts))
    return pool


def make_text(rng: random.Random, pool, nlines: int) -> bytes:
    """Lines drawn from a pool of distinct ones: the brute force runs once per distinct piece."""
    return b"\n".join(rng.choice(pool) for _ in range(nlines)) + (b"\n" if rng.random() < 0.8 else b"")


def tier_set(tiers):
    pats = [p for t in tiers for p, _ in TIER_SETS[t]] + UNFILTERED
    need = [v for t in tiers for _, v in TIER_SETS[t]] + [None] * len(UNFILTERED)
    return pats, need


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(8 << 20)
    yield a
    a.free()


_EXPECT_CACHE: dict = {}


def piece_reports(pats, flags, ids, need, piece):
    key = (tuple(pats), tuple(flags), tuple(ids), tuple(need), piece)
    if key not in _EXPECT_CACHE:
        _EXPECT_CACHE[key] = expected_piece(pats, flags, ids, need, piece)
    return _EXPECT_CACHE[key]


def expected(text, pats, flags, ids, need, bs):
    """[(line, id, to, from)] in (line, id, to) order"""
    out = []
    for idx, _a, piece in somsim_py.pieces(text, bs):
        if piece:
            out.extend((idx, rid, to, frm) for rid, to, frm in piece_reports(pats, flags, ids, need, piece))
    return out


def gpu_hits(arena, text, pats, flags, ids, need, bs):
    from hypergrep_amd import device

    db = device.Database(pats, flags=flags, ids=ids, ext=exts_for(need) if need is not None else None)
    sc = device.Scanner(db, 0)
    stats = sc.scan(arena.place(text), len(text), buffer_size=bs)
    return [(h[0], h[1], h[2], int(f)) for h, f in zip(sc.hits(), sc.hit_starts())], stats


def check(arena, text, pats, flags, ids, need, bs):
    """The GPU's reports equal the brute force; returns (delivered, delivered without the parameter)."""
    got, stats = gpu_hits(arena, text, pats, flags, ids, need, bs)
    want = expected(text, pats, flags, ids, need, bs)
    assert got == want, (pats, flags, need, bs)
    plain = expected(text, pats, flags, ids, [None] * len(pats), bs)
    assert stats.n_raw_hits >= len(plain) - sum(1 for f in flags if f & COMBINATION)  # (n_raw_hits: reports before the filter)
    return len(want), len(plain)


@pytest.mark.parametrize("tier", sorted(TIER_SETS))
def test_every_tier(arena, tier):
    from hypergrep_amd import device

    rng = random.Random(sum(tier.encode()))
    pats, need = tier_set([tier])
    nf = len(TIER_SETS[tier])
    info = device.Database(pats[:nf], flags=[6] * nf, ids=list(range(nf)), ext=exts_for(need[:nf])).info()
    if tier == "anchored":
        assert info["n_literal_anchored"] == nf and info["byte_windows"] == 0
    elif tier == "byte_windows":
        assert info["n_literal_anchored"] == nf and info["byte_windows"] != 0
    else:
        assert info["n_always_on"] == nf
        words = info["max_state_words"]
        assert (words == 1) if tier == "always_on_1w" else (words == 2) if tier == "always_on_2w" else (words > 2)
    text = make_text(rng, line_pool(rng, [tier]), 500)
    ids = list(range(len(pats)))
    for flags, bs in (([6] * len(pats), 262140), ([6] * len(pats), 40), ([6 | SINGLE] * len(pats), 262140)):
        kept, before = check(arena, text, pats, flags, ids, need, bs)
        # some reports go and some stay (pieces of 39 bytes hold no match of the long expressions at all: nothing to remove there)
        assert 20 < kept <= before and (kept < before or bs == 40), (tier, bs, kept, before)


def test_singlematch_and_shared_ids(arena):
    # SINGLEMATCH: the smallest end that passes; two expressions on one id with different lengths
    rng = random.Random(11)
    pats = [r"abc[0-9]+", r"abc[0-9]{2,}", r"[0-9]+x", r"ERROR [0-9]+ failed", "needle-in-hay", r"a.?b"]
    need = [6, 8, 4, 17, None, 3]
    ids = [1, 1, 2, 3, 3, 4]
    text = make_text(rng, line_pool(rng, ["anchored", "byte_windows", "always_on_1w"]), 600)
    for flags in ([6 | SINGLE] * 6, [6, 6 | SINGLE, 6, 6 | SINGLE, 6, 6], [6] * 6):
        for bs in (262140, 33):
            kept, before = check(arena, text, pats, flags, ids, need, bs)
            assert 20 < kept < before


def test_start_of_match_with_min_length(arena):
    # `from` through hit_starts(): unchanged alone on an id; on a shared id the smallest start over the surviving expressions
    rng = random.Random(12)
    pats = [r"abc[0-9]+", r"[a-c]+[0-9]+", r"[0-9]+x", r"user=[a-z0-9_]{4,12} status=5[0-9]{2}", r"zz+"]
    need = [None, 9, 4, 24, None]
    ids = [1, 1, 2, 3, 4]
    flags = [6 | SOM, 6 | SOM, 6 | SOM, 6 | SOM, 6]
    pool = line_pool(rng, ["anchored", "byte_windows", "always_on_1w"]) + [b"cababc12 x", b"zz bcabc1234567", b"ab;cabc1"]
    text = make_text(rng, pool, 600)
    for bs in (262140, 50):
        got, _ = gpu_hits(arena, text, pats, flags, ids, need, bs)
        assert got == expected(text, pats, flags, ids, need, bs), bs
        assert sum(1 for r in got if r[3]) > 20
    # the filter changes starts on the shared id: somewhere the longer expression starts further left but is too short
    loose = expected(text, pats, flags, ids, [None] * 5, 262140)
    tight = {(r[0], r[1], r[2]): r[3] for r in expected(text, pats, flags, ids, need, 262140)}
    assert any(r[1] == 1 and (r[0], r[1], r[2]) in tight and tight[(r[0], r[1], r[2])] > r[3] for r in loose)


def test_combinations_and_quiet_see_surviving_reports_only(arena):
    rng = random.Random(13)
    pats = [r"abc[0-9]+", r"[0-9]+x", r"ERROR [0-9]+ failed", "needle-in-hay", "1 & !2", "3 & 4", "2 | 3"]
    need = [6, 4, 17, None, None, None, None]
    ids = [1, 2, 3, 4, 100, 101, 102]
    flags = [6, 6 | QUIET, 6 | QUIET, 6, COMBINATION, COMBINATION | SINGLE, COMBINATION]
    text = make_text(rng, line_pool(rng, ["anchored", "byte_windows", "always_on_1w"]), 600)
    for bs in (262140, 60):
        got, _ = gpu_hits(arena, text, pats, flags, ids, need, bs)
        want = expected(text, pats, flags, ids, need, bs)
        assert got == want, bs
        assert got != expected(text, pats, flags, ids, [None] * len(pats), bs)
        assert sum(1 for r in got if r[1] >= 100) > 20 and not any(r[1] in (2, 3) for r in got)


def test_many_lines_pipeline_chunks_and_segments(arena, monkeypatch):
    # a report limit below the text's reports: the scan is split into segments, each of which filters its own raw reports
    # before its finalize; and three pipeline chunks (several stream launches)
    from hypergrep_amd import device

    rng = random.Random(14)
    pats, need = tier_set(["anchored", "byte_windows", "always_on_1w", "always_on_2w"])
    ids = list(range(len(pats)))
    flags = [6] * len(pats)
    text = make_text(rng, line_pool(rng, ["anchored", "byte_windows", "always_on_1w", "always_on_2w"], 60), 60000)
    assert len(text) > (1 << 20)
    sc = device.Scanner(device.Database(pats, flags=flags, ids=ids, ext=exts_for(need)), 0)
    raw = sc.scan(arena.place(text), len(text), buffer_size=1000).n_raw_hits
    want = expected(text, pats, flags, ids, need, 1000)
    assert raw > len(want) > 4000
    for env in ({"HG_HIT_LIMIT": str(raw * 3 // 4)}, {"HG_HIT_LIMIT": str(raw // 3)}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got, stats = gpu_hits(arena, text, pats, flags, ids, need, 1000)
            assert got == want, env
            assert stats.n_raw_hits >= raw  # (segments overlap: a piece's reports may be counted by two passes before they are dropped)
    # chunks of 1024 tiles (the engine honours no smaller one) on more than 2048 tiles: lines of the pool around the two cuts, a
    # few repeated lines between them
    pool = line_pool(rng, ["anchored", "byte_windows", "always_on_1w", "always_on_2w"], 60)
    parts = [[ln + b"\n" for ln in make_text(rng, pool, 1500).rstrip(b"\n").split(b"\n")] for _ in range(4)]
    parts[2].append(b"abc12345 ERROR 4 failed " + b"q" * 300 + b" user=abcdefgh_12 status=599 timeout=12345ms\n")  # the line across the second cut
    fillers = [b"lorem ipsum dolor " * 45 + b"\n", b"zz needle-in-hay abc1 abc12345 " + b"lorem " * 140 + b"\n", b"- " * 300 + b"\n",
               b"ERROR 1234 failed; 12345x " + b"q " * 300 + b"timeout=123ms\n"]
    big_text = chunk_texts.build(parts, fillers)
    big = device.GuardedArena(chunk_texts.SIZE + 64)
    try:
        raw = gpu_hits(big, big_text, pats, flags, ids, need, 1000)[1].n_raw_hits
        want = expected(big_text, pats, flags, ids, need, 1000)
        assert raw > len(want) > 4000
        with monkeypatch.context() as m:
            for k, v in chunk_texts.CHUNK_ENV.items():
                m.setenv(k, v)
            got, stats = gpu_hits(big, big_text, pats, flags, ids, need, 1000)
            assert stats.stream_launches >= 2
            assert got == want
            assert stats.n_raw_hits >= raw
    finally:
        big.free()


# ---- Face A

def block_expected(data, pats, flags, ids, need, som):
    """hs_scan's reports of one block whose expressions cannot match across '\\n' nor tell a line's edge from the block's:
    the lines' reports, shifted, in delivery order (to, id)."""
    out, off = [], 0
    every = [f & ~SINGLE for f in flags]  # (SINGLEMATCH holds for the block, not per line: applied below; ids are distinct)
    for line in data.split(b"\n"):
        for rid, to, frm in piece_reports(pats, every, ids, need, line):
            out.append((rid, frm + off if som else 0, to + off))
        off += len(line) + 1
    out.sort(key=lambda r: (r[2], r[0]))
    seen = set()
    kept = []
    for r in out:
        if flags[ids.index(r[0])] & SINGLE and r[0] in seen:
            continue
        seen.add(r[0])
        kept.append(r)
    return [r if som else (r[0], r[2]) for r in kept]


BLOCK_PATS = [r"abc[0-9]+", r"[0-9]+x", r"ERROR [0-9]+ failed", "needle-in-hay", r"\bxyz\d+"]
BLOCK_NEED = [6, 4, 17, None, 6]


def block_data(rng, nbytes):
    pool = [ln.replace(b"\0", b"-") for ln in line_pool(rng, ["anchored", "byte_windows", "always_on_1w"])]
    return make_text(rng, pool, nbytes // 12)[:nbytes]


def test_face_a_short_and_long_blocks():
    from hypergrep_amd import device

    rng = random.Random(15)
    ids = list(range(len(BLOCK_PATS)))
    for flags in ([2] * 5, [2 | SINGLE] * 5, [2 | SOM] * 5):
        som = bool(flags[0] & SOM)
        db = device.BlockDatabase(BLOCK_PATS, flags, ids, exts_for(BLOCK_NEED))
        plain = device.BlockDatabase(BLOCK_PATS, flags, ids)
        for nbytes in (300, 6000, 200000):  # short blocks would take the one-launch path: a filtering database must leave it
            data = block_data(rng, nbytes)
            want = block_expected(data, BLOCK_PATS, flags, ids, BLOCK_NEED, som)
            assert db.scan(data) == want, (flags, nbytes)
            assert plain.scan(data) == block_expected(data, BLOCK_PATS, flags, ids, [None] * 5, som), (flags, nbytes)
            assert len(want) <= len(plain.scan(data))


def test_hg_scan_blocks_equals_per_item_hs_scan():
    from hypergrep_amd import device

    rng = random.Random(16)
    ids = list(range(len(BLOCK_PATS)))
    flags = [2] * 5
    db = device.BlockDatabase(BLOCK_PATS, flags, ids, exts_for(BLOCK_NEED))
    items = [block_data(rng, n) for n in (0, 40, 9000, 700, 1, 30000, 2500, 8192, 8193, 64)]
    per_item = [db.scan(d) for d in items]
    assert db.scan_blocks(items) == per_item
    for d, got in zip(items, per_item):
        assert got == block_expected(d, BLOCK_PATS, flags, ids, BLOCK_NEED, False)
    assert sum(len(r) for r in per_item) > 100


# ---- Face B

def test_face_b_scan_with_ext_and_max_match_count():
    import hypergrep_amd

    rng = random.Random(17)
    pats = [r"abc[0-9]+", r"[0-9]+x", r"ERROR [0-9]+ failed"]
    need = [6, 4, 17]
    flags, ids = [6 | SINGLE] * 3, [0, 1, 2]
    text = make_text(rng, [ln.replace(b"\0", b"-") for ln in line_pool(rng, ["anchored", "byte_windows", "always_on_1w"])], 3000)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "f.log")
        with open(path, "wb") as f:
            f.write(text)
        runs = {}
        for name, lengths in (("with", need), ("without", None), ("again", need)):  # (the compile cache keys on the parameters)
            want_hits = expected(text, pats, flags, ids, lengths or [None] * 3, 262140)
            lines = {}
            for line, rid, to, _ in want_hits:
                lines.setdefault(line, []).append((to, rid))
            for max_count in (0, 1, 25):
                want = []
                for line in sorted(lines):
                    want.extend((line, rid) for _, rid in sorted(lines[line]))
                    if max_count and len(want) >= max_count:
                        break
                rows = []

                def on_match(matches, n, rows=rows):
                    rows.extend((matches[k].line_number, matches[k].id) for k in range(n))

                ext = exts_for(lengths) if lengths else None
                assert hypergrep_amd.scan(path, pats, on_match, flags=flags, ids=ids, max_match_count=max_count, ext=ext) == 0
                assert rows == want, (name, max_count)
                if not max_count:
                    runs[name] = rows
    assert runs["with"] == runs["again"] and runs["with"] != runs["without"]
    # a line whose only reports are filtered away is not a matching line
    assert {r[0] for r in runs["without"]} - {r[0] for r in runs["with"]}


# ---- databases without the parameter

_MEMLOG_SCRIPT = r"""
import sys
import torch  # one HIP runtime per process: torch's
sys.path.insert(0, sys.argv[1])
from hypergrep_amd import device
from minlensim_py import exts_for
need = [6, None] if sys.argv[2] == "filter" else [4, None]   # abc[0-9]+: 4 is its shortest match, dropped by the compiler
db = device.Database([r"abc[0-9]+", "needle-in-hay"], flags=[6, 6], ids=[0, 1], ext=exts_for(need))
sc = device.Scanner(db, 0)
arena = device.GuardedArena(1 << 16)
text = b"abc1 abc123 needle-in-hay\n" * 200
sc.scan(arena.place(text), len(text))
print("hits", len(sc.hits()))
del sc
arena.free()
"""


@pytest.mark.parametrize("mode", ["filter", "trivial"])
def test_no_second_raw_array_without_the_parameter(mode):
    # the library's allocation log (HG_MEMLOG) names every buffer: a database without a filtering min_length never
    # allocates the match-length pass's arrays
    tests = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        script, log = os.path.join(tmp, "job.py"), os.path.join(tmp, "mem.log")
        with open(script, "w", encoding="utf-8") as f:
            f.write(_MEMLOG_SCRIPT)
        path = [os.path.dirname(tests), tests] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]
        env = dict(os.environ, HG_MEMLOG=log, PYTHONPATH=os.pathsep.join(path))
        out = subprocess.run([sys.executable, script, tests, mode], env=env, capture_output=True, text=True, timeout=300, check=False)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip() == ("hits 400" if mode == "filter" else "hits 1000"), out.stdout
        with open(log, encoding="utf-8") as f:
            names = {ln.split()[2] for ln in f if ln.startswith("alloc dev")}
    assert "d_hits_raw_" in names
    assert ({"d_minlen_hits_", "d_minlen_aux_", "d_min_lengths_"} <= names) == (mode == "filter"), names
    if mode == "trivial":
        assert not any("minlen" in n or "min_length" in n for n in names), names
