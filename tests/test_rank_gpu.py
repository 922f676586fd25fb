"""Ranked matched values on the MI355X: hg_rank_values (the rank stage, hypergrep_amd/csrc/hg_rank.hip and the segment-keyed
instantiations of the values stage's passes) behind hg_scan_device_parts and hg_scan_device_segments_parts.  Every expectation
is rank_ref's plain Python dict, sort and slice over Scanner.parts(), the starts in Scanner.hits() and the text, never anything
the stage computes.  Texts are a few KiB and sit at the end of guarded buffers: a read past them faults.  The tightest table of
any test still has more slots than parts."""
from __future__ import annotations

import ctypes
import random

import pytest

import rank_ref as rr

pytestmark = pytest.mark.gpu

A = 14  # DOTALL | MULTILINE | SINGLEMATCH
LANE_MAX = 256
SET_KV = (["[a-z]+=[0-9]+", "ERR[0-9]+"], [A, A])
SET_X = (["x[a-w]*"], [A])
SET_TWO = (["user=[a-z]+", "[a-z]+=bob"], [A, A])  # both match `user=bob`: equal bytes from different expressions
MODES = ((False, False), (False, True), (True, False), (True, True))  # (by_pattern, per_segment)
ARRAYS = ("off", "count", "first", "pattern", "line_number")


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 21)
    yield a
    _scanners.clear()  # (before the interpreter takes the module's globals away)
    a.free()


_scanners = {}


def scanner(pset):
    from hypergrep_amd import device

    key = tuple(pset[0])
    if key not in _scanners:
        _scanners[key] = device.Scanner(device.Database(pset[0], flags=pset[1], ids=list(range(1, len(pset[0]) + 1))), 0)
    return _scanners[key]


def tight(n_parts: int) -> int:
    """The smallest legal explicit table: 2 ** k > n_parts."""
    return max(1, n_parts.bit_length())


def collision_settings(n_parts):
    return ({}, {"hash_bits": 1}, {"hash_bits": 4}, {"table_log2": tight(n_parts)}, {"hash_bits": 4, "table_log2": tight(n_parts)})


def scan_files(arena, files, pset):
    """One scan with segments and parts over the files joined.  Returns (scanner, ptr, text, parts with their segment, starts
    {(segment, line): start}, the files' offsets)."""
    text = b"".join(files)
    seg_start = [sum(len(f) for f in files[:i]) for i in range(len(files))]
    ends = [s + len(f) for s, f in zip(seg_start, files)]
    sc = scanner(pset)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), segments=(seg_start, ends), segment_parts=True)
    parts = [p + (s,) for p, s in zip(sc.parts(), sc.segment_parts()["part_segment"].tolist())]
    starts = {(s, h[0]): h[3] for h, s in zip(sc.hits(), sc.segments()["record_segment"].tolist())}
    return sc, ptr, text, parts, starts, seg_start


def compare(sc, stats, rows, seg_arrays, n_distinct, n_parts, segments, where):
    want = rr.arrays(rows, segments=segments)
    a = sc.ranked_values_arrays()
    assert (stats.n_values, stats.n_distinct, stats.n_parts, stats.n_bytes) == (len(rows), n_distinct, n_parts, len(want["bytes"])), where
    assert a["bytes"] == want["bytes"], where
    for name in ARRAYS:
        assert a[name].tolist() == want[name], (name, where)
    if segments:
        assert a["segment"].tolist() == want["segment"], where
    else:
        assert a["segment"] is None, where
    listed = sc.ranked_values()
    assert listed == [(r["value"], r["count"], r["pattern"], r["line_number"]) + ((r["segment"],) if segments else ()) for r in rows], where
    if seg_arrays is None:
        with pytest.raises(ValueError, match="per_segment"):
            sc.ranked_segments()
    else:
        assert {k: v.tolist() for k, v in sc.ranked_segments().items()} == seg_arrays, where
    return a


def check_files(arena, files, pset, tops=(0, 1, 2), modes=MODES, settings=({},)):
    """Every mode and cut, at every setting, against the reference.  Returns {(by_pattern, per_segment, top): (rows, seg arrays)}."""
    sc, ptr, text, parts, starts, seg_start = scan_files(arena, files, pset)
    assert all((p[4], p[0]) in starts for p in parts)  # every part has a record
    out = {}
    for bp, ps in modes:
        for top in tops:
            rows, seg_arrays, n_distinct = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=ps, top=top, seg_start=seg_start, n_seg=len(files))
            for kw in settings:
                st = sc.rank_values(ptr, len(text), top=top, per_segment=ps, by_pattern=bp, **kw)
                compare(sc, st, rows, seg_arrays, n_distinct, len(parts), True, (bp, ps, top, kw))
            out[(bp, ps, top)] = (rows, seg_arrays)
    return out


def check_plain(arena, text, pset, tops=(0, 1, 2), settings=({},)):
    """The same after a scan without segments (per_segment is refused there)."""
    sc = scanner(pset)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    parts = sc.parts()
    starts = {(0, h[0]): h[3] for h in sc.hits()}
    out = {}
    for bp in (False, True):
        for top in tops:
            rows, _seg, n_distinct = rr.ranking(text, parts, starts, by_pattern=bp, top=top)
            for kw in settings:
                st = sc.rank_values(ptr, len(text), top=top, by_pattern=bp, **kw)
                compare(sc, st, rows, None, n_distinct, len(parts), False, (bp, top, kw))
            out[(bp, top)] = rows
    return out


def mix_text(rng, lines):
    vocab = [b"%s=%d" % (rng.choice([b"user", b"code", b"req", b"n"]), rng.randrange(12)) for _ in range(50)] + [b"ERR%d" % rng.randrange(5) for _ in range(5)]
    filler = [b"lorem", b"-", b"GET /index", b"=", b"a=", b"=7"]
    return b"".join(b" ".join(rng.choice(vocab + filler) for _ in range(rng.randint(0, 5))) + b"\n" for _ in range(lines))


def test_no_parts_and_one_part(arena):
    out = check_plain(arena, b"nothing here\nnor here\n", SET_KV)
    assert all(rows == [] for rows in out.values())
    assert scanner(SET_KV).ranked_values_arrays()["off"].tolist() == [0]
    out = check_files(arena, [b"nothing\n", b"", b"nor here\n"], SET_KV)
    assert out[(False, True, 0)] == ([], {"first_value": [0, 0, 0, 0], "seg_distinct": [0, 0, 0], "seg_parts": [0, 0, 0]})
    out = check_plain(arena, b"a=1\n", SET_KV)
    assert [r["value"] for r in out[(False, 0)]] == [b"a=1"] == [r["value"] for r in out[(True, 1)]]
    check_files(arena, [b"a=1\n"], SET_KV)  # one file (n_seg 1)


def test_the_cut_and_its_tie(arena):
    """c x3, a x2, b x2, d x1: top 0, 1, 2 (a tie in count exactly at the cut: the smaller first stays), 4 (the number of distinct
    values) and 5 (above it); then all counts equal."""
    text = b"a=1 b=1 c=1\nc=1 b=1 a=1\nc=1 d=1\n"
    out = check_plain(arena, text, SET_KV, tops=(0, 1, 2, 3, 4, 5), settings=collision_settings(8))
    assert [(r["value"], r["count"], r["first"]) for r in out[(False, 0)]] == [(b"c=1", 3, 2), (b"a=1", 2, 0), (b"b=1", 2, 1), (b"d=1", 1, 7)]
    assert [r["value"] for r in out[(False, 2)]] == [b"c=1", b"a=1"] and out[(False, 4)] == out[(False, 0)] == out[(False, 5)]
    out = check_files(arena, [text, text[:12]], SET_KV, tops=(0, 2, 3), modes=((False, True),), settings=collision_settings(11))
    assert [r["value"] for r in out[(False, True, 2)][0]] == [b"c=1", b"a=1", b"a=1", b"b=1"]
    out = check_plain(arena, b"x=1 y=22 z=3\nz=3 x=1 y=22\n", SET_KV, tops=(0, 2))
    assert [r["value"] for r in out[(False, 0)]] == [b"x=1", b"y=22", b"z=3"] and [r["value"] for r in out[(False, 2)]] == [b"x=1", b"y=22"]


def test_the_same_value_in_two_files_and_empty_files_at_both_ends(arena):
    files = [b"", b"none\n", b"n=1 n=2\nzz\nn=3\n", b"none\n", b"n=9\nn=2 n=1 n=2\n", b"ERR7\nn=3 n=9\n", b"nothing\n", b""]
    out = check_files(arena, files, SET_KV, settings=collision_settings(11))
    whole, per_file = out[(False, False, 0)][0], out[(False, True, 0)]
    assert [(r["value"], r["count"]) for r in whole] == [(b"n=2", 3), (b"n=1", 2), (b"n=3", 2), (b"n=9", 2), (b"ERR7", 1)]
    assert [(r["value"], r["count"], r["segment"]) for r in per_file[0]] == [(b"n=1", 1, 2), (b"n=2", 1, 2), (b"n=3", 1, 2), (b"n=2", 2, 4), (b"n=9", 1, 4), (b"n=1", 1, 4),
                                                                             (b"ERR7", 1, 5), (b"n=3", 1, 5), (b"n=9", 1, 5)]
    assert per_file[1] == {"first_value": [0, 0, 0, 3, 3, 6, 9, 9, 9], "seg_distinct": [0, 0, 3, 0, 3, 3, 0, 0], "seg_parts": [0, 0, 3, 0, 4, 3, 0, 0]}
    assert out[(False, True, 1)][1]["first_value"] == [0, 0, 0, 1, 1, 2, 3, 3, 3]


@pytest.mark.parametrize("n", [64, 65, 128])
def test_a_wave_of_equal_parts_across_a_file_boundary(arena, n):
    """n equal-byte parts, the first n // 2 in one file and the rest in the next: the lanes of one wavefront of the insert pass hold
    equal bytes of two keys, so the wave may not add its population count to one slot."""
    a, b = n // 2, n - n // 2
    files = [b"v=7 v=7\n" * (a // 2) + (b"v=7\n" if a % 2 else b""), b"v=7 v=7\n" * (b // 2) + (b"v=7\n" if b % 2 else b"")]
    out = check_files(arena, files, SET_KV, tops=(0, 1), modes=((False, False), (False, True)), settings=({}, {"hash_bits": 1, "table_log2": tight(n)}))
    assert [(r["count"], r["first"]) for r in out[(False, False, 0)][0]] == [(n, 0)]
    assert [(r["count"], r["first"], r["segment"]) for r in out[(False, True, 0)][0]] == [(a, 0, 0), (b, a, 1)]
    assert out[(False, True, 1)][1] == {"first_value": [0, 1, 2], "seg_distinct": [1, 1], "seg_parts": [a, b]}


def test_a_long_value_in_two_files(arena):
    """Parts a wavefront hashes and compares, with the segment in the key: one of 3 * 256 + 6 bytes once in the first file and
    twice in the second, one of 257 bytes in both, at different alignments."""
    rng = random.Random(3)
    big = b"x" + bytes(97 + rng.randrange(23) for _ in range(3 * LANE_MAX + 5))
    edge = b"x" + bytes(97 + k % 23 for k in range(LANE_MAX))
    files = [b"." + big + b"\n" + edge + b"\n", b".." + big + b" " + big + b"\n..." + edge + b"\nxq\n"]
    out = check_files(arena, files, SET_X, tops=(0, 1), modes=((False, False), (False, True)), settings=({}, {"hash_bits": 1, "table_log2": tight(6)}))
    assert [(len(r["value"]), r["count"]) for r in out[(False, False, 0)][0]] == [(len(big), 3), (len(edge), 2), (2, 1)]
    assert [(len(r["value"]), r["count"], r["segment"]) for r in out[(False, True, 0)][0]] == [(len(big), 1, 0), (len(edge), 1, 0), (len(big), 2, 1), (len(edge), 1, 1), (2, 1, 1)]


def test_by_pattern_and_per_segment(arena):
    files = [b"user=bob x=bob user=bob\nuser=al user=bob\n", b"k=bob\nuser=bob\n", b"user=al\n"]
    out = check_files(arena, files, SET_TWO, settings=collision_settings(10))
    assert len(out[(True, True, 0)][0]) >= len(out[(False, True, 0)][0]) > len(out[(False, False, 0)][0])  # (a span is one part: whichever expression the parts stage gives it)
    assert {r["pattern"] for r in out[(True, True, 0)][0]} == {0, 1}
    check_plain(arena, b"".join(files), SET_TWO, settings=collision_settings(10))


def test_random_logs_over_several_files(arena):
    rng = random.Random(21)
    for n_files in (2, 5, 9):
        files = [mix_text(rng, rng.randrange(0, 40)) for _ in range(n_files)]
        n = sum(f.count(b"=") for f in files)
        check_files(arena, files, SET_KV, tops=(0, 1, 3), settings=({}, {"hash_bits": 2, "table_log2": tight(n)}))


def test_more_than_one_workgroup(arena):
    """5000 parts (20 workgroups of the hash and insert pass) in 300 groups (two workgroups of the rank passes) over 3 files."""
    rng = random.Random(2)
    files = [b"".join(b"id=%d k=%d\n" % (rng.randrange(100), rng.randrange(3)) for _ in range(n)) for n in (1000, 300, 1200)]
    out = check_files(arena, files, SET_KV, tops=(0, 20), modes=((False, False), (False, True)))
    assert out[(False, True, 20)][1]["first_value"] == [0, 20, 40, 60] and out[(False, True, 0)][1]["seg_parts"] == [2000, 600, 2400]
    assert len(out[(False, True, 0)][0]) > 256


def test_against_count_values_on_the_same_scan(arena):
    """per_segment=False, top=0: the same set of (value, count, first[, pattern, line, segment]) as hg_count_values."""
    files = [mix_text(random.Random(s), 60) for s in (31, 32, 33)]
    sc, ptr, text, _parts, _starts, _seg = scan_files(arena, files, SET_KV)
    for bp in (False, True):
        sc.count_values(ptr, len(text), by_pattern=bp)
        v = sc.values_arrays()
        sc.rank_values(ptr, len(text), by_pattern=bp)
        r = sc.ranked_values_arrays()

        def rows(a):
            off = a["off"].tolist()
            return sorted((a["bytes"][off[j]:off[j + 1]],) + tuple(int(a[k][j]) for k in ("count", "first", "pattern", "line_number", "segment")) for j in range(len(off) - 1))

        assert rows(v) == rows(r) and len(rows(v)) > 30
        assert sc.values_arrays()["bytes"] == v["bytes"]  # the count is still there after the ranking


def test_collisions_and_tight_tables_against_the_default(arena):
    files = [mix_text(random.Random(s), 100) for s in (6, 7)]
    sc, ptr, text, parts, _starts, _seg = scan_files(arena, files, SET_KV)
    assert len(parts) > 200
    for bp, ps in MODES:
        sc.rank_values(ptr, len(text), top=7, per_segment=ps, by_pattern=bp)
        base, base_seg = sc.ranked_values_arrays(), sc.ranked_segments() if ps else None
        for kw in collision_settings(len(parts))[1:]:
            sc.rank_values(ptr, len(text), top=7, per_segment=ps, by_pattern=bp, **kw)
            a = sc.ranked_values_arrays()
            assert a["bytes"] == base["bytes"] and all(a[k].tolist() == base[k].tolist() for k in ARRAYS + ("segment",)), (bp, ps, kw)
            if ps:
                assert all(v.tolist() == base_seg[k].tolist() for k, v in sc.ranked_segments().items()), (bp, ps, kw)


def test_two_runs_are_identical(arena):
    files = [mix_text(random.Random(s), 700) for s in (8, 9, 10)]
    sc, ptr, text, _parts, _starts, _seg = scan_files(arena, files, SET_KV)
    runs = []
    for _ in range(2):
        sc.rank_values(ptr, len(text), top=5, per_segment=True, by_pattern=True)
        a = sc.ranked_values_arrays()
        runs.append((a["bytes"],) + tuple(a[k].tolist() for k in ARRAYS + ("segment",)) + tuple(v.tolist() for v in sc.ranked_segments().values()))
    assert runs[0] == runs[1]


def test_other_results_untouched(arena):
    files = [mix_text(random.Random(s), 150) for s in (10, 11)]
    sc, ptr, text, _parts, _starts, _seg = scan_files(arena, files, SET_KV)
    sc.gather(ptr, len(text))
    sc.count(per_segment=True)
    sc.count_values(ptr, len(text))
    before = (sc.hits(), sc.parts(), sc.values(), sc.counts(), sc.lines())
    sc.rank_values(ptr, len(text), top=3, per_segment=True)
    sc.rank_values(ptr, len(text), by_pattern=True, hash_bits=3)
    assert (sc.hits(), sc.parts(), sc.values(), sc.counts(), sc.lines()) == before
    ranked = sc.ranked_values()
    sc.count_values(ptr, len(text), by_pattern=True)  # and a count leaves the ranking as it is
    assert sc.ranked_values() == ranked


def test_refusals(arena):
    from hypergrep_amd import device

    text = b"a=1 b=2\n"
    sc = device.Scanner(device.Database(SET_KV[0], flags=SET_KV[1], ids=[1, 2]), 0)
    ptr = arena.place(text)
    with pytest.raises(ValueError, match="no successful scan"):
        sc.rank_values(ptr, len(text))
    with pytest.raises(ValueError, match="no ranking"):
        sc.ranked_values_arrays()
    sc.scan(ptr, len(text))
    with pytest.raises(ValueError, match="not one with parts"):
        sc.rank_values(ptr, len(text))
    sc.scan(ptr, len(text), parts=True)
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.rank_values(ptr, len(text) - 1)
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.rank_values(ptr + 4, len(text))
    with pytest.raises(ValueError, match="hash_bits above 64"):
        sc.rank_values(ptr, len(text), hash_bits=65)
    with pytest.raises(ValueError, match="table_log2 above 40"):
        sc.rank_values(ptr, len(text), table_log2=41)
    with pytest.raises(ValueError, match="must exceed the number of parts"):
        sc.rank_values(ptr, len(text), table_log2=1)  # 2 slots, 2 parts
    with pytest.raises(ValueError, match="unknown flag bits"):
        sc._rank_values(ptr, len(text), device.HgRankParams(flags=4))  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="HG_RANK_PER_SEGMENT after a scan without segments"):
        sc.rank_values(ptr, len(text), per_segment=True)
    with pytest.raises(ValueError, match="negative"):
        sc.rank_values(ptr, len(text), top=-1)
    with pytest.raises(ValueError, match="no ranking"):
        sc.ranked_values()
    assert sc._rank_values(ptr, len(text), None).n_values == 2  # params NULL: the defaults  # pylint: disable=protected-access
    assert sc.rank_values(ptr, len(text), table_log2=2).n_values == 2 and sc.ranked_values() == [(b"a=1", 1, 0, 0), (b"b=2", 1, 0, 0)]
    with pytest.raises(ValueError, match="per_segment"):
        sc.ranked_segments()
    # a refused call leaves no earlier ranking behind in the C ABI either
    off = (ctypes.c_uint64 * 4)()
    copy = lambda: device.lib().hg_copy_ranked_values(sc._h, None, 0, off, None, None, None, None, None, 2)  # noqa: E731  # pylint: disable=protected-access
    assert copy() == 0 and list(off[:3]) == [0, 3, 6]
    assert device.lib().hg_copy_ranked_segments(sc._h, None, None, None) == -1  # pylint: disable=protected-access
    seg = (ctypes.c_uint32 * 4)()
    assert device.lib().hg_copy_ranked_values(sc._h, None, 0, None, None, None, None, None, seg, 2) == -1  # (no segments)  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="hash_bits above 64"):
        sc.rank_values(ptr, len(text), hash_bits=65)
    assert copy() == -1
    sc.rank_values(ptr, len(text))
    sc.scan(ptr, len(text), parts=True)
    with pytest.raises(ValueError, match="no ranking"):  # a scan forgets the last ranking
        sc.ranked_values()
    assert copy() == -1


def test_copy_ranked_values_to_device(arena):
    import torch

    text = b"a=1 b=22 b=22\n"
    sc = scanner(SET_KV)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    v = sc.rank_values(ptr, len(text))
    dst = torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert sc.copy_ranked_values_to(dst.data_ptr(), 16) == v.n_bytes == 7
    torch.cuda.synchronize()
    assert bytes(dst.cpu().tolist()[:7]) == b"b=22a=1"
    assert sc.rank_values(ptr, len(text), top=1).n_bytes == 4 and sc.ranked_values() == [(b"b=22", 2, 0, 0)]
