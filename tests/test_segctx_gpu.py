"""Context lines of many files in one scan on the MI355X: hg_scan_device_segments_context (the per-file context stage,
hypergrep_amd/csrc/hg_segctx.hip) against the SAME device's hg_scan_device_context of every segment's bytes alone, and against
segctx_ref (plain Python on the segment's bytes and the lines the device reports for them alone).  The records, segments and
summaries must stay those of hg_scan_device_segments.  Texts are a few 16 KiB tiles at the most and sit, like the segment
arrays, at the end of guarded buffers: a read past them faults."""
from __future__ import annotations

import json
import os

import pytest

import segctx_ref as cr
import segments_ref as sr

pytestmark = pytest.mark.gpu

TILE = sr.TILE
SOM = 256
CTX = 0xFFFFFFFE
# a literal-anchored expression and an always-on one, so that both tiers feed the stage; NL adds one that matches the pad's "\n"
SET_AB = (["abc", "[0-9]+x|q"], [14, 14])
SET_NL = (["abc", "[0-9]+x|q", "\\n"], [14, 14, 14])
SET_LIT = (["abc"], [14])
SET_SOM = (["a+b", "z"], [6 | SOM, 14])


def quiet(n):
    """n bytes of lines no expression of the sets matches (n >= 1)."""
    return sr.filler(n, b"xy abd w\n")


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 20)
    yield a
    _scanners.clear()  # (before the interpreter takes the module's globals away)
    a.free()


_scanners = {}
_alone = {}  # (set, bytes, buffer_size, invert, before, after) -> the segment scanned on its own: computed once, never changed


def scanner(pset):
    from hypergrep_amd import device

    key = tuple(pset[0])
    if key not in _scanners:
        db = device.Database(pset[0], flags=pset[1], ids=list(range(1, len(pset[0]) + 1)))
        _scanners[key] = (device.Scanner(db, 0), db.info())
    return _scanners[key][0]


def alone(arena, pset, data, bs, invert, before, after):
    """(records, n_lines, context records) of `data` scanned on its own with hg_scan_device_context."""
    key = (tuple(pset[0]), data, bs, invert, before, after)
    if key not in _alone:
        sc = scanner(pset)
        st = sc.scan(arena.place(data), len(data), buffer_size=bs, invert=invert, context=(before, after))
        assert st.n_tail == 0
        _alone[key] = (sc.hits(), st.n_lines, sc.context())
    return _alone[key]


def check(arena, pset, files, bs, invert, before, after, limit=0):
    """One packed scan with context against every file alone.  Returns (stats, per-file context rows)."""
    sc = scanner(pset)
    data, starts, ends = sr.pack(files)
    assert len(data) <= 1 << 20
    plain = sc.scan(arena.place(data), len(data), buffer_size=bs, invert=invert, segments=(starts, ends), max_per_segment=limit)
    plain_hits, plain_from, plain_seg = sc.hits(), sc.hit_starts().tolist(), sc.segments()
    st = sc.scan(arena.place(data), len(data), buffer_size=bs, invert=invert, segments=(starts, ends), max_per_segment=limit, context=(before, after))
    # the records, their starts and the per-file arrays are exactly those of the call without context
    assert (st.n_hits, st.n_lines, st.n_candidates, st.n_raw_hits) == (plain.n_hits, plain.n_lines, plain.n_candidates, plain.n_raw_hits)
    assert sc.hits() == plain_hits and sc.hit_starts().tolist() == plain_from
    seg = sc.segments()
    for k in ("record_segment", "first_record", "n_lines", "n_selected"):
        assert seg[k].tolist() == plain_seg[k].tolist(), k
    assert st.n_tail == 0 and st.owed_after == 0
    rows, sx = sc.context(), sc.segment_context()
    first = sx["first_context"].tolist()
    assert len(rows) == st.n_context and len(first) == len(files) + 1 and first[0] == 0 and first[-1] == len(rows)
    per_file = []

    def scan_alone(own):
        hits, n_lines, _ = alone(arena, pset, own, bs, invert, before, after)
        return hits, n_lines

    want_ref = cr.expected(data, starts, ends, scan_alone, bs, before, after, limit)
    for s, f in enumerate(files):  # no segment is left out
        lo, hi = first[s], first[s + 1]
        assert sx["context_segment"][lo:hi].tolist() == [s] * (hi - lo)
        assert rows[lo:hi] == [tuple(r) for r in want_ref[s]], (s, limit, invert, f[-24:])
        if not limit:  # the contract: the device's own context scan of the file alone
            assert rows[lo:hi] == alone(arena, pset, f, bs, invert, before, after)[2], (s, invert, f[-24:])
        per_file.append(rows[lo:hi])
    return st, per_file


def test_nothing_crosses_a_file_boundary(arena):
    # a match on the last line of file 0 and on the first line of file 1, A = B = 2: the after-window of the first, unclamped,
    # would take the second's before-context (free_from), and either would reach into the other file
    files = [b"x\nx\nx\nabc\n", b"abc\nx\nx\nx\n", b"x\nx\nx\n", b"x\nx\nabc"]
    for bs in (8, 64, 262140):
        _, per_file = check(arena, SET_AB, files, bs, False, 2, 2)
        assert [[r[0] for r in rows] for rows in per_file] == [[1, 2], [1, 2], [], [0, 1]]
    _, per_file = check(arena, SET_LIT, files, 64, False, 2, 2)  # the literal tier alone
    assert [[r[0] for r in rows] for rows in per_file] == [[1, 2], [1, 2], [], [0, 1]]


def test_300_matching_one_line_files_have_no_context(arena):
    files = [b"abc\n" if i % 3 else b"q\n" for i in range(300)]
    st, _ = check(arena, SET_AB, files, 64, False, 3, 3)
    assert st.n_context == 0 and st.n_hits == 300
    st, _ = check(arena, SET_AB, [f if i % 2 else b"" for i, f in enumerate(files)], 64, False, 3, 3)
    assert st.n_context == 0 and st.n_hits == 150
    # ... and with a quiet line in each, every file has exactly that one
    st, per_file = check(arena, SET_AB, [b"abc\nx\n"] * 300, 64, False, 3, 3)
    assert st.n_context == 300 and all(rows == [(1, CTX, 0, 4, 2)] for rows in per_file)


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_file_boundaries_around_a_tile_end(arena, d):
    # file 0 ends d bytes from the tile's end with a match on its last line, file 1 starts with one
    files = [quiet(TILE + d - 4) + b"abc\n", b"abc\n" + quiet(50), quiet(30)]
    for before, after in ((2, 2), (0, 3), (3, 0)):
        _, per_file = check(arena, SET_AB, files, 64, False, before, after)
        assert len(per_file[0]) == before and len(per_file[1]) == after and per_file[2] == []
    check(arena, SET_AB, files, 64, True, 1, 1)


def test_windows_over_two_and_three_tiles(arena):
    # one match in the middle of a file of three tiles, ~1820 lines a tile: 1000 / 1000 spans two, 3000 / 3000 all three
    above, below = quiet(TILE + TILE // 2), quiet(TILE + TILE // 2)
    files = [quiet(TILE // 2), above + b"abc\n" + below, b"abc\n" + quiet(100)]
    for before, after in ((1000, 1000), (3000, 3000), (2, 3)):
        _, per_file = check(arena, SET_AB, files, 64, False, before, after)
        assert per_file[0] == [] and len(per_file[1]) == min(before, above.count(b"\n")) + min(after, below.count(b"\n"))
        assert len(per_file[2]) == min(after, quiet(100).count(b"\n"))


@pytest.mark.parametrize("bs", [8, 64, 262140])
@pytest.mark.parametrize("invert", [False, True])
def test_every_segment_equals_its_own_context_scan(arena, bs, invert):
    # (pieces of 256 KiB: last lines of one piece's length only, the texts of two take seconds to compare)
    for name, files in sr.cases(TILE, bs, multiples=(1, 2) if bs < TILE else (1,)):
        for before, after in ((2, 3), (1000, 1000)):  # saturation meets the clamp: 1000 is more than most files have
            try:
                check(arena, SET_AB, files, bs, invert, before, after)
            except AssertionError as e:
                raise AssertionError(f"{name} context={before, after}: {e}") from e


@pytest.mark.parametrize("bs", [8, 64])
def test_unterminated_last_lines_leave_no_phantom_context(arena, bs):
    bs1 = bs - 1
    for k in (1, 2):
        for d in (0, -1, -2, 1):
            n = k * bs1 + d
            files = [b"abc\n" + (b"zw" * n)[:n], b"x\nabc\n", (b"zw" * n)[:n], b"abc\n"]
            for pset in (SET_AB, SET_NL):
                st, per_file = check(arena, pset, files, bs, False, 3, 3)
                n_lines = [alone(arena, pset, f, bs, False, 3, 3)[1] for f in files]
                assert all(r[0] < n_lines[s] for s, rows in enumerate(per_file) for r in rows)
                check(arena, pset, files, bs, True, 3, 3)


@pytest.mark.parametrize("bs", [8, 64])
def test_a_nul_only_last_piece_is_context_with_an_empty_record(arena, bs):
    # packed, the piece's scanned bytes are the pad's "\n", where SET_NL reports; that hit is dropped and the piece is context
    files = [b"abc\n\0\0\0", b"abc\n", b"x\n\0\0", b"q\n"]
    _, per_file = check(arena, SET_NL, files, bs, False, 1, 1)
    assert per_file[0] == [(1, CTX, 0, 7, 0)]
    _, per_file = check(arena, SET_AB, files, bs, False, 1, 1)
    assert per_file[0] == [(1, CTX, 0, 7, 0)] and per_file[2] == []
    # inverted under SET_NL every line with a newline matches: the NUL piece is the one selected line, the line before it context
    _, per_file = check(arena, SET_NL, files, bs, True, 1, 1)
    assert per_file[0] == [(0, CTX, 0, 0, 4)] and per_file[2] == [(0, CTX, 0, 0, 2)]
    for limit in (1, 2):
        check(arena, SET_NL, files, bs, True, 1, 1, limit=limit)
        check(arena, SET_NL, files, bs, False, 1, 1, limit=limit)


def test_the_limit_ends_the_context_before_the_next_matching_piece(arena):
    near = b"abc\nx\nabc\nx\nx\n"       # the next matching piece lies within `after` of the last kept line
    far = b"abc\nx\nx\nx\nx\nabc\nx\n"  # ... beyond it
    last = b"x\nabc\nx\n"               # ... in the NEXT file only: nothing truncates
    files = [near, far, last, b"abc\nx\n"]
    for bs in (8, 64):
        _, per_file = check(arena, SET_AB, files, bs, False, 1, 3, limit=1)
        assert [[r[0] for r in rows] for rows in per_file] == [[1], [1, 2, 3], [0, 2], [1]]
        _, per_file = check(arena, SET_AB, files, bs, False, 1, 3, limit=2)
        assert [[r[0] for r in rows] for rows in per_file] == [[1, 3, 4], [1, 2, 3, 4, 6], [0, 2], [1]]


@pytest.mark.parametrize("limit", [0, 1, 2])
def test_inverted_with_and_without_a_limit(arena, limit):
    files = [b"abc\nx\nabc\nx\nx\nabc\n", b"x\nx\nabc\nabc\nabc\nx", b"abc\n", b"", b"x\n" * 5, b"abc abc abc abc\nx\nabc"]
    for bs in (8, 64, 262140):  # (8: "abc abc abc abc" is a line of three pieces)
        check(arena, SET_AB, files, bs, True, 1, 2, limit=limit)
        check(arena, SET_AB, files, bs, False, 2, 1, limit=limit)


def test_no_context_asked_for_is_the_segment_scan(arena):
    files = [b"abc\nx\n", b"x\nabc"]
    st, per_file = check(arena, SET_AB, files, 64, False, 0, 0)
    assert st.n_context == 0 and st.context_us == 0 and per_file == [[], []]
    sc = scanner(SET_AB)
    data, starts, ends = sr.pack(files)
    sc.scan(arena.place(data), len(data), buffer_size=64, segments=(starts, ends), context=(0, 0))
    assert sc.context() == [] and sc.segment_context()["first_context"].tolist() == [0, 0, 0]


def test_starts_of_match_follow_the_records(arena):
    files = [b"xaab aab\nab\nx\n", (b"aab " * 9)[:13], b"q\n", b"zaaab\nq\nab ab ab\n", b"", b"ab"]
    for bs in (8, 64):
        for limit in (0, 1):
            st, _ = check(arena, SET_SOM, files, bs, False, 1, 1, limit=limit)  # (the starts are compared with the call without context)
            assert st.n_context > 0
            sc = scanner(SET_SOM)
            data, starts, ends = sr.pack(files)
            sc.scan(arena.place(data), len(data), buffer_size=bs, segments=(starts, ends), max_per_segment=limit, context=(1, 1))
            assert any(f > 0 for f in sc.hit_starts().tolist())


def test_errors(arena):
    sc = scanner(SET_AB)
    data = b"qb\nqb\nqb\nqb\n"
    with pytest.raises(ValueError, match="line start"):
        sc.scan(arena.place(data), len(data), buffer_size=64, segments=([0, 4], [3, 9]), context=(1, 1))
    assert sc.hits() == [] and sc.context() == []  # HG_ERR_ARG: nothing was scanned
    st = sc.scan(arena.place(data), len(data), buffer_size=64, segments=([0, 6], [6, 12]), context=(1, 1))  # the scanner is fine afterwards
    assert st.n_hits == 4 and st.n_context == 0
    for kw in ({"tail": True}, {"carry_after": 1}, {"line_base": 5}):
        with pytest.raises(ValueError, match="segments"):
            sc.scan(arena.place(data), len(data), buffer_size=64, segments=([0, 6], [6, 12]), context=(1, 1), **kw)
    with pytest.raises(ValueError):
        sc.scan(arena.place(data), len(data), buffer_size=64, segments=([0, 6], [6, 12]), parts=True)
    sc.scan(arena.place(data), len(data), buffer_size=64)
    with pytest.raises(ValueError):
        sc.segment_context()  # a plain scan
    sc.scan(arena.place(data), len(data), buffer_size=64, context=(1, 1))
    with pytest.raises(ValueError):
        sc.segment_context()  # context without segments
    sc.scan(arena.place(data), len(data), buffer_size=64, segments=([0, 6], [6, 12]))
    with pytest.raises(ValueError):
        sc.segment_context()  # segments without context


def test_kernel_resources():
    """The stage's kernels are in the build's table with no scratch and no spills, and every kernel the build had before the
    stage is unchanged (tests/golden/kernel_resources_before_segctx.json: that build's table)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "hypergrep_amd", "lib", "kernel_resources.json"), encoding="utf-8") as f:
        table = json.load(f)
    with open(os.path.join(root, "tests", "golden", "kernel_resources_before_segctx.json"), encoding="utf-8") as f:
        before = json.load(f)
    mine = {k: v for k, v in table.items() if "hg_segctx_" in k}
    assert sorted(k.split("hg_segctx_")[1].split("_kernel")[0] for k in mine) == ["count", "first", "map", "prep", "write"]
    for k, v in mine.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    for k, v in before.items():
        assert table.get(k) == v, k
