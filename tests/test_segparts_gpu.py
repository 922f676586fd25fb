"""Matched parts of many files in one scan on the MI355X: hg_scan_device_segments_parts (the per-file parts stage,
hypergrep_amd/csrc/hg_segparts.hip) against the SAME device's hg_scan_device_parts of every segment's bytes alone, filtered to
the lines the segment keeps, and against parts_ref (plain Python) on those bytes.  The records, their starts and the per-file
arrays must stay those of hg_scan_device_segments.  Texts are a few 16 KiB tiles at the most and sit, like the segment
arrays, at the end of guarded buffers: a read past them faults."""
from __future__ import annotations

import json
import os

import pytest

import parts_ref
import segments_ref as sr

pytestmark = pytest.mark.gpu

TILE = sr.TILE
A = 14  # DOTALL | MULTILINE | SINGLEMATCH
SOM = 256
# parts_ref tries every (start, end) pair of a piece: it is the second reference for every segment whose pieces are at most this
# long.  Only the unterminated last lines of 256 KiB (pieces of 262139 bytes with 87 000 parts) lie above it; the same device's
# scan of the file alone, which never sees a pack, stays their reference.
REF_MAX_PIECE = 4096
# a literal-anchored expression and an always-on one, so that both tiers feed the stage; NL adds one that matches the pad's "\n"
SET_AB = (["abc", "[0-9]+x|q"], [A, A])
SET_NL = (["abc", "[0-9]+x|q", "\\n"], [A, A, A])
SET_END = (["abc$", "[0-9]+x|q"], [10, A])  # `$` without MULTILINE: the end of the piece's scanned bytes
SET_END_NL = (["abc$", "[0-9]+x|q", "\\n"], [10, A, A])
SET_LDS = (["[a-z]{70}X", "abc"], [A, A])  # more than 64 positions: three state words, the walk's state lies in LDS
SET_40 = ([f"w{i:02d}k" for i in range(39)] + ["abc"], [A] * 40)  # 40 expressions: the first-byte bitmap has two words
SET_SOM = (["a+b", "z"], [6 | SOM, A])


def quiet(n):
    """n bytes of lines no expression of the sets matches (n >= 1)."""
    return sr.filler(n, b"xy abd v\n")


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
_alone = {}  # (set, bytes, buffer_size) -> the segment scanned on its own with parts: computed once, never changed
_ref = {}    # (set, bytes, buffer_size, kept lines) -> parts_ref's rows


def scanner(pset):
    from hypergrep_amd import device

    key = tuple(pset[0])
    if key not in _scanners:
        db = device.Database(pset[0], flags=pset[1], ids=list(range(1, len(pset[0]) + 1)))
        _scanners[key] = device.Scanner(db, 0)
    return _scanners[key]


def alone(arena, pset, data, bs):
    """(records, parts) of `data` scanned on its own with hg_scan_device_parts."""
    key = (tuple(pset[0]), data, bs)
    if key not in _alone:
        if not data:
            _alone[key] = ([], [])
        else:
            sc = scanner(pset)
            sc.scan(arena.place(data), len(data), buffer_size=bs, parts=True)
            _alone[key] = (sc.hits(), sc.parts())
    return _alone[key]


def reference(pset, data, bs, lines):
    key = (tuple(pset[0]), data, bs, tuple(lines))
    if key not in _ref:
        _ref[key] = parts_ref.expected(data, bs, pset[0], pset[1], lines)
    return _ref[key]


def check(arena, pset, files, bs, limit=0):
    """One packed scan with parts against every file alone.  Returns (stats, per-file parts)."""
    sc = scanner(pset)
    data, starts, ends = sr.pack(files)
    assert len(data) <= 1 << 20
    plain = sc.scan(arena.place(data), len(data), buffer_size=bs, segments=(starts, ends), max_per_segment=limit)
    plain_hits, plain_from, plain_seg = sc.hits(), sc.hit_starts().tolist(), sc.segments()
    st = sc.scan(arena.place(data), len(data), buffer_size=bs, segments=(starts, ends), max_per_segment=limit, segment_parts=True)
    # the records, their starts and the per-file arrays are exactly those of the call without parts
    assert (st.n_hits, st.n_lines, st.n_candidates, st.n_raw_hits) == (plain.n_hits, plain.n_lines, plain.n_candidates, plain.n_raw_hits)
    assert sc.hits() == plain_hits and sc.hit_starts().tolist() == plain_from
    seg = sc.segments()
    for k in ("record_segment", "first_record", "n_lines", "n_selected"):
        assert seg[k].tolist() == plain_seg[k].tolist(), k
    rows, sp = sc.parts(), sc.segment_parts()
    first, first_record = sp["first_part"].tolist(), seg["first_record"].tolist()
    assert len(rows) == st.n_parts and len(first) == len(files) + 1 and first[0] == 0 and first[-1] == st.n_parts
    assert st.n_context == 0
    per_file = []
    for s, f in enumerate(files):  # no segment is left out
        lo, hi = first[s], first[s + 1]
        assert sp["part_segment"][lo:hi].tolist() == [s] * (hi - lo)  # constant per run
        kept = sorted({h[0] for h in plain_hits[first_record[s]:first_record[s + 1]]})
        own_hits, own_parts = alone(arena, pset, f, bs)
        if not limit:  # the restriction removes nothing
            assert kept == sorted({h[0] for h in own_hits}), (s, f[-24:])
        want = [p for p in own_parts if p[0] in set(kept)]
        assert rows[lo:hi] == want, (s, limit, f[-24:], rows[lo:hi][:4], want[:4])
        if bs <= REF_MAX_PIECE or max((len(line) for line in f.split(b"\n")), default=0) <= REF_MAX_PIECE:
            assert rows[lo:hi] == reference(pset, f, bs, kept), (s, limit, f[-24:])
        assert sorted({p[0] for p in rows[lo:hi]}) == kept  # every kept line has a part, no other line has one
        per_file.append(rows[lo:hi])
    return st, per_file


def test_one_line_files_stay_apart(arena):
    """Every matching line is line 0 of its file: a piece is named by (segment, line)."""
    _, per_file = check(arena, SET_AB, [b"abc\n", b"abc\n"], 64)
    assert per_file == [[(0, 0, 3, 0)], [(0, 0, 3, 0)]]
    files = [b"abc\n" if i % 3 else b"q\n" for i in range(300)]
    st, per_file = check(arena, SET_AB, files, 64)
    assert st.n_parts == 300 and all(len(p) == 1 for p in per_file)
    st, per_file = check(arena, SET_AB, [f if i % 2 else b"" for i, f in enumerate(files)], 64)
    assert st.n_parts == 150 and [len(p) for p in per_file] == [i % 2 for i in range(300)]


@pytest.mark.parametrize("bs", [8, 64, 262140])
@pytest.mark.parametrize("pset", [SET_AB, SET_NL], ids=["ab", "nl"])
def test_every_segment_equals_its_own_parts_scan(arena, bs, pset):
    # (SET_NL reports in the pads: those hits head no piece)
    # (pieces of 256 KiB: last lines of one piece's length only, two of the texts of two pieces' length outgrow the arena)
    for name, files in sr.cases(TILE, bs, multiples=(1, 2) if bs < TILE else (1,)):
        try:
            check(arena, pset, files, bs)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("bs", [8, 64])
def test_unterminated_last_lines_end_where_the_file_ends(arena, bs):
    """Last lines of k * (bs - 1) + d bytes that end in "abc": `abc$` matches at the file's end and not in the pad, the pad's
    phantom piece has no part."""
    bs1 = bs - 1
    for k in (1, 2):
        for d in (0, -1, -2, 1):
            n = k * bs1 + d
            last = ((b"zw" * n)[:n - 3] + b"abc")[-n:]
            files = [b"abc\n" + last, b"q\n", last, b"abc\n"]
            for pset in (SET_END, SET_END_NL):
                _, per_file = check(arena, pset, files, bs)
                r = n % bs1 or bs1  # the bytes of the file's last piece
                if r >= 3:  # ("abc" lies inside it)
                    assert per_file[2][-1][1:] == (r - 3, r, 0) and per_file[0][-1][1:] == (r - 3, r, 0)
                assert all(p[2] <= bs1 for rows in per_file for p in rows)


@pytest.mark.parametrize("bs", [8, 64])
def test_a_nul_only_last_piece_has_no_part(arena, bs):
    # packed, the piece's scanned bytes are the pad's "\n", where SET_NL reports; that hit is dropped and heads no piece
    files = [b"abc\n\0\0\0", b"abc\n", b"x\n\0\0", b"q\n"]
    for limit in (0, 1, 2):
        _, per_file = check(arena, SET_NL, files, bs, limit)
        assert [p[0] for p in per_file[0]] == [0, 0] and [p[0] for p in per_file[2]] == [0]
    _, per_file = check(arena, SET_AB, files, bs)
    assert per_file[0] == [(0, 0, 3, 0)] and per_file[2] == []


def test_the_limit_counts_whole_lines(arena):
    """A line two expressions report: the whole line counts and keeps all its parts; the lines behind the limit have none."""
    files = [b"abc q\nabc\nq\n", b"x\nabc q\nabc\n", b"abc\n", b"x\n"]
    for bs in (64, 262140):
        for limit, lines in ((1, [[0], [1], [0], []]), (2, [[0], [1], [0], []]), (0, [[0, 1, 2], [1, 2], [0], []])):
            _, per_file = check(arena, SET_AB, files, bs, limit)
            assert [sorted({p[0] for p in rows}) for rows in per_file] == lines
            assert per_file[0][:2] == [(0, 0, 3, 0), (0, 4, 5, 1)]


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_file_boundaries_around_a_tile_end(arena, d):
    # file 0 ends d bytes from the tile's end with a match on its last line, file 1 starts with one
    files = [quiet(TILE + d - 4) + b"abc\n", b"abc\n" + quiet(50), quiet(30)]
    _, per_file = check(arena, SET_AB, files, 64)
    assert [len(p) for p in per_file] == [1, 1, 0] and per_file[1] == [(0, 0, 3, 0)]
    files = [quiet(TILE + d - 3) + b"abc", b"abc\n" + quiet(50), quiet(30)]  # ... unterminated: the pad lies around the tile's end
    _, per_file = check(arena, SET_NL, files, 64)
    assert per_file[0][-1][1:] == (0, 3, 0) and per_file[1][:2] == [(0, 0, 3, 0), (0, 3, 4, 2)]


def test_state_in_lds(arena):
    """An expression of more than 64 positions walks with its state in LDS; its hit line of 300 bytes lies in the second file."""
    line = b"q" * 100 + b"abc " + b"k" * 70 + b"X" + b" abc " + b"m" * 69 + b"X" + b"z" * 49 + b"\n"
    assert len(line) == 300
    files = [b"abc\nq\n", quiet(40) + line + b"abc\n", b"r" * 70 + b"X"]
    for bs in (512, 262140):
        _, per_file = check(arena, SET_LDS, files, bs)
        # (quiet(40) is five lines: the hit line is line 5)
        assert per_file[1][:3] == [(5, 100, 103, 1), (5, 104, 175, 0), (5, 176, 179, 1)] and per_file[2] == [(0, 0, 71, 0)]


def test_two_words_of_first_byte_bitmap(arena):
    files = [b"w00k w38k abc\n", b"x\nabc w37k\n", b"w3", b"abcw31kw32k"]
    _, per_file = check(arena, SET_40, files, 64)
    assert [[p[3] for p in rows] for rows in per_file] == [[0, 38, 39], [39, 37], [], [39, 31, 32]]


def test_starts_of_match_are_unchanged(arena):
    files = [b"xaab aab\nab\nx\n", (b"aab " * 9)[:13], b"q\n", b"zaaab\nq\nab ab ab\n", b"", b"ab"]
    sc = scanner(SET_SOM)
    for bs in (8, 64):
        for limit in (0, 1):
            st, _ = check(arena, SET_SOM, files, bs, limit)  # (the starts are compared with the call without parts)
            assert st.n_parts > 0
            data, starts, ends = sr.pack(files)  # (check()'s last scans were those of the files alone)
            sc.scan(arena.place(data), len(data), buffer_size=bs, segments=(starts, ends), max_per_segment=limit, segment_parts=True)
            assert any(f > 0 for f in sc.hit_starts().tolist())


def test_errors(arena):
    from hypergrep_amd import device, utils

    sc = scanner(SET_AB)
    data = b"qb\nqb\nqb\nqb\n"
    ptr = arena.place(data)
    good = ([0, 6], [6, 12])
    for kw in ({"invert": True}, {"context": (1, 1)}, {"parts": True}, {"carry_after": 1}, {"tail": True}, {"line_base": 2}):
        with pytest.raises(ValueError):
            sc.scan(ptr, len(data), buffer_size=64, segments=good, segment_parts=True, **kw)
    with pytest.raises(ValueError, match="segments"):
        sc.scan(ptr, len(data), buffer_size=64, segment_parts=True)
    # malformed segments: nothing is scanned
    for segs, word in ((([0, 4], [3, 9]), "line start"), (([6, 0], [12, 6]), "ascending"), (([0, 6], [6, 13]), "past the buffer")):
        with pytest.raises(ValueError, match=word):
            sc.scan(ptr, len(data), buffer_size=64, segments=segs, segment_parts=True)
        assert sc.hits() == [] and sc.parts() == []
    st = sc.scan(ptr, len(data), buffer_size=64, segments=good, segment_parts=True)  # the scanner is fine afterwards
    assert st.n_hits == 4 and st.n_parts == 4 and sc.segment_parts()["first_part"].tolist() == [0, 2, 4]
    # segment_parts() after scans of any other kind
    for kw in ({}, {"parts": True}, {"context": (1, 1)}, {"segments": good}, {"segments": good, "context": (1, 1)}, {"invert": True}):
        sc.scan(ptr, len(data), buffer_size=64, **kw)
        with pytest.raises(ValueError):
            sc.segment_parts()
        assert device.lib().hg_copy_segment_parts(sc._h, None, None) == -1  # pylint: disable=protected-access
    # the databases the parts stage is not offered for: refused with the reason, nothing scanned
    text = b"foo bar\nfoo\n"
    tptr = arena.place(text)
    for pats, flags, ids, ext, word in ((["foo.{0,3000}bar"], [6], [0], None, "HG_MAX_NODES"), (["foo", "bar", "1 & 2"], [6, 6, 512], [1, 2, 3], None, "COMBINATION"),
                                        (["foo", "bar"], [6 | 1024, 6], [1, 2], None, "QUIET"),
                                        (["foo", "bar"], [6, 6], [1, 2], [None, utils.ExprExt(flags=1, min_offset=2)], "hs_expr_ext_t")):
        other = device.Scanner(device.Database(pats, flags=flags, ids=ids, ext=ext), 0)
        with pytest.raises(ValueError, match=word):
            other.scan(tptr, len(text), buffer_size=64, segments=([0, 8], [8, 12]), segment_parts=True)
        assert other.hits() == [] and other.parts() == []
        with pytest.raises(ValueError):
            other.segment_parts()
        assert other.scan(tptr, len(text), buffer_size=64, segments=([0, 8], [8, 12])).n_lines == 2  # usable afterwards
    ptr = arena.place(data)  # (the arena holds one text at a time: `text` took its place)
    st = sc.scan(ptr, len(data), buffer_size=64, segments=good, segment_parts=True)
    assert st.n_parts == 4


def test_kernel_resources():
    """The stage's kernels are in the build's table with no scratch and no spills, and every kernel the build had before the
    stage is unchanged (tests/golden/kernel_resources_before_segparts.json: that build's table), hg_parts_kernel among them:
    moving its lane routine into a shared header changed nothing."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "hypergrep_amd", "lib", "kernel_resources.json"), encoding="utf-8") as f:
        table = json.load(f)
    with open(os.path.join(root, "tests", "golden", "kernel_resources_before_segparts.json"), encoding="utf-8") as f:
        before = json.load(f)
    mine = {k: v for k, v in table.items() if "hg_segparts_" in k}
    assert len(mine) == 3 and sum("hg_segparts_kernel" in k for k in mine) == 2 and sum("hg_segparts_first_kernel" in k for k in mine) == 1
    assert not any("hg_segctx_" in k for k in mine)
    for k, v in mine.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert sum("hg_parts_kernel" in k for k in before) == 2
    for k, v in before.items():
        assert table.get(k) == v, k
