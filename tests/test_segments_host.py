"""The segment stage on the host: tests/native/segsim.cpp replays hypergrep_amd/csrc/hg_segments.h over tiles of 4 to 16384
bytes, and every segment's records, line count and selected count must be those of the segment's bytes scanned ALONE
(segments_ref.expected): line bases, the mapping, the summaries, the limit and the phantom rule, with pieces cut
(buffer_size 8 and 64)."""
from __future__ import annotations

import pytest

import segments_ref as sr

TILES = (4, 16, 17, 64, 1000, 16384)
BUFFER_SIZES = (8, 64)
AB = [(1, rb"ab")]
AB_NL = [(1, rb"ab"), (2, rb"\n"), (3, rb"b$")]  # id 2 matches the pad's bare newline


def check(files, tile, buffer_size, patterns, invert, limit):
    data, starts, ends = sr.pack(files)
    packed = sr.packed_records(data, starts, ends, sr.re_scan(patterns, buffer_size), buffer_size, invert)
    got = sr.replay(data, tile, buffer_size, packed, starts, ends, limit=limit, invert=invert)
    want = sr.expected(data, starts, ends, sr.re_scan(patterns, buffer_size, invert), limit)
    assert len(got["first_record"]) == len(files) + 1 and got["first_record"][0] == 0
    assert got["first_record"][-1] == len(got["records"])
    for s, (records, n_lines, n_selected) in enumerate(want):  # no segment is left out
        lo, hi = got["first_record"][s], got["first_record"][s + 1]
        assert got["records"][lo:hi] == [tuple(r) for r in records], (s, files[s][-20:])
        assert got["segment"][lo:hi] == [s] * (hi - lo)
        assert got["n_lines"][s] == n_lines, s
        assert got["n_selected"][s] == n_selected, s
    return data, packed, got


@pytest.mark.parametrize("buffer_size", BUFFER_SIZES)
@pytest.mark.parametrize("tile", TILES)
def test_every_case_equals_the_segments_scanned_alone(tile, buffer_size):
    for name, files in sr.cases(tile, buffer_size):
        for patterns in (AB, AB_NL):
            for invert in (False, True):
                for limit in (0, 1, 2, 10 ** 6):
                    try:
                        check(files, tile, buffer_size, patterns, invert, limit)
                    except AssertionError as e:
                        raise AssertionError(f"{name} invert={invert} limit={limit} patterns={len(patterns)}: {e}") from e


@pytest.mark.parametrize("buffer_size", BUFFER_SIZES)
def test_phantom_pieces_are_dropped_and_not_counted(buffer_size):
    bs1 = buffer_size - 1
    # a last line of bs1 - 1 bytes: the pad's "\n" is a piece of its own, one byte past the content, and id 2 matches it
    files = [(b"ab" * bs1)[:bs1 - 1], b"ab\n"]
    data, packed, got = check(files, 16, buffer_size, AB_NL, False, 0)
    phantom = [r for r in packed if r[3] >= len(files[0]) and r[3] < len(files[0]) + 2]
    assert phantom and phantom[0][1] == 2, "the packed scan must report the pad's newline for this test to mean anything"
    assert got["n_lines"] == [1, 1]
    assert len(got["records"]) == len(packed) - len(phantom)
    # ... and does not count against the limit of the next segment or of its own
    check(files, 16, buffer_size, AB_NL, False, 1)
    check(files, 16, buffer_size, AB_NL, True, 1)
    # a last line of exactly bs1 bytes leaves the piece "\0\n": an inverted scan selects it, the stage drops it
    files = [(b"zq" * bs1)[:bs1], b"q\n"]
    data, packed, got = check(files, 16, buffer_size, AB, True, 0)
    assert len(packed) == 3 and len(got["records"]) == 2 and got["n_lines"] == [1, 1]


def test_a_nul_only_last_piece_keeps_its_empty_record_when_inverted():
    files = [b"ab\n\0\0\0", b"ab\n"]
    data, packed, got = check(files, 16, 8, AB, True, 0)
    assert got["records"] == [(1, 0xFFFFFFFF, 0, 6, 0)] and got["n_lines"] == [2, 1]


@pytest.mark.parametrize("buffer_size", BUFFER_SIZES)
def test_a_nul_only_last_piece_under_an_expression_that_matches_the_pads_newline(buffer_size):
    # packed, the piece's scanned bytes are the pad's "\n" and id 2 reports there; alone the piece is empty and selected
    files = [b"ab\n\0\0\0", b"ab\n", b"\0", b"q\n\0\0", b""]
    data, starts, ends = sr.pack(files)
    hits, _ = sr.re_scan(AB_NL, buffer_size)(data)
    assert sum(1 for h in hits if h[1] == 2 and any(e <= h[3] < e + 2 for e in ends[:4])) == 3, "the packed scan must report in the pads"
    for limit in (0, 1, 2):
        for invert in (False, True):
            _data, _packed, got = check(files, 16, buffer_size, AB_NL, invert, limit)
    assert got["n_selected"][2] == 1 and got["records"][got["first_record"][2]] == (0, 0xFFFFFFFF, 0, 1, 0)


def test_tiles_without_a_boundary_are_not_walked():
    files = [sr.filler(10 * 64), b"ab\n", sr.filler(5 * 64 + 3)]
    data, starts, ends = sr.pack(files)
    packed, _ = sr.re_scan(AB, 8)(data)
    got = sr.replay(data, 64, 8, packed, starts, ends)
    assert got["tiles_walked"] <= 3  # the tiles of offset 0, of the boundaries at 640 / 643; none at the text's end
    assert got["base"] == [0, sr.re_scan(AB, 8)(data[:640])[1], sr.re_scan(AB, 8)(data[:643])[1]]


def test_starts_of_match_follow_the_surviving_records():
    files = [b"ab ab\n" * 3, (b"ab" * 7)[:6], b"ab\nab\n"]
    data, starts, ends = sr.pack(files)
    packed, _ = sr.re_scan(AB_NL, 8)(data)
    froms = [1000 + i for i in range(len(packed))]
    got = sr.replay(data, 16, 8, packed, starts, ends, limit=2, froms=froms)
    kept = [i for i in range(len(packed)) if 1000 + i in got["from"]]
    assert got["from"] == [1000 + i for i in kept] and len(kept) == len(got["records"]) < len(packed)
    for at, i in enumerate(kept):  # the same record, made file-relative
        assert got["records"][at][1:3] == packed[i][1:3]


@pytest.mark.parametrize("starts,ends,bit", [
    ([0, 6, 3], [3, 9, 6], 1),   # not ascending
    ([0, 3], [6, 9], 1),         # overlapping
    ([3, 0], [3, 3], 1),         # a start before its predecessor's end
    ([0, 6], [3, 13], 2),        # an end past the buffer
    ([0, 4], [3, 9], 4),         # a start that does not follow a newline
    ([0, 6], [7, 9], 1),         # an end past the next start
])
def test_malformed_segments_are_refused(starts, ends, bit):
    data = b"ab\nab\nab\nab\n"
    with pytest.raises(sr.Malformed) as e:
        sr.replay(data, 16, 8, [], starts, ends)
    assert e.value.args[0] & bit
