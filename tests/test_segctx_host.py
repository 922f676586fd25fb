"""The per-file context stage on the host: tests/native/segctxsim.cpp replays hypergrep_amd/csrc/hg_segctx.h over tiles of 4
to 16384 bytes (per-tile counts and the tile walk, which must agree tile by tile), and every segment's context records must
be those of the segment's bytes scanned ALONE (segctx_ref.expected): windows, clamps, the limit rule, phantoms and pads, with
pieces cut (buffer_size 8 and 64)."""
from __future__ import annotations

import subprocess

import pytest

import segctx_ref as cr
import segments_ref as sr

TILES = (4, 16, 17, 64, 1000, 16384)
BUFFER_SIZES = (8, 64)
AB = [(1, rb"ab")]
AB_NL = [(1, rb"ab"), (2, rb"\n"), (3, rb"b$")]  # id 2 matches the pad's bare newline


def check(files, tile, buffer_size, patterns, invert, limit, before, after):
    data, starts, ends = sr.pack(files)
    packed = sr.packed_records(data, starts, ends, sr.re_scan(patterns, buffer_size), buffer_size, invert)
    got = cr.replay(data, tile, buffer_size, packed, starts, ends, before, after, limit=limit, invert=invert)
    want = cr.expected(data, starts, ends, sr.re_scan(patterns, buffer_size, invert), buffer_size, before, after, limit)
    assert len(got["first_context"]) == len(files) + 1 and got["first_context"][0] == 0
    assert got["first_context"][-1] == len(got["rows"])
    for s, rows in enumerate(want):  # no segment is left out
        lo, hi = got["first_context"][s], got["first_context"][s + 1]
        assert got["rows"][lo:hi] == [tuple(r) for r in rows], (s, files[s][-20:])
        assert got["segment"][lo:hi] == [s] * (hi - lo)
    return data, packed, got


@pytest.mark.parametrize("buffer_size", BUFFER_SIZES)
@pytest.mark.parametrize("tile", TILES)
def test_every_case_equals_the_segments_scanned_alone(tile, buffer_size):
    for name, files in sr.cases(tile, buffer_size):
        for before, after in cr.CONTEXTS:
            for invert in (False, True):
                for limit in (0, 1, 2):
                    try:
                        check(files, tile, buffer_size, AB, invert, limit, before, after)
                    except AssertionError as e:
                        raise AssertionError(f"{name} invert={invert} limit={limit} context={before, after}: {e}") from e


@pytest.mark.parametrize("buffer_size", BUFFER_SIZES)
def test_under_an_expression_that_matches_the_pads_newline(buffer_size):
    for name, files in sr.cases(64, buffer_size):
        for invert in (False, True):
            for limit in (0, 1):
                try:
                    check(files, 64, buffer_size, AB_NL, invert, limit, 2, 2)
                except AssertionError as e:
                    raise AssertionError(f"{name} invert={invert} limit={limit}: {e}") from e


def test_context_stops_at_the_file_boundary_both_ways():
    # a match on the last line of file 0 and on the first line of file 1: the unclamped after-window of the first would take
    # the before-context of the second (free_from), and either would reach into the other file
    files = [b"q\nq\nq\nab\n", b"ab\nq\nq\nq\n", b"q\nq\nq\n", b"q\nq\nab"]
    data, packed, got = check(files, 16, 64, AB, False, 0, 2, 2)
    per_file = [got["rows"][got["first_context"][s]:got["first_context"][s + 1]] for s in range(4)]
    assert [[r[0] for r in rows] for rows in per_file] == [[1, 2], [1, 2], [], [0, 1]]


def test_every_file_matching_leaves_no_context():
    files = [b"ab\n"] * 300
    _, _, got = check(files, 16384, 64, AB, False, 0, 3, 3)
    assert got["rows"] == [] and got["tiles_read"] == 0
    _, _, got = check([f if i % 2 else b"" for i, f in enumerate(files)], 16384, 64, AB, False, 0, 3, 3)
    assert got["rows"] == []


@pytest.mark.parametrize("buffer_size", BUFFER_SIZES)
def test_a_phantom_piece_is_never_context(buffer_size):
    bs1 = buffer_size - 1
    for d in (0, -1, -2, 1):
        files = [b"ab\n" + (b"zq" * bs1)[:bs1 + d], b"q\nab\n"]
        data, packed, got = check(files, 16, buffer_size, AB, False, 0, 3, 3)
        n_lines = [sr.re_scan(AB, buffer_size)(f)[1] for f in files]
        assert all(r[0] < n_lines[s] for r, s in zip(got["rows"], got["segment"]))


def test_a_nul_only_last_piece_is_context_with_an_empty_record():
    files = [b"ab\n\0\0\0", b"ab\n"]
    for patterns in (AB, AB_NL):
        _, _, got = check(files, 16, 8, patterns, False, 0, 1, 1)
        assert got["rows"] == [(1, 0xFFFFFFFE, 0, 6, 0)] and got["segment"] == [0]
    # inverted under an expression that matches "\n": the piece is the one selected line, the line before it its context
    _, _, got = check([b"q\n\0\0\0", b"q\n"], 16, 8, AB_NL, True, 1, 1, 1)
    assert got["rows"] == [(0, 0xFFFFFFFE, 0, 0, 2)] and got["segment"] == [0]


def test_the_limit_ends_the_context_before_the_next_matching_piece():
    near = b"ab\nq\nab\nq\nq\n"       # the next matching piece lies within `after` of the last kept line
    far = b"ab\nq\nq\nq\nq\nab\nq\n"  # ... beyond it
    last = b"q\nab\nq\n"              # ... in the NEXT file only: nothing truncates
    _, _, got = check([near, far, last, b"ab\nq\n"], 16, 64, AB, False, 1, 1, 3)
    per_file = [[r[0] for r in got["rows"][got["first_context"][s]:got["first_context"][s + 1]]] for s in range(4)]
    assert per_file == [[1], [1, 2, 3], [0, 2], [1]]
    _, _, got = check([near, far, last, b"ab\nq\n"], 16, 64, AB, False, 2, 1, 3)
    per_file = [[r[0] for r in got["rows"][got["first_context"][s]:got["first_context"][s + 1]]] for s in range(4)]
    assert per_file == [[1, 3, 4], [1, 2, 3, 4, 6], [0, 2], [1]]


def test_tiles_without_context_are_not_read():
    files = [sr.filler(10 * 64), b"q\nab\nq\n", sr.filler(5 * 64 + 3)]
    data, starts, ends = sr.pack(files)
    packed, _ = sr.re_scan([(1, rb"ab$")], 8)(data)
    got = cr.replay(data, 64, 8, packed, starts, ends, 1, 1)
    assert [r[0] for r in got["rows"]] == [0, 2] and got["segment"] == [1, 1] and got["tiles_read"] <= 2


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (segctxsim.cpp's main), built with AddressSanitizer and UBSan: packs of 24 files
    against a piece-by-piece restatement of the rules on each file's own bytes."""
    exe = str(tmp_path / "segctxsim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DSEGCTXSIM_MAIN", "-o", exe, cr.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout
