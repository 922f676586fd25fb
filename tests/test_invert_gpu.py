"""Inverted match (grep -v) on the MI355X: hg_scan_device_invert (the invert stage, hypergrep_amd/csrc/hg_invert.hip) behind
every scan path, the file API (hg_hyperscan_invert) and the command line.  Every expectation is invert_ref's plain Python
reference (split at '\\n', cut into buffer_size - 1 pieces, trim) minus the matching lines of the oracle (oracle_py), or of the
Python `re` brute force (minlensim_py.expected_piece) for sets with combinations, QUIET or min_length, which the oracle does
not have.  Each case also asserts the complement identity with a normal scan.  Texts sit at the end of guarded buffers: a
read past them faults."""
from __future__ import annotations

import os
import random
import re

import pytest

import chunk_texts
import huge_cases
import invert_ref
import oracle_py
import regex_gen
from minlensim_py import COMBINATION, QUIET, expected_piece, exts_for

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")
TILE = 16384
LITERALS = ["needle-in-hay", "ERROR 42 failed"]  # literal tier (SINGLEMATCH, the default flags)
WORDS = [b"needle-in-hay", b"ERROR 42 failed", b"user=abc", b"12x", b"abc", b" ", b"-", b"quiet", b"zz", b"lorem ipsum dolor"]


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 20)
    yield a
    a.free()


def log_text(rng: random.Random, nbytes: int, final_newline: bool = True) -> bytes:
    """Lines of 0..~90 bytes, about a third of them with a match of LITERALS, cut to exactly nbytes."""
    out = bytearray()
    while len(out) < nbytes:
        out += b" ".join(rng.choice(WORDS) for _ in range(rng.randint(0, 6))) + b"\n"
    out = out[:nbytes]
    if nbytes:
        out[-1:] = b"\n" if final_newline else b"q"
    return bytes(out)


def oracle_matching(text, pats, flags, ids, bs, line_base):
    rc, hits, n_lines = oracle_py.scan_buffer(text, pats, flags, ids, buffer_size=bs)
    assert rc == 0
    return {line_base + h[0] for h in hits}, n_lines


def re_matching(text, pats, flags, ids, need, bs, line_base):
    """The lines with a delivered report by the Python `re` brute force (combinations, QUIET, min_length)."""
    cache, lines = {}, set()
    pcs = invert_ref.pieces(text, bs)
    for i, (_a, piece) in enumerate(pcs):
        if piece not in cache:
            cache[piece] = bool(piece) and bool(expected_piece(pats, flags, ids, need, piece))
        if cache[piece]:
            lines.add(line_base + i)
    return lines, len(pcs)


def check(arena, text, pats, flags=None, ids=None, bs=262140, line_base=0, need=None, by_re=False, min_launches=0):
    """The inverted scan equals the reference and complements the normal scan.  Returns (selected, pieces)."""
    from hypergrep_amd import device

    ids = ids or list(range(len(pats)))
    db = device.Database(pats, flags=flags, ids=ids, ext=exts_for(need) if need is not None else None)
    sc = device.Scanner(db, 0)
    ptr = arena.place(text)
    normal = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base)
    normal_lines = {h[0] for h in sc.hits()}
    inverted = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base, invert=True)
    assert normal.stream_launches >= min_launches and inverted.stream_launches >= min_launches
    got = sc.hits()
    starts = sc.hit_starts()
    if by_re:
        matching, n_lines = re_matching(text, pats, flags, ids, need or [None] * len(pats), bs, line_base)
    else:
        matching, n_lines = oracle_matching(text, pats, flags, ids, bs, line_base)
    assert normal_lines == matching
    assert got == invert_ref.expected(text, bs, matching, line_base), (pats, bs, len(text))
    assert inverted.n_hits == len(got) and not starts.any()
    assert inverted.n_lines == normal.n_lines == n_lines
    assert (inverted.n_candidates, inverted.n_raw_hits) == (normal.n_candidates, normal.n_raw_hits)
    assert len(normal_lines) + inverted.n_hits == inverted.n_lines  # the complement identity
    # the normal path is untouched by an inverted scan on the same scanner
    again = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base)
    assert {h[0] for h in sc.hits()} == normal_lines and again.n_hits == normal.n_hits and again.invert_us == 0
    return inverted.n_hits, n_lines


@pytest.mark.parametrize("bs", [262140, 4097, 1025, 100, 64])  # buffer_size - 1: above a tile, dividing 16384 (4096, 1024) and not (99, 63)
def test_three_tiles_and_a_ragged_tail(arena, bs):
    rng = random.Random(bs)
    text = log_text(rng, 3 * TILE + 5, final_newline=False)  # 49157 bytes; the last line has no '\n'
    assert len(text) == 49157 and any(text[k * TILE - 1] != 10 and text[k * TILE] != 10 for k in (1, 2, 3))  # a line crosses a tile boundary
    selected, n = check(arena, text, LITERALS, bs=bs)
    assert 0 < selected < n
    check(arena, text, LITERALS, bs=bs, line_base=(1 << 33) + 7)


@pytest.mark.parametrize("bs", [64, 4096, 262140])
def test_a_long_line_without_newline(arena, bs):
    """40 KiB in one line: the piece cuts (every buffer_size - 1 bytes) against the tile cuts (every 16 KiB)."""
    rng = random.Random(5)
    body = bytearray(rng.choice(b"abcdefgh ") for _ in range(40 << 10))
    for at in (100, 16380, 20000, 32768 - 6, 40000):
        body[at:at + 13] = b"needle-in-hay"
    selected, n = check(arena, bytes(body), LITERALS, bs=bs)
    assert n == -(-len(body) // (bs - 1)) and 0 <= selected < n
    # ... and with lines around it, a NUL inside it, and a newline at its end
    body[30000] = 0
    check(arena, b"abc\nneedle-in-hay\n" + bytes(body) + b"\nlast", LITERALS, bs=bs)


@pytest.mark.parametrize("text", [b"", b"\n", b"q", b"needle-in-hay\n\n", b"\n\n\n", b"\n" * 40, b"\0abc\nab\0needle-in-hay\n\0\0needle-in-hay\n\0\n\0\0\0", b"abc\nneedle-in-hay",
                                  b"0123456789abcde"],
                         ids=["0", "newline", "1", "15", "empty3", "empty40", "nuls", "no-final-newline", "15b"])
def test_small_buffers_empty_lines_and_nuls(arena, text):
    for bs in (262140, 8, 3):
        selected, n = check(arena, text, LITERALS + ["abc"], bs=bs, line_base=3)
        if text == b"\n\n\n" and bs == 262140:
            assert (selected, n) == (3, 3)


def test_every_line_matches_and_no_line_matches(arena):
    rng = random.Random(3)
    text = b"".join(b"x needle-in-hay %d\n" % rng.randint(0, 10**rng.randint(1, 9)) for _ in range(2500))  # > 3 tiles
    assert len(text) > 3 * TILE
    assert check(arena, text, LITERALS) == (0, 2500)
    assert check(arena, text, ["no-such-thing", "neither-this"]) == (2500, 2500)
    assert check(arena, text, LITERALS, bs=10)[0] > 0  # pieces of 9 bytes: most hold no match


def chunked_text(rng: random.Random) -> bytes:
    """More than 2048 tiles (chunk_texts): lines of log_text around the two cuts, a few repeated lines between them."""
    parts = [log_text(rng, 40000).splitlines(keepends=True) for _ in range(4)]
    parts[2].append(b"abc zz needle-in-hay " + b"q" * 300 + b" ERROR 42 failed\n")  # the line across the second cut
    fillers = [b"lorem ipsum dolor " * 45 + b"\n", b"zz - needle-in-hay " + b"quiet " * 100 + b"\n", b"12x " * 200 + b"\n"]
    return chunk_texts.build(parts, fillers)


def test_pipeline_chunks_and_segmented_scans(arena, monkeypatch):
    """A buffer the engine scans in several pipeline chunks, or in segments whose hits are put one after the other: the invert
    stage runs once over the whole buffer's tile states and the concatenated hits."""
    from hypergrep_amd import device

    rng = random.Random(29)
    text = log_text(rng, (40 << 14) + 123)
    sc = device.Scanner(device.Database(LITERALS + ["abc"], flags=[6] * 3, ids=[0, 1, 2]), 0)
    raw = sc.scan(arena.place(text), len(text), buffer_size=1000).n_raw_hits
    assert raw > 4000
    for env in ({"HG_HIT_LIMIT": str(raw * 3 // 4)}, {"HG_HIT_LIMIT": str(raw * 11 // 20)}):  # (segments are 16 tiles at least)
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            selected, n = check(arena, text, LITERALS + ["abc"], [6] * 3, bs=1000)
            assert 1000 < selected < n, env
    # three pipeline chunks of 1024 tiles (the engine honours no smaller one): the matching lines by the `re` brute force, once
    # per distinct line
    big = device.GuardedArena(chunk_texts.SIZE + 64)
    try:
        with monkeypatch.context() as m:
            for k, v in chunk_texts.CHUNK_ENV.items():
                m.setenv(k, v)
            selected, n = check(big, chunked_text(rng), LITERALS + ["abc"], [6] * 3, bs=1000, by_re=True, min_launches=2)
            assert 1000 < selected < n
    finally:
        big.free()


def test_quiet_combination_and_min_length(arena):
    rng = random.Random(17)
    frags = [b"foo", b"bar", b"quiet", b"abc1", b"abc12345", b"zz", b" ", b"-", b"x"]
    # three tiles and more (the hit list is merged across rows and tiles); few distinct lines: the brute force runs once per distinct piece
    text = b"".join(b" ".join(rng.choice(frags) for _ in range(rng.randint(0, 3))) + b" " + b"." * 60 + b"\n" for _ in range(800))
    assert len(text) > 3 * TILE
    # a QUIET-only line is selected: "quiet" reports only to the combination, which also needs "foo"
    pats, flags, ids = ["foo", "quiet", "101 & 102"], [6, 6 | QUIET, COMBINATION], [101, 102, 200]
    selected, n = check(arena, text, pats, flags, ids, by_re=True)
    quiet_only = sum(1 for line in text.split(b"\n")[:-1] if b"quiet" in line and b"foo" not in line)
    assert quiet_only > 20 and selected >= quiet_only
    # a combination alone decides: lines with foo but not bar
    check(arena, text, ["foo", "bar", "1 & !2"], [6 | QUIET, 6 | QUIET, COMBINATION], [1, 2, 9], by_re=True)
    check(arena, text, ["foo", "bar", "1 & !2"], [6 | QUIET, 6 | QUIET, COMBINATION], [1, 2, 9], bs=12, by_re=True)
    # min_length removes a line's only report: abc[0-9]+ must span 6 bytes, "abc1" lines go to the selected side
    with_filter, _ = check(arena, text, [r"abc[0-9]+", "needle-in-hay"], [6, 6], [1, 2], need=[6, None], by_re=True)
    without, _ = check(arena, text, [r"abc[0-9]+", "needle-in-hay"], [6, 6], [1, 2])
    assert with_filter > without


@pytest.mark.parametrize("kind", ["literal", "always_on", "huge"])
def test_behind_every_scan_path(arena, kind):
    from hypergrep_amd import device

    rng = random.Random(len(kind))
    pats = {"literal": LITERALS, "always_on": [r"[0-9]+x", r"^[a-c]+"], "huge": [r"needle[^\n]{0,5000}thread", "ERROR 42 failed"]}[kind]
    flags = [6] * len(pats) if kind != "literal" else None
    info = device.Database(pats, flags=flags).info()
    if kind == "literal":
        assert info["n_literal_anchored"] == 2 and info["n_always_on"] == 0
    elif kind == "always_on":
        assert info["n_always_on"] == 2
    else:
        assert pats[0] in huge_cases.ACCEPTED_HUGE  # (more than 1024 positions: the sparse tables and routines of hg_huge.hip)
    text = log_text(rng, 2 * TILE + 777)
    if kind == "huge":
        text = text[:9000] + b"\nneedle " + b"q" * 3000 + b" thread\nneedle " + b"q" * 5100 + b" thread\n" + text[9000:]
    for bs in (262140, 50):
        selected, n = check(arena, text, pats, flags, bs=bs)
        assert 0 < selected < n


def test_random_set_on_mixed_text(arena):
    import hypergrep_amd

    rng = random.Random(2024)
    pats = []
    while len(pats) < 20:
        p = regex_gen.random_pattern(rng)
        if hypergrep_amd.check_compatibility([p], flags=[6]) == 0 and oracle_py.check_patterns([p], [6], [0]) == 0:
            pats.append(p)
    text = bytearray()
    while len(text) < 64 << 10:
        text += regex_gen.random_line(rng, 60) if rng.random() < 0.8 else rng.choice(WORDS) + b"\0" * rng.randint(0, 2) + regex_gen.random_line(rng, 200)
        text += b"\n"
    text = bytes(text[:64 << 10])
    for bs in (262140, 33):
        check(arena, text, pats, [6] * 20, bs=bs)


def test_file_api(arena):
    """hg_hyperscan_invert on a plain and a gzip file: the same rows, equal to the reference; max_match_count stops it."""
    import hypergrep_amd

    data = open(os.path.join(FILES, "samplefile.txt"), "rb").read()
    matching, _ = oracle_matching(data, ["bar"], [14], [0], 262140, 0)
    want = [(line, rid, data[a:a + n]) for line, rid, _to, a, n in invert_ref.expected(data, 262140, matching)]
    assert want and len(want) + len(matching) == len(invert_ref.pieces(data, 262140))

    def rows_of(name, **kwargs):
        rows = []
        rc = hypergrep_amd.scan(os.path.join(FILES, name), ["bar"], lambda m, c: rows.extend((m[i].line_number, m[i].id, m[i].line) for i in range(c)), invert=True, **kwargs)
        assert rc == 0
        return rows

    plain, gz = rows_of("samplefile.txt"), rows_of("samplefile.txt.gz")
    assert plain == gz == want
    assert rows_of("samplefile.txt", buffer_count=1) == want
    # a file with more selected lines than the limit
    big = os.path.join(FILES, "greptest1.txt")
    all_rows = rows_of("greptest1.txt")
    assert len(all_rows) > 3 and rows_of("greptest1.txt", max_match_count=3) == all_rows[:3]
    assert hypergrep_amd.grep(big, ["bar"], invert=True, max_match_count=3)[0] == [(n + 1, line.decode()) for n, _id, line in all_rows[:3]]


@pytest.mark.parametrize("pattern", ["foo", "bar<"])
def test_command_line(arena, pattern, capsys, monkeypatch):
    from hypergrep_amd import multiscanner

    path = os.path.join(FILES, "greptest1.txt")
    lines = open(path, encoding="utf-8").read().splitlines(keepends=True)
    want = [(i + 1, line) for i, line in enumerate(lines) if not re.search(pattern, line)]
    assert 0 < len(want) < len(lines)
    for argv, out in ((["-v", "-n"], "".join(f"{n}:{line}" for n, line in want)), (["-v", "-c"], f"{len(want)}\n"), (["-v", "-o"], ""),
                      (["-v", "-m", "2"], "".join(line for _n, line in want[:2]))):
        monkeypatch.setattr("sys.argv", ["hyperscanner", "-P"] + argv + [pattern, path])
        with pytest.raises(SystemExit) as exit_info:
            multiscanner.main()
        assert capsys.readouterr().out == out, argv
        assert exit_info.value.code == 0  # (-o -v prints nothing, and the selected lines still decide the exit code, as in GNU grep)
