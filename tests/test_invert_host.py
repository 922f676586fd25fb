"""Inverted match (grep -v) on the host: the scalar routines of hypergrep_amd/csrc/hg_invert.h (the piece walk of one tile,
the first piece number of a tile from the scan's tile states, the membership test against the ordered hit lines) replayed
through tests/native/invertsim.cpp over random tile sizes and buffer sizes, against a plain Python reference that knows
nothing of tiles, with the oracle's matching lines; the new names of the C ABI and of the Python layers; the command line.
No GPU needed."""
from __future__ import annotations

import ctypes
import inspect
import os
import random

import pytest

import invert_ref
import oracle_py

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ["foo", "ba+r", r"^[0-9]+$", r"x\b"]
FLAGS = [6, 6, 6, 6]  # DOTALL | MULTILINE, no SINGLEMATCH: several reports per line


def random_text(rng: random.Random, nbytes: int) -> bytes:
    """Lines of wildly different lengths with matches, NULs (leading, inner) and empty lines."""
    words = [b"foo", b"bar", b"baaar", b"123", b"x", b" ", b"qq", b"\0", b"", b"zzzzzzzzzzzz", b"x y"]
    out = bytearray()
    while len(out) < nbytes:
        r = rng.random()
        if r < 0.1:
            line = b""
        elif r < 0.15:
            line = bytes(rng.choice(b"ab \0x") for _ in range(rng.randint(100, 700)))
        else:
            line = b"".join(rng.choice(words) for _ in range(rng.randint(1, 6)))
        out += line + b"\n"
    out = bytes(out[:nbytes])
    return out if rng.random() < 0.5 else out.rstrip(b"\n") + b"q"


def oracle_lines(data: bytes, buffer_size: int, line_base: int = 0):
    rc, hits, n_lines = oracle_py.scan_buffer(data, PATTERNS, FLAGS, [1, 2, 3, 4], buffer_size=buffer_size)
    assert rc == 0
    return [line_base + h[0] for h in hits], n_lines


@pytest.mark.parametrize("seed", range(12))
def test_tile_walk_against_the_python_reference(seed):
    rng = random.Random(1000 + seed)
    data = random_text(rng, rng.choice([0, 1, 15, 700, 3000, 6000]))
    for _ in range(6):
        tile = rng.choice([1, 7, 16, 64, 100, 256, 1024, 16384])
        buffer_size = rng.choice([2, 3, 8, 17, 65, 101, 257, 1025, 262140])
        line_base = rng.choice([0, 0, 5, 1 << 33])
        lines, n_lines = oracle_lines(data, buffer_size, line_base)
        assert lines == sorted(lines)
        got, n_pieces = invert_ref.replay(data, tile, buffer_size, lines, line_base)
        assert n_pieces == n_lines == len(invert_ref.pieces(data, buffer_size))
        assert got == invert_ref.expected(data, buffer_size, lines, line_base), (seed, tile, buffer_size)
        assert len(set(lines)) + len(got) == n_pieces  # the complement identity


def test_fixed_cases():
    cases = [
        (b"", 64), (b"\n", 64), (b"\n\n\n", 64), (b"a", 64), (b"foo\nqq\nbar", 64), (b"\0foo\nq\0foo\n\0\0\n", 64),
        (b"q" * 40 + b"foo" + b"q" * 57, 10), (b"q" * 40 + b"foo" + b"q" * 57 + b"\n", 11), (b"q" * 99 + b"\n", 101), (b"q" * 100 + b"\n", 101),
    ]
    for data, buffer_size in cases:
        lines, n_lines = oracle_lines(data, buffer_size)
        for tile in (1, 16, 32, 16384):
            got, n_pieces = invert_ref.replay(data, tile, buffer_size, lines)
            assert (got, n_pieces) == (invert_ref.expected(data, buffer_size, lines), n_lines), (data, buffer_size, tile)
    # every piece matches / none does
    data = b"foo\n" * 50
    lines, _ = oracle_lines(data, 64)
    assert invert_ref.replay(data, 16, 64, lines)[0] == []
    assert len(invert_ref.replay(data, 16, 64, [])[0]) == 50
    # leading NULs are skipped (the trim rule); a piece of NULs only has no scanned bytes and is selected with len 0
    assert invert_ref.replay(b"\0qq\n\0\0\0", 16, 64, [])[0] == [(0, invert_ref.HG_ID_INVERT, 0, 1, 3), (1, invert_ref.HG_ID_INVERT, 0, 7, 0)]


def test_new_names_are_declared_exported_and_loadable():
    import hypergrep_amd
    from hypergrep_amd import device, utils

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    assert "#define HG_ID_INVERT 0xFFFFFFFFu" in header
    assert "n_lines" in header and "Complement identity" in header
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_scan_device_invert", "hg_hyperscan_invert"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    assert device.HG_ID_INVERT == utils.HG_ID_INVERT == 0xFFFFFFFF
    assert hasattr(device.lib(), "hg_scan_device_invert")
    for fn in (device.Scanner.scan, hypergrep_amd.scan, hypergrep_amd.grep):
        assert inspect.signature(fn).parameters["invert"].default is False
    assert device.HgScanResult.invert_us.offset == 76 and ctypes.sizeof(device.HgScanResult) == 80
    # without a GPU the file entry point fails as the others do (no CPU path); a missing file is reported first
    called = []
    rc = hypergrep_amd.scan(os.path.join(REPO, "no", "such", "file"), ["foo"], lambda m, c: called.append(c), invert=True)
    assert rc == 6 and not called  # HYPERSCANNER_GZ_OPEN


def test_command_line_accepts_invert_match(monkeypatch):
    from hypergrep_amd import multiscanner

    for argv in (["-v", "foo", "f"], ["--invert-match", "foo", "f"], ["-vn", "foo", "f"], ["-c", "-v", "-e", "foo", "f"]):
        assert multiscanner.parse_args(argv).invert_match is True
    assert not hasattr(multiscanner.parse_args(["foo", "f"]), "invert_match")  # (the namespace of other command lines is unchanged)
    seen = {}

    def fake_parallel_grep(**kwargs):
        seen.update(kwargs)
        return 0

    monkeypatch.setattr(multiscanner, "parallel_grep", fake_parallel_grep)
    for argv, want in ((["hyperscanner", "-v", "-n", "foo", "f"], True), (["hyperscanner", "-n", "foo", "f"], False)):
        monkeypatch.setattr("sys.argv", argv)
        with pytest.raises(SystemExit) as exit_info:
            multiscanner.main()
        assert exit_info.value.code == 0 and seen["invert_match"] is want and seen["with_line_number"] is True


def test_only_matching_with_invert_prints_nothing(monkeypatch, capsys, tmp_path):
    """-o -v: a selected line has no matched part.  The sink drops the rows; counting still counts (GNU grep's -c -o -v)."""
    import hypergrep_amd
    from hypergrep_amd import multiscanner, utils

    path = tmp_path / "f.txt"
    path.write_text("foo\nbar\nqux\n")
    calls = []

    def fake_scan(file, patterns, callback, **kwargs):  # the file API without a GPU: it hands over the lines without "foo"
        calls.append(kwargs)
        batch = (utils.Result * 2)(utils.Result(utils.HG_ID_INVERT, 1, b"bar\n"), utils.Result(utils.HG_ID_INVERT, 2, b"qux\n"))
        callback(batch, 2)
        return 0

    monkeypatch.setattr(utils, "scan", fake_scan)
    assert hypergrep_amd.grep(str(path), ["foo"], invert=True) == ([(2, "bar\n"), (3, "qux\n")], 0)
    assert hypergrep_amd.grep(str(path), ["foo"], invert=True, only_matching=True) == ([], 0)
    assert hypergrep_amd.grep(str(path), ["foo"], invert=True, only_matching=True, count_only=True) == (2, 0)
    assert all(k["invert"] is True for k in calls)
    rc = multiscanner.parallel_grep([str(path)], ["foo"], only_matching=True, invert_match=True)
    assert capsys.readouterr().out == "" and rc == 0  # nothing printed; lines were selected (GNU grep's exit code)
    rc = multiscanner.parallel_grep([str(path)], ["foo"], only_matching=True, invert_match=True, files_with_matches=True)
    assert capsys.readouterr().out == f"{path}\n" and rc == 0
    rc = multiscanner.parallel_grep([str(path)], ["foo"], with_line_number=True, invert_match=True)
    assert capsys.readouterr().out == "2:bar\n3:qux\n" and rc == 0
    rc = multiscanner.parallel_grep([str(path)], ["foo"], count_results=True, invert_match=True)
    assert capsys.readouterr().out == "2\n" and rc == 0
