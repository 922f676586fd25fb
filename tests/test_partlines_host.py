"""The parts gather on the host: tests/native/partlinesim.cpp replays hypergrep_amd/csrc/hg_partlines.h (the entry pass, the entry
layout, the copy pass's 16-byte chunks over output spans of 16 and 64 bytes) and must equal partlines_ref's plain Python
reference byte for byte: every flag combination with and without marks, pieces shorter than lines, packs of files, starts above
2^32, the decimal widths of both numbers, marks of 0, 1, 15 and 16 bytes, every alignment of a chunk's source and destination,
and entries of no bytes between others.  The reference's print-ready forms are held against the local GNU grep; the replay also
runs as a sanitized program of its own; the C ABI and the Python layer have the new names.  No GPU needed."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import pytest

import invert_ref
import partlines_ref as pr
import parts_ref
import segments_ref as sr

REPO = pr.REPO
TILES = (16, 64)
A = 14  # DOTALL | MULTILINE | SINGLEMATCH
SET = (["abc", "[0-9]+x|q"], [A, A])
TEXT = (b"xx abc\nq\n\nlong line without a match, longer than one sixteen-byte chunk of output\nabc abc 12x and a tail of the line that is long enough\nzz\n" * 3
        + b"q\0tail abc\n\0\0\0\nabc\n" + b"w" * 70 + b" abc unterminated q")
MARKS = ((b"", b""), (b"<", b">"), (b"[0123456789abcd", b"0123456789abcde]"), (b"{0123456789abcde", b"}"))  # lengths 0, 1, 15, 16


def scan(data, bs, pset=SET, line_base=0, segment=0):
    """(records [(line, start, len, segment)], parts [(line, from, to, pattern, segment)]) of a text scanned alone: the lines
    in which an expression matches (two records on each, as two reports would leave) and parts_ref's parts of them."""
    lines = parts_ref.matching_lines(data, bs, pset[0], pset[1], line_base)
    pieces = invert_ref.pieces(data, bs)
    records = [(q, pieces[q - line_base][0], len(pieces[q - line_base][1]), segment) for q in lines for _ in (0, 1)]
    parts = [p + (segment,) for p in parts_ref.expected(data, bs, pset[0], pset[1], lines, line_base)]
    return records, parts


def check(data, tile, bs, flags, mark=(b"", b""), byte_base=0, line_base=0, base=0):
    records, parts = scan(data, bs, line_base=line_base)
    pieces = {k: (S, start + base, n) for k, (S, start, n) in pr.pieces_of(data, bs, line_base).items()}
    want, arrays = pr.expected(data, pieces, parts, flags, mark, byte_base)
    got, got_arrays = pr.replay(data, tile, records, parts, flags, mark, byte_base, base=base)
    assert got == want, (flags, tile, bs, mark)
    assert got_arrays["line_number"] == arrays["line_number"] and got_arrays["kind"] == arrays["kind"] and got_arrays["pattern"] == arrays["pattern"]
    return got, parts


@pytest.mark.parametrize("bs", [262140, 24, 8])
@pytest.mark.parametrize("tile", TILES)
def test_every_flag_combination_equals_the_reference(tile, bs):
    for flags in pr.ALL_FLAGS:
        for mark in MARKS[:2]:
            got, parts = check(TEXT, tile, bs, flags, mark, byte_base=7 if flags & pr.BYTE_OFFSET else 0, line_base=3)
            if flags == 0 and mark == (b"", b""):  # the identity
                assert len(got) == len(parts) and sum(map(len, got)) == sum(p[2] - p[1] for p in parts)
            if flags == pr.LINE and mark == (b"", b""):  # line mode alone: the pieces that have parts, as they are
                pieces = pr.pieces_of(TEXT, bs, 3)
                assert b"".join(got) == b"".join(TEXT[S:S + n] for (_s, q), (S, _a, n) in sorted(pieces.items()) if q in {p[0] for p in parts})


@pytest.mark.parametrize("mark", MARKS)
def test_mark_lengths(mark):
    for flags in (0, pr.LINE, 7, 15):
        got, _ = check(TEXT, 16, 64, flags, mark)
        assert all(mark[0] in e and mark[1] in e for e in got)


def test_the_issue_s_example():
    data = b"foo abc bar abc\n"
    records, parts = scan(data, 64)
    assert pr.replay(data, 16, records, parts, pr.NUMBER | pr.BYTE_OFFSET | pr.TERMINATE)[0] == [b"1:4:abc\n", b"1:12:abc\n"]
    got, arrays = pr.replay(data, 16, records, parts, pr.LINE | pr.TERMINATE, pr.COLOR)
    assert pr.joined(got, arrays) == [b"foo \x1b[01;31m\x1b[Kabc\x1b[m\x1b[K bar \x1b[01;31m\x1b[Kabc\x1b[m\x1b[K\n"] and arrays["kind"] == [pr.FIRST, pr.LAST]


@pytest.mark.parametrize("tile", TILES)
def test_starts_above_4_gib(tile):
    for base in ((1 << 32) + 16, (5 << 32) + 4):
        for flags in pr.ALL_FLAGS:
            check(TEXT, tile, 64, flags, (b"<<", b">>"), base=base)
            check_files([b"abc\nq\n", b"q\nabc", b"", b"abc\n" + b"z" * 40 + b" 7x\n"], tile, 64, flags, base=base)


def check_files(files, tile, bs, flags, mark=(b"", b""), base=0):
    data, starts, _ends = sr.pack(files)
    records, parts, pieces = [], [], {}
    for s, f in enumerate(files):
        r, p = scan(f, bs, segment=s)
        records += r
        parts += p
        pieces.update(pr.pieces_of(f, bs, segment=s, at=starts[s]))
    want, arrays = pr.expected(data, pieces, parts, flags, mark)
    got, got_arrays = pr.replay(data, tile, records, parts, flags, mark, seg_start=starts, base=base)
    assert got == want, (flags, tile, bs)
    assert got_arrays == arrays
    return got, arrays


@pytest.mark.parametrize("bs", [64, 8])
@pytest.mark.parametrize("tile", TILES)
def test_packs_of_files(tile, bs):
    for name, files in sr.cases(64, bs):
        if sum(map(len, files)) > 3000:  # (the tile-boundary cases of the segment stage: nothing this stage depends on)
            continue
        for flags in (0, 7, 8, 15):
            try:
                check_files(files, tile, bs, flags, (b"<", b">") if flags & 1 else (b"", b""))
            except AssertionError as e:
                raise AssertionError(f"{name} flags={flags}: {e}") from e


def test_one_line_files_that_all_hold_line_0():
    got, arrays = check_files([b"abc\n", b"abc\n", b"", b"abc q"], 16, 64, 15, (b"<", b">"))
    assert pr.joined(got, arrays) == [b"1:0:<abc>\n", b"1:0:<abc>\n", b"1:0:<abc> <q>\n"]
    assert arrays["kind"] == [3, 3, 1, 2] and arrays["segment"] == [0, 1, 3, 3]


def test_decimal_widths_of_both_numbers():
    lib = pr.lib()
    for d in range(1, 20):
        assert lib.partlinesim_digits(10 ** d - 1) == d and lib.partlinesim_digits(10 ** d) == d + 1
    assert lib.partlinesim_digits(0) == 1 and lib.partlinesim_digits(2 ** 32 - 1) == 10 and lib.partlinesim_digits(2 ** 32) == 10 and lib.partlinesim_digits(2 ** 64 - 1) == 20
    data = b"abc\nabc\nabc q\n"  # lines n, n + 1, n + 2 are numbered n + 1 ..; the parts' offsets are byte_base + 0, 4, 8, 12
    for edge in (9, 99, 2 ** 32 - 1, 2 ** 64 - 1):
        for flags in (pr.NUMBER, pr.BYTE_OFFSET, 7, 15):
            got, _ = check(data, 16, 64, flags, line_base=edge - 2, byte_base=edge - 4)
            if flags & pr.NUMBER and not flags & pr.BYTE_OFFSET:
                assert [e.split(b":")[0] for e in got[:3]] == [str(edge - 1).encode(), str(edge).encode(), str((edge + 1) % 2 ** 64).encode()]
            if flags == pr.BYTE_OFFSET:
                assert [e.split(b":")[0] for e in got] == [str((edge - 4 + o) % 2 ** 64).encode() for o in (0, 4, 8, 12)]


def test_chunks_at_every_alignment_of_source_and_destination():
    """A part of 70 bytes whose first byte lies at text offset s (mod 16 all residues, so mod 4 all four) and at output offset d
    (the mark in front of it has d bytes): its inner chunks are the aligned-dword path, its edges the byte path."""
    body = bytes(range(65, 65 + 26)) * 3
    for s in range(16):
        data = b"." * s + body[:70] + b"!" * 21 + b"\n"
        records = [(0, 0, len(data), 0)]
        for d in range(17):
            parts = [(0, s, s + 70, 0, 0)]
            for flags in (0, pr.LINE):
                mark = (b"m" * d, b"")
                want, _ = pr.expected(data, {(0, 0): (0, 0, len(data))}, parts, flags, mark)
                assert pr.replay(data, 64, records, parts, flags, mark)[0] == want, (s, d, flags)
    # ... and a gap and a trail of 40 bytes each at every source alignment
    for s in range(4):
        data = b"#" * s + b"g" * 40 + b"PART" + b"t" * 40 + b"\n"  # (the piece begins at s)
        records = [(0, s, len(data) - s, 0)]
        pieces = {(0, 0): (s, s, len(data) - s)}
        parts = [(0, 40, 44, 0, 0)]
        for d in range(16):
            mark = (b"", b"x" * d)
            assert pr.replay(data, 16, records, parts, pr.LINE, mark)[0] == pr.expected(data, pieces, parts, pr.LINE, mark)[0], (s, d)


def test_entries_of_no_bytes_between_others():
    """Parts whose piece has no record have no bytes; their neighbours keep theirs, and the lane that lands on a shared offset
    takes the last entry there."""
    data = b"abc abc\nq\nabc\n"
    records = [(0, 0, 8, 0), (2, 10, 4, 0)]
    parts = [(0, 0, 3, 0, 0), (0, 4, 7, 0, 0), (1, 0, 1, 1, 0), (1, 0, 1, 1, 0), (2, 0, 3, 0, 0), (3, 0, 3, 0, 0)]
    pieces = {(0, 0): (0, 0, 8), (0, 2): (10, 10, 4)}
    for flags in pr.ALL_FLAGS:
        for tile in TILES:
            got, arrays = pr.replay(data, tile, records, parts, flags, (b"<", b">"))
            assert got == pr.expected(data, pieces, parts, flags, (b"<", b">"))[0]
            assert got[2] == got[3] == got[5] == b"" and arrays["kind"] == [1, 2, 1, 2, 3, 3]
    assert pr.replay(data, 16, records, [], 15) == ([], {"line_number": [], "kind": [], "pattern": [], "segment": []})  # zero parts


def test_print_ready_output_equals_gnu_grep(tmp_path):
    """Parts mode with number, offset and terminator is `grep -o -n -b`; line mode with terminator and grep's own escapes is
    `grep --color=always`: the reference equals the local GNU grep for one ERE on plain text, and the replay the reference."""
    import context_cli_cases as cli

    if cli.GREP is None:
        pytest.skip("no grep binary on this machine")
    data = open(os.path.join(REPO, "tests", "golden", "files", "greptest1.txt"), "rb").read() + b"foo abc bar abc\nlast line abc"
    assert b"\0" not in data and max(map(len, data.split(b"\n"))) < 4000
    path = tmp_path / "text.txt"
    path.write_bytes(data)
    env = dict(os.environ, LC_ALL="C", GREP_COLORS="")
    env.pop("GREP_COLOR", None)
    n = 0
    for ere in ("abc|ba[a-z]", "fo+", "[0-9]+"):
        records, parts = scan(data, 4096, ([ere], [6]))
        pieces = pr.pieces_of(data, 4096)
        want = subprocess.run([cli.GREP, "-E", "-o", "-n", "-b", "-e", ere, str(path)], capture_output=True, check=False, env=env).stdout
        flags = pr.NUMBER | pr.BYTE_OFFSET | pr.TERMINATE
        assert b"".join(pr.expected(data, pieces, parts, flags)[0]) == want, ere
        assert b"".join(pr.replay(data, 64, records, parts, flags)[0]) == want, ere
        want = subprocess.run([cli.GREP, "-E", "--color=always", "-e", ere, str(path)], capture_output=True, check=False, env=env).stdout
        flags = pr.LINE | pr.TERMINATE
        assert b"".join(pr.expected(data, pieces, parts, flags, pr.COLOR)[0]) == want, ere
        assert b"".join(pr.replay(data, 64, records, parts, flags, pr.COLOR)[0]) == want, ere
        n += bool(want)
    assert n >= 2
    # the issue's example, to the byte
    path.write_bytes(b"foo abc bar abc\n")
    assert subprocess.run([cli.GREP, "-E", "-o", "-n", "-b", "-e", "abc", str(path)], capture_output=True, check=False, env=env).stdout == b"1:4:abc\n1:12:abc\n"
    assert subprocess.run([cli.GREP, "-E", "--color=always", "-e", "abc", str(path)], capture_output=True, check=False, env=env).stdout == \
        b"foo " + pr.COLOR[0] + b"abc" + pr.COLOR[1] + b" bar " + pr.COLOR[0] + b"abc" + pr.COLOR[1] + b"\n"


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (partlinesim.cpp's main), built with AddressSanitizer and UBSan: the text lives in a
    heap block of exactly the readable bytes, and every record's start carries a base above 2^32."""
    exe = str(tmp_path / "partlinesim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DPARTLINESIM_MAIN", "-o", exe, pr.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout


def test_abi_and_python_names():
    import inspect

    from hypergrep_amd import device

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    for line in ("#define HG_PARTS_NUMBER 1u", "#define HG_PARTS_BYTE_OFFSET 2u", "#define HG_PARTS_TERMINATE 4u", "#define HG_PARTS_LINE 8u", "#define HG_PART_FIRST 1u",
                 "#define HG_PART_LAST 2u", "#define HG_PARTS_MARK_MAX 16"):
        assert line in header, line
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_gather_parts", "hg_copy_part_lines", "hg_copy_part_lines_first", "hg_copy_part_lines_device"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    # the structs, field by field as the header declares them, and their layout as the C compiler sees it
    for c_name, cls in (("hg_part_lines_params", device.HgPartLinesParams), ("hg_part_lines_result", device.HgPartLinesResult)):
        body = header[header.index("typedef struct %s {" % c_name):header.index("} %s_t;" % c_name)]
        names = re.findall(r"[\s*](\w+)(?:\[16\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert names == [n for n, _ in cls._fields_], c_name
    sizes = (ctypes.c_uint32 * 21)()
    pr.lib().partlinesim_sizes(sizes)
    P, R = device.HgPartLinesParams, device.HgPartLinesResult
    assert list(sizes[:2]) == [ctypes.sizeof(P), ctypes.sizeof(R)] == [56, 80]
    assert list(sizes[2:8]) == [getattr(P, n).offset for n in ("flags", "byte_base", "mark_on_len", "mark_off_len", "mark_on", "mark_off")] == [0, 8, 16, 20, 24, 40]
    assert list(sizes[8:18]) == [getattr(R, n).offset for n, _ in R._fields_[:-1]] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    assert list(sizes[18:]) == [48, 16384, 16] and device.HG_PARTS_MARK_MAX == 16
    # the scan's and the other stages' structs are untouched
    assert (ctypes.sizeof(device.HgScanResult), ctypes.sizeof(device.HgLinesResult), ctypes.sizeof(device.HgPartsResult), ctypes.sizeof(device.HgPart)) == (80, 72, 32, 16)
    assert (device.HG_PARTS_NUMBER, device.HG_PARTS_BYTE_OFFSET, device.HG_PARTS_TERMINATE, device.HG_PARTS_LINE) == (pr.NUMBER, pr.BYTE_OFFSET, pr.TERMINATE, pr.LINE)
    assert (device.HG_PART_FIRST, device.HG_PART_LAST) == (pr.FIRST, pr.LAST)
    assert list(inspect.signature(device.Scanner.gather_parts).parameters) == ["self", "d_text", "nbytes", "number", "byte_offset", "terminate", "whole_line", "mark",
                                                                                "byte_base", "stream"]
    assert list(inspect.signature(device.Scanner.gather).parameters)[-1] == "stream" and list(inspect.signature(device.Scanner.scan).parameters)[-1] == "segment_parts"
    for name in ("part_lines", "part_lines_arrays", "copy_part_lines_to"):
        assert callable(getattr(device.Scanner, name))
    # NULL arguments are refused before anything touches a GPU
    l = device.lib()
    res, params = device.HgPartLinesResult(), device.HgPartLinesParams()
    assert l.hg_gather_parts(None, None, 0, ctypes.byref(params), None, ctypes.byref(res)) == -1 and l.hg_gather_parts(None, None, 0, None, None, None) == -1
    assert l.hg_copy_part_lines(None, None, 0, None, None, None, None, None, 0) == -1 and l.hg_copy_part_lines_device(None, None, 0, None) == -1
    assert l.hg_copy_part_lines_first(None, None) == -1
    # the build recipe: the stage is compiled with the resource remarks, its table is a second file
    from hypergrep_amd import build

    assert "hg_partlines.hip" in build.HIP_SOURCES and "hg_partlines.h" in build.HEADERS and "hg_partlines.hip" not in build.KERNEL_SOURCES
