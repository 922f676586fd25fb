"""The gather stage on the host: tests/native/gathersim.cpp replays hypergrep_amd/csrc/hg_gather.h (head flags, merge ranks, entry
layout, the copy pass's 16-byte chunks over output spans of 16 and 64 bytes) and must equal gather_ref's plain Python reference
byte for byte, for every combination of the four flags: plain and inverted scans, context and tail, packs of files with a
limit and per-file context, and records whose starts lie above 2^32.  The reference's print-ready form is held against the
local GNU grep; the replay also runs as a sanitized program of its own; the C ABI and the Python layer have the new names.
No GPU needed."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import pytest

import context_ref
import gather_ref as gr
import invert_ref
import segctx_ref
import segments_ref as sr

REPO = gr.REPO
FILES = os.path.join(REPO, "tests", "golden", "files")
TILES = (16, 64)
AB = [(1, rb"ab"), (2, rb"b")]  # two expressions: several reports on some lines
TEXT = (b"xx ab\nq\n\nlong line without a match, longer than one sixteen-byte chunk of output\nab ab\nzz\n" * 3 + b"q\0tail\n\0\0\0\nb\n" + b"w" * 70 + b" ab unterminated")


def scan(data, buffer_size, invert=False, patterns=AB):
    return sr.re_scan(patterns, buffer_size, invert)(data)


def check_plain(data, tile, buffer_size, flags, invert=False, context=None, carry_after=0, tail=False, line_base=0, base=0):
    hits, n_lines = scan(data, buffer_size)
    matching = {line_base + h[0] for h in hits}
    selected = set(range(line_base, line_base + n_lines)) - matching if invert else matching
    main = [(line_base + r[0],) + tuple(r[1:]) for r in scan(data, buffer_size, invert)[0]]
    ctx = []
    if context is not None or carry_after or tail:
        before, after = context or (0, 0)
        ctx = context_ref.expected(data, buffer_size, selected, before, after, line_base, carry_after, tail)[0]
    got = gr.replay(data, tile, main, ctx, flags, base=base)
    want, items = gr.expected(data, buffer_size, selected, flags, line_base, context, carry_after, tail)
    assert got["entries"] == want, (flags, tile, buffer_size)
    assert got["line_number"] == [i[1] for i in items] and got["kind"] == [i[2] for i in items]
    return got


@pytest.mark.parametrize("buffer_size", [262140, 24, 8])
@pytest.mark.parametrize("tile", TILES)
def test_every_flag_combination_equals_the_reference(tile, buffer_size):
    for flags in gr.ALL_FLAGS:
        for invert in (False, True):
            got = check_plain(TEXT, tile, buffer_size, flags, invert)
            if flags == 0:  # the identity: distinct lines, the sum of their lengths
                recs = scan(TEXT, buffer_size, invert)[0]
                distinct = {r[0]: r[4] for r in recs}
                assert len(got["entries"]) == len(distinct) and sum(map(len, got["entries"])) == sum(distinct.values())
            for context, carry, tail in (((1, 2), 0, False), ((0, 3), 2, False), ((5, 0), 0, True), ((1, 1), 0, True)):
                check_plain(TEXT, tile, buffer_size, flags, invert, context, carry, tail, line_base=7)


def test_tail_records_are_kind_2_in_order():
    data = b"ab\nq\nq\nq\nq\nq\n"
    got = check_plain(data, 16, 64, 15, context=(2, 1), tail=True)
    assert got["kind"] == [0, 1, 2, 2] and got["entries"] == [b"1:ab\n", b"2-q\n", b"--\n5-q\n", b"6-q\n"]
    assert check_plain(data, 16, 64, 14, context=(2, 1), tail=True)["kind"] == [0]  # without the flag the context list is ignored


@pytest.mark.parametrize("tile", TILES)
def test_starts_above_4_gib(tile):
    """Every record's start carries a base above 2^32, taken off again where the text is read: 64-bit offsets throughout."""
    for base in ((1 << 32) + 16, (5 << 32) + 4):
        for flags in gr.ALL_FLAGS:
            check_plain(TEXT, tile, 64, flags, context=(1, 1), base=base)
            check_files([b"ab\nq\n", b"q\nab", b"", b"ab\n" + b"z" * 40 + b"\n"], tile, 64, flags, context=(1, 1), base=base)


def check_files(files, tile, buffer_size, flags, invert=False, limit=0, context=None, base=0):
    data, starts, ends = sr.pack(files)
    alone = sr.re_scan(AB, buffer_size, invert)
    per_file = sr.expected(data, starts, ends, alone, limit)
    main, first_record = [], [0]
    for s, (records, _n, _sel) in enumerate(per_file):
        main += [tuple(r) + (s,) for r in records]
        first_record.append(len(main))
    ctx, first_context, ctx_lines = [], None, None
    if context is not None:
        rows = segctx_ref.expected(data, starts, ends, alone, buffer_size, context[0], context[1], limit)
        first_context = [0]
        for s, r in enumerate(rows):
            ctx += [tuple(x) + (s,) for x in r]
            first_context.append(len(ctx))
        ctx_lines = [[x[0] for x in r] for r in rows]
    got = gr.replay(data, tile, main, ctx, flags, segments=(starts, first_record, first_context), base=base)
    selected = [{r[0] for r in records} for records, _n, _sel in per_file]
    want, items, first_entry = gr.expected_files(files, buffer_size, selected, flags, ctx_lines)
    assert got["entries"] == want, (flags, tile, buffer_size, limit)
    assert got["segment"] == [i[0] for i in items] and got["line_number"] == [i[1] for i in items] and got["kind"] == [i[2] for i in items]
    assert got["first_entry"] == first_entry
    return got


@pytest.mark.parametrize("buffer_size", [64, 8])
@pytest.mark.parametrize("tile", TILES)
def test_packs_of_files(tile, buffer_size):
    for name, files in sr.cases(64, buffer_size):
        if sum(map(len, files)) > 3000:  # (the tile-boundary cases of the segment stage: nothing the gather depends on)
            continue
        for flags in (0, 6, 14, 15):
            for invert in (False, True):
                for limit in (0, 1):
                    try:
                        check_files(files, tile, buffer_size, flags, invert, limit)
                        check_files(files, tile, buffer_size, flags, invert, limit, context=(1, 2))
                    except AssertionError as e:
                        raise AssertionError(f"{name} flags={flags} invert={invert} limit={limit}: {e}") from e


def test_one_line_files_are_two_entries_and_a_separator_at_every_file_change():
    got = check_files([b"ab\n", b"ab\n", b"", b"ab"], 16, 64, gr.NUMBER | gr.SEPARATOR | gr.TERMINATE)
    assert got["entries"] == [b"1:ab\n", b"--\n1:ab\n", b"--\n1:ab\n"] and got["first_entry"] == [0, 1, 2, 2, 3]


def test_zero_entries_and_empty_bodies():
    got = gr.replay(b"q\nq\n", 16, [], [], 15)
    assert got["entries"] == []
    # a piece of NULs only is selected by an inverted scan with len == 0: an empty entry, a bare newline with TERMINATE
    data = b"ab\n\0\0\n\0\0\0"  # (the piece "\0\0\n" has the scanned bytes "\n"; the last piece has none)
    assert check_plain(data, 16, 64, 0, invert=True)["entries"] == [b"\n", b""]
    assert check_plain(data, 16, 64, gr.TERMINATE | gr.NUMBER, invert=True)["entries"] == [b"2:\n", b"3:\n"]
    assert check_plain(b"\0\0", 16, 64, 0, invert=True)["entries"] == [b""]  # an output of no bytes at all


def test_decimal_width():
    lib = gr.lib()
    for d in range(1, 20):
        assert lib.gathersim_digits(10 ** d - 1) == d and lib.gathersim_digits(10 ** d) == d + 1
    assert lib.gathersim_digits(0) == 1 and lib.gathersim_digits(2 ** 64 - 1) == 20
    data = b"ab\nab\nab\nq\nab\n"
    for line_base in (8, 98, 9_999_998, (1 << 33) + 7, 9_999_999_999_999_999_998):
        for flags in (gr.NUMBER, 15):
            got = check_plain(data, 16, 64, flags, context=(1, 1), line_base=line_base)
            assert got["entries"][0].startswith(str(line_base + 1).encode() + b":")


def grep_n_c(path, pattern, context):
    import context_cli_cases as cli

    return subprocess.run([cli.GREP, "-n", "-C", str(context), "-e", pattern, path], capture_output=True, check=False).stdout


@pytest.mark.parametrize("name", ["greptest1.txt", "greptest2.txt", "samplefile.txt"])
def test_print_ready_output_equals_gnu_grep(name):
    """NUMBER | TERMINATE | SEPARATOR | CONTEXT is `grep -n -C`: the reference's output for the golden files (no NUL, no line
    longer than the buffer size) equals the local GNU grep's, and the replay equals the reference."""
    import context_cli_cases as cli

    if cli.GREP is None:
        pytest.skip("no grep binary on this machine")
    path = os.path.join(FILES, name)
    data = open(path, "rb").read()
    assert b"\0" not in data and max(map(len, data.split(b"\n"))) < 4000
    n = 0
    for pattern in ("bar", "foo"):
        lines = data.split(b"\n")
        matching = {i for i, line in enumerate(lines[:-1] if data.endswith(b"\n") else lines) if re.search(pattern.encode(), line)}
        for c in (1, 2, 3):
            want = grep_n_c(path, pattern, c)
            entries, _ = gr.expected(data, 4096, matching, 15, context=(c, c))
            assert b"".join(entries) == want, (name, pattern, c)
            n += bool(want)
            main = [r for r in sr.re_scan([(1, pattern.encode())], 4096)(data)[0]]
            assert {r[0] for r in main} == matching
            ctx = context_ref.expected(data, 4096, matching, c, c)[0]
            assert b"".join(gr.replay(data, 64, main, ctx, 15)["entries"]) == want
    assert n


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (gathersim.cpp's main), built with AddressSanitizer and UBSan: the text lives in a
    heap block of exactly the readable bytes, and every record's start carries a base above 2^32."""
    exe = str(tmp_path / "gathersim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DGATHERSIM_MAIN", "-o", exe, gr.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout


def test_abi_and_python_names():
    import inspect

    from hypergrep_amd import device

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    for line in ("#define HG_LINES_CONTEXT 1u", "#define HG_LINES_TERMINATE 2u", "#define HG_LINES_NUMBER 4u", "#define HG_LINES_SEPARATOR 8u", "#define HG_LINE_MATCH 0u",
                 "#define HG_LINE_CONTEXT 1u", "#define HG_LINE_TAIL 2u", "#define HG_GATHER_TILE 16384u"):
        assert line in header, line
    exports = open(os.path.join(REPO, "hypergrep_amd", "csrc", "exports.map"), encoding="utf-8").read()
    assert "hg_*;" in exports  # every hg_ name leaves the shared object
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_gather_lines", "hg_copy_lines", "hg_copy_lines_device"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    # the struct, field by field as the header declares it
    body = header[header.index("typedef struct hg_lines_result {"):header.index("} hg_lines_result_t;")]
    names = re.findall(r"[\s*](\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in device.HgLinesResult._fields_]
    assert ctypes.sizeof(device.HgLinesResult) == 72
    assert [getattr(device.HgLinesResult, n).offset for n, _ in device.HgLinesResult._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68]
    assert ctypes.sizeof(device.HgScanResult) == 80  # hg_scan_result_t is untouched
    assert (device.HG_LINES_CONTEXT, device.HG_LINES_TERMINATE, device.HG_LINES_NUMBER, device.HG_LINES_SEPARATOR) == (gr.CONTEXT, gr.TERMINATE, gr.NUMBER, gr.SEPARATOR)
    assert (device.HG_LINE_MATCH, device.HG_LINE_CONTEXT, device.HG_LINE_TAIL) == (gr.MATCH, gr.KIND_CONTEXT, gr.KIND_TAIL)
    assert device.HG_GATHER_TILE == gr.lib().gathersim_tile() == 16384
    assert list(inspect.signature(device.Scanner.gather).parameters) == ["self", "d_text", "nbytes", "context", "terminate", "number", "separator", "stream"]
    assert list(inspect.signature(device.Scanner.scan).parameters)[-1] == "segment_parts"  # scanning is untouched
    for name in ("lines", "lines_arrays", "copy_lines_to"):
        assert callable(getattr(device.Scanner, name))
    # NULL arguments are refused before anything touches a GPU
    l = device.lib()
    res = device.HgLinesResult()
    assert l.hg_gather_lines(None, None, 0, 0, None, ctypes.byref(res)) == -1 and l.hg_gather_lines(None, None, 0, 0, None, None) == -1
    assert l.hg_copy_lines(None, None, 0, None, None, None, None, 0) == -1 and l.hg_copy_lines_device(None, None, 0, None) == -1
