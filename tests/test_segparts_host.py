"""Matched parts of many files in one scan (grep -r -o) on the host: the rules of hg_segparts.h and the walk of hg_parts.h
(replayed through tests/native/segpartssim.cpp over the records the segment stage's replay keeps) against parts_ref on every
file alone, the new names, the signatures, and the routing of grep_files_outcomes.  No GPU needed."""
from __future__ import annotations

import ctypes
import inspect
import os
import subprocess

import pytest

import parts_ref
import segments_ref as sr
import segpartssim_py

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (expressions, flags) for the compiler and the same as [(id, bytes regex)] for the stand-in scan of segments_ref
AB = (["abc", "[0-9]+x|q"], [14, 14])
AB_NL = (["abc", "[0-9]+x|q", "\\n"], [14, 14, 14])
END = (["abc$", "q"], [10, 14])  # `$` without MULTILINE: the end of the piece's scanned bytes (or before their last newline)

_dbs = {}


def db_of(pset):
    key = tuple(pset[0])
    if key not in _dbs:
        _dbs[key] = segpartssim_py.Db(*pset)
    return _dbs[key]


def check(files, tile, bs, pset, limit=0):
    """The replay over one pack against parts_ref on every file alone; returns the per-file parts."""
    pats, flags = pset
    scan = sr.re_scan([(i + 1, p.encode()) for i, p in enumerate(pats)], bs)
    data, starts, ends = sr.pack(files)
    packed = sr.packed_records(data, starts, ends, scan, bs, False)
    kept = sr.replay(data, tile, bs, packed, starts, ends, limit=limit)
    first_record = kept["first_record"]
    rows, part_segment, first = db_of(pset).run(data, kept["records"], kept["segment"], starts, first_record)
    assert len(first) == len(files) + 1 and first[0] == 0 and first[-1] == len(rows)
    per_file = []
    for s, f in enumerate(files):  # no segment is left out
        lo, hi = first[s], first[s + 1]
        assert part_segment[lo:hi] == [s] * (hi - lo)
        own = sr.limited(scan(f)[0], limit)  # the file alone, the limit applied: the lines it keeps
        lines = sorted({r[0] for r in own})
        assert sorted({r[0] for r in kept["records"][first_record[s]:first_record[s + 1]]}) == lines
        want = parts_ref.expected(f, bs, pats, flags, lines)
        assert rows[lo:hi] == want, (s, limit, f[-24:], rows[lo:hi], want)
        assert sorted({r[0] for r in want}) == lines  # every kept line has a part, no other line has one
        per_file.append(rows[lo:hi])
    return per_file


@pytest.mark.parametrize("bs", [8, 64])
def test_one_line_files_stay_apart(bs):
    """Every matching line is line 0 of its file: the head rule goes by (segment, line)."""
    assert check([b"abc\n", b"abc\n"], 64, bs, AB) == [[(0, 0, 3, 0)], [(0, 0, 3, 0)]]
    files = [b"abc\n" if i % 3 else b"q\n" for i in range(300)]
    per_file = check(files, 64, bs, AB)
    assert [len(p) for p in per_file] == [1] * 300
    per_file = check([f if i % 2 else b"" for i, f in enumerate(files)], 64, bs, AB)
    assert [len(p) for p in per_file] == [i % 2 for i in range(300)]


@pytest.mark.parametrize("bs", [8, 64])
@pytest.mark.parametrize("limit", [0, 1, 2])
def test_every_case_equals_the_files_alone(bs, limit):
    for name, files in sr.cases(256, bs):
        for pset in (AB, AB_NL):  # (AB_NL reports in the pads: those hits head no piece)
            try:
                check(files, 256, bs, pset, limit)
            except AssertionError as e:
                raise AssertionError(f"{name} limit={limit}: {e}") from e


@pytest.mark.parametrize("bs", [8, 64])
def test_unterminated_last_lines_end_where_the_file_ends(bs):
    """Last lines of k * (bs - 1) + d bytes that end in "abc": `abc$` matches at the file's end, the pad's bytes are in no part
    and its phantom piece has none."""
    bs1 = bs - 1
    for k in (1, 2):
        for d in (0, -1, -2, 1):
            n = k * bs1 + d
            last = ((b"zw" * n)[:n - 3] + b"abc")[-n:]
            files = [b"abc\n" + last, b"q\n", last, b"abc\n"]
            for pset in (END, (END[0] + ["\\n"], END[1] + [14])):
                for limit in (0, 1, 2):
                    per_file = check(files, 64, bs, pset, limit)
                    r = n % bs1 or bs1  # the bytes of the file's last piece
                    if r >= 3:  # ("abc" lies inside it)
                        assert per_file[2][-1][1:] == (r - 3, r, 0)
                        assert limit or per_file[0][-1][1:] == (r - 3, r, 0)  # (a limit may keep file 0's first line only)


@pytest.mark.parametrize("bs", [8, 64])
def test_a_nul_only_last_piece_has_no_part(bs):
    files = [b"abc\n\0\0\0", b"abc\n", b"x\n\0\0", b"q\n"]
    for limit in (0, 1, 2):
        per_file = check(files, 64, bs, AB_NL, limit)
        assert [r[0] for r in per_file[0]] == [0, 0] and [r[0] for r in per_file[2]] == [0]


def test_the_limit_counts_whole_lines():
    """A line two expressions report: with a limit of 1 the whole line stays, with its parts; the lines behind have none."""
    files = [b"abc q\nabc\nq\n", b"x\nabc q\nabc\n", b"abc\n"]
    assert [sorted({r[0] for r in p}) for p in check(files, 64, 64, AB, 1)] == [[0], [1], [0]]
    assert [sorted({r[0] for r in p}) for p in check(files, 64, 64, AB, 2)] == [[0], [1], [0]]
    assert [sorted({r[0] for r in p}) for p in check(files, 64, 64, AB, 3)] == [[0, 1], [1, 2], [0]]
    assert [sorted({r[0] for r in p}) for p in check(files, 64, 64, AB, 0)] == [[0, 1, 2], [1, 2], [0]]


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (segpartssim.cpp's main), built with AddressSanitizer and UBSan: each piece is walked
    in a heap block of its exact size.  (-O0: the compiler's translation unit is most of the build time.)"""
    exe = str(tmp_path / "segpartssim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DSEGPARTSSIM_MAIN", "-o", exe, segpartssim_py.SRC, segpartssim_py.COMPILER])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "segparts case ok" in out.stdout


def test_new_names_are_declared_exported_and_loadable():
    from hypergrep_amd import device, utils

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    exports = open(os.path.join(REPO, "hypergrep_amd", "csrc", "exports.map"), encoding="utf-8").read()
    assert "hg_*;" in exports  # every hg_ name leaves the shared object
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_scan_device_segments_parts", "hg_copy_segment_parts", "hg_hyperscan_files_parts"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    assert "typedef struct hg_segment_parts_result {" in header and "hg_segment_parts_result_t;" in header
    assert ctypes.sizeof(device.HgPartsResult) == 32 and device.HgPartsResult.parts_us.offset == 24  # hg_parts_result_t keeps its layout
    assert ctypes.sizeof(device.HgSegmentPartsResult) == 16 and device.HgSegmentPartsResult.d_first_part.offset == 8
    assert ctypes.sizeof(device.HgScanResult) == 80 and ctypes.sizeof(device.HgSegmentResult) == 40
    # the arguments are checked before any device work: HG_ERR_ARG on NULL
    res, sres, pres, spres = device.HgScanResult(), device.HgSegmentResult(), device.HgPartsResult(), device.HgSegmentPartsResult()
    seg = device.HgSegments(None, None, 0, 0)
    fn = device.lib().hg_scan_device_segments_parts
    assert fn(None, None, 0, 64, None, ctypes.byref(seg), ctypes.byref(res), ctypes.byref(sres), ctypes.byref(pres), ctypes.byref(spres)) == -1  # no scanner
    assert fn(None, None, 0, 64, None, None, ctypes.byref(res), ctypes.byref(sres), ctypes.byref(pres), ctypes.byref(spres)) == -1
    assert fn(None, None, 0, 64, None, ctypes.byref(seg), ctypes.byref(res), None, ctypes.byref(pres), ctypes.byref(spres)) == -1
    assert fn(None, None, 0, 64, None, ctypes.byref(seg), ctypes.byref(res), ctypes.byref(sres), None, ctypes.byref(spres)) == -1
    assert fn(None, None, 0, 64, None, ctypes.byref(seg), ctypes.byref(res), ctypes.byref(sres), ctypes.byref(pres), None) == -1
    assert device.lib().hg_copy_segment_parts(None, None, None) == -1
    assert utils._get_hyperscanner_lib().hg_hyperscan_files_parts is not None  # pylint: disable=protected-access


def test_signatures():
    import hypergrep_amd
    from hypergrep_amd import device, utils

    params = inspect.signature(device.Scanner.scan).parameters
    assert params["segment_parts"].default is False and list(params)[-1] == "segment_parts" and params["parts"].default is False
    assert hasattr(device.Scanner, "segment_parts") and hasattr(device.Scanner, "parts")
    stats = device.ScanStats(0, 0, 0, 0, 0.0, 0.0, 0)
    assert (stats.n_parts, stats.parts_us) == (0, 0) and len(inspect.signature(device.ScanStats).parameters) == 18  # nothing new
    params = inspect.signature(utils.scan_files).parameters
    assert params["parts"].default is False and list(params)[-1] == "parts"
    for fn in (utils.grep_files_outcomes, utils.grep_files, hypergrep_amd.grep_files):
        assert list(inspect.signature(fn).parameters) == ["files", "patterns", "grep_kwargs"]
    with pytest.raises(ValueError, match="parts"):
        utils.scan_files(["a", "b"], ["foo"], None, parts=True, invert=True)
    with pytest.raises(ValueError, match="parts"):
        utils.scan_files(["a", "b"], ["foo"], None, parts=True, after_context=1)


def test_scanner_argument_rules():
    """Scanner.scan(segment_parts=True) raises before it touches the scanner; parts with segments keeps raising."""
    from hypergrep_amd import device

    sc = device.Scanner.__new__(device.Scanner)  # (no database, no GPU: the checks come first)
    with pytest.raises(ValueError, match="segment_parts"):
        device.Scanner.scan(sc, 0, 0, segment_parts=True)  # needs segments
    for kwargs in ({"invert": True}, {"context": (1, 1)}, {"carry_after": 1}, {"tail": True}, {"line_base": 3}):
        with pytest.raises(ValueError, match="segment_parts"):
            device.Scanner.scan(sc, 0, 0, segments=([0], [1]), segment_parts=True, **kwargs)
    with pytest.raises(ValueError, match="segment_parts"):  # (its message names the keyword to use)
        device.Scanner.scan(sc, 0, 0, segments=([0], [1]), parts=True)
    with pytest.raises(ValueError):
        device.Scanner.scan(sc, 0, 0, segments=([0], [1]), parts=True, segment_parts=True)


def test_routing(monkeypatch, tmp_path):
    """grep_files_outcomes(matched_parts=True): two or more scannable files make ONE scan_files(parts=True) call; one file,
    invert and count_only make none."""
    import hypergrep_amd
    from hypergrep_amd import utils

    paths = []
    for i in range(3):
        paths.append(tmp_path / f"f{i}.txt")
        paths[-1].write_text("foo bar\nx\nfoo\n")
    names = [str(p) for p in paths]
    file_calls, single_calls = [], []

    def rows_of(parts):
        if parts:
            return [(0, 0, b"foo"), (0, 0, b"bar\n"), (2, 0, b"foo"), (2, 0, b"\n")]
        return [(0, 0, b"foo bar\n"), (2, 0, b"foo\n")]

    def batch_of(rows):
        return (utils.Result * len(rows))(*[utils.Result(rid, line, text) for line, rid, text in rows])

    def fake_scan_files(files, patterns, on_match, **kwargs):
        file_calls.append((list(files), kwargs))
        rows = rows_of(kwargs.get("parts"))
        for which in range(len(files)):
            on_match(which, batch_of(rows), len(rows))
        return [(0, 3, 2)] * len(files)

    def fake_scan(file, patterns, callback, **kwargs):
        single_calls.append((file, kwargs))
        rows = rows_of(kwargs.get("parts"))
        callback(batch_of(rows), len(rows))
        return 0

    monkeypatch.setattr(utils, "scan_files", fake_scan_files)
    monkeypatch.setattr(utils, "scan", fake_scan)
    want = ([(1, "foo\n"), (1, "bar\n"), (3, "foo\n")], 0)
    assert hypergrep_amd.grep_files(names, ["foo", "bar.?"], matched_parts=True) == [want] * 3
    assert len(file_calls) == 1 and not single_calls
    assert file_calls[0][0] == names and file_calls[0][1]["parts"] is True and not file_calls[0][1]["invert"]
    # a missing file and a directory are not scannable: two remain, still one call
    mixed = [names[0], str(tmp_path / "missing"), str(tmp_path), names[1]]
    got = hypergrep_amd.grep_files(mixed, ["foo", "bar.?"], matched_parts=True, no_messages=True)
    assert got == [want, ([], 101), ([], 101), want] and len(file_calls) == 2 and file_calls[1][0] == [names[0], names[1]] and not single_calls
    # one scannable file: grep()'s own route
    assert hypergrep_amd.grep_files([names[0]], ["foo", "bar.?"], matched_parts=True) == [want]
    assert hypergrep_amd.grep_files([names[0], str(tmp_path / "missing")], ["foo", "bar.?"], matched_parts=True, no_messages=True) == [want, ([], 101)]
    assert len(file_calls) == 2 and len(single_calls) == 2 and all(kw.get("parts") is True for _f, kw in single_calls)
    # invert and count_only: no parts call anywhere, results as grep()'s
    n_single = len(single_calls)
    assert hypergrep_amd.grep_files(names, ["foo"], matched_parts=True, invert=True) == [([], 0)] * 3
    assert hypergrep_amd.grep_files(names, ["foo"], matched_parts=True, count_only=True) == [(2, 0)] * 3
    assert all(not kw.get("parts") for _f, kw in file_calls[2:]) and all(not kw.get("parts") for _f, kw in single_calls[n_single:])
    assert "parts" not in file_calls[-1][1]  # (passed on only when it is set)
    # context arguments are refused for every file, as grep() refuses them; nothing is scanned
    n_calls = len(file_calls) + len(single_calls)
    outcomes = utils.grep_files_outcomes(names, ["foo"], matched_parts=True, after_context=1)
    assert all(isinstance(o, ValueError) for o in outcomes) and len(file_calls) + len(single_calls) == n_calls
