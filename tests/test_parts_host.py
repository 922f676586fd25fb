"""Matched parts (grep -o over all expressions) on the host: the scalar routines of hg_parts.h (replayed through
tests/native/partssim.cpp over databases of the product's compiler) against the plain Python reference parts_ref, the refusals,
the new names, and grep(matched_parts=True)'s argument rules.  No GPU needed."""
from __future__ import annotations

import ctypes
import inspect
import os
import subprocess

import pytest

import accept_rules
import invert_ref
import parts_cases
import parts_ref
import partssim_py
import regex_gen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_text(pats, flags, data, buffer_size=1 << 20):
    """The replay's parts of every piece against the reference's; returns (pieces with a part, parts)."""
    db = partssim_py.Db(pats, flags, [0] * len(pats))
    assert db.ok(), db.error
    assert db.refusal() is None
    pieces = parts = 0
    for _a, piece in invert_ref.pieces(data, buffer_size):
        want = parts_ref.piece_parts(pats, flags, piece)
        got = db.piece(piece)
        assert got == want, (pats, flags, piece, got, want)
        for f, t, _p in got:  # never empty, never overlapping, in order
            assert f < t <= len(piece)
        assert all(got[i][1] <= got[i + 1][0] for i in range(len(got) - 1))
        pieces += bool(got)
        parts += len(got)
    return pieces, parts


def _compile_one(pat, flags):
    db = partssim_py.Db([pat], [flags])
    return db.ok(), db.error


@pytest.mark.parametrize("seed", range(20))
def test_replay_against_reference(seed):
    """Random expressions (the only cases left out are those the compiler rejects, each checked against the oracle's decision)."""
    tally = accept_rules.Tally()
    cases = pieces = parts = 0
    for pat, flags, data, _ in regex_gen.end_offset_cases(seed, accepts=tally.accepts(_compile_one)):
        a, b = check_text([pat], [flags], data)
        cases, pieces, parts = cases + 1, pieces + a, parts + b
    print(f"seed {seed}: {cases} expressions, {pieces} pieces with parts, {parts} parts checked; {tally.report()}")
    assert parts > 0


def test_ends_are_reportable_ends():
    """Every part's `to` is an end the same expression reports on that piece without SINGLEMATCH (regex_gen's brute force)."""
    checked = 0
    for pat, flags, data, want in regex_gen.end_offset_cases(3, accepts=accept_rules.Tally().accepts(_compile_one)):
        db = partssim_py.Db([pat], [flags])
        ends = set(want)
        for line, _f, t, _p in db.text(data):
            assert (line, t) in ends, (pat, flags, data, line, t)
            checked += 1
    assert checked


@pytest.mark.parametrize("row", parts_cases.TABLE, ids=[r[0] for r in parts_cases.TABLE])
def test_fixed_table(row):
    _name, pats, flags, data, buffer_size, strings = row
    _pieces, n = check_text(pats, flags, data, buffer_size)
    assert n > 0
    db = partssim_py.Db(pats, flags, [0] * len(pats))
    want = parts_ref.expected(data, buffer_size, pats, flags, range(len(invert_ref.pieces(data, buffer_size))))
    assert db.text(data, buffer_size) == want
    if strings is not None:
        got = []
        pieces = invert_ref.pieces(data, buffer_size)
        for line, f, t, _p in want:
            got.append(pieces[line][1][f:t])
        assert got == strings


def test_fixed_table_patterns_and_shapes():
    """The expression index on ties, and the automata the table is meant to reach."""
    assert [r[3] for r in partssim_py.Db(["abc", "ab|abc"], [6, 6], [0, 0]).text(b"abcab\n")] == [0, 1]
    assert [r[3] for r in partssim_py.Db(["ab", "abc"], [6, 6], [0, 0]).text(b"abcab\n")] == [1, 0]
    assert partssim_py.Db([r"x\d{2,40}y"], [6]).info()["max_nw"] > 1
    info = partssim_py.Db(["[a-z]{1000}x"], [6]).info()
    assert 1000 <= info["nnodes0"] <= 1024 and info["max_nw"] == 32
    assert partssim_py.Db(["needle"], [6]).info()["simple0"] == 1


def test_refusals_name_their_reason():
    huge = partssim_py.Db(["foo.{0,3000}bar"], [6])
    assert huge.ok() and "HG_MAX_NODES" in huge.refusal()
    comb = partssim_py.Db(["foo", "bar", "1 & 2"], [6, 6, 512], [1, 2, 3])
    assert comb.ok(), comb.error
    assert "HS_FLAG_COMBINATION" in comb.refusal()
    quiet = partssim_py.Db(["foo", "bar"], [6 | 1024, 6], [1, 2])
    assert quiet.ok(), quiet.error
    assert "HS_FLAG_QUIET" in quiet.refusal()
    ext = partssim_py.Db(["foo", "bar"], [6, 6], [1, 2], min_offsets=[0, 5])
    assert ext.ok(), ext.error
    assert "hs_expr_ext_t" in ext.refusal()
    assert partssim_py.Db(["foo", "bar"], [6, 6], [1, 2], min_offsets=[0, 0]).refusal() is None


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (partssim.cpp's main), built with AddressSanitizer and UBSan, over the fixed table:
    each piece in a heap block of its exact size.  (-O0: the compiler's translation unit is most of the build time.)"""
    exe = str(tmp_path / "partssim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DPARTSSIM_MAIN", "-o", exe, partssim_py.SRC, partssim_py.COMPILER])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout


def test_new_names_are_declared_exported_and_loadable():
    import hypergrep_amd
    from hypergrep_amd import device, multiscanner, utils

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    exports = open(os.path.join(REPO, "hypergrep_amd", "csrc", "exports.map"), encoding="utf-8").read()
    assert "hg_*;" in exports  # every hg_ name leaves the shared object
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_scan_device_parts", "hg_copy_parts", "hg_copy_parts_device", "hg_hyperscan_parts"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    assert "MATCHES EXACTLY" in header and "typedef struct hg_part {" in header and "hg_parts_result_t" in header
    assert ctypes.sizeof(device.HgPart) == 16 and device.HgPart.to.offset == 12
    assert ctypes.sizeof(device.HgPartsResult) == 32 and device.HgPartsResult.parts_us.offset == 24
    assert ctypes.sizeof(device.HgScanResult) == 80  # hg_scan_result_t keeps its layout
    params = inspect.signature(device.Scanner.scan).parameters
    assert params["parts"].default is False and hasattr(device.Scanner, "parts")
    stats = device.ScanStats(0, 0, 0, 0, 0.0, 0.0, 0)
    assert (stats.n_parts, stats.parts_us) == (0, 0)
    assert inspect.signature(utils.scan).parameters["parts"].default is False
    for fn in (hypergrep_amd.grep, utils.grep):
        assert inspect.signature(fn).parameters["matched_parts"].default is False
    assert multiscanner.parse_args(["-o", "--gnu-parts", "foo", "f"]).gnu_parts is True
    assert not hasattr(multiscanner.parse_args(["-o", "foo", "f"]), "gnu_parts")  # (the namespace of other command lines is unchanged)
    assert inspect.signature(multiscanner.parallel_grep).parameters["gnu_parts"].default is False
    # the arguments are checked before any device work
    res = device.HgScanResult()
    assert device.lib().hg_scan_device_parts(None, None, 0, 64, 0, None, ctypes.byref(res), None) == -1  # HG_ERR_ARG
    pres = device.HgPartsResult()
    assert device.lib().hg_scan_device_parts(None, None, 0, 64, 0, None, ctypes.byref(res), ctypes.byref(pres)) == -1


def test_scanner_rejects_parts_with_other_stages():
    """Scanner.scan(parts=True) with invert, context or segments raises before it touches the scanner."""
    from hypergrep_amd import device

    sc = device.Scanner.__new__(device.Scanner)  # (no database, no GPU: the check comes first)
    for kwargs in ({"invert": True}, {"context": (1, 1)}, {"segments": ([0], [1])}):
        with pytest.raises(ValueError, match="parts"):
            device.Scanner.scan(sc, 0, 0, parts=True, **kwargs)


def test_grep_matched_parts_arguments(monkeypatch, tmp_path):
    """grep(matched_parts=True) over a file API that hands back parts (no GPU): rows, the newline rules, invert, counts, and
    the context arguments it refuses; only_matching alone stays the old route."""
    import hypergrep_amd
    from hypergrep_amd import utils

    path = tmp_path / "f.txt"
    path.write_text("foo bar\nx\nfoo\n")
    calls = []

    def fake_scan(file, patterns, callback, **kwargs):
        calls.append(kwargs)
        if kwargs.get("parts"):
            rows = [(0, 0, b"foo"), (0, 0, b"bar\n"), (2, 0, b"foo"), (2, 0, b"\n")]
        else:
            rows = [(0, 0, b"foo bar\n"), (2, 0, b"foo\n")]
        batch = (utils.Result * len(rows))(*[utils.Result(rid, line, text) for line, rid, text in rows])
        callback(batch, len(rows))
        return 0

    monkeypatch.setattr(utils, "scan", fake_scan)
    rows, rc = hypergrep_amd.grep(str(path), ["foo", "bar.?"], matched_parts=True, ignore_case=True)
    assert rc == 0 and rows == [(1, "foo\n"), (1, "bar\n"), (3, "foo\n")]  # one trailing newline stripped, a part that was only one dropped
    assert calls[-1]["parts"] is True and calls[-1]["flags"] == [2 | 4 | 8 | 1] * 2
    assert hypergrep_amd.grep(str(path), ["foo"], matched_parts=True, invert=True) == ([], 0) and not calls[-1].get("parts")
    assert hypergrep_amd.grep(str(path), ["foo"], matched_parts=True, count_only=True) == (2, 0) and not calls[-1].get("parts")
    for kwargs in ({"before_context": 1}, {"after_context": 2}):
        n = len(calls)
        with pytest.raises(ValueError, match="context"):
            hypergrep_amd.grep(str(path), ["foo"], matched_parts=True, **kwargs)
        assert len(calls) == n  # nothing was scanned
    assert hypergrep_amd.grep(str(path), ["fo+", "bar"], only_matching=True)[0] == [(1, "foo\n"), (3, "foo\n")] and not calls[-1].get("parts")
    with pytest.raises(FileNotFoundError):
        hypergrep_amd.grep(str(tmp_path / "missing"), ["foo"], matched_parts=True)
    assert hypergrep_amd.grep_files([str(path)], ["foo"], matched_parts=True) == [([(1, "foo\n"), (1, "bar\n"), (3, "foo\n")], 0)]
