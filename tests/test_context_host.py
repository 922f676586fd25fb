"""Context lines (grep -A / -B / -C) on the host: the scalar routines of hypergrep_amd/csrc/hg_context.h (the class of a piece,
the textless count of a tile, the tile walk) replayed through tests/native/contextsim.cpp over tiles of any size, against
context_ref's plain Python reference that knows nothing of tiles; the chaining identity on both; a sanitized stand-alone
build of the same replay; the new names of the C ABI and of the Python layer.  No GPU needed."""
from __future__ import annotations

import ctypes
import inspect
import os
import random
import subprocess

import pytest

import context_ref
import invert_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA = [(0, 0), (1, 0), (0, 1), (2, 3), (5, 1), (1000, 1000)]
BIG_BASE = (1 << 33) + 7


def random_text(rng: random.Random, nbytes: int) -> bytes:
    """Empty lines, NULs (leading, inner), lines longer than the small tiles, with or without a final newline."""
    words = [b"foo", b"bar", b"x", b" ", b"\0", b"", b"zzzzzzzzzzzz", b"\0\0q"]
    out = bytearray()
    while len(out) < nbytes:
        r = rng.random()
        if r < 0.15:
            line = b""
        elif r < 0.2:
            line = bytes(rng.choice(b"ab \0x") for _ in range(rng.randint(100, 400)))
        else:
            line = b"".join(rng.choice(words) for _ in range(rng.randint(1, 5)))
        out += line + b"\n"
    out = bytes(out[:nbytes])
    return out if rng.random() < 0.5 else out.rstrip(b"\n") + b"q"


def hit_sets(rng: random.Random, n_pieces: int, line_base: int):
    """Empty, full, single at the first / the last piece, several records per line, random at 1 %, 30 %, 90 %."""
    every = list(range(line_base, line_base + n_pieces))
    yield "empty", []
    yield "full", every
    if n_pieces:
        yield "first", [line_base]
        yield "last", [line_base + n_pieces - 1]
        yield "repeats", sorted(rng.sample(every, max(1, n_pieces // 10)) * 3)
    for share in (0.01, 0.3, 0.9):
        yield f"{share}", [q for q in every if rng.random() < share]


def check_replay(data, tile, buffer_size, lines, before, after, line_base, carry, tail):
    rows, owed, n_tail, n_pieces = context_ref.replay(data, tile, buffer_size, lines, before, after, line_base, carry, tail)
    want, want_owed, want_tail = context_ref.expected(data, buffer_size, lines, before, after, line_base, carry, tail)
    where = (len(data), tile, buffer_size, before, after, line_base, carry, tail)
    assert n_pieces == len(invert_ref.pieces(data, buffer_size)), where
    assert rows == want, where
    assert (owed, n_tail) == (want_owed, want_tail), where
    assert not {r[0] for r in rows} & set(lines), where
    return rows


@pytest.mark.parametrize("bs1", [2, 7, 63, 99, 1024, 262139])
def test_replay_against_the_python_reference(bs1):
    rng = random.Random(bs1)
    for nbytes in (0, 1, 15, 600, 2500):
        data = random_text(rng, nbytes)
        n_pieces = len(invert_ref.pieces(data, bs1 + 1))
        for line_base in (0, BIG_BASE):
            for name, lines in hit_sets(rng, n_pieces, line_base):
                # every (B, A) with one draw of the other dimensions; the corners of those are swept in full below
                for before, after in BA:
                    tile = rng.choice([4, 7, 64, 16384])
                    carry = rng.choice([0, 1, n_pieces + 5])
                    check_replay(data, tile, bs1 + 1, lines, before, after, line_base, carry, rng.random() < 0.5)


def test_replay_full_product_on_one_text():
    rng = random.Random(77)
    data = random_text(rng, 900)
    for bs1 in (7, 99):
        n_pieces = len(invert_ref.pieces(data, bs1 + 1))
        for name, lines in hit_sets(rng, n_pieces, 0):
            for before, after in BA:
                for tile in (4, 7, 64, 16384):
                    for carry in (0, 1, n_pieces + 5):
                        for tail in (False, True):
                            check_replay(data, tile, bs1 + 1, lines, before, after, 0, carry, tail)


def test_fixed_cases():
    data = b"".join(b"l%d\n" % i for i in range(10))  # pieces 0..9, 3 or 4 bytes each
    ctx, tl = context_ref.HG_ID_CONTEXT, context_ref.HG_ID_CONTEXT_TAIL

    def lines_of(hits, before, after, **kw):
        return [(r[0], r[1]) for r in check_replay(data, 7, 64, hits, before, after, kw.get("line_base", 0), kw.get("carry", 0), kw.get("tail", False))]

    assert lines_of([4], 1, 2) == [(3, ctx), (5, ctx), (6, ctx)]
    assert lines_of([2, 5], 1, 1) == [(1, ctx), (3, ctx), (4, ctx), (6, ctx)]  # after-context of 2 and before-context of 5 meet
    assert lines_of([2, 6], 1, 1) == [(1, ctx), (3, ctx), (5, ctx), (7, ctx)]  # ... and leave a one-piece gap
    assert lines_of([2, 4], 2, 2) == [(0, ctx), (1, ctx), (3, ctx), (5, ctx), (6, ctx)]  # ... and overlap
    assert lines_of([], 2, 2) == [] and lines_of([], 2, 2, tail=True) == [(8, tl), (9, tl)]
    assert lines_of([], 50, 0, tail=True) == [(q, tl) for q in range(10)]
    assert lines_of([], 0, 0, carry=3) == [(0, ctx), (1, ctx), (2, ctx)]
    assert lines_of([1], 0, 0, carry=3) == [(0, ctx), (2, ctx)]
    assert lines_of([9], 3, 0, carry=1, tail=True) == [(0, ctx), (6, ctx), (7, ctx), (8, ctx)]
    assert lines_of([7], 0, 0, tail=True) == [] and lines_of(list(range(10)), 5, 5, carry=4, tail=True) == []
    # owed_after: from the last match, else what is left of the carry
    assert context_ref.replay(data, 16, 64, [8], 0, 5)[1] == 4 and context_ref.replay(data, 16, 64, [], 0, 5, carry_after=13)[1] == 3
    assert context_ref.replay(data, 16, 64, [0], 0, 5, carry_after=100)[1] == 0
    assert context_ref.replay(b"", 16, 64, [], 2, 2, carry_after=2, tail=True) == ([], 2, 0, 0)
    # saturation: piece 0 with the largest B, the last piece with the largest A, a line base above 2^33
    big = 0xFFFFFFFF
    assert [r[0] - BIG_BASE for r in check_replay(data, 4, 64, [BIG_BASE + 5], big, big, BIG_BASE, 0, True)] == [0, 1, 2, 3, 4, 6, 7, 8, 9]


def merged(rows_per_buffer, matches, before):
    """The chaining rule of include/hypergrep_amd.h over the buffers' records: the merged context piece numbers."""
    out, held = [], []
    matches = sorted(set(matches))
    for base, n, rows in rows_per_buffer:
        first = next((m for m in matches if base <= m < base + n), None)
        if first is not None:
            out += [q for q in held if q >= first - before]
            held = []
        out += [r[0] for r in rows if r[1] == context_ref.HG_ID_CONTEXT]
        held = (held + [r[0] for r in rows if r[1] == context_ref.HG_ID_CONTEXT_TAIL])[-before:] if before else []
    return sorted(out)


@pytest.mark.parametrize("before,after", [(1, 0), (0, 1), (2, 3), (5, 1), (1000, 1000)])
def test_chaining_identity_at_every_cut(before, after):
    """A 200-piece text cut into two buffers at every piece boundary, and into three at a sweep of cut pairs: the reference and
    the replay, chained by owed_after and the tail rule, give the whole text's context."""
    rng = random.Random(before * 31 + after)
    lines = [b"x" * rng.randint(0, 9) + b"\n" for _ in range(200)]
    offs = [0]
    for line in lines:
        offs.append(offs[-1] + len(line))
    data = b"".join(lines)
    for matches in ([], [0], [199], [57], sorted(rng.sample(range(200), 12)), sorted(rng.sample(range(200), 70))):
        whole = [r[0] for r in context_ref.expected(data, 64, matches, before, after)[0]]
        assert whole == [r[0] for r in context_ref.replay(data, 64, 64, matches, before, after)[0]]
        cuts = [(c,) for c in range(1, 200)] + [(c, d) for c in range(1, 200, 9) for d in range(c + 1, 200, 13)] + [(c, c + 1) for c in range(1, 199, 7)]
        for cut in cuts:
            edges = (0,) + cut + (200,)
            assert context_ref.chain([b - a for a, b in zip(edges, edges[1:])], matches, before, after) == whole, cut
            rows_per_buffer, carry = [], 0
            for a, b in zip(edges, edges[1:]):
                part = data[offs[a]:offs[b]]
                here = [m for m in matches if a <= m < b]
                rows, carry, _n_tail, n = context_ref.replay(part, rng.choice([7, 64]), 64, here, before, after, a, carry, True)
                assert n == b - a
                rows_per_buffer.append((a, n, rows))
            assert merged(rows_per_buffer, matches, before) == whole, cut


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (contextsim.cpp's main), built with AddressSanitizer and UBSan, over the corner cases:
    tiles of 4 .. 16384 bytes, A and B up to 2^32 - 1, a line base above 2^33, carries beyond the buffer."""
    exe = str(tmp_path / "contextsim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DCONTEXTSIM_MAIN", "-o", exe, context_ref.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout


def test_new_names_are_declared_exported_and_loadable():
    from hypergrep_amd import device

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    assert "#define HG_ID_CONTEXT 0xFFFFFFFEu" in header and "#define HG_ID_CONTEXT_TAIL 0xFFFFFFFDu" in header
    assert "Chaining identity" in header and "HG_CONTEXT_TAIL" in header
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_scan_device_context", "hg_copy_context", "hg_copy_context_device"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    assert (device.HG_ID_CONTEXT, device.HG_ID_CONTEXT_TAIL) == (context_ref.HG_ID_CONTEXT, context_ref.HG_ID_CONTEXT_TAIL)
    params = inspect.signature(device.Scanner.scan).parameters
    assert params["context"].default is None and params["carry_after"].default == 0 and params["tail"].default is False
    assert hasattr(device.Scanner, "context")
    # hg_scan_result_t keeps its layout; the new structs are what the header declares
    assert device.HgScanResult.invert_us.offset == 76 and ctypes.sizeof(device.HgScanResult) == 80
    assert ctypes.sizeof(device.HgContext) == 24 and device.HgContext.carry_after.offset == 8 and device.HgContext.flags.offset == 16
    assert ctypes.sizeof(device.HgContextResult) == 48 and device.HgContextResult.context_us.offset == 40
    stats = device.ScanStats(0, 0, 0, 0, 0.0, 0.0, 0)
    assert (stats.n_context, stats.owed_after, stats.n_tail, stats.context_us) == (0, 0, 0, 0)
    # the arguments are checked before any device work: unknown flags, a missing context or result
    res, cres = device.HgScanResult(), device.HgContextResult()
    bad = device.HgContext(1, 1, 0, 2)
    assert device.lib().hg_scan_device_context(None, None, 0, 64, 0, None, ctypes.byref(bad), 0, ctypes.byref(res), ctypes.byref(cres)) == -1  # HG_ERR_ARG
    assert device.lib().hg_scan_device_context(None, None, 0, 64, 0, None, None, 0, ctypes.byref(res), ctypes.byref(cres)) == -1


def test_command_line_options_parse(monkeypatch):
    from hypergrep_amd import multiscanner

    assert multiscanner.parse_args(["-A", "2", "foo", "f"]).after_context == 2
    assert multiscanner.parse_args(["--before-context=3", "foo", "f"]).before_context == 3
    assert multiscanner.parse_args(["-C", "1", "-vn", "foo", "f"]).context == 1
    for bad in (["-A", "-1", "foo", "f"], ["-C", "x", "foo", "f"], ["--before-context=-3", "foo", "f"]):  # GNU grep: "invalid context length argument", exit 2
        with pytest.raises(SystemExit) as exit_info:
            multiscanner.parse_args(bad)
        assert exit_info.value.code == 2, bad
    plain = multiscanner.parse_args(["foo", "f"])
    assert not any(hasattr(plain, name) for name in ("after_context", "before_context", "context"))  # (the namespace of other command lines is unchanged)
    assert list(inspect.signature(multiscanner.parallel_grep).parameters)[-2:] == ["before_context", "after_context"]
    seen = {}

    def fake_parallel_grep(**kwargs):
        seen.update(kwargs)
        return 0

    monkeypatch.setattr(multiscanner, "parallel_grep", fake_parallel_grep)
    for argv, want in ((["-C", "2", "foo", "f"], (2, 2)), (["-C", "2", "-A", "5", "foo", "f"], (2, 5)), (["-B", "1", "foo", "f"], (1, 0)), (["foo", "f"], (0, 0))):
        monkeypatch.setattr("sys.argv", ["hyperscanner"] + argv)
        with pytest.raises(SystemExit):
            multiscanner.main()
        assert (seen["before_context"], seen["after_context"]) == want
    import hypergrep_amd

    for fn in (hypergrep_amd.scan, hypergrep_amd.grep):
        sig = inspect.signature(fn).parameters
        assert sig["before_context"].default == 0 and sig["after_context"].default == 0


def test_output_format_against_gnu_grep():
    """The function that turns grep()'s merged rows into output, fed the rows `re` works out for the golden files, against the
    local GNU grep with -A / -B / -C: one and two files, -n, -H, -h, -v, -m 2, -o, -i.  Every case must be equal."""
    import context_cli_cases as cli
    from hypergrep_amd import multiscanner

    if cli.GREP is None:
        pytest.skip("no grep binary on this machine")
    n = 0
    for pattern, options, paths in cli.cases():
        opt = cli.parse(options)
        with_file_name = opt["H"] or (len(paths) > 1 and not opt["h"])
        want = cli.grep_output(pattern, options, paths)
        state = {"printed": False}
        got = ""
        for path in paths:
            if not (opt["o"] and opt["v"]):
                got += multiscanner.format_context_results(cli.rows_for(path, pattern, opt), path, with_file_name, opt["n"], opt["o"], state)
        assert got == want, (pattern, options, paths)
        n += 1
    assert n == 240


def test_match_limit_with_trailing_context(monkeypatch):
    """grep() under max_match_count with after_context: it asks the file API for after_context selected lines more and ends the
    rows as GNU grep 3.5 and later end their output: the lines behind the last counted one are context, matching or not."""
    import hypergrep_amd
    from hypergrep_amd import utils

    calls = []
    lines = [b"a\n", b"foo\n", b"foo\n", b"b\n", b"foo\n", b"c\n"]

    def fake_scan(file, patterns, callback, **kwargs):  # the file API's contract on those lines, no GPU
        calls.append(kwargs)
        before, after, limit = kwargs.get("before_context", 0), kwargs.get("after_context", 0), kwargs["max_match_count"]
        matching = [i for i, line in enumerate(lines) if b"foo" in line]
        kept = matching[:limit] if limit else matching
        rows = []
        for i, line in enumerate(lines):
            if i in kept:
                rows.append((i, 0, line))
            elif i not in matching and any(m - before <= i < m or m < i <= m + after and not any(m < x < i for x in matching) for m in kept):
                rows.append((i, utils.HG_ID_CONTEXT, line))
        batch = (utils.Result * len(rows))(*[utils.Result(rid, n, text) for n, rid, text in rows])
        callback(batch, len(rows))
        return 0

    monkeypatch.setattr(utils, "scan", fake_scan)
    path = os.path.join(REPO, "README.md")  # (any existing file: the scan is the fake's)
    rows, _rc = hypergrep_amd.grep(path, ["foo"], max_match_count=1, after_context=2, before_context=1)
    assert rows == [(1, "a\n", False), (2, "foo\n", True), (3, "foo\n", False), (4, "b\n", False)]  # printf 'a\nfoo\nfoo\nb\n' | grep -m1 -A2 -n foo
    assert calls[-1]["max_match_count"] == 3
    assert hypergrep_amd.grep(path, ["foo"], max_match_count=2, after_context=1)[0] == [(2, "foo\n", True), (3, "foo\n", True), (4, "b\n", False)]
    assert hypergrep_amd.grep(path, ["foo"], max_match_count=1, after_context=2, count_only=True) == (1, 0) and calls[-1]["max_match_count"] == 1
    assert hypergrep_amd.grep(path, ["foo"], max_match_count=1, before_context=1)[0] == [(1, "a\n", False), (2, "foo\n", True)] and calls[-1]["max_match_count"] == 1


def test_grep_rows_with_context(monkeypatch, capsys, tmp_path):
    """grep() and parallel_grep() over a file API that hands back merged results (no GPU): rows carry is_match, counts count
    matching lines only, listing modes ask for no context at all."""
    import hypergrep_amd
    from hypergrep_amd import multiscanner, utils

    path = tmp_path / "f.txt"
    path.write_text("a\nfoo\nb\nc\nd\nfoo\n")
    calls = []

    def fake_scan(file, patterns, callback, **kwargs):
        calls.append(kwargs)
        rows = [(0, utils.HG_ID_CONTEXT, b"a\n"), (1, 0, b"foo\n"), (2, utils.HG_ID_CONTEXT, b"b\n"), (4, utils.HG_ID_CONTEXT, b"d\n"), (5, 0, b"foo\n")]
        if not kwargs.get("before_context") and not kwargs.get("after_context"):
            rows = [r for r in rows if r[1] == 0]
        batch = (utils.Result * len(rows))(*[utils.Result(rid, line, text) for line, rid, text in rows])
        callback(batch, len(rows))
        return 0

    monkeypatch.setattr(utils, "scan", fake_scan)
    assert hypergrep_amd.grep(str(path), ["foo"]) == ([(2, "foo\n"), (6, "foo\n")], 0)  # rows exactly as before
    rows, rc = hypergrep_amd.grep(str(path), ["foo"], before_context=1, after_context=1)
    assert rc == 0 and rows == [(1, "a\n", False), (2, "foo\n", True), (3, "b\n", False), (5, "d\n", False), (6, "foo\n", True)]
    assert calls[-1]["before_context"] == 1 and calls[-1]["after_context"] == 1
    assert hypergrep_amd.grep(str(path), ["foo"], before_context=1, after_context=1, count_only=True) == (2, 0)
    assert hypergrep_amd.grep(str(path), ["fo+"], before_context=1, only_matching=True)[0][1] == (2, "foo\n", True)
    rc = multiscanner.parallel_grep([str(path)], ["foo"], with_line_number=True, before_context=1, after_context=1)
    assert capsys.readouterr().out == "1-a\n2:foo\n3-b\n--\n5-d\n6:foo\n" and rc == 0
    for listing in ({"count_results": True}, {"total_results": True}, {"files_with_matches": True}, {"quiet": True}):
        multiscanner.parallel_grep([str(path)], ["foo"], before_context=1, after_context=1, **listing)
        assert not calls[-1].get("before_context") and not calls[-1].get("after_context"), listing
    capsys.readouterr()
