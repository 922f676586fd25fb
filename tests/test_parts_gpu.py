"""Matched parts (grep -o over all expressions) on the MI355X: hg_scan_device_parts (the parts stage,
hypergrep_amd/csrc/hg_parts.hip), the file API (hg_hyperscan_parts), grep(matched_parts=True) and `hyperscanner -o --gnu-parts`.
Every expectation is parts_ref's plain Python reference (pieces, then the parts of a piece by the definition) on the matching
lines of the oracle (oracle_py).  Texts sit at the end of guarded buffers: a read past them faults."""
from __future__ import annotations

import os
import random
import subprocess
import sys

import pytest

import invert_ref
import oracle_py
import parts_cases
import parts_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FILES = os.path.join(HERE, "golden", "files")
TILE = 16384
A = 6  # DOTALL | MULTILINE
LITERALS = ["needle-in-hay", "ERROR 42 failed"]
FILLER = [b"user=abc", b"12x", b"abc", b" ", b"-", b"quiet", b"zz", b"lorem ipsum dolor"]


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 20)
    yield a
    a.free()


def log_text(rng: random.Random, nbytes: int, share: float) -> bytes:
    """Lines of 0..~90 bytes, `share` of them with a match of LITERALS, cut to exactly nbytes."""
    out = bytearray()
    while len(out) < nbytes:
        words = [rng.choice(FILLER) for _ in range(rng.randint(0, 6))]
        if rng.random() < share:
            words.insert(rng.randint(0, len(words)), rng.choice(LITERALS).encode())
        out += b" ".join(words) + b"\n"
    out = out[:nbytes]
    if nbytes:
        out[-1:] = b"\n"
    return bytes(out)


def check(arena, text, pats, flags=None, bs=262140, line_base=0, ids=None):
    """One scanner, one text: the scan with parts leaves the hits of the scan without, parts() equals the reference on the
    oracle's matching lines, and the identity on distinct line numbers holds.  Returns the parts."""
    from hypergrep_amd import device

    flags = flags or [A] * len(pats)
    ids = ids or [0] * len(pats)
    db = device.Database(pats, flags=flags, ids=ids)
    sc = device.Scanner(db, 0)
    ptr = arena.place(text)
    plain = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base)
    plain_hits = sc.hits()
    assert sc.parts() == [] and (plain.n_parts, plain.parts_us) == (0, 0)
    rc, hits, n_lines = oracle_py.scan_buffer(text, pats, flags, ids, buffer_size=bs)
    assert rc == 0
    matching = {line_base + h[0] for h in hits}
    assert {h[0] for h in plain_hits} == matching and plain.n_lines == n_lines
    where = (pats, flags, bs, len(text), line_base)
    st = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base, parts=True)
    assert sc.hits() == plain_hits, where  # hits() is identical to the scan without parts
    assert (st.n_hits, st.n_lines, st.n_candidates, st.n_raw_hits) == (plain.n_hits, plain.n_lines, plain.n_candidates, plain.n_raw_hits), where
    got = sc.parts()
    want = parts_ref.expected(text, bs, pats, flags, matching, line_base)
    assert got == want, where
    assert st.n_parts == len(want)
    assert {r[0] for r in got} == matching, where  # the identity: a line has a hit iff it has a part
    assert got == sorted(got) and all(f < t for _l, f, t, _p in got)
    # a following plain scan is unchanged and reports no parts
    again = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base)
    assert sc.hits() == plain_hits and again.n_parts == 0 and again.parts_us == 0 and sc.parts() == []
    return got


@pytest.mark.parametrize("row", parts_cases.TABLE, ids=[r[0] for r in parts_cases.TABLE])
def test_fixed_table(arena, row):
    _name, pats, flags, data, bs, strings = row
    got = check(arena, data, pats, flags, bs=bs)
    assert got
    if strings is not None:
        pieces = invert_ref.pieces(data, bs)
        assert [pieces[line][1][f:t] for line, f, t, _p in got] == strings


def test_empty_no_hit_and_every_line(arena):
    assert check(arena, b"", ["foo"]) == []
    assert check(arena, b"bar\nbaz\n\n", ["foo"]) == []
    text = b"".join(b"%d foo%d\n" % (i, i) for i in range(300))
    got = check(arena, text, ["foo[0-9]+", "[0-9]+ "])
    assert len({r[0] for r in got}) == 300 and len(got) == 600


@pytest.mark.parametrize("length", [1, 63, 64, 65, 300])
def test_candidate_starts_wrap_the_wavefront(arena, length):
    """A hit line of `length` bytes: parts before, across and after every 64-byte boundary of the candidate starts."""
    body = bytearray(b"." * length)  # "abbb" at chosen offsets: 61..65 lies across the first boundary, 126..130 across the second
    for at in (0, 30, 61, 66, 100, 126, 131, 190, 255, 295):
        if at < length:
            body[at:at + 4] = b"abbb"
    if length == 1:
        text = b"nothing here\n" + b"a"  # the hit line is the last one, one byte, no newline
    else:
        text = b"nothing here\n" + bytes(body[:length - 1]) + b"\n" + b"tail\n"  # the hit line with its newline has `length` bytes
    got = check(arena, text, ["ab*", "b{2}"])
    assert got
    if length == 300:
        assert any(f < 64 < t for _l, f, t, _p in got) and any(f < 128 < t for _l, f, t, _p in got)


def test_line_across_a_tile_boundary(arena):
    rng = random.Random(5)
    text = bytearray(log_text(rng, 2 * TILE, 0.05))
    at = TILE - 40
    text[at - 1:at] = b"\n"
    text[at:at + 90] = b"x" * 30 + b" key=" + b"v" * 20 + b"; " + b"y" * 32 + b"\n"  # the part key=v...; lies across offset 16384
    got = check(arena, bytes(text), [r"key=\w+;", "needle-in-hay", "ERROR 42 failed"])
    line_start = at
    assert any(line_start + f < TILE < line_start + t for _l, f, t, p in got if p == 0)


def test_seventy_expressions(arena):
    """More expressions than lanes: each of 70 words is its own expression and wins somewhere; a longer alternative of a
    high index beats a lower one at the same start."""
    words = [f"w{i:02d}x" for i in range(70)]
    pats = words[:69] + ["w0[0-9]x+"]  # the last expression is longer wherever a w0?x is followed by x
    text = b" ".join(w.encode() for w in words) + b"\n" + b"w03xxx w68x w10x\n" + b"nothing\n"
    got = check(arena, text, pats)
    assert {p for _l, _f, _t, p in got} >= set(range(69))
    assert (1, 0, 6, 69) in got  # w03xxx: expression 69 is the longest at offset 0 of line 1


def test_buffer_size_8_and_line_base(arena):
    text = b"abbbbbbbbcd abcdabcd\nab\n\nxcdcdab\n"
    check(arena, text, ["ab+", "cd"], bs=8)
    got = check(arena, text, ["ab+", "cd"], bs=8, line_base=(1 << 33) + 7)
    assert got[0][0] >= (1 << 33) + 7


@pytest.mark.parametrize("share", [0.01, 0.9])
def test_log_text_at_two_hit_shares(arena, share):
    rng = random.Random(int(share * 100))
    text = log_text(rng, 3 * TILE + 77, share)
    got = check(arena, text, LITERALS + [r"ERROR \d+", "quiet|qui"], flags=[A, A, A, A])
    assert got


def test_grep_flags_and_report_limits_do_not_change_parts(arena):
    """SINGLEMATCH expressions on one id (grep()'s flags): one report per line, every part of the line."""
    text = b"foo foo bar foo\nnone\nbar\n"
    got = check(arena, text, ["foo", "bar"], flags=[14, 14])
    assert [(l, f, t) for l, f, t, _p in got] == [(0, 0, 3), (0, 4, 7), (0, 8, 11), (0, 12, 15), (2, 0, 3)]


def test_copy_parts_device_round_trips(arena):
    import torch

    from hypergrep_amd import device

    text = b"foo bar\nbaz\nfoofoo\n"
    sc = device.Scanner(device.Database(["foo", "ba."], flags=[A, A], ids=[0, 1]), 0)
    st = sc.scan(arena.place(text), len(text), parts=True)
    want = sc.parts()
    assert st.n_parts == len(want) == 5
    dst = torch.zeros(2 * st.n_parts, dtype=torch.int64, device="cuda:0")
    assert sc.copy_parts_to(dst.data_ptr(), st.n_parts) == st.n_parts
    torch.cuda.synchronize()
    rows = dst.cpu().tolist()
    assert [(rows[2 * i], rows[2 * i + 1] & 0xFFFFFFFF, rows[2 * i + 1] >> 32) for i in range(st.n_parts)] == [(l, f, t) for l, f, t, _p in want]
    sc.scan(arena.place(text), len(text))  # after a scan without parts nothing is copied
    assert sc.copy_parts_to(dst.data_ptr(), 5) == 0 and sc.parts() == []


def test_refused_databases_and_combinations_of_stages(arena):
    from hypergrep_amd import device, utils

    text = b"foo bar\n"
    ptr = arena.place(text)
    for pats, flags, ids, ext, word in ((["foo.{0,3000}bar"], [A], [0], None, "HG_MAX_NODES"), (["foo", "bar", "1 & 2"], [A, A, 512], [1, 2, 3], None, "COMBINATION"),
                                        (["foo", "bar"], [A | 1024, A], [1, 2], None, "QUIET"),
                                        (["foo", "bar"], [A, A], [1, 2], [None, utils.ExprExt(flags=1, min_offset=2)], "hs_expr_ext_t")):
        sc = device.Scanner(device.Database(pats, flags=flags, ids=ids, ext=ext), 0)
        with pytest.raises(ValueError, match=word):
            sc.scan(ptr, len(text), parts=True)
        assert sc.parts() == [] and sc.hits() == []  # nothing was scanned
        sc.scan(ptr, len(text))  # the plain scan of the same scanner is untouched
    sc = device.Scanner(device.Database(["foo"], flags=[A]), 0)
    for kwargs in ({"invert": True}, {"context": (1, 1)}, {"segments": ([0], [len(text)])}):
        with pytest.raises(ValueError, match="parts"):
            sc.scan(ptr, len(text), parts=True, **kwargs)


def _file_parts(path, pats, flags, ids, **kwargs):
    from hypergrep_amd import utils

    rows = []

    def on_match(matches, count):
        rows.extend((matches[i].line_number, matches[i].id, matches[i].line) for i in range(count))

    return utils.scan(path, pats, on_match, flags=flags, ids=ids, parts=True, **kwargs), rows


@pytest.mark.parametrize("name", ["samplefile.txt", "samplefile.txt.gz", "samplefile.txt.zst"])
def test_file_api(arena, name):
    """hg_hyperscan_parts on the golden file, plain and compressed: one Result per part with its expression's id, in order;
    max_match_count 2 goes by the reports and lets every part of a delivered line out."""
    data = open(os.path.join(FILES, "samplefile.txt"), "rb").read()
    pats, flags, ids = ["foo", "ba?r", "o+d"], [A, A, A], [7, 8, 9]
    pieces = invert_ref.pieces(data, 262140)

    def want_for(limit):
        rc, hits, _n = oracle_py.scan_buffer(data, pats, flags, ids, max_match_count=limit)
        assert rc == 0
        lines = {h[0] for h in hits}
        return [(l, ids[p], pieces[l][1][f:t]) for l, f, t, p in parts_ref.expected(data, 262140, pats, flags, lines)]

    rc, rows = _file_parts(os.path.join(FILES, name), pats, flags, ids)
    assert rc == 0 and rows == want_for(0) and len(rows) > len(pieces) - 1
    rc, rows = _file_parts(os.path.join(FILES, name), pats, flags, ids, max_match_count=2)
    assert rc == 0 and rows == want_for(2) and rows
    assert len({r[0] for r in rows}) < len({r[0] for r in want_for(0)})


def test_file_api_refuses_what_the_stage_does_not_offer(arena):
    from hypergrep_amd import utils

    path = os.path.join(FILES, "samplefile.txt")
    assert utils.scan(path, ["foo", "bar"], lambda m, c: None, flags=[A, A], ids=[1, 2], ext=[None, utils.ExprExt(flags=1, min_offset=2)], parts=True) == 4
    assert utils.scan(path, ["foo", "bar", "1 & 2"], lambda m, c: None, flags=[A, A, 512], ids=[1, 2, 3], parts=True) == 4


def test_grep_matched_parts_against_only_matching(arena, tmp_path):
    """Two patterns: matched_parts returns both patterns' parts, leftmost-longest; only_matching returns the first pattern's
    only, by Python's leftmost-first rule (pinned: the old route is untouched)."""
    import hypergrep_amd

    path = tmp_path / "f.txt"
    path.write_text("aaaa bar\nnothing\nBAR a\n")
    pats = ["a|aaa", "bar"]
    # the first pattern only, leftmost-first: the four a of aaaa, the a of bar, the a of line 3
    assert hypergrep_amd.grep(str(path), pats, only_matching=True) == ([(1, "a\n")] * 5 + [(3, "a\n")], 0)
    assert hypergrep_amd.grep(str(path), pats, matched_parts=True) == ([(1, "aaa\n"), (1, "a\n"), (1, "bar\n"), (3, "a\n")], 0)
    assert hypergrep_amd.grep(str(path), pats, matched_parts=True, ignore_case=True)[0] == [(1, "aaa\n"), (1, "a\n"), (1, "bar\n"), (3, "BAR\n"), (3, "a\n")]
    assert hypergrep_amd.grep(str(path), pats, matched_parts=True, count_only=True) == (2, 0)
    assert hypergrep_amd.grep(str(path), pats, matched_parts=True, invert=True) == ([], 0)
    assert hypergrep_amd.grep(str(path), pats, matched_parts=True, max_match_count=1)[0] == [(1, "aaa\n"), (1, "a\n"), (1, "bar\n")]
    assert hypergrep_amd.grep(str(path), ["r.*"], matched_parts=True)[0] == [(1, "r\n")]  # DOTALL: the part held the newline, one is stripped
    assert hypergrep_amd.grep_files([str(path), str(path)], pats, matched_parts=True) == [hypergrep_amd.grep(str(path), pats, matched_parts=True)] * 2


def test_command_line_gnu_parts(arena, tmp_path):
    """hyperscanner -o --gnu-parts -e p1 -e p2: the reference's parts; -o alone stays the old route."""
    path = tmp_path / "f.txt"
    data = b"aaaa bar\nnothing\nbar a\n"
    path.write_bytes(data)
    pats = ["a|aaa", "bar"]
    pieces = invert_ref.pieces(data, 262140)
    want = "".join(f"{l + 1}:{pieces[l][1][f:t].decode()}\n" for l, f, t, _p in parts_ref.expected(data, 262140, pats, [A, A], {0, 2}))

    def run(*options):
        cmd = [sys.executable, "-m", "hypergrep_amd.multiscanner", "-E", "-n", *options, "-e", pats[0], "-e", pats[1], str(path)]
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=REPO)

    out = run("-o", "--gnu-parts")
    assert out.returncode == 0 and out.stdout == want == "1:aaa\n1:a\n1:bar\n3:bar\n3:a\n", out.stdout + out.stderr
    old = run("-o")
    assert old.returncode == 0 and old.stdout == "1:a\n" * 5 + "3:a\n" * 2, old.stdout + old.stderr
    assert run("--gnu-parts").stdout == run().stdout == "1:aaaa bar\n3:bar a\n"  # without -o the option has no effect
