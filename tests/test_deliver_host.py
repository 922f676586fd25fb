"""Face B's delivery on the host: the result ring, the line routines and the per-chunk state object of
hypergrep_amd/csrc/hg_deliver.h, and the reader's cut rule (hg_reader.h), through tests/native/deliversim.cpp.  Every chunk's
input is made in plain Python (deliver_ref.play); the expectation (deliver_ref.expected) knows nothing of chunks.  No GPU needed."""
from __future__ import annotations

import random
import subprocess
import struct

import pytest

import deliver_ref
from deliver_ref import Text

BA = [(0, 0), (1, 0), (0, 1), (2, 3), (5, 1), (1000, 1000)]
BUFFER_COUNTS = (1, 2, 5)


def lines_of(n: int):
    return [b"" if i % 9 == 4 else b"line %d %s" % (i, b"x" * (i % 5)) for i in range(n)]


def chunkings(n: int):
    """The line numbers at which the text is cut: the 7-line text at every line position, the 30-line text in chunks of 1, 2, 3
    and 11 lines; shorter texts are one chunk (none for the empty text)."""
    if n == 7:
        return [[0, 7]] + [[0, c, 7] for c in range(1, 7)]
    if n == 30:
        return [sorted(set(range(0, 30, size)) | {30}) for size in (1, 2, 3, 11)]
    return [[0, n]] if n else [[0]]


def matching_sets(rng: random.Random, n: int, edges):
    yield "empty", []
    yield "all", list(range(n))
    if n:
        yield "first", [0]
        yield "last", [n - 1]
        yield "random", [q for q in range(n) if rng.random() < 0.3]
    inner = edges[1:-1]
    if inner:  # adjacent pairs across a cut: the last line of a chunk and the first of the next
        yield "across", sorted({q for c in inner[:3] for q in (c - 1, c)})


def reports_for(rng: random.Random, text: Text, lines):
    """One to three reports per line with distinct (to, id), in shuffled order."""
    out = {}
    for q in lines:
        pairs = rng.sample([(to, rid) for to in (1, 2, len(text.piece[q]) + 1) for rid in (3, 5, 900)], rng.randint(1, 3))
        rng.shuffle(pairs)
        out[q] = pairs
    return out


def parts_for(rng: random.Random, text: Text, lines):
    """One to three parts per line, in order, inside the line where it has bytes (an empty line has one empty part)."""
    out = {}
    for q in lines:
        n = len(text.piece[q])
        cuts = sorted(rng.sample(range(n + 1), min(n + 1, 2 * rng.randint(1, 3))))
        out[q] = [(cuts[i], cuts[i + 1], rng.randrange(3)) for i in range(0, len(cuts) - 1, 2)] or [(0, 0, rng.randrange(3))]
    return out


def limits(reports):
    total = sum(len(v) for v in reports.values())
    return sorted({0, 1, 2, 3, total, total + 1})


def check_batches(batches, n_results, buffer_count, where):
    assert sum(batches) == n_results, where
    assert all(b == buffer_count for b in batches[:-1]) and all(1 <= b <= buffer_count for b in batches[-1:]), where


def sweep(n_lines: int, seed: int, with_parts: bool, record=None, ba=BA, play=deliver_ref.play):
    rng = random.Random(seed)
    cases = 0
    for final_newline in (True, False):
        text = Text(lines_of(n_lines), final_newline)
        for edges in chunkings(n_lines):
            for name, lines in matching_sets(rng, n_lines, edges):
                reports = reports_for(rng, text, lines)
                parts = parts_for(rng, text, lines) if with_parts else None
                for before, after in ([(0, 0)] if with_parts else ba):
                    for limit in limits(reports):
                        buffer_count = BUFFER_COUNTS[cases % 3]
                        where = (n_lines, final_newline, edges, name, before, after, limit, buffer_count)
                        got, batches, n_chunks = play(text, edges, reports, before, after, limit, buffer_count, parts, record)
                        assert got == deliver_ref.expected(text, reports, before, after, limit, parts), where
                        assert n_chunks in (None, deliver_ref.expected_chunks(text, edges, reports, after, limit, parts)), where  # (it says when the call stops)
                        check_batches(batches, len(got), buffer_count, where)
                        cases += 1
    return cases


@pytest.mark.parametrize("n_lines", [0, 1, 7, 30])
def test_chunked_delivery_against_the_whole_text(n_lines):
    assert sweep(n_lines, 1000 + n_lines, with_parts=False) >= 2 * 6 * 2


@pytest.mark.parametrize("n_lines", [0, 1, 7, 30])
def test_chunked_parts_delivery(n_lines):
    """Each kept line delivers its parts in order with the expression's id; the limit still counts reports."""
    assert sweep(n_lines, 2000 + n_lines, with_parts=True) >= 2 * 2


def test_every_batch_size_on_one_text():
    rng = random.Random(5)
    text = Text(lines_of(7))
    reports = reports_for(rng, text, [0, 2, 3, 6])
    for edges in chunkings(7):
        for before, after in BA:
            for limit in limits(reports):
                for buffer_count in BUFFER_COUNTS:
                    got, batches, _ = deliver_ref.play(text, edges, reports, before, after, limit, buffer_count)
                    assert got == deliver_ref.expected(text, reports, before, after, limit), (edges, before, after, limit, buffer_count)
                    check_batches(batches, len(got), buffer_count, (edges, before, after, limit, buffer_count))


def test_fixed_cases():
    """printf 'a\\nfoo\\nfoo\\nb\\nfoo\\nc\\n' | grep -m1 -A2 -n foo, cut everywhere: the trailing context ends before the next match."""
    ctx = deliver_ref.context_ref.HG_ID_CONTEXT
    text = Text([b"a", b"foo", b"foo", b"b", b"foo", b"c"])
    reports = {1: [(3, 0)], 2: [(3, 0)], 4: [(3, 0)]}

    def plain(*args):  # (a result holds the line with its newline)
        return [(rid, line, data.rstrip(b"\n")) for rid, line, data in deliver_ref.play(*args)[0]]

    for edges in ([0, 6], [0, 2, 6], [0, 1, 2, 3, 4, 5, 6], [0, 3, 6]):
        assert plain(text, edges, reports, 1, 2, 1, 4) == [(ctx, 0, b"a"), (0, 1, b"foo")], edges
        assert plain(text, edges, reports, 0, 2, 2, 4) == [(0, 1, b"foo"), (0, 2, b"foo"), (ctx, 3, b"b")], edges
        assert plain(text, edges, reports, 0, 2, 3, 4) == [(0, 1, b"foo"), (0, 2, b"foo"), (ctx, 3, b"b"), (0, 4, b"foo"), (ctx, 5, b"c")], edges
        assert plain(text, edges, reports, 1, 0, 0, 4) == [(ctx, 0, b"a"), (0, 1, b"foo"), (0, 2, b"foo"), (ctx, 3, b"b"), (0, 4, b"foo")], edges
    # reports of one line: by end offset, then id, however they were handed over
    one = Text([b"abcdef"])
    assert [r[0] for r in deliver_ref.play(one, [0, 1], {0: [(5, 1), (2, 9), (2, 3)]}, 0, 0, 0, 2)[0]] == [3, 9, 1]
    # parts carry their expression's id; the limit counts the line's reports, not its parts
    two = Text([b"abcdef", b"ghij", b"kl"])
    parts = {0: [(0, 2, 1), (3, 6, 0)], 1: [(1, 2, 2)], 2: [(0, 2, 0)]}
    got = deliver_ref.play(two, [0, 2, 3], {0: [(2, 5)], 1: [(2, 5), (3, 5)], 2: [(2, 5)]}, 0, 0, 3, 5, parts)[0]
    assert got == [(7, 0, b"ab"), (11, 0, b"def"), (4000000000, 1, b"h")]


@pytest.mark.parametrize("n_lines", [0, 1, 7, 30])
def test_whole_file_line_routines(n_lines):
    """The packed route's delivery of one file: every line with the context records merged in front and behind."""
    rng = random.Random(n_lines)
    text = Text(lines_of(n_lines), final_newline=n_lines != 7)
    for name, lines in matching_sets(rng, n_lines, [0, n_lines]):
        reports = reports_for(rng, text, lines)
        for before, after in BA:
            got, batches = deliver_ref.play_file(text, reports, before, after, 3)
            assert got == deliver_ref.expected(text, reports, before, after, 0), (name, before, after)
            check_batches(batches, len(got), 3, name)
        parts = parts_for(rng, text, lines)
        assert deliver_ref.play_file(text, reports, 0, 0, 2, parts)[0] == deliver_ref.expected(text, reports, 0, 0, 0, parts), name


def test_cut_rule():
    """Behind the last newline; without one at the largest multiple of buffer_size - 1; else everything."""
    bs1 = 7
    assert deliver_ref.cut(b"abc\ndefgh\n", bs1) == 10  # a newline last
    assert deliver_ref.cut(b"abc\ndefghijklmnopqrstuvw", bs1) == 4  # a newline in the middle, however long the rest
    assert deliver_ref.cut(b"\nabc", bs1) == 1
    assert deliver_ref.cut(b"x" * 23, bs1) == 21  # no newline, above buffer_size - 1: a forced break
    assert deliver_ref.cut(b"x" * 14, bs1) == 14
    assert deliver_ref.cut(b"x" * 7, bs1) == 7  # equal
    assert deliver_ref.cut(b"x" * 6, bs1) == 6  # below: everything
    assert deliver_ref.cut(b"x", 262139) == 1


def test_sanitized_stand_alone_replay(tmp_path):
    """The same replay as a program of its own (deliversim.cpp's main), built with AddressSanitizer and UBSan: the calls of the
    7-line sweep, recorded as they were fed, give the same results there."""
    record = []
    cases = sweep(7, 1007, with_parts=False, record=record, ba=[(2, 3), (1000, 1000)]) + sweep(7, 2007, with_parts=True, record=record)
    calls = tmp_path / "calls.bin"
    calls.write_bytes(struct.pack(f"<{len(record)}Q", *record))
    exe = str(tmp_path / "deliversim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-pthread", "-DDELIVERSIM_MAIN", "-o", exe, deliver_ref.SRC, "-lz", "-ldl"])
    out = subprocess.run([exe, str(calls)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == cases and f"{cases} calls replayed" in out.stderr
    # the same sweeps again, in the same order, against the program's lines
    replayed = iter(lines)

    def compare(text, edges, reports, before, after, limit, buffer_count, parts=None, record=None):
        results, _, batches = next(replayed).partition("|")
        got = [(int(r.split(":")[0]), int(r.split(":")[1]), bytes.fromhex(r.split(":")[2])) for r in results.split()]
        return got, [int(b) for b in batches.split()], None  # (sweep asserts them against the expectation)

    sweep(7, 1007, with_parts=False, ba=[(2, 3), (1000, 1000)], play=compare)
    sweep(7, 2007, with_parts=True, play=compare)
