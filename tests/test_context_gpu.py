"""Context lines (grep -A / -B / -C) on the MI355X: hg_scan_device_context (the context stage, hypergrep_amd/csrc/hg_context.hip)
behind every scan path, the file API (hg_hyperscan_context), grep() and the command line.  Every expectation is context_ref's
plain Python reference (pieces, then the class of each piece by the definition) around the matching lines of the oracle
(oracle_py), or of the Python `re` brute force (minlensim_py.expected_piece) for sets with combinations, QUIET or min_length,
which the oracle does not have.  Texts sit at the end of guarded buffers: a read past them faults."""
from __future__ import annotations

import os
import random

import pytest

import chunk_texts
import context_ref
import huge_cases
import invert_ref
import oracle_py
from minlensim_py import COMBINATION, QUIET, expected_piece, exts_for

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")
TILE = 16384
LITERALS = ["needle-in-hay", "ERROR 42 failed"]  # literal tier (SINGLEMATCH, the default flags)
FILLER = [b"user=abc", b"12x", b"abc", b" ", b"-", b"quiet", b"zz", b"lorem ipsum dolor"]
BA = [(1, 0), (0, 1), (2, 3), (1000, 1000)]
BIG_BASE = (1 << 33) + 7
CTX, TAIL = context_ref.HG_ID_CONTEXT, context_ref.HG_ID_CONTEXT_TAIL


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 20)
    yield a
    a.free()


def log_text(rng: random.Random, nbytes: int, final_newline: bool = True, share: float = 0.08) -> bytes:
    """Lines of 0..~90 bytes, `share` of them with a match of LITERALS, cut to exactly nbytes."""
    out = bytearray()
    while len(out) < nbytes:
        words = [rng.choice(FILLER) for _ in range(rng.randint(0, 6))]
        if rng.random() < share:
            words.insert(rng.randint(0, len(words)), rng.choice(LITERALS).encode())
        out += b" ".join(words) + b"\n"
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


def check(arena, text, pats, flags=None, ids=None, bs=262140, line_base=0, need=None, by_re=False, invert=False, calls=((2, 3, 0, False),), min_launches=0):
    """One scanner, one text: for every (before, after, carry_after, tail) of `calls`, the scan with context leaves the hits of
    the scan without, and context() equals the reference.  Returns [(n_context, n_tail)] per call and the piece count."""
    from hypergrep_amd import device

    ids = ids or list(range(len(pats)))
    db = device.Database(pats, flags=flags, ids=ids, ext=exts_for(need) if need is not None else None)
    sc = device.Scanner(db, 0)
    ptr = arena.place(text)
    plain = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base, invert=invert)
    plain_hits = sc.hits()
    assert sc.context() == [] and (plain.n_context, plain.owed_after, plain.n_tail, plain.context_us) == (0, 0, 0, 0)
    if by_re:
        matching, n_lines = re_matching(text, pats, flags, ids, need or [None] * len(pats), bs, line_base)
    else:
        matching, n_lines = oracle_matching(text, pats, flags, ids, bs, line_base)
    if invert:
        matching = set(range(line_base, line_base + n_lines)) - matching
    assert {h[0] for h in plain_hits} == matching and plain.n_lines == n_lines
    out = []
    for before, after, carry, tail in calls:
        where = (pats, bs, len(text), line_base, before, after, carry, tail, invert)
        st = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base, invert=invert, context=(before, after), carry_after=carry, tail=tail)
        assert sc.hits() == plain_hits, where  # hits() is identical to the scan without context
        assert plain.stream_launches >= min_launches and st.stream_launches >= min_launches, where
        assert (st.n_hits, st.n_lines, st.n_candidates, st.n_raw_hits) == (plain.n_hits, plain.n_lines, plain.n_candidates, plain.n_raw_hits), where
        got = sc.context()
        want, owed, n_tail = context_ref.expected(text, bs, matching, before, after, line_base, carry, tail)
        assert got == want, where
        assert not {r[0] for r in got} & matching, where  # match and context lines are disjoint
        assert (st.n_context, st.owed_after, st.n_tail) == (len(want), owed, n_tail), where
        out.append((st.n_context, st.n_tail))
    # a following plain scan is unchanged and reports no context
    again = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base, invert=invert)
    assert sc.hits() == plain_hits and again.n_hits == plain.n_hits and again.context_us == 0 and again.n_context == 0 and sc.context() == []
    return out, n_lines


@pytest.mark.parametrize("bs", [262140, 4097, 100, 64])  # buffer_size - 1: above a tile, dividing 16384 (4096) and not (99, 63)
def test_three_tiles_and_a_ragged_tail(arena, bs):
    rng = random.Random(bs)
    text = bytearray(log_text(rng, 3 * TILE + 5, final_newline=False))  # 49157 bytes; the last line has no '\n'
    for k in (1, 2, 3):  # a line across each tile boundary: no newline on either side of it
        for at in (k * TILE - 1, k * TILE):
            if text[at] == 10:
                text[at] = ord("z")
    text = bytes(text)
    assert len(text) == 49157 and all(text[k * TILE - 1] != 10 and text[k * TILE] != 10 for k in (1, 2, 3))  # a line crosses a tile boundary
    calls = [(b, a, 0, False) for b, a in BA] + [(2, 3, 0, True)]
    counts, n = check(arena, text, LITERALS, bs=bs, calls=calls)
    assert all(0 < c < n for c, _t in counts)
    check(arena, text, LITERALS, bs=bs, line_base=BIG_BASE, calls=calls)


def planted(rng, npieces, at):
    """npieces short lines, the pieces of `at` matching, nothing else; (text, offsets of the lines)."""
    lines = [(b"needle-in-hay " if i in at else b"") + bytes(rng.choice(b"abcdefgh ") for _ in range(rng.randint(0, 40))) + b"\n" for i in range(npieces)]
    offs = [0]
    for line in lines:
        offs.append(offs[-1] + len(line))
    return b"".join(lines), offs


def test_contexts_that_meet_overlap_and_leave_a_gap(arena):
    """Two matches whose after- and before-context (A = 1, B = 2, and the reverse) overlap (3 pieces apart), meet (4) and leave
    one piece between them (5): inside a tile, and with the tile boundary between the two matches."""
    rng = random.Random(11)
    text, offs = planted(rng, 1700, ())
    boundary = next(i for i in range(len(offs)) if offs[i] >= TILE)  # the first line that starts in the second tile
    assert 3 * TILE > len(text) > 2 * TILE and boundary > 100
    for first in (50, boundary - 2):  # both matches in the first tile; one on each side of the boundary
        for gap in (3, 4, 5):
            at = {first, first + gap}
            text, offs = planted(random.Random(11), 1700, at)
            assert (offs[first] < TILE) and (offs[first + gap] >= TILE) == (first != 50)
            counts, _n = check(arena, text, LITERALS, calls=[(2, 1, 0, False), (1, 2, 0, False)])
            assert counts[0][0] == 2 + min(gap - 1, 3) + 1, (first, gap)
    # a match in the first piece and a match in the last piece
    text, _offs = planted(random.Random(12), 1700, {0, 1699})
    assert check(arena, text, LITERALS, calls=[(2, 3, 0, False), (2, 3, 0, True), (1000, 1000, 0, False)])[0] == [(5, 0), (5, 0), (1698, 0)]


@pytest.mark.parametrize("bs", [64, 4096, 262140])
def test_a_long_line(arena, bs):
    """40 KiB in one line: the piece cuts (every buffer_size - 1 bytes) against the tile cuts (every 16 KiB); with a NUL inside."""
    rng = random.Random(5)
    body = bytearray(rng.choice(b"abcdefgh ") for _ in range(40 << 10))
    for at in (100, 16380, 20000, 40000):
        body[at:at + 13] = b"needle-in-hay"
    calls = [(1, 0, 0, False), (0, 1, 0, False), (2, 3, 0, True), (0, 0, 1, False)]
    check(arena, bytes(body), LITERALS, bs=bs, calls=calls)
    body[30000] = 0
    check(arena, b"abc\nqq\nneedle-in-hay\n" + bytes(body) + b"\nlast\nline", LITERALS, bs=bs, calls=calls)


@pytest.mark.parametrize("text", [b"", b"\n", b"q", b"needle-in-hay\n\n", b"\n\n\n", b"\0abc\nab\0needle-in-hay\n\0\0needle-in-hay\n\0\n\0\0\0", b"0123456789abcde"],
                         ids=["0", "newline", "1", "15", "empty3", "nuls", "15b"])
def test_small_buffers_empty_lines_and_nuls(arena, text):
    for bs in (262140, 8, 3):
        check(arena, text, LITERALS + ["abc"], bs=bs, line_base=3, calls=[(1, 1, 0, False), (2, 3, 1, True), (0, 0, 5, False), (0, 0, 0, True)])


def test_every_line_matches_no_line_matches_and_carries(arena):
    rng = random.Random(3)
    text = b"".join(b"x needle-in-hay %d\n" % rng.randint(0, 10**rng.randint(1, 9)) for _ in range(2500))  # > 3 tiles
    assert len(text) > 3 * TILE
    # every line matches: no context record (the write launch is skipped), whatever is asked
    assert check(arena, text, LITERALS, calls=[(2, 2, 0, False), (1000, 1000, 7, True)]) == ([(0, 0), (0, 0)], 2500)
    # no line matches: no context; with the tail flag exactly the last min(B, n_lines) pieces, as tail records
    none = ["no-such-thing", "neither-this"]
    assert check(arena, text, none, calls=[(2, 2, 0, False), (2, 2, 0, True), (5000, 0, 0, True)])[0] == [(0, 0), (2, 2), (2500, 2500)]
    # the previous buffer's after-context: 1, 5, more than the buffer has pieces
    assert check(arena, text, none, calls=[(0, 2, 1, False), (0, 2, 5, False), (0, 2, 2501, False), (3, 2, 5, True)])[0] == [(1, 0), (5, 0), (2500, 0), (8, 3)]
    check(arena, log_text(rng, 2 * TILE + 100), LITERALS, calls=[(2, 2, 1, False), (2, 2, 5, True), (0, 0, 100000, False)])


def test_chaining_identity_on_the_device(arena):
    """The 49 157-byte text as two buffers, cut after the first piece, inside a context run, directly after a match and before
    the last piece: chained by owed_after and the tail rule, the two scans give the whole text's context."""
    from hypergrep_amd import device

    rng = random.Random(64)
    text = log_text(rng, 3 * TILE + 5, final_newline=False)
    before, after = 2, 3
    matching, n = oracle_matching(text, LITERALS, None, [0, 1], 262140, 0)
    offs = [0]
    for a, piece in invert_ref.pieces(text, 262140):
        offs.append(offs[-1] + len(piece))  # (no NULs: the pieces are the lines)
    assert offs[-1] == len(text)
    whole, _owed, _t = context_ref.expected(text, 262140, matching, before, after)
    m = next(x for x in sorted(matching) if x > n // 3 and not {x + 1, x + 2, x + 3} & matching)  # a match with three plain pieces behind it
    sc = device.Scanner(device.Database(LITERALS, ids=[0, 1]), 0)
    for cut in (1, m + 2, m + 1, n - 1):
        rows, carry, base, held = [], 0, 0, []
        for part in (text[:offs[cut]], text[offs[cut]:]):
            st = sc.scan(arena.place(part), len(part), line_base=base, context=(before, after), carry_after=carry, tail=True)
            hits = sorted({h[0] for h in sc.hits()})
            assert hits == [x for x in sorted(matching) if base <= x < base + st.n_lines]
            got = sc.context()
            if hits:
                rows += [r for r in held if r[0] >= hits[0] - before]
                held = []
            shift = offs[base]  # the second buffer's offsets are relative to its own start
            rows += [(r[0], CTX, 0, r[3] + shift, r[4]) for r in got if r[1] == CTX]
            held = [(r[0], CTX, 0, r[3] + shift, r[4]) for r in got if r[1] == TAIL]
            assert len(held) == st.n_tail
            base, carry = base + st.n_lines, st.owed_after
        assert base == n and sorted(rows) == whole, cut


def chunked_text(rng: random.Random) -> bytes:
    """More than 2048 tiles (chunk_texts): lines of log_text around the two cuts, a few repeated lines between them."""
    parts = [log_text(rng, 40000, share=0.3).splitlines(keepends=True) for _ in range(4)]
    parts[2].append(b"abc zz needle-in-hay " + b"q" * 300 + b" ERROR 42 failed\n")  # the line across the second cut
    fillers = [b"lorem ipsum dolor " * 45 + b"\n", b"zz - needle-in-hay " + b"quiet " * 100 + b"\n", b"12x " * 200 + b"\n", b"user=q " * 120 + b"\n", b"- " * 300 + b"\n"]
    return chunk_texts.build(parts, fillers)


def test_pipeline_chunks_and_segmented_scans(arena, monkeypatch):
    """A buffer the engine scans in several pipeline chunks, or in segments whose hits are put one after the other: the
    context stage runs once over the whole buffer's tile states and the concatenated hits."""
    from hypergrep_amd import device

    rng = random.Random(29)
    text = log_text(rng, (40 << 14) + 123, share=0.3)
    sc = device.Scanner(device.Database(LITERALS + ["abc"], flags=[6] * 3, ids=[0, 1, 2]), 0)
    raw = sc.scan(arena.place(text), len(text), buffer_size=1000).n_raw_hits
    assert raw > 4000
    for env in ({"HG_HIT_LIMIT": str(raw * 3 // 4)}, {"HG_HIT_LIMIT": str(raw * 11 // 20)}):  # (segments are 16 tiles at least)
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            counts, n = check(arena, text, LITERALS + ["abc"], [6] * 3, bs=1000, calls=[(1, 1, 0, True)])
            assert 500 < counts[0][0] < n, env
    # three pipeline chunks of 1024 tiles (the engine honours no smaller one): the matching lines by the `re` brute force, once
    # per distinct line
    big = device.GuardedArena(chunk_texts.SIZE + 64)
    try:
        with monkeypatch.context() as m:
            for k, v in chunk_texts.CHUNK_ENV.items():
                m.setenv(k, v)
            counts, n = check(big, chunked_text(rng), LITERALS + ["abc"], [6] * 3, bs=1000, by_re=True, calls=[(1, 1, 0, True)], min_launches=2)
            assert 500 < counts[0][0] < n
    finally:
        big.free()


def test_inverted_scan_with_context(arena):
    """invert=True: the records are the pieces without a match, so their context is matching pieces."""
    rng = random.Random(8)
    text = log_text(rng, 2 * TILE + 777, share=0.9)
    for bs in (262140, 50):
        counts, n = check(arena, text, LITERALS, bs=bs, invert=True, calls=[(2, 2, 0, False), (2, 2, 3, True)])
        assert 0 < counts[0][0] < n


@pytest.mark.parametrize("kind", ["literal", "always_on", "huge", "quiet"])
def test_behind_every_scan_path(arena, kind):
    from hypergrep_amd import device

    rng = random.Random(len(kind))
    calls = [(2, 3, 0, False), (1, 1, 2, True)]
    if kind == "quiet":  # QUIET + combination + min_length, checked by `re`: "quiet" reports only to the combination; abc[0-9]+ must span 6 bytes
        frags = [b"foo", b"bar", b"quiet", b"abc1", b"abc12345", b"zz", b" ", b"-", b"x"]
        text = b"".join(b" ".join(rng.choice(frags) for _ in range(rng.randint(0, 3)) if rng.random() < 0.3) + b" " + b"." * 60 + b"\n" for _ in range(800))
        pats, flags, ids = ["foo", "quiet", "101 & 102", r"abc[0-9]+"], [6, 6 | QUIET, COMBINATION, 6], [101, 102, 200, 7]
        counts, n = check(arena, text, pats, flags, ids, need=[None, None, None, 6], by_re=True, calls=calls)
        assert len(text) > 3 * TILE and 0 < counts[0][0] < n
        return
    pats = {"literal": LITERALS, "always_on": [r"[0-9]+xq", r"^[a-c]+q"], "huge": [r"needle[^\n]{0,5000}thread", "ERROR 42 failed"]}[kind]
    flags = [6] * len(pats) if kind != "literal" else None
    info = device.Database(pats, flags=flags).info()
    if kind == "literal":
        assert info["n_literal_anchored"] == 2 and info["n_always_on"] == 0
    elif kind == "always_on":
        assert info["n_always_on"] == 2
    else:
        assert pats[0] in huge_cases.ACCEPTED_HUGE  # (more than 1024 positions: the sparse tables and routines of hg_huge.hip)
    text = log_text(rng, 2 * TILE + 777)
    if kind == "always_on":
        text = text.replace(b"12x ", b"12xq ", 40).replace(b"\nabc ", b"\nabcq ", 40)
    if kind == "huge":
        text = text[:9000] + b"\nneedle " + b"q" * 3000 + b" thread\nneedle " + b"q" * 5100 + b" thread\n" + text[9000:]
    for bs in (262140, 50):
        counts, n = check(arena, text, pats, flags, bs=bs, calls=calls)
        assert 0 < counts[0][0] < n


# ---------------------------------------------------------------------------------------------------------- the file API
LINE = 40  # bytes per line of the chunked file: planting a match moves no chunk cut


def chunk_file(tmp_path, nlines, planted_at):
    """A file of `nlines` lines of LINE bytes, those of `planted_at` with a match.  Returns (path, data)."""
    rng = random.Random(nlines)
    rows = []
    for i in range(nlines):
        body = b"%07d " % i + bytes(rng.choice(b"abcdefgh0123456789 ") for _ in range(LINE - 9))
        if i in planted_at:
            body = body[:10] + b"needle-in-hay" + body[23:]
        rows.append(body + b"\n")
    data = b"".join(rows)
    path = tmp_path / f"chunks_{len(planted_at)}_{min(planted_at, default=0)}.txt"
    path.write_bytes(data)
    return str(path), data


def reader_cuts(data: bytes, cap: int):
    """The first line of every chunk after the first, by the reader's rule: a chunk is the bytes carried over plus what fills
    `cap`, cut behind its last newline."""
    cuts, pos = [], 0
    while len(data) - pos > cap:
        pos += data.rfind(b"\n", pos, pos + cap) + 1 - pos
        cuts.append(pos // LINE)
    return cuts


def file_rows(path, pats=("needle-in-hay",), **kwargs):
    import hypergrep_amd

    rows = []
    rc = hypergrep_amd.scan(path, list(pats), lambda m, c: rows.extend((m[i].line_number, m[i].id, m[i].line) for i in range(c)), **kwargs)
    assert rc == 0
    return rows


def expected_file_rows(data, matching, before, after):
    """The merged order: the matches (id 0) and the reference's context lines of the whole file scanned at once."""
    ctx, _owed, _t = context_ref.expected(data, 262140, matching, before, after)
    rows = [(q, 0, data[q * LINE:(q + 1) * LINE]) for q in matching] + [(r[0], CTX, data[r[3]:r[3] + r[4]]) for r in ctx]
    return sorted(rows)


def test_file_api_across_chunk_cuts(arena, tmp_path, monkeypatch):
    """A 2.5 MiB file read in 1 MiB chunks, matches within A and B pieces of both cuts and none elsewhere near them: the context
    of a match crosses the cut in both directions."""
    monkeypatch.setenv("HYPERGREP_CHUNK_MB", "1")
    nlines = (5 << 19) // LINE
    _path, data = chunk_file(tmp_path, nlines, set())
    c1, c2 = reader_cuts(data, 1 << 20)
    assert 0 < c1 < c2 < nlines and (c1 * LINE) % (1 << 20) != 0
    before, after = 2, 3
    planted = {c1 - 2, c2 + 1, c2 - 40, 5, nlines - 1}  # after-context over the first cut, before-context over the second
    path, data = chunk_file(tmp_path, nlines, planted)
    assert reader_cuts(data, 1 << 20) == [c1, c2]
    want = expected_file_rows(data, planted, before, after)
    got = file_rows(path, before_context=before, after_context=after)
    assert got == want
    lines = [r[0] for r in got]
    assert {c1 - 1, c1, c1 + 1, c2 - 1, c2} <= set(lines) and c1 + 2 not in lines and c2 - 2 not in lines
    assert file_rows(path, before_context=before, after_context=after, buffer_count=1) == want
    # a match directly on either side of a cut
    planted = {c1, c2 - 1}
    path, data = chunk_file(tmp_path, nlines, planted)
    assert file_rows(path, before_context=3, after_context=1) == expected_file_rows(data, planted, 3, 1)
    # inverted: every line but the planted ones is selected, the planted ones are their context
    got = file_rows(path, before_context=1, after_context=0, invert=True, max_match_count=0)
    assert len(got) == nlines
    assert sorted(r[0] for r in got if r[1] == CTX) == sorted(planted) and all(r[1] in (CTX, 0xFFFFFFFF) for r in got)


def test_file_api_before_context_longer_than_a_chunk(arena, tmp_path, monkeypatch):
    """Matches only in the first and in the last chunk, and more before-context than the chunk between them has pieces: that
    chunk has no match and fewer than B pieces, so the held tail is the last B of what was held plus all of its pieces."""
    monkeypatch.setenv("HYPERGREP_CHUNK_MB", "1")
    nlines = (5 << 19) // LINE
    _path, data = chunk_file(tmp_path, nlines, set())
    c1, c2 = reader_cuts(data, 1 << 20)
    before = c2 - c1 + 3000  # the middle chunk's pieces and 3000 of the first chunk's
    assert before < c2 - 4
    planted = {3, c2 + 10}
    path, data = chunk_file(tmp_path, nlines, planted)
    want = expected_file_rows(data, planted, before, 1)
    got = file_rows(path, before_context=before, after_context=1)
    assert got == want and len(got) == 3 + 1 + 1 + before + 1 + 1
    first_context = c2 + 10 - before
    assert c1 - 3000 < first_context < c1 and [r[0] for r in got[:6]] == [0, 1, 2, 3, 4, first_context]


def test_file_api_max_match_count(arena, tmp_path, monkeypatch):
    """max_match_count counts matches only; the trailing context of the last delivered line still goes out, ends before the
    next matching piece, and crosses a chunk cut when it has to."""
    monkeypatch.setenv("HYPERGREP_CHUNK_MB", "1")
    nlines = (5 << 19) // LINE
    _path, data = chunk_file(tmp_path, nlines, set())
    c1, _c2 = reader_cuts(data, 1 << 20)
    # the second match is followed by a match two lines on: one trailing line
    path, data = chunk_file(tmp_path, nlines, {10, 12, 14, 30})
    got = file_rows(path, before_context=1, after_context=3, max_match_count=2)
    assert [(r[0], r[1]) for r in got] == [(9, CTX), (10, 0), (11, CTX), (12, 0), (13, CTX)]
    assert got[2][2] == data[11 * LINE:12 * LINE]
    # ... by nothing: all three; without after-context the call ends with the match
    path, data = chunk_file(tmp_path, nlines, {10, 12, 30})
    assert [r[0] for r in file_rows(path, before_context=1, after_context=3, max_match_count=2)] == [9, 10, 11, 12, 13, 14, 15]
    assert [r[0] for r in file_rows(path, before_context=1, after_context=0, max_match_count=2)] == [9, 10, 11, 12]
    # the second match is the last line of the first chunk: its trailing context is the head of the next chunk, up to a match
    path, data = chunk_file(tmp_path, nlines, {7, c1 - 1, c1 + 5})
    got = file_rows(path, before_context=0, after_context=3, max_match_count=2)
    assert [(r[0], r[1]) for r in got] == [(7, 0), (8, CTX), (9, CTX), (10, CTX), (c1 - 1, 0), (c1, CTX), (c1 + 1, CTX), (c1 + 2, CTX)]
    assert got[-1][2] == data[(c1 + 2) * LINE:(c1 + 3) * LINE]
    path, data = chunk_file(tmp_path, nlines, {7, c1 - 1, c1 + 1})
    assert [r[0] for r in file_rows(path, before_context=0, after_context=3, max_match_count=2)] == [7, 8, 9, 10, c1 - 1, c1]


def test_file_api_gz_and_refused_ids(arena):
    import hypergrep_amd

    data = open(os.path.join(FILES, "samplefile.txt"), "rb").read()
    matching, _ = oracle_matching(data, ["bar"], [14], [0], 262140, 0)
    ctx, _owed, _t = context_ref.expected(data, 262140, matching, 1, 1)
    pcs = invert_ref.pieces(data, 262140)
    want = sorted([(q, 0, pcs[q][1]) for q in matching] + [(r[0], CTX, data[r[3]:r[3] + r[4]]) for r in ctx])
    assert any(r[1] == CTX for r in want)
    plain = file_rows(os.path.join(FILES, "samplefile.txt"), ["bar"], before_context=1, after_context=1)
    assert plain == file_rows(os.path.join(FILES, "samplefile.txt.gz"), ["bar"], before_context=1, after_context=1) == want
    called = []
    for rid in (0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF):
        assert hypergrep_amd.scan(os.path.join(FILES, "samplefile.txt"), ["bar"], lambda m, c: called.append(c), ids=[rid], after_context=1) == 4
    assert not called
    assert hypergrep_amd.scan(os.path.join(FILES, "samplefile.txt"), ["bar"], lambda m, c: called.append(c), ids=[0xFFFFFFFC], after_context=1) == 0 and called


def test_grep_and_command_line_end_to_end(arena, capsys, monkeypatch):
    """grep() and the `hyperscanner` command on the golden files: the rows and the output of the host formatting test's cases,
    every one equal to the local GNU grep's output and exit code."""
    import context_cli_cases as cli
    import hypergrep_amd
    from hypergrep_amd import multiscanner

    if cli.GREP is None:
        pytest.skip("no grep binary on this machine")
    for pattern, options, paths in cli.cases():
        opt = cli.parse(options)
        for path in paths:
            rows, rc = hypergrep_amd.grep(path, [pattern], ignore_case=opt["i"], only_matching=opt["o"] and not opt["v"], max_match_count=opt["m"], invert=opt["v"],
                                          before_context=opt["before"], after_context=opt["after"])
            assert rc == 0 and rows == cli.rows_for(path, pattern, opt), (pattern, options, path)
        monkeypatch.setattr("sys.argv", ["hyperscanner"] + options + ["-e", pattern] + paths)
        with pytest.raises(SystemExit) as exit_info:
            multiscanner.main()
        want, want_code = cli.grep_run(pattern, options, paths)
        assert (capsys.readouterr().out, exit_info.value.code) == (want, want_code), (pattern, options, paths)  # (exit 1: no line selected)
    # where lines are only counted or listed the options change nothing
    path = os.path.join(FILES, "greptest1.txt")
    for listing in (["-c"], ["-l"], ["-L"], ["-q"], ["-t"]):
        outs = []
        for extra in ([], ["-C", "2"]):
            monkeypatch.setattr("sys.argv", ["hyperscanner"] + listing + extra + ["bar", path])
            with pytest.raises(SystemExit) as exit_info:
                multiscanner.main()
            outs.append((capsys.readouterr().out, exit_info.value.code))
        assert outs[0] == outs[1], listing
