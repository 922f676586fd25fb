"""The gathered parts on the MI355X: hg_gather_parts (the parts gather, hypergrep_amd/csrc/hg_partlines.hip) behind
hg_scan_device_parts and hg_scan_device_segments_parts.  Every expectation is partlines_ref's plain Python reference (the entry
layout of include/hypergrep_amd.h) fed invert_ref's pieces, the matching lines of the oracle (oracle_py.scan_buffer) and
parts_ref's parts of them, never anything the stage computes.  Texts are a few 16 KiB tiles at the most and sit at the end of
guarded buffers: a read past them faults."""
from __future__ import annotations

import ctypes
import json
import os
import random

import pytest

import oracle_py
import partlines_ref as pr
import parts_ref
import segments_ref as sr

pytestmark = pytest.mark.gpu

TILE = 16384
A = 14  # DOTALL | MULTILINE | SINGLEMATCH
SET_AB = (["abc", "[0-9]+x|q"], [A, A])  # a literal-anchored expression and an always-on one
SET_DOT = (["abc.", "q"], [A, A])        # DOTALL: a part may include the line's '\n'
WORDS = [b"needle-in-hay", b"ERROR 42 failed", b"user=abc", b"12x", b"abc", b" ", b"-", b"quiet", b"zz", b"lorem ipsum dolor", b"7", b"x"]
MARKS = ((b"", b""), pr.COLOR)


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 20)
    yield a
    _scanners.clear()  # (before the interpreter takes the module's globals away)
    a.free()


_scanners = {}
_ref = {}  # (set, bytes, buffer_size) -> (hit lines, parts): computed once, never changed


def scanner(pset):
    from hypergrep_amd import device

    key = tuple(pset[0])
    if key not in _scanners:
        _scanners[key] = device.Scanner(device.Database(pset[0], flags=pset[1], ids=list(range(1, len(pset[0]) + 1))), 0)
    return _scanners[key]


def reference(pset, data, bs, limit=0):
    """(records, parts) of a text scanned alone: the oracle's hits (up to the limit's line) and parts_ref's parts of their
    lines, line numbers from 0."""
    key = (tuple(pset[0]), data, bs, limit)
    if key not in _ref:
        hits = []
        if data:
            rc, hits, _n = oracle_py.scan_buffer(data, pset[0], pset[1], list(range(1, len(pset[0]) + 1)), buffer_size=bs)
            assert rc == 0
        hits = sr.limited(hits, limit)
        _ref[key] = (hits, parts_ref.expected(data, bs, pset[0], pset[1], sorted({h[0] for h in hits})))
    return _ref[key]


def log_text(rng: random.Random, nbytes: int, final_newline: bool = True) -> bytes:
    """Lines of 0..~90 bytes, many of them with parts of SET_AB (some with several), cut to exactly nbytes."""
    out = bytearray()
    while len(out) < nbytes:
        out += b" ".join(rng.choice(WORDS) for _ in range(rng.randint(0, 6))) + b"\n"
    out = out[:nbytes]
    if nbytes:
        out[-1:] = b"\n" if final_newline else b"q"
    return bytes(out)


def _running(lengths):
    total = 0
    for n in lengths:
        total += n
        yield total


def compare(sc, stats, want, arrays, where, segments=False):
    a = sc.part_lines_arrays()
    off = a["entry_off"].tolist()
    assert off[0] == 0 and len(off) == len(want) + 1 and off[-1] == len(a["bytes"]) == stats.n_bytes and stats.n_entries == len(want), where
    assert a["bytes"] == b"".join(want), where  # (one comparison of the whole blob, then the cuts)
    assert off == [0] + list(_running(map(len, want))), where
    for name in ("line_number", "kind", "pattern") + (("segment",) if segments else ()):
        assert a[name].tolist() == arrays[name], (name, where)
    if not segments:
        assert a["segment"] is None and a["first_entry"] is None
    return a


def check(arena, text, bs, pset=SET_AB, line_base=0, byte_base=0, flag_sets=pr.ALL_FLAGS, marks=MARKS):
    """One scan with parts, then a parts gather per flag combination and pair of marks against the reference; the scan's own
    results stay as they were.  Returns (parts, {(flags, marks): (entries, arrays of the device)})."""
    sc = scanner(pset)
    ptr = arena.place(text)
    st = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base, parts=True)
    hits, rows = sc.hits(), sc.parts()
    _ohits, oparts = reference(pset, text, bs)
    parts = [(line_base + p[0], p[1], p[2], p[3], 0) for p in oparts]
    assert rows == [p[:4] for p in parts] and st.n_parts == len(parts)
    pieces = pr.pieces_of(text, bs, line_base)
    out = {}
    for flags in flag_sets:
        for mark in marks:
            g = sc._gather_parts(ptr, len(text), flags, mark, byte_base)  # pylint: disable=protected-access
            want, arrays = pr.expected(text, pieces, parts, flags, mark, byte_base)
            out[(flags, mark)] = (want, compare(sc, g, want, arrays, (flags, bs, mark)))
            if flags & pr.LINE:
                assert sc.part_lines() == pr.joined(want, arrays)
            if flags == 0 and mark == (b"", b""):  # the identity
                assert g.n_entries == st.n_parts and g.n_bytes == sum(p[2] - p[1] for p in parts)
    assert sc.hits() == hits and sc.parts() == rows  # a parts gather leaves the scan's results untouched
    return parts, out


@pytest.mark.parametrize("bs", [262140, 100, 64])
def test_every_flag_set_in_both_modes(arena, bs):
    rng = random.Random(bs)
    text = b"abc " * 40 + b"\n" + log_text(rng, 2 * TILE + 5, final_newline=False)  # a line of 160 bytes; the last line has no '\n'
    parts, out = check(arena, text, bs, byte_base=1000)
    assert len(parts) > len({p[0] for p in parts}) > 100  # several parts on some lines
    assert len(b"".join(out[(15, pr.COLOR)][0])) > TILE  # more than one workgroup
    if bs < 262140:
        assert max(p[2] for p in parts) < bs and len(pr.pieces_of(text, bs)) > text.count(b"\n") + 1  # pieces shorter than lines


def test_line_mode_alone_is_the_gathered_lines(arena):
    rng = random.Random(11)
    text = log_text(rng, TILE + 77)
    for bs in (262140, 64):
        sc = scanner(SET_AB)
        check(arena, text, bs, flag_sets=(pr.LINE,), marks=MARKS[:1])
        ptr = arena.place(text)
        sc.scan(ptr, len(text), buffer_size=bs, parts=True)
        sc.gather(ptr, len(text))
        lines = sc.lines_arrays()["bytes"]
        sc.gather_parts(ptr, len(text), whole_line=True)
        assert sc.part_lines_arrays()["bytes"] == lines and sc.part_lines() == sc.lines()


FILES = [
    b"", b"abc\n", b"abc\n", b"q\n", b"", b"x\n", b"abc", b"zz abc", b"abc\n" + (b"abc" * 21)[:63],  # (a last line of buffer_size - 1 bytes)
    b"q\nxabc yabc", b"abc\nx\nx\nx\nabc q\nx\n", b"x\nx\nx\n", b"x\nabc 12x q\nx\nx\nx\nx\nx\nq\nx\n", b"",
    b"q", b"x\n" * 40 + b"abc q abc\n" + b"x\n" * 3, b"abc\n", b"w" * 200 + b" 5x\nabc\n", b"\n\n\nq\n\n", b"", b"last abc",
]


@pytest.mark.parametrize("bs", [64, 262140])
def test_segments(arena, bs):
    """Files packed into one text: one-line files that all hold line 0, empty files, an unterminated last file (its pad),
    max_per_segment."""
    files = FILES
    sc = scanner(SET_AB)
    data, starts, ends = sr.pack(files)
    assert data[ends[-1]:] != b""  # the last file is unterminated: the pad follows it
    ptr = arena.place(data)
    for limit in (0, 1, 2):
        parts, pieces, first = [], {}, [0]
        for s, f in enumerate(files):
            _hits, own = reference(SET_AB, f, bs, limit)
            parts += [p + (s,) for p in own]
            first.append(len(parts))
            pieces.update(pr.pieces_of(f, bs, segment=s, at=starts[s]))
        st = sc.scan(ptr, len(data), buffer_size=bs, segments=(starts, ends), max_per_segment=limit, segment_parts=True)
        hits, rows, sp = sc.hits(), sc.parts(), sc.segment_parts()
        assert rows == [p[:4] for p in parts] and sp["first_part"].tolist() == first
        for flags in pr.ALL_FLAGS if limit == 0 else (0, 7, 15):
            for mark in MARKS:
                g = sc._gather_parts(ptr, len(data), flags, mark)  # pylint: disable=protected-access
                want, arrays = pr.expected(data, pieces, parts, flags, mark)
                a = compare(sc, g, want, arrays, (flags, bs, limit, mark), segments=True)
                assert a["first_entry"].tolist() == first
        assert sc.hits() == hits and sc.parts() == rows and sc.segment_parts()["first_part"].tolist() == first
        assert st.n_parts == len(parts)
    lines = sc.part_lines()  # (limit 2, flags 15, grep's colours) the one-line files 1 and 2: two lines, both line 1 at offset 0
    assert lines[0] == lines[1] == b"1:0:" + pr.COLOR[0] + b"abc" + pr.COLOR[1] + b"\n"


def test_parts_and_markers_across_an_output_tile_and_lines_of_many_parts(arena):
    """Lines of 100 parts each ("abc " a hundred times): with marks of 4 + 4 bytes an entry is 11 bytes and a part straddles
    output offset 16384, with 6 + 4 bytes an entry is 13 bytes and the opening mark does."""
    text = (b"abc " * 100 + b"\n") * 16
    for mark, what in (((b"<<<<", b">>>>"), "part"), ((b"<<<<<<", b">>>>"), "mark")):
        parts, out = check(arena, text, 262140, flag_sets=(0,), marks=(mark,))
        size = len(mark[0]) + 3 + len(mark[1])
        j = TILE // size  # the entry that holds output byte 16384
        lo = j * size + (len(mark[0]) if what == "part" else 0)
        hi = lo + (3 if what == "part" else len(mark[0]))
        assert len(parts) == 1600 and lo < TILE < hi, (what, lo, hi)
    parts, _ = check(arena, text, 262140, flag_sets=(pr.LINE, 15, 7), marks=MARKS)
    assert max(sum(1 for p in parts if p[0] == line) for line in range(16)) == 100  # more than 64 parts on a line


def test_long_parts_at_every_source_alignment(arena):
    """Parts of 41 bytes that begin at text offsets of every residue mod 4 (and mod 16): with flags 0 the output is the parts
    one after the other, so every part straddles 16-byte output chunks and its inner chunks are whole aligned dwords."""
    text = b"".join(b"." * k + b"1234567890" * 4 + b"x tail\n" for k in range(19))
    parts, _ = check(arena, text, 262140, flag_sets=(0, pr.LINE, 15), marks=((b"", b""), (b"<", b"")))
    pieces = pr.pieces_of(text, 262140)
    begins = {(pieces[(0, p[0])][0] + p[1]) % 16 for p in parts if p[2] - p[1] == 41}
    assert len(parts) == 19 and begins == set(range(16))


def test_more_entries_in_a_span_than_fit_the_staged_offsets(arena):
    """5000 lines of "q": one-byte parts without prefixes, all in one output span of 16 KiB: more than 2048 entries, so the lanes
    search the offsets in memory."""
    text = b"q\n" * 5000
    parts, out = check(arena, text, 262140, flag_sets=(0, pr.NUMBER, pr.LINE), marks=MARKS[:1])
    want, a = out[(0, (b"", b""))]
    assert len(parts) == 5000 > 2048 and a["bytes"] == b"q" * 5000 and a["entry_off"].tolist() == list(range(5001))


def test_a_part_that_includes_the_newline_and_first_and_last_edges(arena):
    # "abc." under DOTALL takes the '\n'; a last part with to == len (terminated and not); a first part with from == 0
    text = b"abc\nx abc\nabc q abcq\nq\nzz abcz"
    for bs in (262140, 8):
        parts, out = check(arena, text, bs, pset=SET_DOT)
    pieces = pr.pieces_of(text, 8)
    assert any(text[pieces[(0, p[0])][0] + p[2] - 1] == 10 for p in parts)  # a part that ends in the newline
    assert any(p[2] == pieces[(0, p[0])][2] for p in parts) and any(p[1] == 0 for p in parts)
    parts, out = check(arena, text, 262140, pset=SET_DOT, flag_sets=(pr.TERMINATE, pr.LINE | pr.TERMINATE), marks=MARKS[:1])
    assert out[(pr.TERMINATE, (b"", b""))][0][:2] == [b"abc\n", b"abc\n"] and out[(pr.LINE | pr.TERMINATE, (b"", b""))][0][-1] == b"zz abcz\n"


def test_zero_parts(arena):
    from hypergrep_amd import device

    sc = scanner(SET_AB)
    text = b"nothing here\nnor here\n"
    ptr = arena.place(text)
    assert sc.scan(ptr, len(text), buffer_size=64, parts=True).n_parts == 0
    for flags in (0, 15):
        g = sc._gather_parts(ptr, len(text), flags, pr.COLOR)  # pylint: disable=protected-access
        assert (g.n_entries, g.n_bytes) == (0, 0) and sc.part_lines() == [] and sc.part_lines_arrays()["entry_off"].tolist() == [0]
    assert isinstance(g, device.PartLinesStats)
    sc.scan(ptr, len(text), buffer_size=64, segments=([0, 13], [13, 22]), segment_parts=True)
    assert sc.gather_parts(ptr, len(text), number=True).n_entries == 0 and sc.part_lines_arrays()["first_entry"].tolist() == [0, 0, 0]


def test_both_decimals_cross_32_bits(arena):
    """line_base = 2^32 - 3 and byte_base = 2^32 - 5 on a small text: line numbers and offsets of 10 digits on both sides of
    2^32, the wide and the narrow division."""
    text = b"abc\nabc\nq abc\nabc\nq\n"
    parts, out = check(arena, text, 64, line_base=(1 << 32) - 3, byte_base=(1 << 32) - 5, flag_sets=(pr.NUMBER, pr.BYTE_OFFSET, 7, 15), marks=MARKS[:1])
    numbers = [int(e.split(b":")[0]) for e in out[(pr.NUMBER, (b"", b""))][0]]
    offsets = [int(e.split(b":")[0]) for e in out[(pr.BYTE_OFFSET, (b"", b""))][0]]
    assert min(numbers) < 1 << 32 <= max(numbers) and min(offsets) < 1 << 32 <= max(offsets)
    check(arena, text, 64, line_base=9_999_999_999_999_999_998, byte_base=(1 << 64) - 3, flag_sets=(7, 15), marks=MARKS[:1])  # 19 -> 20 digits; the offset wraps


def test_windows_of_a_larger_text(arena):
    """Windows [lo, hi) of a larger text with d_text = base + lo (lo a multiple of 16): what lies around the window is the real
    continuation of the text, and the result is the reference on data[lo:hi] alone.  hi falls inside a part, behind a part in
    the middle of a line, on a newline and behind it, so the terminator test and the trailing run end where nbytes says."""
    rng = random.Random(3)
    data = log_text(rng, 3000) + b"zz abc abc q tail of the line\n" + log_text(rng, 600)
    sc = scanner(SET_AB)
    ptr = arena.place(data)
    at = data.index(b"zz abc abc q tail")
    n = 0
    for lo in (0, 16, 496):
        for hi in (at + 5, at + 6, at + 8, at + 10, at + 12, at + 20, at + 29, at + 30, len(data) - 7):
            window = data[lo:hi]
            _hits, oparts = reference(SET_AB, window, 262140)
            parts = [p + (0,) for p in oparts]
            sc.scan(ptr + lo, hi - lo, buffer_size=262140, parts=True)
            assert sc.parts() == [p[:4] for p in parts], (lo, hi)
            pieces = pr.pieces_of(window, 262140)
            for flags in (0, 7, pr.LINE | pr.TERMINATE, 15):
                g = sc._gather_parts(ptr + lo, hi - lo, flags, (b"<", b">"), lo)  # pylint: disable=protected-access
                want, arrays = pr.expected(window, pieces, parts, flags, (b"<", b">"), lo)
                compare(sc, g, want, arrays, (lo, hi, flags))
                n += 1
    assert n == 108


def test_refusals(arena):
    from hypergrep_amd import device

    text = b"abc q\nx\nabc\n"
    ptr = arena.place(text)
    sc = device.Scanner(device.Database(SET_AB[0], flags=SET_AB[1], ids=[1, 2]), 0)
    err = lambda: device.lib().hg_scanner_error(sc._h).decode()  # noqa: E731  pylint: disable=protected-access
    with pytest.raises(ValueError, match="no successful scan"):
        sc.gather_parts(ptr, len(text))
    with pytest.raises(ValueError):
        sc.part_lines()
    with pytest.raises(ValueError):  # a refused scan: the last scan failed
        sc.scan(ptr, len(text), buffer_size=64, segments=([0, 4], [3, 12]), segment_parts=True)
    with pytest.raises(ValueError, match="no successful scan"):
        sc.gather_parts(ptr, len(text))
    for kw in ({}, {"invert": True}, {"context": (1, 1)}, {"segments": ([0, 6], [6, 12])}):
        sc.scan(ptr, len(text), buffer_size=64, **kw)
        with pytest.raises(ValueError, match="not one with parts"):
            sc.gather_parts(ptr, len(text))
    sc.scan(ptr, len(text), buffer_size=64, parts=True)
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.gather_parts(ptr + 16, len(text))
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.gather_parts(ptr, len(text) - 1)
    with pytest.raises(ValueError, match="unknown flag"):
        sc._gather_parts(ptr, len(text), 16)  # pylint: disable=protected-access
    for lens in ((17, 0), (0, 17), (1 << 31, 1)):
        with pytest.raises(ValueError, match="more than 16 bytes"):
            sc._gather_parts(ptr, len(text), 0, mark_lens=lens)  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="16 bytes"):
        sc.gather_parts(ptr, len(text), mark=(b"x" * 17, b""))
    params, res = device.HgPartLinesParams(), device.HgPartLinesResult()
    h = sc._h  # pylint: disable=protected-access
    assert device.lib().hg_gather_parts(h, ctypes.c_void_p(ptr), len(text), None, None, ctypes.byref(res)) == -1 and "params is NULL" in err()
    assert device.lib().hg_gather_parts(h, ctypes.c_void_p(ptr), len(text), ctypes.byref(params), None, None) == -1 and "result is NULL" in err()
    with pytest.raises(ValueError):
        sc.part_lines()  # nothing was gathered by any of these
    assert sc.gather_parts(ptr, len(text), mark=(b"x" * 16, b"y" * 16)).n_entries == 3  # 16 is allowed; the scanner is fine
    sc.scan(ptr, len(text), buffer_size=64, segments=([0, 6], [6, 12]), segment_parts=True)
    with pytest.raises(ValueError, match="byte_base must be 0"):
        sc.gather_parts(ptr, len(text), byte_offset=True, byte_base=1)
    assert sc.gather_parts(ptr, len(text), byte_offset=True, terminate=True).n_entries == 3 and sc.part_lines() == [b"0:abc\n", b"4:q\n", b"2:abc\n"]


def test_the_other_results_stay_as_they_are(arena):
    import torch

    from hypergrep_amd import device

    sc = device.Scanner(device.Database(SET_AB[0], flags=SET_AB[1], ids=[1, 2]), 0)
    text = b"abc q 12x\nx\nabc\nq q\n"
    ptr = arena.place(text)
    for kw in ({"parts": True}, {"segments": ([0, 12], [12, 20]), "segment_parts": True}):
        sc.scan(ptr, len(text), buffer_size=64, **kw)
        sc.gather(ptr, len(text), number=True, terminate=True)
        sc.count()
        before = (sc.hits(), sc.parts(), sc.lines(), sc.lines_arrays()["line_number"].tolist(), sc.counts())
        seg_before = sc.segment_parts()["first_part"].tolist() if "segments" in kw else None
        g = sc.gather_parts(ptr, len(text), number=True, byte_offset=True, terminate=True, whole_line=True, mark=(b"[", b"]"))
        assert g.n_entries == 6 and len(sc.part_lines()) == 3
        assert (sc.hits(), sc.parts(), sc.lines(), sc.lines_arrays()["line_number"].tolist(), sc.counts()) == before
        if seg_before is not None:
            assert sc.segment_parts()["first_part"].tolist() == seg_before and sc.part_lines()[2] == b"2:4:[q] [q]\n"
        else:
            assert sc.part_lines() == [b"1:0:[abc] [q] [12x]\n", b"3:12:[abc]\n", b"4:16:[q] [q]\n"]
    # the bytes into a device buffer
    blob = sc.part_lines_arrays()["bytes"]
    dst = torch.zeros(len(blob) + 8, dtype=torch.uint8, device="cuda")
    assert sc.copy_part_lines_to(dst.data_ptr(), len(blob) + 8) == len(blob)
    torch.cuda.synchronize()
    assert bytes(dst.cpu().numpy().tobytes()) == blob + b"\0" * 8
    # a scan takes the gather's result away
    sc.scan(ptr, len(text), buffer_size=64, parts=True)
    with pytest.raises(ValueError):
        sc.part_lines()


def test_kernel_resources():
    """The stage's kernels are in a table of their own with no scratch and no spills; the first table is what it was: the build
    before the counts stage (tests/golden/kernel_resources_before_counts.json) plus the counts kernels."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "hypergrep_amd", "lib", "kernel_resources_stages.json"), encoding="utf-8") as f:
        stages = json.load(f)
    with open(os.path.join(root, "hypergrep_amd", "lib", "kernel_resources.json"), encoding="utf-8") as f:
        table = json.load(f)
    with open(os.path.join(root, "tests", "golden", "kernel_resources_before_counts.json"), encoding="utf-8") as f:
        before = json.load(f)
    names = ("hg_partlines_entry_kernel", "hg_partlines_span_kernel", "hg_partlines_copy_kernel")
    assert len(stages) == 3 and all(sum(name in k for k in stages) == 1 for name in names) and not any("hg_gather_" in k for k in stages)
    for k, v in stages.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["Dynamic Stack"] == "False", (k, v)
    assert [v["LDS Size [bytes/block]"] for k, v in sorted(stages.items())] == [16384, 0, 0]  # the copy pass's staged offsets
    assert not any("hg_partlines_" in k for k in table)
    assert set(table) == set(before) | {k for k in table if "hg_counts_" in k}
    for k, v in before.items():
        assert table.get(k) == v, k
