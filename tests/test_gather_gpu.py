"""The gathered lines on the MI355X: hg_gather_lines (the gather stage, hypergrep_amd/csrc/hg_gather.hip) behind every kind of
scan.  Every expectation is gather_ref's plain Python reference (invert_ref.pieces, context_ref.classify, the entry layout of
include/hypergrep_amd.h) fed the matching lines of the oracle (oracle_py.scan_buffer), never anything the stage computes.
Texts are a few 16 KiB tiles at the most and sit at the end of guarded buffers: a read past them faults."""
from __future__ import annotations

import json
import os
import random

import pytest

import gather_ref as gr
import invert_ref
import oracle_py
import segctx_ref
import segments_ref as sr

pytestmark = pytest.mark.gpu

TILE = 16384
A = 14  # DOTALL | MULTILINE | SINGLEMATCH
LITERALS = (["needle-in-hay", "ERROR 42 failed"], [A, A])
SET_AQ = (["abc", "q"], [A, A])
WORDS = [b"needle-in-hay", b"ERROR 42 failed", b"user=abc", b"12x", b"abc", b" ", b"-", b"quiet", b"zz", b"lorem ipsum dolor"]


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
_oracle = {}  # (set, bytes, buffer_size) -> (hits, n_lines): computed once, never changed


def scanner(pset):
    from hypergrep_amd import device

    key = tuple(pset[0])
    if key not in _scanners:
        _scanners[key] = device.Scanner(device.Database(pset[0], flags=pset[1], ids=list(range(1, len(pset[0]) + 1))), 0)
    return _scanners[key]


def oracle(pset, data, bs):
    key = (tuple(pset[0]), data, bs)
    if key not in _oracle:
        if not data:
            _oracle[key] = ([], 0)
        else:
            rc, hits, n_lines = oracle_py.scan_buffer(data, pset[0], pset[1], list(range(1, len(pset[0]) + 1)), buffer_size=bs)
            assert rc == 0
            _oracle[key] = (hits, n_lines)
    return _oracle[key]


def log_text(rng: random.Random, nbytes: int, final_newline: bool = True) -> bytes:
    """Lines of 0..~90 bytes, about a third of them with a match of LITERALS (some with both), cut to exactly nbytes."""
    out = bytearray()
    while len(out) < nbytes:
        out += b" ".join(rng.choice(WORDS) for _ in range(rng.randint(0, 6))) + b"\n"
    out = out[:nbytes]
    if nbytes:
        out[-1:] = b"\n" if final_newline else b"q"
    return bytes(out)


def compare(sc, got_stats, want, items, where):
    a = sc.lines_arrays()
    off = a["entry_off"].tolist()
    assert off[0] == 0 and len(off) == len(want) + 1 and off[-1] == len(a["bytes"]) == got_stats.n_bytes and got_stats.n_entries == len(want), where
    assert a["bytes"] == b"".join(want), where  # (one comparison of the whole blob, then the cuts)
    assert off == [0] + list(_running(map(len, want))), where
    assert a["line_number"].tolist() == [i[1] for i in items] and a["kind"].tolist() == [i[2] for i in items], where
    return a


def _running(lengths):
    total = 0
    for n in lengths:
        total += n
        yield total


def check(arena, text, bs, pset=LITERALS, invert=False, context=None, carry_after=0, tail=False, line_base=0, flag_sets=gr.ALL_FLAGS):
    """One scan, then a gather per flag combination against the reference; the scan's own results stay as they were."""
    sc = scanner(pset)
    ptr = arena.place(text)
    st = sc.scan(ptr, len(text), buffer_size=bs, line_base=line_base, invert=invert, context=context, carry_after=carry_after, tail=tail)
    hits, ctx = sc.hits(), sc.context()
    ohits, n_lines = oracle(pset, text, bs)
    matching = {line_base + h[0] for h in ohits}
    selected = set(range(line_base, line_base + n_lines)) - matching if invert else matching
    assert {h[0] for h in hits} == selected and st.n_lines == n_lines
    out = None
    for flags in flag_sets:
        g = sc._gather(ptr, len(text), flags)  # pylint: disable=protected-access
        want, items = gr.expected(text, bs, selected, flags, line_base, context, carry_after, tail)
        out = compare(sc, g, want, items, (flags, bs, invert, context))
        if flags == 0:  # the identity
            distinct = {h[0]: h[4] for h in hits}
            assert g.n_entries == len(distinct) and g.n_bytes == sum(distinct.values())
    assert sc.hits() == hits and sc.context() == ctx  # a gather leaves the scan's results untouched
    return st, out


@pytest.mark.parametrize("bs", [262140, 100, 64])
def test_three_tiles_and_a_ragged_tail(arena, bs):
    rng = random.Random(bs)
    text = log_text(rng, 3 * TILE + 5, final_newline=False)  # 49157 bytes; the last line has no '\n'
    assert len(text) == 49157
    hits, _ = oracle(LITERALS, text, bs)
    assert len(hits) > len({h[0] for h in hits}) > 100  # several reports on some lines
    check(arena, text, bs)
    check(arena, text, bs, invert=True)
    check(arena, text, bs, context=(1, 2))


def test_pieces_that_end_at_a_nul_and_leading_nuls(arena):
    text = b"\0abc\nab\0needle-in-hay\n\0\0needle-in-hay\n\0\n\0\0needle-in-hay\0x\n\0\0\0"  # no trailing newline; the last piece is NULs only
    for bs in (262140, 8):
        check(arena, text, bs)
        _, a = check(arena, text, bs, invert=True, flag_sets=(gr.TERMINATE,))
        assert a["bytes"].endswith(b"\n\n")  # the piece of NULs only has len 0: TERMINATE makes it a bare newline
        check(arena, text, bs, invert=True)
    check(arena, b"needle-in-hay", 262140, flag_sets=(0, gr.TERMINATE, 15))


@pytest.mark.parametrize("line_base", [8, 98, 9_999_998, (1 << 33) + 7, 9_999_999_999_999_999_998])
def test_decimal_width(arena, line_base):
    """Entries on both sides of every width change (9 -> 10, 99 -> 100, 9 999 999 -> 10 000 000, 19 -> 20 digits)."""
    text = b"needle-in-hay\nq\nneedle-in-hay\nneedle-in-hay\nq\nq\n"
    for invert in (False, True):
        _, a = check(arena, text, 64, invert=invert, context=(1, 1), line_base=line_base, flag_sets=(gr.NUMBER, 5, 15))
        widths = {len(str(n + 1)) for n in a["line_number"].tolist()}
        assert len(widths) == (1 if line_base == (1 << 33) + 7 else 2)


def test_one_entry_larger_than_several_output_tiles(arena):
    rng = random.Random(5)
    body = bytearray(rng.choice(b"abcdefgh ") for _ in range(40 << 10))
    body[20000:20013] = b"needle-in-hay"
    text = b"before\n" + bytes(body) + b"\nafter\nneedle-in-hay x\n"
    st, a = check(arena, text, 262140, context=(1, 1))
    assert len(a["bytes"]) > 2 * TILE
    check(arena, text, 262140, invert=True, flag_sets=(0, 15))
    check(arena, text, 4096, flag_sets=(0, 15))  # ... and cut into pieces of 4095 bytes


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_entry_boundaries_on_tile_boundaries(arena, d):
    """Under an inverted scan without a match every line is an entry: the first ends d bytes from the first output tile's end,
    the third exactly on the second tile's end (flags 0)."""
    from hypergrep_amd import device

    first = b"a" * (device.HG_GATHER_TILE + d - 1) + b"\n"
    second = b"b" * 29 + b"\n"
    third = b"c" * (2 * device.HG_GATHER_TILE - len(first) - len(second) - 1) + b"\n"
    text = first + second + third + b"dddd\n"
    _, a = check(arena, text, 262140, invert=True, flag_sets=tuple(reversed(gr.ALL_FLAGS)))  # (flags 0 last: `a` is its result)
    assert a["entry_off"].tolist()[:4] == [0, device.HG_GATHER_TILE + d, device.HG_GATHER_TILE + d + 30, 2 * device.HG_GATHER_TILE]


def test_many_entries_per_dword(arena):
    """70 000 lines of one newline under invert: entries of one byte, four per stored dword; with NUMBER the widths change
    inside a tile."""
    text = b"\n" * 70000
    st, a = check(arena, text, 262140, invert=True, flag_sets=(0, gr.NUMBER, 15))
    assert st.n_hits == 70000 and len(a["entry_off"]) == 70001


def test_zero_entries(arena):
    from hypergrep_amd import device

    sc = scanner(LITERALS)
    text = b"nothing here\nnor here\n"
    ptr = arena.place(text)
    sc.scan(ptr, len(text), buffer_size=64)
    for flags in (0, 15):
        g = sc._gather(ptr, len(text), flags)  # pylint: disable=protected-access
        assert (g.n_entries, g.n_bytes) == (0, 0) and sc.lines() == [] and sc.lines_arrays()["entry_off"].tolist() == [0]
    assert isinstance(g, device.GatherStats)


@pytest.mark.parametrize("context", [(1, 2), (0, 3), (5, 0)])
def test_context(arena, context):
    q = b"quiet line\n"
    hit = b"a needle-in-hay\n"
    # adjacent groups (their context touches), separated groups, a match on the first and on the last line
    text = hit + q * 2 + hit + q * 3 + hit + hit + q * 9 + hit + q * 12 + hit + q * 7 + hit
    for bs in (262140, 24):
        _, a = check(arena, text, bs, context=context)
        check(arena, text, bs, context=context, invert=True, flag_sets=(1, 15))
        st, a = check(arena, text, bs, context=context, carry_after=2, tail=True, line_base=40)
        if context[0]:
            assert st.n_tail == 0  # (the last line matches: nothing is left for a tail)
    text += q * 9
    st, a = check(arena, text, 262140, context=context, carry_after=1, tail=True)
    kinds = a["kind"].tolist()
    if context[0]:
        assert st.n_tail > 0 and kinds[-st.n_tail:] == [gr.KIND_TAIL] * st.n_tail and gr.KIND_TAIL not in kinds[:-st.n_tail]  # kind 2 appears, in order
    # with and without HG_LINES_CONTEXT after the same scan: check() ran flags 0 .. 15 on one scan


FILES_24 = [
    b"", b"abc\n", b"abc\n", b"q\n", b"", b"x\n", b"abc", b"zz abc", b"abc\n" + (b"abc" * 63)[:63],  # (a last line of buffer_size - 1 bytes: a phantom piece in the pad)
    b"abc\n\0\0\0", b"q\nxabc\0yabc", b"\0", b"abc\nx\nx\nx\nabc q\nx\n", b"x\nx\nx\n", b"x\nabc\nx\nx\nx\nx\nx\nq\nx\n", b"", b"abc\n" + (b"abd" * 62)[:62],
    b"q", b"x\n" * 40 + b"abc q abc\n" + b"x\n" * 3, b"abc\n", b"w" * 200 + b"\nabc\n", b"\n\n\nq\n\n", b"", b"last abc",
]


def file_scan(bs, invert):
    """bytes -> (ordered records, n_lines) of a file scanned alone, from the oracle."""
    def scan_alone(data):
        hits, n_lines = oracle(SET_AQ, data, bs)
        if invert:
            return invert_ref.expected(data, bs, [h[0] for h in hits]), n_lines
        return hits, n_lines
    return scan_alone


@pytest.mark.parametrize("bs", [64, 262140])
@pytest.mark.parametrize("invert", [False, True])
def test_segments(arena, bs, invert):
    files = FILES_24
    assert len(files) == 24
    sc = scanner(SET_AQ)
    data, starts, ends = sr.pack(files)
    ptr = arena.place(data)
    for limit, context in ((0, None), (1, None), (2, None), (0, (1, 2)), (1, (2, 1))):
        per_file = sr.expected(data, starts, ends, file_scan(bs, invert), limit)
        selected = [{r[0] for r in records} for records, _n, _sel in per_file]
        ctx_lines = None
        if context is not None:
            rows = segctx_ref.expected(data, starts, ends, file_scan(bs, invert), bs, context[0], context[1], limit)
            ctx_lines = [[r[0] for r in file_rows] for file_rows in rows]
        st = sc.scan(ptr, len(data), buffer_size=bs, invert=invert, segments=(starts, ends), max_per_segment=limit, context=context)
        hits, seg = sc.hits(), sc.segments()
        assert [sorted({h[0] for h in hits[a:z]}) for a, z in zip(seg["first_record"].tolist(), seg["first_record"].tolist()[1:])] == [sorted(s) for s in selected]
        for flags in gr.ALL_FLAGS if limit == 0 else (0, 15):
            g = sc._gather(ptr, len(data), flags)  # pylint: disable=protected-access
            want, items, first_entry = gr.expected_files(files, bs, selected, flags, ctx_lines)
            a = compare(sc, g, want, items, (flags, bs, invert, limit, context))
            assert a["segment"].tolist() == [i[0] for i in items] and a["first_entry"].tolist() == first_entry
            if flags & gr.SEPARATOR:  # a separator at every file change
                assert all(w.startswith(b"--\n") for k, w in enumerate(want) if k and items[k][0] != items[k - 1][0])
        assert sc.hits() == hits and sc.segments()["first_record"].tolist() == seg["first_record"].tolist()
    # several one-line files whose line is line 0: two entries, not one
    if not invert:
        lines = sc.lines()
        assert want[0].endswith(b"abc\n") and want[1].endswith(b"abc\n") and items[0][:2] == (1, 0) and items[1][:2] == (2, 0) and len(lines) == len(want)


def test_life_cycle(arena):
    import ctypes

    import torch

    from hypergrep_amd import device

    sc = device.Scanner(device.Database(LITERALS[0], flags=LITERALS[1], ids=[1, 2]), 0)
    text = b"a needle-in-hay\nq\nERROR 42 failed needle-in-hay\nq\nq\n"
    ptr = arena.place(text)
    with pytest.raises(ValueError, match="no successful scan"):
        sc.gather(ptr, len(text))
    with pytest.raises(ValueError):
        sc.lines()
    st = sc.scan(ptr, len(text), buffer_size=64, context=(1, 1))
    hits, ctx = sc.hits(), sc.context()
    assert st.n_hits == 3 and len(ctx) == 2
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.gather(ptr + 16, len(text))
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.gather(ptr, len(text) - 1)
    with pytest.raises(ValueError, match="unknown flag"):
        sc._gather(ptr, len(text), 16)  # pylint: disable=protected-access
    assert device.lib().hg_gather_lines(sc._h, ctypes.c_void_p(ptr), len(text), 0, None, None) == -1  # pylint: disable=protected-access
    with pytest.raises(ValueError):
        sc.lines()  # no gather since the scan
    g = sc.gather(ptr, len(text), context=True, terminate=True, number=True, separator=True)
    assert sc.lines() == [b"1:a needle-in-hay\n", b"2-q\n", b"3:ERROR 42 failed needle-in-hay\n", b"4-q\n"] and g.n_entries == 4
    assert sc.hits() == hits and sc.context() == ctx  # unchanged by the gather
    assert sc.gather(ptr, len(text)).n_entries == 2 and sc.lines() == [b"a needle-in-hay\n", b"ERROR 42 failed needle-in-hay\n"]
    # the bytes into a device buffer
    blob = sc.lines_arrays()["bytes"]
    dst = torch.zeros(len(blob) + 8, dtype=torch.uint8, device="cuda")
    assert sc.copy_lines_to(dst.data_ptr(), len(blob) + 8) == len(blob)
    torch.cuda.synchronize()
    assert bytes(dst.cpu().numpy().tobytes()) == blob + b"\0" * 8
    # a second scan followed by a gather describes the second scan
    other = b"q\nERROR 42 failed\n"
    ptr = arena.place(other)
    sc.scan(ptr, len(other), buffer_size=64, invert=True)
    with pytest.raises(ValueError):
        sc.lines()
    assert sc.gather(ptr, len(other), number=True).n_entries == 1 and sc.lines() == [b"1:q\n"]
    # ... after scans with segments and with parts
    seg_text = b"needle-in-hay\nneedle-in-hay\n"
    ptr = arena.place(seg_text)
    sc.scan(ptr, len(seg_text), buffer_size=64, segments=([0, 14], [14, 28]))
    assert sc.gather(ptr, len(seg_text), number=True, separator=True).n_entries == 2 and sc.lines() == [b"1:needle-in-hay\n", b"--\n1:needle-in-hay\n"]
    assert sc.segments()["first_record"].tolist() == [0, 1, 2] and sc.lines_arrays()["first_entry"].tolist() == [0, 1, 2]
    sc.scan(ptr, len(seg_text), buffer_size=64, parts=True)
    assert sc.gather(ptr, len(seg_text)).n_bytes == 28 and len(sc.parts()) == 2 and sc.lines_arrays()["segment"] is None


def test_kernel_resources():
    """The stage's kernels are in the build's table with no scratch and no spills, and every kernel the build had before the
    stage is unchanged (tests/golden/kernel_resources_before_gather.json: that build's table)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "hypergrep_amd", "lib", "kernel_resources.json"), encoding="utf-8") as f:
        table = json.load(f)
    with open(os.path.join(root, "tests", "golden", "kernel_resources_before_gather.json"), encoding="utf-8") as f:
        before = json.load(f)
    mine = {k: v for k, v in table.items() if "hg_gather_" in k}
    names = ("hg_gather_flag_kernel", "hg_gather_entry_kernel", "hg_gather_first_kernel", "hg_gather_span_kernel", "hg_gather_copy_kernel")
    assert len(mine) == 5 and all(sum(name in k for k in mine) == 1 for name in names)
    assert not any("hg_segparts_" in k or "hg_segctx_" in k for k in mine)
    for k, v in mine.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert len(before) > 100 and not any("hg_gather_" in k for k in before)
    for k, v in before.items():
        assert table.get(k) == v, k
