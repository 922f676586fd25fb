"""Counts per report id on the MI355X: hg_count_records (the counts stage, hypergrep_amd/csrc/hg_counts.hip) behind every kind
of scan it accepts.  Every expectation is counts_ref's plain Python count of the records the same scan delivers
(Scanner.hits(), Scanner.segments()), which the parity tests hold to the oracle; nothing the stage computes is its own
yardstick.  Texts are some tens of kilobytes and sit at the end of a guarded buffer."""
from __future__ import annotations

import random

import pytest

import counts_ref
import segments_ref as sr

pytestmark = pytest.mark.gpu

S = 14  # DOTALL | MULTILINE | SINGLEMATCH
M = 6  # DOTALL | MULTILINE: every match end is a report
# 'a' and 'b' share id 1 and ' ' has id 2: the line "ab ab" leaves the records (id 1: to 1, 2, 4, 5), (id 2: to 3), so a run
# boundary can fall inside a (line, id) group, between the two ids of a line and between lines
ABS = (["a", "b", " "], [M, M, M], [1, 1, 2])


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


def scanner(pset, ext=None, fresh=False):
    from hypergrep_amd import device

    key = (tuple(pset[0]), tuple(pset[1]), tuple(pset[2]))
    if fresh or key not in _scanners:
        sc = device.Scanner(device.Database(pset[0], flags=pset[1], ids=pset[2], ext=ext), 0)
        if fresh:
            return sc
        _scanners[key] = sc
    return _scanners[key]


def want_of(sc, hits, segments=None):
    """{id: (lines, reports)} over every bin of the database, from the delivered records."""
    seg = segments if segments is not None else [0] * len(hits)
    ref = counts_ref.counts([(s, h[0], h[1]) for s, h in zip(seg, hits)])
    return {int(i): ref.get(int(i), (0, 0)) for i in sc.db.report_ids()}


def check(sc, where=None, **count_kwargs):
    hits = sc.hits()
    st = sc.count(**count_kwargs)
    assert st.n_records == len(hits) and st.n_bins == len(sc.db.report_ids()), where
    assert sc.counts() == want_of(sc, hits), where
    ids, n_lines, n_reports = sc.counts_arrays()
    assert ids.tolist() == sc.db.report_ids().tolist() and int(n_reports.sum()) == len(hits) and (n_lines <= n_reports).all(), where
    assert sc.hits() == hits, where  # the scan's own results stay as they were
    return st


def ab_text(n_records: int) -> bytes:
    """A text that leaves exactly n_records records under ABS: lines "ab ab" (5 records) and lines "a" (1 record)."""
    full, single = divmod(n_records, 5)
    lines = [b"ab ab\n"] * full
    for k in range(single):  # the short lines spread over the text
        lines.insert((k + 1) * len(lines) // (single + 1), b"a\n")
    return b"".join(lines)


@pytest.mark.parametrize("runs", [1, 2, 3])
def test_run_boundaries(arena, runs):
    from hypergrep_amd import device

    sc = scanner(ABS)
    for delta in (-1, 0, 1):
        n = runs * device.HG_COUNTS_RUN + delta
        text = ab_text(n)
        st = sc.scan(arena.place(text), len(text))
        assert st.n_hits == n
        check(sc, (runs, delta))
        got = sc.counts()
        assert got[1][1] + got[2][1] == n and got[2][0] == got[2][1] == n // 5 and got[1][0] == text.count(b"\n")


def test_hot_bin(arena):
    rng = random.Random(5)
    text = b"".join(b"line %d a%s\n" % (i, b" k07z" * rng.randint(0, 2)) for i in range(5000))
    for pset in ((["a"], [S], [3]), (["a", "line"], [S, S], [3, 9]), ([f"k{i:02d}z" for i in range(63)] + ["a"], [M] * 64, [7] * 64)):
        sc = scanner(pset)
        st = sc.scan(arena.place(text), len(text))
        assert st.n_hits >= 5000
        check(sc, len(pset[0]))
        assert sc.counts()[pset[2][0]][0] == 5000  # every line
    assert list(sc.counts()) == [7] and sc.counts()[7][1] > 5000  # 64 expressions, one bin


@pytest.mark.parametrize("extra", [0, 1])
def test_bin_count_limits(arena, extra):
    """HG_COUNTS_LDS_BINS bins are counted in LDS, one more in memory; sparse ids with 0 and 0xFFFFFFFC among them."""
    from hypergrep_amd import device

    n = device.HG_COUNTS_LDS_BINS + extra
    words = [f"w{i:04x}q" for i in range(n)]
    ids = [0, 0xFFFFFFFC] + [(i * 2654435761 + 12345) % 0xFFFFFFF0 + 1 for i in range(2, n)]
    assert len(set(ids)) == n
    rng = random.Random(n)
    order = list(range(n))
    rng.shuffle(order)  # expression order is not id order
    pset = ([words[i] for i in order], [S] * n, [ids[i] for i in order])
    sc = scanner(pset, fresh=True)
    assert len(sc.db.report_ids()) == n
    text = "".join(" ".join(words[rng.randrange(n)] for _ in range(rng.randint(0, 3))) + "\n" for _ in range(3000)).encode()
    text += " ".join([words[0], words[1], words[n - 1]] * 3).encode() + b"\n"  # the first, the second and the last bin for sure
    st = sc.scan(arena.place(text), len(text))
    assert st.n_hits > 3000
    check(sc, n)
    got = sc.counts()
    assert got[0][0] >= 1 and got[0xFFFFFFFC][0] >= 1 and sum(1 for v in got.values() if v[1]) > 1000


def test_report_rules(arena):
    from hypergrep_amd import device, utils

    text = b"foo bar foo\nfoobar\nbar\nfoo\n\nxfoooo bar\n" * 300
    quiet = device.DEFAULT_FLAGS | device.HS_FLAG_QUIET
    cases = [
        ((["foo", "ba."], [S, S], [4, 2]), None),  # SINGLEMATCH: one report per (line, id)
        ((["foo", "o+"], [M | device.HS_FLAG_SOM_LEFTMOST, M], [4, 2]), None),  # SOM
        ((["fo+", "bar"], [M, M], [1, 1]), [utils.ExprExt(flags=utils.HS_EXT_FLAG_MIN_LENGTH, min_length=4), None]),  # min_length
        ((["foo", "bar", "101 & !102"], [quiet, device.DEFAULT_FLAGS, device.HS_FLAG_COMBINATION], [101, 102, 5]), None),
    ]
    for pset, ext in cases:
        sc = scanner(pset, ext=ext, fresh=True)
        st = sc.scan(arena.place(text), len(text))
        assert st.n_hits > 300
        check(sc, pset[0])
        got = sc.counts()
        if 101 in got:  # the QUIET operand's bin stays 0, the combination's is counted
            assert got[101] == (0, 0) and got[5][1] > 0 and got[102][1] > 0
        if ext:
            assert got[1][1] < text.count(b"fo") + text.count(b"bar")  # the filter removed reports


def pack_case(run):
    """One pack: many one-line files inside one run, a file that spans three runs, empty files, files without a record, and an
    unterminated last line (it takes the pad)."""
    big = b"ab ab\n" * ((2 * run) // 5 + 40)  # more than two runs of records: it spans three
    return [b"ab\n", b"", b"a\n"] + [b"b a\n"] * 50 + [b"xyz\n", b"", big, b"xyz\nq\n", b"a\n", b"", b"ab ab\nxyz\nab a"]


@pytest.mark.parametrize("limit", [0, 1])
def test_segments(arena, limit):
    from hypergrep_amd import device

    sc = scanner(ABS)
    files = pack_case(device.HG_COUNTS_RUN)
    data, starts, ends = sr.pack(files)
    data = bytes(data)
    assert data.endswith(b"\0\n")
    sc.scan(arena.place(data), len(data), segments=(starts, ends), max_per_segment=limit)
    hits, seg = sc.hits(), sc.segments()
    rec_seg = seg["record_segment"].tolist()
    if not limit:
        assert len(hits) > 2 * device.HG_COUNTS_RUN
    st = sc.count(per_segment=True)
    assert (st.n_records, st.n_seg, st.n_bins) == (len(hits), len(files), 2)
    assert sc.counts() == want_of(sc, hits, rec_seg)
    lines, reports = sc.segment_counts()
    assert lines.shape == reports.shape == (len(files), 2)
    ids = sc.db.report_ids().tolist()
    for s in range(len(files)):
        row = counts_ref.counts([(s, h[0], h[1]) for h, g in zip(hits, rec_seg) if g == s])
        assert {i: (int(lines[s][b]), int(reports[s][b])) for b, i in enumerate(ids) if reports[s][b]} == row, s
        assert int(lines[s].sum()) >= int(seg["n_selected"][s])
    _, n_lines, n_reports = sc.counts_arrays()
    assert lines.sum(axis=0).tolist() == n_lines.tolist() and reports.sum(axis=0).tolist() == n_reports.tolist()
    assert not lines[1].any() and not lines[53].any() and reports[len(files) - 1].any()  # an empty file, one without a record, the padded one
    assert sc.hits() == hits and sc.segments()["record_segment"].tolist() == rec_seg
    # a single bin: a row's lines are the file's selected lines
    one = scanner((["a", "b"], [M, M], [8, 8]))
    one.scan(arena.place(data), len(data), segments=(starts, ends), max_per_segment=limit)
    one.count(per_segment=True)
    assert one.segment_counts()[0][:, 0].tolist() == one.segments()["n_selected"].tolist()
    # without the flag there are no matrices
    one.count()
    with pytest.raises(ValueError):
        one.segment_counts()


def test_other_scan_kinds(arena):
    rng = random.Random(11)
    text = b"".join(rng.choice([b"ab ab\n", b"xyz\n", b"a\n", b"\n", b"q b\n"]) for _ in range(4000))
    ptr = arena.place(text)
    sc = scanner(ABS)
    sc.scan(ptr, len(text))
    plain = want_of(sc, sc.hits())
    sc.scan(ptr, len(text), context=(1, 2))
    assert sc.context()
    check(sc, "context")
    assert sc.counts() == plain
    sc.scan(ptr, len(text), parts=True)
    assert sc.parts()
    check(sc, "parts")
    assert sc.counts() == plain
    sc.scan(ptr, len(text))
    sc.gather(ptr, len(text), number=True, terminate=True)
    gathered = sc.lines()
    check(sc, "after a gather")
    assert sc.counts() == plain and sc.lines() == gathered


def test_accumulate(arena):
    text = b"ab ab\nxyz\na\n" * 2500 + b"b"
    cut = text.index(b"\n", len(text) // 3) + 1  # a piece boundary
    sc = scanner(ABS, fresh=True)
    sc.scan(arena.place(text[:cut]), cut)
    first = want_of(sc, sc.hits())
    n_first = sc.count(accumulate=True).n_records  # the first call after the scanner is made starts from zero either way
    assert sc.counts() == first
    sc.scan(arena.place(text[cut:]), len(text) - cut, line_base=text[:cut].count(b"\n"))
    second = want_of(sc, sc.hits())
    st = sc.count(accumulate=True)
    both = sc.counts()
    assert n_first + st.n_records == sum(v[1] for v in both.values())
    sc.count()
    assert sc.counts() == second  # without the flag: the second buffer only
    sc.scan(arena.place(text), len(text))
    check(sc, "whole")
    assert sc.counts() == both == {i: (first[i][0] + second[i][0], first[i][1] + second[i][1]) for i in first}


def test_zero_records(arena):
    sc = scanner(ABS)
    text = b"xyz\nq\n" * 100
    st = sc.scan(arena.place(text), len(text))
    assert st.n_hits == 0
    c = sc.count()
    assert c.n_records == 0 and sc.counts() == {1: (0, 0), 2: (0, 0)}
    sc.scan(arena.place(b""), 0)
    assert sc.count().n_records == 0 and sc.counts() == {1: (0, 0), 2: (0, 0)}


def test_refusals(arena):
    from hypergrep_amd import device

    sc = scanner(ABS, fresh=True)
    with pytest.raises(device.DeviceError, match="no successful scan"):
        sc.count()
    text = b"ab ab\nxyz\n" * 50
    ptr = arena.place(text)
    sc.scan(ptr, len(text), invert=True)
    with pytest.raises(device.DeviceError, match="inverted"):
        sc.count()
    sc.scan(ptr, len(text))
    with pytest.raises(device.DeviceError, match="without segments"):
        sc.count(per_segment=True)
    res = device.HgCountsResult()
    import ctypes

    assert device.lib().hg_count_records(sc._h, 4, None, ctypes.byref(res)) == -1 and b"unknown flag" in device.lib().hg_scanner_error(sc._h)  # pylint: disable=protected-access
    assert device.lib().hg_count_records(sc._h, 0, None, None) == -1 and b"NULL" in device.lib().hg_scanner_error(sc._h)  # pylint: disable=protected-access
    check(sc, "after the refusals")
    assert sc.counts() == {1: (50, 200), 2: (50, 50)}
