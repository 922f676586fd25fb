"""Every stream-mode cell (flow_cells.py) through Face A on the GPU, compared exactly with the cells' reference (Python `re`,
the construction and the stream rules; no product code).  A cell's runs are the streams of ONE batch: round r of
hg_scan_stream_batch carries every run's r-th write (a close is a zero-length LAST item), so a sweep of hundreds of cuts costs
a few launches; the batch runs twice on the same streams, which the end of data has reset, the second time with the items in
another order in every round.  Some runs of every cell also go through hs_scan_stream, hs_close_stream, hs_reset_stream and hs_copy_stream.
That the cells sit where they claim to, and that the reference is sound, is checked without a GPU in test_flow_cells.py."""
from __future__ import annotations

import pytest

import flow_cells as fc
from hypergrep_amd import device

pytestmark = pytest.mark.gpu
CELL_IDS = dict(ids=lambda c: c.name)


def database(cell):
    return device.StreamDatabase(cell.patterns, cell.flags, cell.ids, som_horizon=cell.horizon)


def batch_calls(sdb, runs, streams, order):
    """[[reports per call] per run]: round r is one scan_streams call over the runs that have a call r, in order(r)."""
    calls = [[] for _ in runs]
    for rnd in range(max(r.ncalls() for r in runs)):
        idx = [i for i in order(rnd) if rnd < runs[i].ncalls()]
        items, last = [], []
        for i in idx:
            w = runs[i].writes()
            a, b = w[rnd] if rnd < len(w) else (0, 0)
            items.append((streams[i], runs[i].data[a:b]))
            last.append(rnd == len(w) if runs[i].end == "close" else rnd == len(w) - 1)
        for i, reports in zip(idx, sdb.scan_streams(items, last=last)):
            calls[i].append(reports)
    return calls


def failures(cell, runs, calls):
    bad, reports = [], 0
    for r, c in zip(runs, calls):
        errors, _ = fc.compare(cell, r, c)
        reports += sum(map(len, c))
        if errors:
            bad.append((r.label, errors))
    return bad, reports


@pytest.mark.parametrize("cell", fc.CELLS, **CELL_IDS)
def test_cell_through_the_batch_call(cell):
    sdb = database(cell)  # (a fresh scratch: its report array has not grown)
    streams = [sdb.open() for _ in cell.runs]
    n = len(cell.runs)
    up = list(range(n))
    # (the second pass: a stream's state row is another one in every round)
    for label, order in (("first pass", lambda rnd: up), ("second pass, the items reversed in the even rounds and rotated in the odd", lambda rnd: up[n // 3:] + up[:n // 3] if rnd & 1 else up[::-1])):
        bad, reports = failures(cell, cell.runs, batch_calls(sdb, cell.runs, streams, order))
        assert not bad, (label, len(bad), bad[:5])
        assert reports > 0


def single_runs(cell):
    runs = [r for r in cell.runs if r.end == "close"]
    k = min(cell.single_entry, len(runs))
    return [runs[(2 * j + 1) * len(runs) // (2 * k)] for j in range(k)] if k else []


@pytest.mark.parametrize("cell", [c for c in fc.CELLS if single_runs(c)], **CELL_IDS)
def test_cell_through_the_single_stream_calls(cell):
    """hs_scan_stream per write, then hs_close_stream; on a second stream hs_reset_stream instead, twice over: a reset stream
    reports as a fresh one (SINGLEMATCH included)."""
    sdb = database(cell)
    bad = []
    for r in single_runs(cell):
        s = sdb.open()
        calls = [s.scan(r.data[a:b]) for a, b in r.writes()] + [s.close()]
        errors, _ = fc.compare(cell, r, calls)
        t = sdb.open()
        for life in range(2):
            calls = [t.scan(r.data[a:b]) for a, b in r.writes()] + [t.reset()]
            errors += fc.compare(cell, r, calls)[0]
        t.close()
        if errors:
            bad.append((r.label, errors))
    assert not bad, bad[:5]


COPIES = [("pieces", "carried/w4096/needle"), ("pieces", "carried/w8193/2-words"), ("pieces", "carried/w12288/29-words"), ("singlematch", "A-in-write-0/B-in-write-2"),
          ("contexts", "left/write/b'\\n'/x"), ("som-large", "three-writes/5/21"), ("som-small", "short/cut2")]


@pytest.mark.parametrize("name,label", COPIES)
def test_copy_mid_match_diverges(name, label):
    """A copy taken after the first write goes on with other bytes than its original: the original completes its match, the
    copy does not (and the other way round on a second pair)."""
    cell = fc.BY_NAME[name]
    run = next(r for r in cell.runs if r.label == label)
    cut = run.writes()[0][1]
    other = fc.Run(label + "/copy", run.data[:cut] + bytes(fc.fill(len(run.data) - cut)), run.cuts, "close")
    assert [w.key for w in fc.reference(cell, run)] != [w.key for w in fc.reference(cell, other)]
    sdb = database(cell)
    for mine, copys in ((run, other), (other, run)):
        s = sdb.open()
        first = s.scan(mine.data[:cut])
        t = s.copy()
        for stream, r in ((s, mine), (t, copys)):
            calls = [first] + [stream.scan(r.data[a:b]) for a, b in r.writes()[1:]] + [stream.close()]
            errors, _ = fc.compare(cell, fc.Run(r.label, r.data, r.cuts, "close"), calls)
            assert not errors, (r.label, errors)
