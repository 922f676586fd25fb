"""The verify cells (tests/verify_cells.py) on the GPU (run with `-m gpu`): for every text of every cell all five columns of
hits() and the line count equal the reference (bytes.find per literal and piece, then the report rules), and the scan's
statistics show what the cell claims: the candidates the filter passed, the false positives among them, the repeated pass of
an overflowing list, the joiner's launches.  Texts sit at the end of a guarded arena: a read past them faults."""
from __future__ import annotations

import time

import pytest

import verify_cells as vc

pytestmark = pytest.mark.gpu

KNOBS = ("HG_FIN_TARGET", "HG_NO_BUCKET_FINALIZE", "HG_CHUNK_TILES", "HG_MAX_CHUNKS", "HG_CHUNK_WEIGHTS", "HG_NO_EARLY_FINALIZE", "HG_JOINER", "HG_JOINER_AHEAD",
         "HG_STREAM_WGS_PER_CU", "HG_HIT_LIMIT", "HG_CAND_LIMIT")
CELLS = vc.CELLS


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(36 << 20)
    yield a
    a.free()


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_verify_cell(arena, cell, monkeypatch):
    from hypergrep_amd import device

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in cell.env.items():
        monkeypatch.setenv(k, v)  # (read when the scanner is created)
    pats, flags, ids = vc.cell_patterns(cell)
    sc = device.Scanner(device.Database(pats, flags=flags, ids=ids), 0)
    claim = cell.claim
    for which, (name, text) in enumerate(cell.texts):
        data = vc.text_bytes(text)
        records, n_lines, verified = vc.cell_reference(cell, which)
        t0 = time.perf_counter()
        stats = sc.scan(arena.place(data), len(data), buffer_size=cell.buffer_size)
        ms = (time.perf_counter() - t0) * 1e3
        if which < 3 or len(cell.texts) < 16:
            print(f"{cell.name}/{name}: reports {stats.n_hits}, candidates {stats.n_candidates}, verified pairs {verified}, reruns {stats.reruns}, "
                  f"stream launches {stats.stream_launches}, joiner launches {stats.joiner_launches}, {ms:.1f} ms")
        got = sc.hits()
        assert stats.n_lines == n_lines, (name, stats.n_lines, n_lines)
        assert stats.n_hits == len(records) == len(got), (name, stats.n_hits, len(records))
        if got != records:
            i = next(i for i, (a, b) in enumerate(zip(got, records)) if a != b)
            pytest.fail(f"{cell.name}/{name}: hits() differs from the reference at position {i}: got {got[max(i - 2, 0):i + 3]}, want {records[max(i - 2, 0):i + 3]}")
        if name in claim.get("candidates", {}):
            assert stats.n_candidates == claim["candidates"][name], name
        if name in claim.get("false_positives_min", {}):
            # more candidates than literal occurrences, by the planted number at least: windows that belong to no literal
            assert stats.n_candidates >= verified + claim["false_positives_min"][name], (name, stats.n_candidates, verified)
        if "reruns_min" in claim:  # the first scan of a fresh scanner overflows the list and repeats the pass; the second fits
            assert (stats.reruns >= claim["reruns_min"]) if which == 0 else (stats.reruns == claim["second_reruns"]), (which, stats.reruns)
        if "joiner_launches_min" in claim:
            assert stats.joiner_launches >= claim["joiner_launches_min"]
        if "stream_launches_min" in claim:
            assert stats.stream_launches >= claim["stream_launches_min"]
