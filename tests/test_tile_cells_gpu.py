"""The tile-scan cells (tests/tile_cells.py) on the GPU (run with `-m gpu`): for every cell all five columns of hits() and the
line count equal the reference, which knows newline positions and nothing of tiles; the launches a cell claims (three
pipeline chunks, two or four segments, one chunk for the large cell) are asserted from the scan's statistics."""
from __future__ import annotations

import time

import numpy as np
import pytest

import tile_cells as tc

pytestmark = pytest.mark.gpu

KNOBS = ("HG_FIN_TARGET", "HG_NO_BUCKET_FINALIZE", "HG_CHUNK_TILES", "HG_MAX_CHUNKS", "HG_CHUNK_WEIGHTS", "HG_NO_EARLY_FINALIZE", "HG_JOINER", "HG_JOINER_AHEAD",
         "HG_STREAM_WGS_PER_CU", "HG_HIT_LIMIT", "HG_CAND_LIMIT")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    return torch


@pytest.fixture(scope="module")
def db():
    from hypergrep_amd import device

    return device.Database([tc.MARKER.decode()], flags=[tc.FLAGS], ids=[tc.MARKER_ID])


_placed = {}


def place(torch, key):
    """A text on the device (one at a time: the cells are ordered by text)."""
    if key not in _placed:
        _placed.clear()
        data = tc.text_array(key)
        buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
        buf[:len(data)] = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        _placed[key] = buf
    return _placed[key]


def compare(sc, stats, rows, n_lines, what):
    got = sc.hits_array()
    assert stats.n_lines == n_lines, (what, stats.n_lines, n_lines)
    assert stats.n_hits == len(rows) == len(got), (what, stats.n_hits, len(rows))
    bad = np.flatnonzero((got != rows).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(rows)} hits differ, the first at {bad[0]}: got {got[bad[0]].tolist()}, want {rows[bad[0]].tolist()} (line, id, to, start, len)"


CELLS = sorted(tc.CELLS, key=lambda c: (c.key.geo.__name__, c.key.bs1s, c.key.straddle))


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_tile_cell(torch_cuda, db, cell, monkeypatch):
    from hypergrep_amd import device

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in cell.env.items():
        monkeypatch.setenv(k, v)  # (read when the scanner is created)
    sc = device.Scanner(db, 0)
    buf = place(torch_cuda, cell.key)
    rows, n_lines = tc.cell_reference(cell)
    t0 = time.perf_counter()
    stats = sc.scan(buf.data_ptr(), cell.nbytes, buffer_size=cell.buffer_size, line_base=cell.line_base)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"{cell.name}: reports {stats.n_hits}, candidates {stats.n_candidates}, reruns {stats.reruns}, stream launches {stats.stream_launches}, "
          f"joiner launches {stats.joiner_launches}, lines {stats.n_lines}, {ms:.1f} ms")
    compare(sc, stats, rows, n_lines, cell.name)
    if "stream_launches_min" in cell.claim:
        assert stats.stream_launches >= cell.claim["stream_launches_min"]
    if "HG_HIT_LIMIT" in cell.env:  # one chunk a segment: as many stream launches as segments
        assert stats.stream_launches == tc.planned_segments(cell)
    elif "HG_CHUNK_TILES" not in cell.env:
        assert stats.stream_launches == 1


def test_large_cell_two_spine_rounds(torch_cuda, db):
    """4 GiB + 16 MiB + 5 tiles + 123 bytes in ONE chunk: 258 tile-scan blocks, so the spine runs a second round with a carried
    state.  The text is made on the device (filler, newlines and markers written by index); the reference is the closed form
    over the planted positions.  Lines of about 1 MiB: the default scan buffer cuts every one into pieces."""
    from hypergrep_amd import device

    torch = torch_cuda
    nl, tiles = tc.big_geometry()
    markers = tc.big_markers(nl, tiles)
    text = torch.full((tc.BIG_BYTES + 64,), ord("."), dtype=torch.uint8, device="cuda:0")
    text[tc.BIG_BYTES:] = 0
    text[torch.from_numpy(nl).cuda()] = 10
    at = torch.from_numpy(markers).cuda()
    for j, c in enumerate(tc.MARKER):
        text[at + j] = c
    torch.cuda.synchronize()
    rows, n_lines = tc.reference(nl, tc.BIG_BYTES, tc.DEFAULT_BS - 1, 0, markers)
    assert len(rows) > 2000 and (rows[:, 0] > 0).any()
    seen_blocks = set(((rows[:, 3] + rows[:, 2]) // (tc.TILE * tc.BLOCK)).tolist())
    assert {0, 1, 255, 256, 257} <= seen_blocks
    sc = device.Scanner(db, 0)
    stats = sc.scan(text.data_ptr(), tc.BIG_BYTES)
    print(f"large cell: reports {stats.n_hits}, candidates {stats.n_candidates}, reruns {stats.reruns}, stream launches {stats.stream_launches}, lines {stats.n_lines}, {stats.ms_total:.1f} ms")
    assert stats.stream_launches == 1
    compare(sc, stats, rows, n_lines, "large cell")
