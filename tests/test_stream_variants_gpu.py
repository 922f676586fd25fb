"""GPU parity of every stream-pass cell (stream_cells.py) against the exact literal reference (run with `-m gpu`).

Each stream cell scans a text of its own literals built to drive its instantiation through the queue, the newline geometry of
a tile, every chunk alignment, near misses and (caseless cells) case variants and fold look-alikes, then prefixes of it that
end inside a partial last tile.  Every text is scanned twice: alone with the defaults, and behind six
copies of the cell's text in 16 MiB pipeline chunks, so that it lies in the second of several stream launches.  The joiner cells repeat their block to 192 MiB
in 64 MiB pipeline chunks with the joiner forced on and put in front of each chunk's stream launch."""
from __future__ import annotations

import random

import numpy as np
import pytest

import stream_cells as sc

pytestmark = pytest.mark.gpu

SIZE = 3 << 20
PREFIX_TILES = 40  # the truncated texts: the queue, geometry, alignment and near-miss sections and a few boundary tiles
JOIN_BYTES = 192 << 20
JOIN_CHUNK_TILES = 4096  # 64 MiB
REPS = 6  # blocks in front of a text in its second scan: past the first 16 MiB pipeline chunk


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    return torch


def _device_text(torch, data: bytes):
    buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda:0")  # (slack past the end: the tail chunk's reads)
    if data:
        buf[: len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return buf


def _database(cell):
    from hypergrep_amd import device

    lits, caseless = sc.literal_set(cell)
    ids = list(range(len(lits)))
    db = device.Database(sc.patterns_of(lits), flags=sc.flags_of(caseless), ids=ids)
    info = db.info()
    assert info["byte_windows"] == cell.dense and (info["fold_mask"] != 0) == cell.fold, info
    assert info["n_always_on"] == 0, info
    return db, lits, caseless, ids


def _scan(db, buf, nbytes):
    from hypergrep_amd import device

    scanner = device.Scanner(db, 0)  # (env knobs are read when the scanner is created)
    stats = scanner.scan(buf.data_ptr(), nbytes)
    return sc.sort_hits(scanner.hits_array()), stats


def _assert_hits(got, want, what):
    if got.shape == want.shape and (got == want).all():
        return
    rows = lambda a: np.ascontiguousarray(a).view([("", np.uint64)] * 5).ravel()  # noqa: E731
    # (line, id, to, line_off, line_len): the byte offset where a hit ends, and its tile
    where = lambda h: f"{tuple(int(x) for x in h)} tile {(int(h[3]) + int(h[2])) // sc.TILE}"  # noqa: E731
    missing, extra = np.setdiff1d(rows(want), rows(got))[:5], np.setdiff1d(rows(got), rows(want))[:5]
    pytest.fail(f"{what}: {len(got)} hits, want {len(want)}; missing {[where(h) for h in missing]}; extra {[where(h) for h in extra]}")


def _repeated(bwant, blines, blen, reps):
    """The hits of a block that ends in a newline, repeated: block i's lines shifted by i * blines, line offsets by i * blen."""
    shift = np.zeros((reps, 1, 5), dtype=np.uint64)
    shift[:, 0, 0] = np.arange(reps, dtype=np.uint64) * np.uint64(blines)
    shift[:, 0, 3] = np.arange(reps, dtype=np.uint64) * np.uint64(blen)
    return (bwant[None, :, :] + shift).reshape(-1, 5)


def _device_repeated(torch, block: bytes, reps: int, tail: bytes = b""):
    n = reps * len(block) + len(tail)
    buf = torch.zeros(n + 32, dtype=torch.uint8, device="cuda:0")
    dev_block = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
    buf[: reps * len(block)].view(reps, len(block)).copy_(dev_block.expand(reps, len(block)))
    if tail:
        buf[reps * len(block):n] = torch.frombuffer(bytearray(tail), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return buf, n


@pytest.mark.parametrize("cell", sc.STREAM_CELLS, ids=lambda c: c.name)
def test_stream_cell(torch_cuda, cell, monkeypatch):
    db, lits, caseless, ids = _database(cell)
    text = sc.cell_text(cell, lits, caseless, SIZE, seed=2)
    rng = random.Random(cell.name)
    texts = [("full", text)] + [(f"tail{r}", sc.truncated(text, lits, PREFIX_TILES * sc.TILE + r, rng)) for r in sc.residues(cell)]
    # the text again, ending in a newline, as the block that goes in front of each text in its second scan
    block = text[:-1] + b"\n"
    bwant, blines = sc.reference_hits(block, lits, caseless, ids), sc.line_table(block)[1]
    for label, data in texts:
        want = sc.reference_hits(data, lits, caseless, ids)
        nl, nlines = sc.line_table(data)
        assert np.diff(np.concatenate([[-1], nl, [len(data)]]).astype(np.int64)).max() < 65536  # (lines, not pieces)
        assert len(want) >= (25000 if label == "full" else 20000), (label, len(want))
        buf = _device_text(torch_cuda, data)
        got, stats = _scan(db, buf, len(data))
        del buf
        assert stats.n_lines == nlines, (label, stats.n_lines, nlines)
        _assert_hits(got, want, f"{cell.name} {label}")
        # behind six blocks, in 16 MiB pipeline chunks with one stream workgroup per CU: two stream launches and the text
        # (its partial last tile) in the second; each wave streams several tiles, its queue carries entries from one tile
        # into the next, and each launch ends with a drain
        # (not a smaller chunk: the engine rounds HG_CHUNK_TILES down to whole tile-scan blocks of TS_BLOCK_TILES = 1024
        # tiles and ignores a value below one, hg_engine.hip run_once)
        buf, n = _device_repeated(torch_cuda, block, REPS, data)
        monkeypatch.setenv("HG_CHUNK_TILES", "1024")
        monkeypatch.setenv("HG_STREAM_WGS_PER_CU", "1")
        got, multi = _scan(db, buf, n)
        monkeypatch.delenv("HG_CHUNK_TILES")
        monkeypatch.delenv("HG_STREAM_WGS_PER_CU")
        del buf
        long_want = np.concatenate([_repeated(bwant, blines, len(block), REPS), want + np.array([REPS * blines, 0, 0, REPS * len(block), 0], dtype=np.uint64)])
        assert multi.stream_launches >= 2 and multi.n_lines == REPS * blines + nlines, (label, multi.stream_launches, multi.n_lines)
        _assert_hits(got, long_want, f"{cell.name} {label} behind {REPS} blocks")


@pytest.mark.parametrize("cell", sc.JOIN_CELLS, ids=lambda c: c.name)
def test_joiner_cell(torch_cuda, cell, monkeypatch):
    """A 16 MiB block of the cell (ending in a newline) repeated to 192 MiB: three 64 MiB pipeline chunks and a joiner launch
    for each chunk but the first.  HG_JOINER_AHEAD puts the joiner in front of its chunk's stream launch, so that it streams
    every tile of those chunks through hg_stream_join_kernel.  (In its normal place, behind the previous chunk's side
    passes, it finds the chunk's cursor used up at these sizes: the stream launch's first draws alone hand out 4096 tiles.)"""
    db, lits, caseless, ids = _database(cell)
    # 1 MiB of the cell's text and 15 MiB of lines that hold no literal: fewer hits to compare
    rng = np.random.default_rng(5)
    quiet = np.frombuffer(b"-=+.,:;!", dtype=np.uint8)[rng.integers(0, 8, size=15 << 20)]
    quiet[rng.random(15 << 20) < 1 / 100] = 10
    block = sc.cell_text(cell, lits, caseless, 1 << 20, seed=5) + quiet.tobytes()[:-1] + b"\n"
    reps = -(-JOIN_BYTES // len(block))
    bwant = sc.reference_hits(block, lits, caseless, ids)
    blines = sc.line_table(block)[1]
    assert len(bwant) >= 15000
    want = _repeated(bwant, blines, len(block), reps)
    buf, n = _device_repeated(torch_cuda, block, reps)
    monkeypatch.setenv("HG_JOINER", "2")
    monkeypatch.setenv("HG_JOINER_AHEAD", "1")
    monkeypatch.setenv("HG_CHUNK_TILES", str(JOIN_CHUNK_TILES))
    got, stats = _scan(db, buf, n)
    assert stats.n_lines == reps * blines
    ntiles = -(-n // sc.TILE)
    assert stats.stream_launches == 3 and stats.joiner_launches == 2, stats
    assert stats.joiner_tiles == ntiles - JOIN_CHUNK_TILES, (stats.joiner_tiles, ntiles)  # every tile of chunks 1 and 2
    _assert_hits(got, want, f"{cell.name} x{reps}")
