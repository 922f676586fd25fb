"""The tile-scan cells (tests/tile_cells.py) without a GPU: the reference against an independent splitter and bytes.find, the
classes the suite is written for against the cells' geometry, and the host replay of the three kernels' decomposition
(tests/native/tilesim.cpp: hg_tile_combine under a Hillis-Steele scan, block aggregates, spine rounds, apply) against the
sequential walk and against the reference, on every cell's summaries and on synthetic ones of 600 blocks."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import finalize_cells as fc
import tile_cells as tc
import tilesim_py as ts

TILE, BLOCK = tc.TILE, tc.BLOCK


@pytest.fixture(scope="module")
def texts():
    cache = {}

    def get(key):
        if key not in cache:
            cache.clear()  # (one text at a time: they are tens of MiB)
            cache[key] = tc.text_array(key)
        return cache[key]
    return get


def by_text(cells):
    return sorted(cells, key=lambda c: (c.key.geo.__name__, c.key.bs1s, c.key.straddle))


def test_reference_against_a_splitter_and_find(texts):
    """reference() (closed form over newline positions) against tests/finalize_cells.py's reference (a loop that cuts pieces as
    gzgets does, bytes.find per expression) on every cell's text: all five columns and the piece count."""
    expr = [fc.Expr(tc.MARKER, tc.MARKER_ID, False)]
    for cell in by_text(tc.CELLS):
        data = texts(cell.key)[:cell.nbytes].tobytes()
        want = fc.reference(data, expr, cell.buffer_size, cell.line_base)
        rows, n_lines = tc.cell_reference(cell)
        assert n_lines == len(want.starts), cell.name
        assert [tuple(int(v) for v in r) for r in rows] == want.records, cell.name
        assert len(rows) >= 1, cell.name


def test_marker_is_a_tier_0_literal():
    import hgsim_py

    db = hgsim_py.Db([tc.MARKER.decode()], flags=[tc.FLAGS], ids=[tc.MARKER_ID])
    assert db.ok() and db.tier(0) == 0 and db.info()["nslow"] == 0


def test_every_class_occurs_in_some_cell():
    seen = set()
    for cell in tc.CELLS:
        seen |= tc.tags(cell)
    assert not (tc.REQUIRED - seen), sorted(tc.REQUIRED - seen)
    # the segmented cells: the engine's rule (more raw reports than HG_HIT_LIMIT: twice as many segments) on the reference's counts
    planned = [tc.planned_segments(c) for c in tc.CELLS if "HG_HIT_LIMIT" in c.env]
    assert planned == [2, 4]
    # every tile's state is seen alone: a marker reports in the tile's carry-in line exactly where that line has room for one inside
    # the tile (its first newline not in the tile's first 8 bytes, the text not shorter); the only other tiles without one are those
    # where a marker was planted across a forced break instead.  A tile without such room is seen through the marker behind its
    # first newline, unless it is a last tile shorter than a marker.
    for cell in tc.CELLS:
        nl, _ = tc.geometry(cell.key.geo)
        nl = nl[nl < cell.nbytes]
        s = tc.summaries(nl, cell.nbytes, cell.bs1)
        rows, _ = tc.cell_reference(cell)
        x = (rows[:, 3] + rows[:, 2] - tc.M).astype(np.int64)  # where the reporting markers stand
        t = x // TILE
        first = np.where(s[:, 0] > 0, s[:, 1].astype(np.int64), TILE)
        room = np.minimum(first, np.minimum(TILE, cell.nbytes - np.arange(len(s)) * TILE))  # bytes of the carry-in line inside the tile
        seen = np.zeros(len(s), dtype=bool)
        seen[t[(x - t * TILE) + tc.M <= room[t]]] = True
        across = tc.straddlers(nl, cell.nbytes, cell.bs1) if cell.key.straddle == cell.bs1 else np.array([], dtype=np.int64)
        allowed = set((across // TILE).tolist()) | set(((across + tc.M) // TILE).tolist())
        wrong = [int(k) for k in np.flatnonzero(seen != (room >= tc.M)) if int(k) not in allowed]
        assert not wrong, (cell.name, wrong[:5])
        any_marker = np.zeros(len(s), dtype=bool)
        any_marker[t] = True
        blind = [int(k) for k in np.flatnonzero(~any_marker) if int(k) not in allowed]
        assert all(k == len(s) - 1 and cell.nbytes - k * TILE < tc.M for k in blind), (cell.name, blind[:5])


def test_markers_keep_off_forced_breaks_but_for_the_planted_ones():
    for cell in tc.CELLS:
        x = tc.text_markers(cell.key)
        x = x[x + tc.M <= cell.nbytes]
        rows, _ = tc.cell_reference(cell)
        silent = len(x) - len(rows)
        if cell.key.straddle == cell.bs1:
            assert 1 <= silent <= 3, (cell.name, silent)
        else:
            assert silent == 0, (cell.name, silent)


def test_summaries_against_the_text(texts):
    """summaries() (from newline positions) against a count over the bytes themselves."""
    for cell in by_text([c for c in tc.CELLS if c.name in ("size-9+16383", "small-lines-1000", "small-lines-8", "small-lines-16383", "size-1025+1")]):
        nl, _ = tc.geometry(cell.key.geo)
        s = tc.summaries(nl, cell.nbytes, cell.bs1)
        data = texts(cell.key)[:cell.nbytes]
        pad = np.zeros(len(s) * TILE, dtype=np.uint8)
        pad[:cell.nbytes] = data
        is_nl = pad.reshape(-1, TILE) == 10
        assert (s[:, 0] == is_nl.sum(axis=1)).all()
        has = s[:, 0] > 0
        assert (s[has, 1] == is_nl[has].argmax(axis=1)).all() and (s[has, 2] == TILE - 1 - is_nl[has, ::-1].argmax(axis=1)).all()
        # inner: the pieces of the lines between the first and the last newline, by the splitter
        raw = data.tobytes()
        for t in np.flatnonzero(s[:, 0] >= 2)[:40]:
            a, b = int(t) * TILE + int(s[t, 1]) + 1, int(t) * TILE + int(s[t, 2]) + 1
            assert s[t, 3] == len(fc.split_pieces(raw[a:b], cell.buffer_size)[0]), (cell.name, t)


def replay(nl, nbytes, bs1, line_base, ranges, what):
    """The replay over `ranges` (tile ranges one after the other, the state chained) against the walk and the reference."""
    s = tc.summaries(nl, nbytes, bs1)
    n = len(s)
    want_cs, want_L = tc.tile_states(nl, nbytes, bs1, line_base)
    walked = np.zeros((n, 2), dtype=np.uint64)
    end_walk = ts.walk(s, 0, n, bs1, (0, line_base), walked)
    assert (walked[:, 0] == want_cs.astype(np.uint64)).all() and (walked[:, 1] == want_L.astype(np.uint64)).all(), f"{what}: the walk against the reference"
    got = np.zeros((n, 2), dtype=np.uint64)
    state, blocks = (0, line_base), 0
    for a, b in ranges:
        state, k = ts.scan(s, a, b, bs1, state, got)
        blocks = max(blocks, k)
    bad = np.flatnonzero((got != walked).any(axis=1))
    assert len(bad) == 0, f"{what}: tile {bad[:5]}: replay {got[bad[:5]].tolist()}, walk {walked[bad[:5]].tolist()}"
    assert state == end_walk, what
    p = tc.pieces(nl, nbytes, bs1)
    ends_with_newline = len(nl[nl < nbytes]) and nl[nl < nbytes][-1] == nbytes - 1
    assert state == ((nbytes, line_base + p.total) if ends_with_newline else (int(p.starts[-1]), line_base + int(p.first[-1]))), what
    return s, walked, blocks


def test_replay_on_every_cell():
    assert ts.sizes() == {"sizeof_sum": 16, "sizeof_base": 16, "sizeof_elem": 32, "tile_bytes": TILE}
    done = set()
    for cell in tc.CELLS:
        ident = (cell.key.geo, cell.nbytes, cell.bs1, cell.line_base, tuple(sorted(cell.env.items())))
        if ident in done:
            continue
        done.add(ident)
        nl, _ = tc.geometry(cell.key.geo)
        ntiles = (cell.nbytes + TILE - 1) // TILE
        s, walked, _ = replay(nl, cell.nbytes, cell.bs1, cell.line_base, tc.chunk_cuts(cell), cell.name)
        if "HG_HIT_LIMIT" in cell.env:  # a segment's pass starts from the state the pass before it left at its first tile
            k = tc.planned_segments(cell)
            got = np.zeros_like(walked)
            for lo, hi, _own in tc.segment_ranges(cell, k):
                ts.scan(s, lo, hi, cell.bs1, (int(walked[lo, 0]), int(walked[lo, 1])), got)
                assert (got[lo:hi] == walked[lo:hi]).all(), (cell.name, lo)
        if ntiles in (9, 1025, 2050):  # ranges that begin on any tile, and hg_tile_combine in other tree orders
            got = np.zeros_like(walked)
            for lo in (1, 2, 3, 5, 7):
                if lo < ntiles:
                    ts.scan(s, lo, ntiles, cell.bs1, (int(walked[lo, 0]), int(walked[lo, 1])), got)
                    assert (got[lo:] == walked[lo:]).all(), (cell.name, lo)
            end = ts.walk(s, 0, ntiles, cell.bs1, (0, cell.line_base), np.zeros_like(walked))
            for split in (0, 1, 2, 77):
                assert ts.tree(s, 0, ntiles, cell.bs1, split, (0, cell.line_base)) == end, (cell.name, split)


def synthetic(nblocks: int, seed: int):
    """Newline positions of a text of nblocks tile-scan blocks that nobody writes out: per tile none, one, two or three
    newlines; block 3, and blocks 200 to 519 (the spine's whole second round and parts of the first and the third), without any."""
    rng = np.random.default_rng(seed)
    ntiles = nblocks * BLOCK
    count = rng.choice([0, 0, 1, 1, 2, 3], size=ntiles)
    count[3 * BLOCK:4 * BLOCK] = 0
    count[200 * BLOCK:520 * BLOCK] = 0
    first = rng.integers(0, 5000, size=ntiles)
    first[rng.random(ntiles) < 0.2] = 0
    last = rng.integers(9000, TILE, size=ntiles)
    last[rng.random(ntiles) < 0.2] = TILE - 1
    mid = rng.integers(5000, 9000, size=ntiles)
    t0 = np.arange(ntiles, dtype=np.int64) * TILE
    nl = np.concatenate([(t0 + first)[count >= 1], (t0 + last)[count >= 2], (t0 + mid)[count >= 3]])
    return np.sort(nl), ntiles * TILE


@pytest.mark.parametrize("bs1", [262139, 16384, 40000, 1000])
def test_replay_on_600_synthetic_blocks(bs1):
    nl, nbytes = synthetic(600, 31)
    _, _, blocks = replay(nl, nbytes, bs1, 2**33 + 5, [(0, nbytes // TILE)], f"600 blocks, bs1 {bs1}")
    assert blocks == 600  # three rounds of the spine
    # and as chunks of 258 blocks (two rounds each, the state handed on)
    step = 258 * BLOCK
    replay(nl, nbytes, bs1, 0, [(a, min(a + step, nbytes // TILE)) for a in range(0, nbytes // TILE, step)], f"600 blocks in chunks, bs1 {bs1}")


def test_replay_on_the_large_cell():
    """The large GPU cell's geometry: 258 blocks, two rounds of the spine."""
    nl, _tiles = tc.big_geometry()
    _, _, blocks = replay(nl, tc.BIG_BYTES, tc.DEFAULT_BS - 1, 0, [(0, tc.BIG_TILES + 1)], "large cell")
    assert blocks == 258
    assert (tc.pieces(nl, tc.BIG_BYTES, tc.DEFAULT_BS - 1).lens > tc.DEFAULT_BS - 1).sum() > 3000  # the default scan buffer forces breaks


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (tilesim.cpp's main) under AddressSanitizer and UBSan: seeded summaries of up to 600
    blocks, every scan buffer of the cells, ranges that begin on any tile; the arrays are heap blocks of exactly their size."""
    exe = str(tmp_path / "tilesim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DTILESIM_MAIN", "-o", exe, ts.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout
