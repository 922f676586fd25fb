"""GPU parity of every confirm cell (confirm_cells.py) against the oracle with the piece geometry of invert_ref.pieces (run
with `-m gpu`): confirm_literal, confirm_simple, confirm_ctx<1> / <2>, the scalar hg_confirm and the huge-automaton kernel,
each on texts that plant every window and piece geometry (chunk alignment of the occurrence, the window start and the match
end; line starts against tile edges; the ends of the text; the NUL rules; forced breaks at six buffer sizes; several
occurrences per line).  All five columns (line, id, to, start, len) and n_lines are compared, with distinct ids and with
every expression of the cell on one id.  That the cells are placed as named, that the reference agrees with a Python `re`
brute force and that every class is planted: test_confirm_cells.py."""
from __future__ import annotations

import numpy as np
import pytest

import confirm_cells as cc

pytestmark = pytest.mark.gpu

QUIET_BYTES = 17 << 20  # in front of the text of the chunked scan: past the first 16 MiB pipeline chunk


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    return torch


def _device_text(torch, data: bytes):
    buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda:0")  # (slack past the end: the tail chunk's reads)
    buf[: len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf


@pytest.mark.parametrize("cell", cc.CELLS, ids=lambda c: c.name)
def test_confirm_cell(torch_cuda, cell):
    from hypergrep_amd import device

    leads = cc.compiled_leads(cell.name)
    texts = cc.cell_texts(cell.name, leads)
    bufs = [_device_text(torch_cuda, t.data) for t in texts]
    torch_cuda.cuda.synchronize()
    bad, tags, total = [], set(), 0
    for shared in (False, True):
        db = device.Database(cell.patterns, flags=cell.flags, ids=cell.ids(shared))
        info = db.info()
        assert info["n_literal_anchored"] == len(cell.exprs) and info["n_always_on"] == 0, info
        scanner = device.Scanner(db, 0)
        for ti, (text, buf) in enumerate(zip(texts, bufs)):
            for bs in text.sizes:
                want, nlines, _ = cc.cell_reference(cell.name, leads, ti, bs, shared)
                stats = scanner.scan(buf.data_ptr(), len(text.data), buffer_size=bs)
                got = cc.sort_hits(scanner.hits_array())
                total += len(want)
                what = f"{cell.name} {text.label} buffer_size {bs} {'one id' if shared else 'distinct ids'}"
                if stats.n_lines != nlines:
                    bad.append(f"{what}: {stats.n_lines} lines, want {nlines}")
                if got.shape != want.shape or not (got == want).all():
                    bad.append(f"{what}: {cc.diff_report(text, got, want)}")
                    tags |= cc.diff_tags(text, got, want)
    assert total >= 600, total  # (300 per id mode: test_confirm_cells.py::test_floors)
    if bad:
        pytest.fail(f"{cell.name}: {len(bad)} scans differ from the reference; geometry tags: {sorted(tags)}\n" + "\n".join(bad[:12]))


def test_mixed_cell_in_the_second_pipeline_chunk(torch_cuda, monkeypatch):
    """The mixed cell's main text behind 17 MiB of lines that hold no literal, in pipeline chunks of 1024 tiles: its tiles
    belong to the second chunk, whose side passes run beside a stream launch with carried tile-scan state and the second
    candidate segment."""
    from hypergrep_amd import device

    cell = cc.BY_NAME["mixed_shared_ids"]
    leads = cc.compiled_leads(cell.name)
    text = cc.cell_texts(cell.name, leads)[0]
    assert text.label == "main"
    rng = np.random.default_rng(7)
    quiet = np.frombuffer(cc.FILLER, dtype=np.uint8)[rng.integers(0, len(cc.FILLER), size=QUIET_BYTES)]
    quiet[rng.random(QUIET_BYTES) < 1 / 100] = 10
    quiet[-1] = 10
    qlines = int((quiet == 10).sum())
    data = quiet.tobytes() + text.data
    buf = _device_text(torch_cuda, data)
    torch_cuda.cuda.synchronize()
    monkeypatch.setenv("HG_CHUNK_TILES", "1024")  # (env knobs are read when the scanner is created)
    for shared in (True, False):
        want, nlines, _ = cc.cell_reference(cell.name, leads, 0, cc.DEFAULT_BS, shared)
        want = want + np.array([qlines, 0, 0, QUIET_BYTES, 0], dtype=np.uint64)
        scanner = device.Scanner(device.Database(cell.patterns, flags=cell.flags, ids=cell.ids(shared)), 0)
        stats = scanner.scan(buf.data_ptr(), len(data))
        got = cc.sort_hits(scanner.hits_array())
        assert stats.stream_launches >= 2 and stats.n_lines == qlines + nlines, (stats.stream_launches, stats.n_lines, qlines + nlines)
        if got.shape != want.shape or not (got == want).all():
            shifted = cc.Text(text.label, text.data, text.sizes, [cc.Case(c.tag, c.lo + QUIET_BYTES, c.hi + QUIET_BYTES, c.fs + QUIET_BYTES, c.expr, c.line + QUIET_BYTES) for c in text.cases])
            pytest.fail(f"{cell.name} behind {QUIET_BYTES} quiet bytes, {'one id' if shared else 'distinct ids'}: {cc.diff_report(shifted, got, want)}")
        assert len(want) >= 200
