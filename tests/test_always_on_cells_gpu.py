"""GPU parity of every always-on cell (always_on_cells.py) against the oracle with the piece geometry of invert_ref.pieces
(run with `-m gpu`): always_on_word<CTX, NT> in its lean steps and in ao_exact_dword, the groups, always_on_word2,
always_on_segment<2, false> and the scalar hg_always_on_kernel, each on texts that plant every segment, lead-in and break
geometry (the match end against the 256-byte lane segments and the 64-byte blocks; splits across lanes and tiles; line starts
carried into a tile; the ends of the text; the NUL rules; forced breaks at nine buffer sizes around the 512 switch; two
matches on one line; long lines; a note list that overflows).  All five columns (line, id, to, start, len) and n_lines are
compared, as multisets, with distinct ids and with every expression of the cell on one id.  That the cells are placed as
named, that the reference agrees with a Python `re` brute force and that every class is planted, in lean and in careful tiles:
test_always_on_cells.py."""
from __future__ import annotations

import numpy as np
import pytest

import always_on_cells as ac

pytestmark = pytest.mark.gpu

QUIET_BYTES = 17 << 20  # in front of the text of the chunked scan: past the first 16 MiB pipeline chunk


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    return torch


def _device_text(torch, data: bytes):
    buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda:0")  # (32 bytes of slack past the end)
    buf[: len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf


@pytest.mark.parametrize("cell", ac.CELLS, ids=lambda c: c.name)
def test_always_on_cell(torch_cuda, cell):
    from hypergrep_amd import device

    texts = ac.cell_texts(cell.name)
    bufs = [_device_text(torch_cuda, t.data) for t in texts]
    torch_cuda.cuda.synchronize()
    bad, tags, total = [], set(), 0
    for shared in (False, True):
        db = device.Database(cell.patterns, flags=cell.flags, ids=cell.ids(shared))
        info = db.info()
        assert info["n_always_on"] == cell.n_always_on and info["n_literal_anchored"] == cell.n_literal and info["max_state_words"] == cell.max_nw, info
        scanner = device.Scanner(db, 0)
        for ti, (text, buf) in enumerate(zip(texts, bufs)):
            dense = text.label == "dense"
            if dense:  # a scanner of its own: the note lists still have their first size
                scanner = device.Scanner(db, 0)
            for bs in text.sizes:
                want, nlines, _ = ac.cell_reference(cell.name, ti, bs, shared)
                stats = scanner.scan(buf.data_ptr(), len(text.data), buffer_size=bs)
                got = ac.sort_hits(scanner.hits_array())  # (sorted rows compared one to one: a duplicate fails)
                total += len(want)
                what = f"{cell.name} {text.label} buffer_size {bs} {'one id' if shared else 'distinct ids'}"
                if stats.n_lines != nlines:
                    bad.append(f"{what}: {stats.n_lines} lines, want {nlines}")
                if got.shape != want.shape or not (got == want).all():
                    bad.append(f"{what}: {ac.diff_report(text, got, want)}")
                    tags |= ac.diff_tags(text, got, want)
                if dense and stats.reruns < 1:  # more notes than a workgroup's list holds: the pass is repeated with larger lists
                    bad.append(f"{what}: {len(want)} reports in five tiles and no repeated pass (reruns {stats.reruns})")
    assert total >= 600, total  # (300 per id mode: test_always_on_cells.py::test_floors)
    if bad:
        pytest.fail(f"{cell.name}: {len(bad)} scans differ from the reference; geometry tags: {sorted(tags)}\n" + "\n".join(bad[:12]))


def test_mixed_cell_in_the_second_pipeline_chunk(torch_cuda, monkeypatch):
    """The mixed cell's first text behind 17 MiB of quiet lines, in pipeline chunks of 1024 tiles: its tiles belong to the
    second chunk, whose always-on pass runs with the tile bases and note lists of a chunk that is not the first."""
    from hypergrep_amd import device

    cell = ac.BY_NAME["mixed_shared_ids"]
    text = ac.cell_texts(cell.name)[0]
    assert text.label == "seg" and any(c.tag == "seg/literal_anchored" for c in text.cases)
    rng = np.random.default_rng(7)
    quiet = np.frombuffer(ac.FILLER, dtype=np.uint8)[rng.integers(0, len(ac.FILLER), size=QUIET_BYTES)]
    quiet[rng.random(QUIET_BYTES) < 1 / 100] = 10
    quiet[-1] = 10
    qlines = int((quiet == 10).sum())
    data = quiet.tobytes() + text.data
    buf = _device_text(torch_cuda, data)
    torch_cuda.cuda.synchronize()
    monkeypatch.setenv("HG_CHUNK_TILES", "1024")  # (env knobs are read when the scanner is created)
    for shared in (True, False):
        want, nlines, _ = ac.cell_reference(cell.name, 0, ac.DEFAULT_BS, shared)
        want = want + np.array([qlines, 0, 0, QUIET_BYTES, 0], dtype=np.uint64)  # shifted by the quiet bytes and lines, never recomputed over them
        scanner = device.Scanner(device.Database(cell.patterns, flags=cell.flags, ids=cell.ids(shared)), 0)
        stats = scanner.scan(buf.data_ptr(), len(data))
        got = ac.sort_hits(scanner.hits_array())
        assert stats.stream_launches >= 2 and stats.n_lines == qlines + nlines, (stats.stream_launches, stats.n_lines, qlines + nlines)
        if got.shape != want.shape or not (got == want).all():
            shifted = ac.Text(text.label, text.data, text.sizes, [ac.Case(c.tag, c.lo + QUIET_BYTES, c.hi + QUIET_BYTES, c.end + QUIET_BYTES, c.expr, c.k) for c in text.cases])
            pytest.fail(f"{cell.name} behind {QUIET_BYTES} quiet bytes, {'one id' if shared else 'distinct ids'}: {ac.diff_report(shifted, got, want)}")
        assert len(want) >= 100
