"""GPU parity of every huge-automaton cell (huge_cells.py) against the oracle (run with `-m gpu`): huge_run_reg<1>, <2>, <4>,
huge_run on staged tables and on tables in L2, under the always-on kernel, the confirm kernel and block mode.  The buffer API
scans the cell's texts at their buffer sizes, with distinct ids and with every expression on one id; all five columns (line,
id, to, start, len) and n_lines are compared as sorted rows, one to one, so a duplicate fails.  Block mode goes through Face A
(hs_scan) on the cell's blocks, against the oracle's libhs.  A failure prints the geometry tags of the differing rows.  That the
cells are placed as named, that every class is planted and that the reference judges every planted case as tagged:
test_huge_cells.py.  The host mirror covers huge_run alone: huge_run_reg (the carry between lanes and slabs, the exception
detour, the staged accept and entry rows) is held by this comparison."""
from __future__ import annotations

import pytest

import huge_cells as hc

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("cell", hc.CELLS, ids=lambda c: c.name)
def test_huge_cell(torch_cuda, cell):
    from hypergrep_amd import device

    texts = hc.cell_texts(cell.name)
    bufs = [_device_text(torch_cuda, t.data) for t in texts]
    torch_cuda.cuda.synchronize()
    bad, tags, total = [], set(), 0
    for shared in (False, True):
        db = device.Database(cell.patterns, flags=cell.flags, ids=cell.ids(shared))
        scanner = device.Scanner(db, 0)
        for ti, (text, buf) in enumerate(zip(texts, bufs)):
            for bs in text.sizes:
                want, nlines, _ = hc.cell_reference(cell.name, ti, bs, shared)
                stats = scanner.scan(buf.data_ptr(), len(text.data), buffer_size=bs)
                got = hc.sort_hits(scanner.hits_array())  # (sorted rows compared one to one: a duplicate fails)
                total += len(want)
                what = f"{cell.name} {text.label} buffer_size {bs} {'one id' if shared else 'distinct ids'}"
                if stats.n_lines != nlines:
                    bad.append(f"{what}: {stats.n_lines} lines, want {nlines}")
                if got.shape != want.shape or not (got == want).all():
                    bad.append(f"{what}: {hc.diff_report(text, got, want)}")
                    tags |= hc.diff_tags(text, got, want)
    print(f"{cell.name}: {total} reports of the reference")
    assert total >= cell.floor > 0, (total, cell.floor)  # a reference that silently loses cases fails here (profiles/huge_cells.txt)
    if bad:
        pytest.fail(f"{cell.name}: {len(bad)} scans differ from the reference; geometry tags: {sorted(tags)}\n" + "\n".join(bad[:12]))


@pytest.mark.parametrize("cell", hc.CELLS, ids=lambda c: c.name)
def test_huge_cell_block_mode(torch_cuda, cell):
    """hs_scan: the whole block is one scan unit of hg_block_huge_kernel, for every routine label."""
    import test_gpu_parity as tg  # (the libhs driver of the Face A tests)
    from hypergrep_amd import utils

    blocks = hc.cell_blocks(cell.name)
    want = hc.block_reference(cell.name)
    got = tg._hs_events(utils._get_hyperscanner_lib(), cell.patterns, cell.flags, cell.ids(False), [blk for _, blk in blocks])  # pylint: disable=protected-access
    assert sum(len(w) for w in want) >= 5 and blocks[-1][0] == "match_ends_the_block" and any(to == len(blocks[-1][1]) for _, to in want[-1])
    bad = []
    for (label, _), g, w in zip(blocks, got, want):
        if sorted(g) != sorted(w):
            names = lambda evs: sorted({f"{cell.exprs[i].pattern[:24]}@{to}" for i, to in evs})[:6]  # noqa: E731
            bad.append(f"{cell.name} block {label}: {len(g)} events, want {len(w)}; missing {names(set(w) - set(g))}; extra {names(set(g) - set(w))}")
    assert not bad, "\n".join(bad)
    if cell.name == "cf_restage":  # the expression whose literal is absent reports nothing, the others report as before
        assert not any(i == 2 for i, _ in want[2]) and any(i == 2 for i, _ in want[0])
