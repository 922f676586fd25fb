"""The finalize cells (tests/finalize_cells.py) on the GPU (run with `-m gpu`): for every cell the hits as delivered, unsorted,
equal the reference list; the expression index of every hit is one the reference admits; the starts of match are what the
set allows; and Scanner.finalize_info() shows the path, the bucket plan and the per-bucket raw report counts the cell claims.
A cell whose claim the readout contradicts fails."""
from __future__ import annotations

import pytest

import finalize_cells as fc

pytestmark = pytest.mark.gpu

CELLS = fc.CELLS
KNOBS = ("HG_FIN_TARGET", "HG_NO_BUCKET_FINALIZE", "HG_CHUNK_TILES", "HG_MAX_CHUNKS", "HG_CHUNK_WEIGHTS", "HG_NO_EARLY_FINALIZE", "HG_JOINER", "HG_JOINER_AHEAD",
         "HG_STREAM_WGS_PER_CU", "HG_HIT_LIMIT", "HG_CAND_LIMIT")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    return torch


_placed = {}


def place(torch, fn):
    """The text of a cell on the device (kept for the cells that share it)."""
    if fn not in _placed:
        data = fc._text(fn)
        buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda:0")
        buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        _placed[fn] = (buf, len(data))
    return _placed[fn]


def check_results(sc, stats, scan, cell, what):
    got = sc.hits()
    print(f"{cell.name} {what}: {stats.n_hits} hits of {stats.n_raw_hits} raw reports, {stats.n_lines} lines, reruns {stats.reruns}, stream launches {stats.stream_launches}, joiner launches {stats.joiner_launches}")
    assert stats.n_hits == len(scan.records) == len(got), (what, stats.n_hits, len(scan.records))
    if got != scan.records:
        i = next(i for i, (a, b) in enumerate(zip(got, scan.records)) if a != b)
        pytest.fail(f"{cell.name} {what}: hits() differs from the reference at position {i}: got {got[max(i - 2, 0):i + 3]}, want {scan.records[max(i - 2, 0):i + 3]}")
    assert stats.n_lines == len(scan.starts)
    patterns = sc.hit_patterns()
    bad = [(i, int(p)) for i, p in enumerate(patterns) if int(p) not in scan.admissible[i]]
    assert not bad, f"{cell.name} {what}: hg_hit_aux_t.pattern outside the admissible set at {bad[:5]}"
    starts = sc.hit_starts()
    # the smallest start over the HS_FLAG_SOM_LEFTMOST expressions that share the report's id and end there; 0 without the flag
    want_starts = [0 if not cell.som or all(cell.exprs[j].single for j in adm) else rec[2] - max(len(cell.exprs[j].lit) for j in adm if not cell.exprs[j].single)
                   for rec, adm in zip(scan.records, scan.admissible)]
    assert list(starts) == want_starts, f"{cell.name} {what}: hit_starts()"


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_finalize_cell(torch_cuda, cell, monkeypatch):
    from hypergrep_amd import device

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in cell.env.items():
        monkeypatch.setenv(k, v)  # (read when the scanner is created)
    db = device.Database([e.lit.decode() for e in cell.exprs], flags=fc.flags_of(cell.exprs, cell.som), ids=[e.id for e in cell.exprs])
    sc = device.Scanner(db, 0)
    assert sc.finalize_info()["path"] == "none"
    if cell.prelude:
        buf, n = place(torch_cuda, cell.prelude)
        stats = sc.scan(buf.data_ptr(), n, buffer_size=cell.buffer_size)
        check_results(sc, stats, fc.cell_scan(cell, "prelude"), cell, "prelude")
    buf, n = place(torch_cuda, cell.text)
    stats = sc.scan(buf.data_ptr(), n, buffer_size=cell.buffer_size, line_base=cell.line_base)
    scan, claim = fc.cell_scan(cell), cell.claim
    info = sc.finalize_info(fill=True)
    fill = [int(f) for f in info.pop("fill")]
    print(f"{cell.name} readout: {info}; buckets in use {sum(1 for f in fill if f)}, fullest {max(fill, default=0)}")
    check_results(sc, stats, scan, cell, "scan")
    # the readout against the claim
    assert info["path"] == claim["path"]
    for key in ("fin_shift", "fin_nb", "fin_cap", "id_bits", "to_bits", "early_buckets", "early_beside_stream", "scan_blocks", "left_bucketed"):
        if key in claim:
            assert info[key] == claim[key], (key, info[key], claim[key])
    if "first_plan" in claim and not claim["left_bucketed"]:  # the bucket regions grew
        assert info["fin_cap"] >= claim["max_fill"] > claim["first_plan"][2]
    if "reruns_min" in claim:
        assert stats.reruns >= claim["reruns_min"]
    if "joiner_launches_min" in claim:
        assert stats.joiner_launches >= claim["joiner_launches_min"]
    if "stream_launches" in claim:
        assert stats.stream_launches == claim["stream_launches"]
    if info["path"] == "bucketed":
        # every bucket's fill level is the raw reports of the pieces that start in it: the cell's geometry as the device saw it
        assert len(fill) == info["fin_nb"] and fill == fc.bucket_fill(scan, info["fin_shift"], info["fin_nb"])
        assert max(fill) <= info["fin_cap"] and stats.n_raw_hits == sum(fill)
        for b, level in claim.get("fills", {}).items():
            assert fill[b] == level, (b, fill[b], level)
        if "classes" in claim:
            assert set(claim["classes"]) <= set(fill)
        if "fill_class" in claim:
            assert all(f == 0 or claim["fill_class"][0] <= f <= claim["fill_class"][1] for f in fill)
        if "max_fill" in claim:
            assert max(fill) == claim["max_fill"]
        if "kept_buckets" in claim:
            assert [b for b, f in enumerate(fill) if f] == claim["kept_buckets"]
    else:
        assert fill == []
    if cell.second:  # the same scanner, another text
        buf, n = place(torch_cuda, cell.second)
        stats = sc.scan(buf.data_ptr(), n, buffer_size=cell.buffer_size)
        check_results(sc, stats, fc.cell_scan(cell, "second"), cell, "second scan")
        info = sc.finalize_info()
        assert info["path"] == claim["second_path"] and info["left_bucketed"] == claim["left_bucketed"]

