"""CPU check of the stream kernels' resources as compiled (hypergrep_amd/lib/kernel_resources.json, written by build()):
the variants the headline workload runs keep three 8-wave workgroups per CU and touch no scratch."""
from __future__ import annotations

import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(os.path.dirname(HERE), "hypergrep_amd", "lib", "kernel_resources.json")

# hg_stream_kernel<12, false, 0, 3, fold> and hg_stream_join_kernel<12, 0, fold>: 4 KiB single-probe filter, dword windows
PREFIXES = ("_Z16hg_stream_kernelILi12ELb0ELi0ELi3ELb", "_Z21hg_stream_join_kernelILi12ELi0ELb")


def _table():
    if not os.path.exists(TABLE):
        pytest.skip("kernel_resources.json is written by build()")
    with open(TABLE, encoding="utf-8") as f:
        return json.load(f)


def test_config3_stream_variants_fit_three_workgroups_without_scratch():
    table = _table()
    found = {k: v for k, v in table.items() if k.startswith(PREFIXES)}
    assert len(found) == 4, sorted(found)
    for name, res in found.items():
        assert res["VGPRs"] <= 80, (name, res["VGPRs"])
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res["ScratchSize [bytes/lane]"])
        # three workgroups of 8 waves per CU = 6 waves per SIMD, and room for three in the CU's 160 KiB of LDS
        assert res["Occupancy [waves/SIMD]"] >= 6, (name, res["Occupancy [waves/SIMD]"])
        assert 3 * res["LDS Size [bytes/block]"] <= 160 * 1024, (name, res["LDS Size [bytes/block]"])


def test_every_stream_instantiation_has_a_cell():
    """The compiled hg_stream_kernel / hg_stream_join_kernel variants are exactly the cell table's (stream_cells.py): a new
    instantiation without a cell, or a cell whose kernel is gone, fails here."""
    import stream_cells

    table = _table()
    compiled = [stream_cells.instantiation_of_symbol(k) for k in table if "hg_stream_kernel" in k or "hg_stream_join_kernel" in k]
    assert None not in compiled
    assert len(compiled) == len(set(compiled)) == 35
    assert set(compiled) == {c.instantiation for c in stream_cells.CELLS}
