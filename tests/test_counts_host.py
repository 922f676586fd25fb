"""The counts stage on the host: tests/native/countsim.cpp replays hypergrep_amd/csrc/hg_counts.h (head rule, bin lookup, the
split into runs) and must equal counts_ref's plain Python count, for run lengths of 1, 2, 3 and the kernel's own, so that a
run boundary falls inside a (line, id) group, between two ids of a line, between lines and between segments.  Also here: the
bins of a compiled database, the C ABI and its Python mirrors, the refusals that need no GPU, and the command line.  No GPU
needed."""
from __future__ import annotations

import ctypes
import os
import random
import re

import pytest

import counts_ref
import countsim_py as cs

REPO = cs.REPO


def ordered(records):
    return sorted(records)  # (segment, line, id): the order a scan leaves (several equal rows: several match ends)


def check(records, ids, n_seg=None):
    records = ordered(records)
    want = counts_ref.counts(records)
    for run_len in (1, 2, 3, cs.lib().countsim_run_length()):
        lines, reports, seg_lines, seg_reports, skipped = cs.replay(records, ids, run_len, n_seg)
        assert skipped == 0
        got = {rid: (lines[b], reports[b]) for b, rid in enumerate(ids) if reports[b] or lines[b]}
        assert got == want, run_len
        if n_seg is not None:
            for s in range(n_seg):
                row = counts_ref.counts([r for r in records if r[0] == s])
                assert {rid: (seg_lines[s][b], seg_reports[s][b]) for b, rid in enumerate(ids) if seg_reports[s][b]} == row, (run_len, s)
            assert [sum(seg_reports[s][b] for s in range(n_seg)) for b in range(len(ids))] == reports
            assert [sum(seg_lines[s][b] for s in range(n_seg)) for b in range(len(ids))] == lines


def generated(seed, n_lines, ids, n_seg=1, per_line=3, ends=2):
    rng = random.Random(seed)
    out = []
    for seg in range(n_seg):
        for line in range(n_lines):
            for rid in rng.sample(ids, rng.randint(0, min(per_line, len(ids)))):
                out += [(seg, line, rid)] * rng.randint(1, ends)
    return out


def test_replay_equals_the_reference_on_generated_lists():
    ids = [0, 3, 4, 77, 0xFFFFFFFC]
    for seed in range(6):
        check(generated(seed, 40, ids), ids)
        check(generated(seed, 9, ids, n_seg=7), ids, n_seg=7)
    check(generated(1, 30, ids[:2]), ids)  # bins that stay zero
    check(generated(2, 8000, ids, per_line=5, ends=3), ids)  # several runs of the kernel's own length
    assert len(generated(2, 8000, ids, per_line=5, ends=3)) > cs.lib().countsim_run_length()


def test_edge_lists():
    check([], [5])
    check([], [])
    check([(0, 0, 5)], [5])
    check([(0, 0, 5)], [1, 5, 9])
    check([(0, line // 3, 9) for line in range(100)], [1, 9])  # all records in one bin, three ends per line
    check([(0, line, 2) for line in range(50)] * 2, [2])  # n_bins = 1
    check([(s, 0, 2) for s in range(40)], [2], n_seg=40)  # one-line files: the same line number in every segment
    check([(1, 0, 2), (3, 0, 2), (3, 1, 2)], [2], n_seg=5)  # empty segments, also the last


def test_same_line_and_id_in_neighbouring_segments_are_two_lines():
    lines, reports, seg_lines, _seg_reports, _ = cs.replay([(0, 4, 7), (1, 4, 7)], [7], 16, n_seg=2)
    assert (lines, reports, seg_lines) == ([2], [2], [[1], [1]])
    # without a segment array the two records are one line
    assert cs.replay([(0, 4, 7), (0, 4, 7)], [7], 16)[:2] == ([1], [2])


def test_accumulate_adds_to_the_totals():
    ids = [1, 2]
    first, second = ordered(generated(3, 20, ids)), ordered([(0, 20 + l, i) for _s, l, i in generated(4, 20, ids)])
    lines, reports, *_ = cs.replay(first, ids, 3)
    lines, reports, *_ = cs.replay(second, ids, 3, totals=(lines, reports))
    whole = counts_ref.counts(first + second)
    assert {rid: (lines[b], reports[b]) for b, rid in enumerate(ids)} == whole


def test_bin_lookup():
    ids = [0, 2, 9, 1000, 0xFFFFFFFC]
    for b, rid in enumerate(ids):
        assert cs.bin_of(ids, rid) == b
    for rid in (1, 3, 999, 1001, 0xFFFFFFFB, 0xFFFFFFFD, 0xFFFFFFFF):
        assert cs.bin_of(ids, rid) == 0xFFFFFFFF
    assert cs.bin_of([], 0) == 0xFFFFFFFF and cs.bin_of([7], 7) == 0 and cs.bin_of([7], 6) == 0xFFFFFFFF
    many = list(range(0, 3 * 4097, 3))
    assert all(cs.bin_of(many, rid) == b for b, rid in enumerate(many)) and cs.bin_of(many, 4) == 0xFFFFFFFF
    # an unknown id is skipped, not counted into a neighbour
    assert cs.replay([(0, 0, 5), (0, 0, 6)], [5, 7], 2)[:2] + (cs.replay([(0, 0, 5), (0, 0, 6)], [5, 7], 2)[4],) == ([1, 0], [1, 0], 1)


def test_report_ids_of_a_database():
    from hypergrep_amd import device

    # shared ids, unsorted and sparse 32-bit ids
    db = device.Database(["foo", "bar", "baz", "qux", "quux"], ids=[7, 0xFFFFFFFC, 7, 0, 1 << 31])
    assert db.report_ids().tolist() == [0, 7, 1 << 31, 0xFFFFFFFC] and db.report_ids().dtype.name == "uint32"
    # a combination with a QUIET operand: the operand's id, the other operand's and the combination's are bins
    db = device.Database(["foo", "bar", "101 & !102"], flags=[device.DEFAULT_FLAGS | device.HS_FLAG_QUIET, device.DEFAULT_FLAGS, device.HS_FLAG_COMBINATION], ids=[101, 102, 5])
    assert db.report_ids().tolist() == [5, 101, 102]
    # 4097 expressions: one bin more than a workgroup counts in LDS
    n = device.HG_COUNTS_LDS_BINS + 1
    db = device.Database([f"w{i:05d}x" for i in range(n)], ids=list(range(n, 0, -1)))
    assert db.report_ids().tolist() == list(range(1, n + 1))
    # the C call: a smaller max fills what fits and still reports the number of bins
    ids, nb = (ctypes.c_uint32 * 2)(), ctypes.c_uint32()
    assert device.lib().hg_db_report_ids(db._h, ids, 2, ctypes.byref(nb)) == 0 and nb.value == n and list(ids) == [1, 2]  # pylint: disable=protected-access
    assert device.lib().hg_db_report_ids(None, ids, 2, ctypes.byref(nb)) == -1 and device.lib().hg_db_report_ids(db._h, ids, 2, None) == -1  # pylint: disable=protected-access


def struct_names(header, name):
    body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name}_t;")]
    return re.findall(r"[\s*](\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_abi_and_python_names():
    import inspect

    import hypergrep_amd
    from hypergrep_amd import device, utils

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    for line in ("#define HG_COUNTS_ACCUMULATE 1u", "#define HG_COUNTS_PER_SEGMENT 2u", "#define HG_COUNTS_LDS_BINS 4096u"):
        assert line in header, line
    assert "hg_*;" in open(os.path.join(REPO, "hypergrep_amd", "csrc", "exports.map"), encoding="utf-8").read()
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_count_records", "hg_copy_counts", "hg_copy_segment_counts", "hg_db_report_ids", "hg_hyperscan_counts", "hg_hyperscan_files_counts"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    assert struct_names(header, "hg_counts_result") == [n for n, _ in device.HgCountsResult._fields_]
    assert ctypes.sizeof(device.HgCountsResult) == 64
    assert [getattr(device.HgCountsResult, n).offset for n, _ in device.HgCountsResult._fields_] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 60]
    assert struct_names(header, "hg_id_count") == [n for n, _ in utils.IdCount._fields_]
    assert ctypes.sizeof(utils.IdCount) == 24 and [getattr(utils.IdCount, n).offset for n, _ in utils.IdCount._fields_] == [0, 4, 8, 16]
    assert ctypes.sizeof(device.HgScanResult) == 80 and ctypes.sizeof(device.HgLinesResult) == 72  # the other results are untouched
    assert (device.HG_COUNTS_ACCUMULATE, device.HG_COUNTS_PER_SEGMENT) == (1, 2)
    assert device.HG_COUNTS_LDS_BINS == cs.lib().countsim_lds_bins() == 4096
    assert device.HG_COUNTS_RUN == cs.lib().countsim_run_length()
    assert list(inspect.signature(device.Scanner.count).parameters) == ["self", "accumulate", "per_segment", "stream"]
    for name in ("counts", "counts_arrays", "segment_counts"):
        assert callable(getattr(device.Scanner, name))
    assert callable(device.Database.report_ids)
    assert hypergrep_amd.count is utils.count and hypergrep_amd.count_files is utils.count_files
    assert {"count", "count_files"} <= set(hypergrep_amd.__all__)
    assert list(inspect.signature(utils.count).parameters) == ["file", "patterns", "flags", "ids", "ext", "buffer_size"]
    # NULL arguments are refused before anything touches a GPU
    l = device.lib()
    res = device.HgCountsResult()
    assert l.hg_count_records(None, 0, None, ctypes.byref(res)) == -1 and l.hg_count_records(None, 0, None, None) == -1
    assert l.hg_copy_counts(None, None, None, None, 0) == -1 and l.hg_copy_segment_counts(None, None, None, 0, 0) == -1


def test_file_calls_refuse_null_arguments_and_report_the_bins_without_a_gpu(tmp_path):
    """A missing file is answered before any device resource is taken: return code 6, every bin present and zero."""
    import hypergrep_amd

    missing = str(tmp_path / "missing.txt")
    assert hypergrep_amd.count(missing, ["foo", "bar", "baz"], ids=[9, 2, 9]) == ({2: (0, 0), 9: (0, 0)}, 6)
    assert hypergrep_amd.count_files([missing, missing], ["foo", "bar"], ids=[1, 0]) == [({0: (0, 0), 1: (0, 0)}, 6)] * 2
    assert hypergrep_amd.count_files([], ["foo"]) == []
    assert hypergrep_amd.count(missing, ["fo(o"]) == ({}, 4)  # the expressions do not compile
    engine = hypergrep_amd.utils._get_hyperscanner_lib()  # pylint: disable=protected-access
    assert engine.hg_hyperscan_counts(None, None, None, None, None, 0, 4096, None, 0, None, None) == 5  # HYPERSCANNER_STATE_MEM


def test_command_line_usage_and_namespace():
    from hypergrep_amd import multiscanner

    plain = multiscanner.parse_args(["-e", "foo", "file"])
    assert not hasattr(plain, "pattern_counts")  # (the reference's command lines give the reference's namespace)
    given = multiscanner.parse_args(["--pattern-counts", "-e", "foo", "-e", "bar", "-i", "-H", "-s", "a", "b"])
    assert given.pattern_counts is True and set(vars(given)) - set(vars(plain)) == {"pattern_counts"}
    for other in (["-v"], ["-o"], ["-c"], ["-l"], ["-L"], ["-q"], ["-A", "1"], ["-B", "1"], ["-C", "0"], ["-m", "3"]):
        with pytest.raises(SystemExit) as stop:
            multiscanner.parse_args(["--pattern-counts", "-e", "foo", "file"] + other)
        assert stop.value.code == 2, other


def test_command_line_on_missing_files(capsys, tmp_path):
    from hypergrep_amd import multiscanner

    names = [str(tmp_path / "a"), str(tmp_path / "b")]
    assert multiscanner.pattern_counts(names, ["foo"], with_file_name=True) == 2
    assert capsys.readouterr().out == "".join(f"hyperscanner: {n}: No such file or directory\n" for n in names)
    assert multiscanner.pattern_counts(names[:1], ["foo"], no_messages=True) == 2 and capsys.readouterr().out == ""


def test_kernel_resources():
    """The stage's kernels are in the build's table with no scratch and no spills, and every kernel the build had before the
    stage is unchanged (tests/golden/kernel_resources_before_counts.json: that build's table)."""
    import json

    with open(os.path.join(REPO, "hypergrep_amd", "lib", "kernel_resources.json"), encoding="utf-8") as f:
        table = json.load(f)
    with open(os.path.join(REPO, "tests", "golden", "kernel_resources_before_counts.json"), encoding="utf-8") as f:
        before = json.load(f)
    mine = {k: v for k, v in table.items() if "hg_counts_" in k}
    assert len(mine) == 4 and all("hg_counts_kernel" in k for k in mine)  # in LDS or in memory, with and without the matrices
    for k, v in mine.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["Dynamic Stack"] == "False", (k, v)
    assert sorted(v["LDS Size [bytes/block]"] for v in mine.values()) == [0, 0, 49152, 49152]
    assert len(before) > 100 and not any("hg_counts_" in k for k in before)
    for k, v in before.items():
        assert table.get(k) == v, k
    assert set(table) == set(before) | set(mine)
