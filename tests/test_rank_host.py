"""The rank stage without a GPU: the scalar rules of hypergrep_amd/csrc/hg_values.h and hg_rank.h, replayed on the host
(tests/native/ranksim.cpp), against rank_ref's plain Python dict, sort and slice; the ABI's names and layouts; the refusals that
need no device; the build's resource table."""
from __future__ import annotations

import ctypes
import inspect
import json
import os
import random
import re
import subprocess

import pytest

import rank_ref as rr
import ranksim_py as rs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_MAX = 256
SETTINGS = [{"hash_bits": b, "table_log2": t} for b in (64, 8, 2, 1) for t in ("default", "tight")]


def layout(files):
    """A text, its records, parts and file offsets from [[(line bytes, [(from, to, pattern), ...]), ...], ...]: a list per file."""
    text, records, parts, seg_start = b"", [], [], []
    for seg, lines in enumerate(files):
        seg_start.append(len(text))
        at = 0
        for no, (line, spans) in enumerate(lines):
            if spans:
                records.append((no, at, len(line), seg))
            parts += [(no, f, t, p, seg) for f, t, p in spans]
            at += len(line)
            text += line
    return text, records, parts, seg_start


def words_line(words, pattern=0):
    """A line of the words, blank-separated, every word a part."""
    spans, at = [], 0
    for w in words:
        spans.append((at, at + len(w), pattern))
        at += len(w) + 1
    return (b" ".join(words) + b"\n", spans)


def check(text, records, parts, seg_start, tops=(0, 1, 2), modes=((False, False), (False, True), (True, False), (True, True)), settings=SETTINGS, drop_records=0, **kw):
    """Every mode (by_pattern, per_segment) and cut against the reference, at every setting and in both insertion orders.  Returns
    {(by_pattern, per_segment, top): (arrays, per-segment arrays)}."""
    records = records[drop_records:]
    starts = {(r[3], r[0]): r[1] for r in records}
    out = {}
    for bp, ps in modes:
        for top in tops:
            rows, seg_arrays, n_distinct = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=ps, top=top, seg_start=seg_start, n_seg=len(seg_start))
            want = rr.arrays(rows, segments=True)
            for s in settings:
                log2 = 0 if s["table_log2"] == "default" else max(1, len(parts).bit_length())
                for seed in (0, 5):
                    got, got_seg, info = rs.replay(text, records, parts, by_pattern=bp, per_segment=ps, top=top, seg_start=seg_start, hash_bits=s["hash_bits"], table_log2=log2,
                                                   order_seed=seed, **kw)
                    assert got == want, (bp, ps, top, s, seed)
                    assert got_seg == seg_arrays and info["n_distinct"] == n_distinct, (bp, ps, top, s, seed)
            if ps:  # seg_parts is the sum of the counts and seg_distinct the number of groups of every file, whatever the cut
                full, _a, _n = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=True, top=0, seg_start=seg_start, n_seg=len(seg_start))
                for f in range(len(seg_start)):
                    mine = [r for r in full if r["segment"] == f]
                    assert seg_arrays["seg_parts"][f] == sum(r["count"] for r in mine) and seg_arrays["seg_distinct"][f] == len(mine)
            out[(bp, ps, top)] = (want, seg_arrays)
    return out


def test_empty_and_one_part():
    out = check(b"nothing\n", [], [], [0])
    assert all(a["off"] == [0] and a["count"] == [] for a, _s in out.values())
    assert out[(False, True, 0)][1] == {"first_value": [0, 0], "seg_distinct": [0], "seg_parts": [0]}
    out = check(*layout([[(b"a=1\n", [(0, 3, 0)])]]))
    for a, _s in out.values():
        assert a["bytes"] == b"a=1" and a["count"] == [1] and a["first"] == [0] and a["segment"] == [0]


def test_the_cut():
    """top 0, 1, equal to and above the number of distinct values; a tie in count exactly at the cut; all counts equal."""
    # c x3, a x2, b x2, d x1, in one file: the tie between a and b is decided by first (a is earlier)
    files = [[words_line([b"a", b"b", b"c"]), words_line([b"c", b"b", b"a"]), words_line([b"c", b"d"])]]
    out = check(*layout(files), tops=(0, 1, 2, 3, 4, 5), modes=((False, False), (False, True)))
    full = out[(False, False, 0)][0]
    assert full["bytes"] == b"cabd" and full["count"] == [3, 2, 2, 1] and full["first"] == [2, 0, 1, 7]
    assert out[(False, False, 1)][0]["bytes"] == b"c" and out[(False, False, 2)][0]["bytes"] == b"ca" and out[(False, False, 2)][0]["first"] == [2, 0]
    assert out[(False, False, 4)][0] == full and out[(False, False, 5)][0] == full
    assert out[(False, True, 2)] == (out[(False, False, 2)][0], {"first_value": [0, 2], "seg_distinct": [4], "seg_parts": [8]})  # one file (n_seg 1): the same rows
    # all counts equal: the order is that of the first occurrences
    out = check(*layout([[words_line([b"x", b"yy", b"z"]), words_line([b"z", b"x", b"yy"])]]), tops=(0, 2), modes=((False, False),))
    assert out[(False, False, 0)][0]["bytes"] == b"xyyz" and out[(False, False, 2)][0]["bytes"] == b"xyy"


def test_the_same_value_in_two_files():
    files = [[words_line([b"n=1", b"n=2"]), (b"zz\n", []), words_line([b"n=3"])], [(b"none\n", [])], [words_line([b"n=9"]), words_line([b"n=2", b"n=1", b"n=2"])]]
    text, records, parts, seg_start = layout(files)
    out = check(text, records, parts, seg_start, base=(1 << 32) + 64)
    whole, per_file = out[(False, False, 0)][0], out[(False, True, 0)]
    assert whole["bytes"] == b"n=2n=1n=3n=9" and whole["count"] == [3, 2, 1, 1] and whole["segment"] == [0, 0, 0, 2]
    assert per_file[0]["bytes"] == b"n=1n=2n=3n=2n=9n=1" and per_file[0]["count"] == [1, 1, 1, 2, 1, 1] and per_file[0]["segment"] == [0, 0, 0, 2, 2, 2]
    assert per_file[1] == {"first_value": [0, 3, 3, 6], "seg_distinct": [3, 0, 3], "seg_parts": [3, 0, 4]}
    assert out[(False, True, 1)][0]["bytes"] == b"n=1n=2" and out[(False, True, 1)][1]["first_value"] == [0, 1, 1, 2]
    # a part whose piece has no record is not counted
    out = check(text, records, parts, seg_start, drop_records=1, tops=(0,))
    assert out[(False, True, 0)][0]["bytes"] == b"n=3n=2n=9n=1" and out[(False, True, 0)][1]["seg_parts"] == [1, 0, 4]


def test_files_without_parts_first_middle_and_last():
    empty, some = [(b"nothing here\n", [])], [words_line([b"k=1", b"k=2", b"k=1"])]
    for files in ([empty, some, some], [some, empty, some], [some, some, empty], [empty, [], some, [], empty], [[], [], []]):
        out = check(*layout(files), modes=((False, True),))
        fv = out[(False, True, 0)][1]["first_value"]
        assert [fv[i + 1] - fv[i] for i in range(len(files))] == [2 if f is some else 0 for f in files]


def test_a_wave_of_equal_parts_across_a_file_boundary():
    """64, 65 and 128 equal-byte parts of which half (or half and one) lie in each of two files: what one wavefront of the insert
    pass sees when its lanes' equal bytes belong to two keys."""
    for n in (64, 65, 128):
        a, b = n // 2, n - n // 2
        files = [[words_line([b"v=7"] * 4)] * (a // 4) + [words_line([b"v=7"] * (a % 4))] * (1 if a % 4 else 0), [words_line([b"v=7"] * b)]]
        text, records, parts, seg_start = layout(files)
        assert len(parts) == n
        out = check(text, records, parts, seg_start, tops=(0, 1), modes=((False, False), (False, True)))
        assert out[(False, False, 0)][0]["count"] == [n] and out[(False, True, 0)][0]["count"] == [a, b] and out[(False, True, 0)][0]["first"] == [0, a]
        assert out[(False, True, 1)][1] == {"first_value": [0, 1, 2], "seg_distinct": [1, 1], "seg_parts": [a, b]}


def test_a_long_value_in_two_files():
    assert rs.sizes()["by_pattern"] == 1 and rs.sizes()["per_segment"] == 2
    rng = random.Random(1)
    big = bytes(rng.randrange(33, 127) for _ in range(3 * LANE_MAX + 5))
    edge = bytes(97 + k % 26 for k in range(LANE_MAX + 1))
    files = [[(b"." + big + b"\n", [(1, 1 + len(big), 0)]), (edge + b"\n", [(0, len(edge), 0)])],
             [(b".." + big + b" " + big + b"\n", [(2, 2 + len(big), 0), (3 + len(big), 3 + 2 * len(big), 0)]), (b"..." + edge + b"\n", [(3, 3 + len(edge), 0)])]]
    text, records, parts, seg_start = layout(files)
    out = check(text, records, parts, seg_start, tops=(0, 1), modes=((False, False), (False, True)), tile=256)
    assert out[(False, False, 0)][0]["count"] == [3, 2] and out[(False, True, 0)][0]["count"] == [1, 1, 2, 1]
    assert out[(False, True, 1)][0]["bytes"] == big + big and out[(False, True, 1)][0]["first"] == [0, 2]
    _got, _seg, info = rs.replay(text, records, parts, per_segment=True, seg_start=seg_start)
    assert info["n_long"] == 5  # every part goes the wave's way


def test_by_pattern_and_per_segment():
    # bob by expression 0 and 1 in file 0, by expression 1 in file 1
    files = [[(b"bob bob\n", [(0, 3, 0), (4, 7, 1)]), (b"bob\n", [(0, 3, 1)])], [(b"bob al\n", [(0, 3, 1), (4, 6, 0)])]]
    out = check(*layout(files))
    assert out[(False, False, 0)][0]["count"] == [4, 1]
    assert out[(True, False, 0)][0]["count"] == [3, 1, 1] and out[(True, False, 0)][0]["pattern"] == [1, 0, 0] and out[(True, False, 0)][0]["first"] == [1, 0, 4]
    assert out[(False, True, 0)][0]["count"] == [3, 1, 1] and out[(False, True, 0)][0]["segment"] == [0, 1, 1]
    both = out[(True, True, 0)]
    assert both[0]["count"] == [2, 1, 1, 1] and both[0]["pattern"] == [1, 0, 1, 0] and both[0]["segment"] == [0, 0, 1, 1] and both[1]["seg_distinct"] == [2, 2]
    assert out[(True, True, 1)][0]["bytes"] == b"bobbob" and out[(True, True, 1)][0]["first"] == [1, 3]


def test_random_small_logs_over_one_to_nine_files():
    rng = random.Random(9)
    words = [b"user=%d" % i for i in range(7)] + [b"ERR%d" % i for i in range(3)] + [b"user=1", b"k"]
    for n_files in range(1, 10):
        files = []
        for _f in range(n_files):
            lines = []
            for _line in range(rng.randrange(0, 25)):
                chosen = [rng.choice(words) for _ in range(rng.randrange(0, 6))]
                line, spans = words_line(chosen) if chosen else (b"lorem\n", [])
                lines.append((line, [(f, t, rng.randrange(2)) for f, t, _p in spans]))
            files.append(lines)
        check(*layout(files), tops=(0, 1, 3), settings=SETTINGS[::3], tile=rng.choice([16, 64, 16384]))


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (ranksim.cpp's main), built with AddressSanitizer and UBSan: the text lives in a heap
    block of exactly the readable bytes, and every start carries a base above 2^32."""
    exe = str(tmp_path / "ranksim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DRANKSIM_MAIN", "-o",
                           exe, rs.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout


def struct_names(header: str, c_name: str):
    body = header[header.index("typedef struct %s {" % c_name):header.index("} %s_t;" % c_name)]
    return re.findall(r"[\s*,](\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_abi_and_python_names():
    from hypergrep_amd import build, device

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    assert "#define HG_RANK_BY_PATTERN 1u" in header and "#define HG_RANK_PER_SEGMENT 2u" in header
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_rank_values", "hg_copy_ranked_values", "hg_copy_ranked_segments", "hg_copy_ranked_values_device"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    P, R = device.HgRankParams, device.HgRankResult
    assert struct_names(header, "hg_rank_params") == [n for n, _ in P._fields_]
    assert struct_names(header, "hg_rank_result") == [n for n, _ in R._fields_]
    s = rs.sizes()
    assert (s["sizeof_params"], s["sizeof_result"]) == (ctypes.sizeof(P), ctypes.sizeof(R)) == (24, 128)
    assert [s["p." + n] for n, _ in P._fields_] == [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 8, 12, 16]
    assert [s["r." + n] for n, _ in R._fields_] == [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 112, 116, 120, 124]
    assert (s["by_pattern"], s["per_segment"]) == (device.HG_RANK_BY_PATTERN, device.HG_RANK_PER_SEGMENT) == (1, 2)
    assert (s["sizeof_values_params"], s["sizeof_values_result"]) == (16, 88)  # the values stage's structs keep their sizes
    assert list(inspect.signature(device.Scanner.rank_values).parameters) == ["self", "d_text", "nbytes", "top", "per_segment", "by_pattern", "stream", "hash_bits", "table_log2"]
    assert [f.name for f in device.RankStats.__dataclass_fields__.values()] == ["n_values", "n_distinct", "n_parts", "n_bytes", "rank_us"]
    for name in ("ranked_values", "ranked_values_arrays", "ranked_segments", "copy_ranked_values_to"):
        assert callable(getattr(device.Scanner, name))
    assert "hg_rank.hip" in build.HIP_SOURCES and "hg_rank.h" in build.HEADERS and "hg_values_dev.h" in build.HEADERS
    assert build.RANK_SOURCES == ("hg_rank.hip",) and "hg_rank.hip" not in build.KERNEL_SOURCES + build.STAGE_SOURCES + build.VALUES_SOURCES


def test_null_arguments_are_refused_without_a_gpu():
    from hypergrep_amd import device

    l = device.lib()
    res, params = device.HgRankResult(), device.HgRankParams()
    assert l.hg_rank_values(None, None, 0, ctypes.byref(params), None, ctypes.byref(res)) == -1 and l.hg_rank_values(None, None, 0, None, None, None) == -1
    assert l.hg_copy_ranked_values(None, None, 0, None, None, None, None, None, None, 0) == -1 and l.hg_copy_ranked_values_device(None, None, 0, None) == -1
    assert l.hg_copy_ranked_segments(None, None, None, None) == -1


def test_kernel_resources():
    """The stage's kernels are in a table of their own, with no scratch, no spills and no dynamic stack; the older tables hold
    none of them."""
    with open(os.path.join(REPO, "hypergrep_amd", "lib", "kernel_resources_rank.json"), encoding="utf-8") as f:
        table = json.load(f)
    names = sorted(re.search(r"hg_rank_\w+?_kernel", k).group(0) for k in table)
    assert names == ["hg_rank_" + n + "_kernel" for n in ("bounds", "counts", "hash", "insert", "keys", "long", "place")]  # (the copy pass is the line gather's)
    for k, v in table.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["Dynamic Stack"] == "False", (k, v)
    for other in ("kernel_resources.json", "kernel_resources_stages.json", "kernel_resources_values.json"):
        with open(os.path.join(REPO, "hypergrep_amd", "lib", other), encoding="utf-8") as f:
            assert not any("hg_rank_" in k for k in json.load(f)), other


def test_file_call_on_missing_files_and_a_bad_set(tmp_path):
    """All are answered before any device resource is taken: return codes 6 and 4, no rows; bad params and a NULL callback give
    the code of a bad buffer_count."""
    import hypergrep_amd

    names = [str(tmp_path / "missing.txt"), str(tmp_path / "gone.txt")]
    totals = []
    assert hypergrep_amd.count_values_files(names, ["foo", "bar"], totals=totals) == [([], 6), ([], 6)] and totals == [(0, 0), (0, 0)]
    assert hypergrep_amd.count_values_files(names, ["foo"], by_pattern=True, top=3) == [([], 6), ([], 6)]
    assert hypergrep_amd.count_values_files(names, ["fo(o"]) == [([], 4), ([], 4)]
    assert hypergrep_amd.count_values_files([], ["foo"]) == []
    with pytest.raises(ValueError):
        hypergrep_amd.count_values_files(names, ["foo"], top=-1)
    assert list(inspect.signature(hypergrep_amd.count_values_files).parameters) == ["files", "patterns", "flags", "ids", "by_pattern", "top", "buffer_size", "totals"]
    assert "count_values_files" in hypergrep_amd.__all__
    engine = hypergrep_amd.utils._get_hyperscanner_lib()  # pylint: disable=protected-access
    engine.hg_hyperscan_files_values.argtypes = None
    assert engine.hg_hyperscan_files_values(None, 0, None, None, None, None, 0, 4096, None, None, None, None) == 5  # HYPERSCANNER_STATE_MEM
    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    assert "int hg_hyperscan_files_values(" in header and "(*hg_file_values_event)" in header
    assert [n for n, _ in hypergrep_amd.utils.RankParams._fields_] == struct_names(header, "hg_rank_params") and ctypes.sizeof(hypergrep_amd.utils.RankParams) == 24


def test_command_line_namespace_with_and_without_top(capsys, tmp_path):
    from hypergrep_amd import multiscanner

    plain = multiscanner.parse_args(["-e", "foo", "file"])
    assert not hasattr(plain, "top")  # (the reference's command lines give the reference's namespace)
    counts = multiscanner.parse_args(["--value-counts", "-e", "foo", "file"])
    assert not hasattr(counts, "top") and set(vars(counts)) - set(vars(plain)) == {"value_counts"}
    given = multiscanner.parse_args(["--value-counts", "--top", "20", "-e", "foo", "-r", "dir"])
    assert given.top == 20 and set(vars(given)) - set(vars(counts)) == {"top", "recursive"}
    for bad in (["--top", "3", "-e", "foo", "file"], ["--top", "3", "--pattern-counts", "-e", "foo", "file"], ["--value-counts", "--top", "0", "-e", "foo", "file"],
                ["--value-counts", "--top", "x", "-e", "foo", "file"]):
        with pytest.raises(SystemExit) as stop:
            multiscanner.parse_args(bad)
        assert stop.value.code == 2, bad
    capsys.readouterr()
    names = [str(tmp_path / "a"), str(tmp_path / "b")]
    assert multiscanner.value_counts(names, ["foo"], with_file_name=True, top=2) == 2
    assert capsys.readouterr().out == "".join(f"hyperscanner: {n}: No such file or directory\n" for n in names)
