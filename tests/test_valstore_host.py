"""The value store without a GPU: the scalar rules of hypergrep_amd/csrc/hg_valstore.h, replayed on the host
(tests/native/valstoresim.cpp), against valstore_ref's plain Python dict over the calls' part lists; the two-source comparison at
every pair of alignments; the ABI's names and layouts; the refusals that need no device; the build's resource table."""
from __future__ import annotations

import ctypes
import inspect
import json
import os
import random
import re
import subprocess

import pytest

import valstore_ref as sr
import valstoresim_py as ss

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_MAX = 256
LENGTHS = list(range(1, 10)) + [255, 256, 257, 1027]


def layout(lines_parts, first_line=0):
    """A buffer and its records and parts from [(line bytes, [(from, to, pattern), ...]), ...]; lines are numbered from first_line
    (the chained line_base)."""
    text, records, parts = b"", [], []
    for k, (line, spans) in enumerate(lines_parts):
        no = first_line + k
        if spans:
            records.append((no, len(text), len(line)))
        parts += [(no, f, t, p) for f, t, p in spans]
        text += line
    return text, records, parts


def find_all(line: bytes, words):
    """Non-overlapping occurrences of the words in the line, as (from, to, index of the word)."""
    spans, at = [], 0
    while at < len(line):
        hit = next(((at, at + len(w), i) for i, w in enumerate(words) if line.startswith(w, at)), None)
        if hit:
            spans.append(hit)
            at = hit[1]
        else:
            at += 1
    return spans


def accumulate(rows, cuts, by_pattern=False, tops=(0, 1, 3), **kw):
    """The rows cut into buffers at `cuts` (line indices), every buffer added to a replayed store and to the reference; every
    ranking compared.  Returns the reference's uncut rows and the replay."""
    ref, sim = sr.Store(by_pattern), ss.Store(by_pattern=by_pattern, **kw)
    bounds = [0] + list(cuts) + [len(rows)]
    for lo, hi in zip(bounds, bounds[1:]):
        text, records, parts = layout(rows[lo:hi], first_line=lo)
        added = ref.add(text, parts, {(0, r[0]): r[1] for r in records})
        sim.add(text, records, parts)
        assert sim.info["n_added"] == added and sim.info["n_distinct"] == len(ref.table), (lo, hi)
    for top in tops:
        for order_first in (False, True):
            got, info = sim.rank(top, order_first)
            assert got == sr.arrays(ref.rows(top, order_first)), (cuts, top, order_first, kw)
            assert info == {"n_distinct": len(ref.table), "n_parts": ref.n_parts}
    return ref.rows(), sim


@pytest.mark.parametrize("wave", [False, True])
def test_two_source_compare_at_every_pair_of_alignments(wave):
    rng = random.Random(3)
    for n in LENGTHS:
        value = bytes(rng.randrange(256) for _ in range(n))
        first = bytes([value[0] ^ 0x40]) + value[1:]
        last = value[:-1] + bytes([value[-1] ^ 1])
        for ta in range(4):
            for aa in range(4):
                # the value ends its buffer on both sides: the last dword read is the buffer's last, at every alignment
                text = bytes(rng.randrange(256) for _ in range(4 + ta)) + value
                for stored, want in ((value, True), (first, False), (last, False)):
                    arena = bytes(rng.randrange(256) for _ in range(8 + aa)) + stored
                    assert ss.equal(text, 4 + ta, arena, 8 + aa, n, wave) is want, (n, ta, aa, wave)
                # ... and with bytes behind it that differ
                assert ss.equal(text + b"\x01\x02\x03", 4 + ta, bytes(8 + aa) + value + b"\xfe\xfd", 8 + aa, n, wave) is True


def test_lookup_apply_and_rehash_over_random_splits():
    rng = random.Random(11)
    words = [b"user=%d" % i for i in range(9)] + [b"ERR%d" % i for i in range(3)] + [b"user=1", b"k"]
    for trial in range(6):
        rows = []
        for _line in range(rng.randrange(20, 160)):
            line = b" ".join(rng.choice(words + [b"lorem", b"-"]) for _ in range(rng.randrange(0, 6))) + b"\n"
            rows.append((line, [(f, t, i % 2) for f, t, i in find_all(line, words)]))
        whole = None
        for n_cuts in (0, 1, 2, 6):
            cuts = sorted(rng.sample(range(len(rows) + 1), n_cuts))  # (0 and len(rows): an empty buffer)
            for bp in (False, True):
                for seed in (0, 5, 9):
                    got, _sim = accumulate(rows, cuts, by_pattern=bp, order_seed=seed, hash_bits=rng.choice([0, 8, 2, 1]), tile=rng.choice([16, 64, 16384]),
                                           base=rng.choice([0, (1 << 32) + 64]))
                    if not bp:
                        whole = whole or got
                        assert got == whole  # the cut identity, first included


def test_growth_rehash_and_a_fixed_table():
    rows = [(b"id=%04d\n" % i, [(0, 7, 0)]) for i in range(2700)] + [(b"id=%04d\n" % i, [(0, 7, 0)]) for i in range(0, 2700, 7)]
    for seed in (0, 3):
        got, sim = accumulate(rows, [600, 1200, 2700], order_seed=seed, tops=(0, 5))
        assert sim.info["store_log2"] == 13 and sim.info["rehashes"] == 2 and sim.info["n_added"] == 0  # 2^11, 2^12, 2^13; the fourth buffer finds every value
        assert [r["count"] for r in got].count(2) == 386 and got[0]["value"] == b"id=0000" and got[1]["value"] == b"id=0007" and got[386]["value"] == b"id=0001"
    # a table fixed at 2^11 holds 1200 values and not 2700: the third call is refused and the store ranks as after the second
    ref, sim = sr.Store(), ss.Store(store_log2=11, hash_bits=4)
    for k, (lo, hi) in enumerate(((0, 600), (600, 1200), (1200, 2700))):
        text, records, parts = layout(rows[lo:hi], first_line=lo)
        rc = sim.add(text, records, parts, allow_nomem=True)
        assert rc == (ss.Store.NOMEM if k == 2 else 0)
        if k < 2:
            ref.add(text, parts, {(0, r[0]): r[1] for r in records})
    assert sim.rank()[0] == sr.arrays(ref.rows()) and sim.rank()[1] == {"n_distinct": 1200, "n_parts": 1200}


def test_long_values_prefixes_and_last_bytes():
    rng = random.Random(2)
    rows = []
    for n in (LANE_MAX, LANE_MAX + 1, 1024, 1027):
        value = bytes(rng.randrange(97, 123) for _ in range(n))
        other = value[:-1] + bytes([value[-1] ^ 1])
        rows += [(b"." * (n % 3) + value + b"\n", [(n % 3, n % 3 + n, 0)]), (other + b"\n", [(0, n, 0)]), (value[:5] + b" " + value + b"\n", [(0, 5, 0), (6, 6 + n, 0)])]
    rows = rows + rows[::-1]
    for cuts in ([], [3], [2, 5, 12, 20]):
        got, sim = accumulate(rows, cuts, hash_bits=2, tile=64, order_seed=4)
        assert sorted(r["count"] for r in got) == [2] * 8 + [4] * 4  # per length: the value four times, its neighbour and its prefix twice


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (valstoresim.cpp's main), built with AddressSanitizer and UBSan: the text and the arena
    live in heap blocks of exactly their readable bytes, and every text start carries a base above 2^32."""
    exe = str(tmp_path / "valstoresim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DVALSTORESIM_MAIN",
                           "-o", exe, ss.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout


def struct_names(header: str, c_name: str):
    body = header[header.index("typedef struct %s {" % c_name):header.index("} %s_t;" % c_name)]
    return re.findall(r"[\s*,](\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_abi_and_python_names():
    import hypergrep_amd
    from hypergrep_amd import build, device

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    for define in ("#define HG_ACC_BY_PATTERN 1u", "#define HG_ACC_RESET 2u", "#define HG_ACC_ORDER_FIRST 1u"):
        assert define in header
    assert "accumulation across scans on the device" not in header
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_accumulate_values", "hg_rank_accumulated", "hg_copy_accumulated", "hg_copy_accumulated_device", "hg_reset_accumulated", "hg_hyperscan_values_top"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    P, R, K = device.HgAccParams, device.HgAccResult, device.HgAccRankResult
    assert struct_names(header, "hg_acc_params") == [n for n, _ in P._fields_]
    assert struct_names(header, "hg_acc_result") == [n for n, _ in R._fields_]
    assert struct_names(header, "hg_acc_rank_result") == [n for n, _ in K._fields_]
    s = ss.sizes()
    assert (s["sizeof_params"], s["sizeof_result"], s["sizeof_rank_result"]) == (ctypes.sizeof(P), ctypes.sizeof(R), ctypes.sizeof(K)) == (16, 56, 88)
    for sizeof in ("sizeof 16", "sizeof 56", "sizeof 88"):
        assert sizeof in header[header.index("typedef struct hg_acc_params"):]
    assert [s["p." + n] for n, _ in P._fields_] == [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 8, 12]
    assert [s["r." + n] for n, _ in R._fields_] == [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 48, 52]
    assert [s["k." + n] for n, _ in K._fields_] == [getattr(K, n).offset for n, _ in K._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84]
    assert (s["by_pattern"], s["reset"], s["order_first"]) == (device.HG_ACC_BY_PATTERN, device.HG_ACC_RESET, device.HG_ACC_ORDER_FIRST) == (1, 2, 1)
    assert (s["sizeof_values_result"], s["sizeof_rank_values_result"]) == (88, 128)  # the neighbours keep their sizes
    assert list(inspect.signature(device.Scanner.accumulate_values).parameters) == ["self", "d_text", "nbytes", "by_pattern", "reset", "stream", "hash_bits", "table_log2",
                                                                                   "store_log2"]
    assert list(inspect.signature(device.Scanner.rank_accumulated).parameters) == ["self", "top", "order_first", "stream"]
    assert [f.name for f in device.AccStats.__dataclass_fields__.values()] == ["n_distinct", "n_added", "n_groups", "n_parts", "n_parts_total", "n_bytes", "store_log2", "acc_us"]
    assert [f.name for f in device.AccRankStats.__dataclass_fields__.values()] == ["n_values", "n_distinct", "n_parts", "n_bytes", "rank_us"]
    for name in ("accumulated_values", "accumulated_values_arrays", "copy_accumulated_to", "reset_accumulated"):
        assert callable(getattr(device.Scanner, name))
    assert list(inspect.signature(hypergrep_amd.count_values_top).parameters) == ["file", "patterns", "top", "flags", "ids", "by_pattern", "buffer_size", "totals"]
    assert "count_values_top" in hypergrep_amd.__all__
    assert "hg_valstore.hip" in build.HIP_SOURCES and "hg_valstore.h" in build.HEADERS
    assert "hg_valstore.hip" not in build.KERNEL_SOURCES + build.STAGE_SOURCES + build.VALUES_SOURCES + build.RANK_SOURCES


def test_null_arguments_are_refused_without_a_gpu():
    from hypergrep_amd import device

    l = device.lib()
    res, params, rank = device.HgAccResult(), device.HgAccParams(), device.HgAccRankResult()
    assert l.hg_accumulate_values(None, None, 0, ctypes.byref(params), None, ctypes.byref(res)) == -1 and l.hg_accumulate_values(None, None, 0, None, None, None) == -1
    assert l.hg_rank_accumulated(None, 0, 0, None, ctypes.byref(rank)) == -1 and l.hg_rank_accumulated(None, 0, 0, None, None) == -1
    assert l.hg_copy_accumulated(None, None, 0, None, None, None, None, None, 0) == -1 and l.hg_copy_accumulated_device(None, None, 0, None) == -1
    assert l.hg_reset_accumulated(None) == -1


def test_file_call_on_a_missing_file_and_a_bad_set(tmp_path):
    """Both are answered before any device resource is taken, as hg_hyperscan_values answers them: return codes 6 and 4, no rows."""
    import hypergrep_amd

    missing = str(tmp_path / "missing.txt")
    totals = []
    assert hypergrep_amd.count_values_top(missing, ["foo", "bar"], 3, totals=totals) == ([], 6) and totals == [(0, 0)]
    assert hypergrep_amd.count_values_top(missing, ["foo"], 0, by_pattern=True) == ([], 6)
    assert hypergrep_amd.count_values_top(missing, ["fo(o"], 3) == ([], 4)
    with pytest.raises(ValueError):
        hypergrep_amd.count_values_top(missing, ["foo"], -1)
    engine = hypergrep_amd.utils._get_hyperscanner_lib()  # pylint: disable=protected-access
    engine.hg_hyperscan_values_top.argtypes = None
    assert engine.hg_hyperscan_values_top(None, None, None, None, None, 0, 4096, None, ctypes.c_uint64(1), None, None, None, None) == 5  # HYPERSCANNER_STATE_MEM


def test_kernel_resources():
    """The stage's kernels are in a table of their own, with no scratch, no spills and no dynamic stack."""
    with open(os.path.join(REPO, "hypergrep_amd", "lib", "kernel_resources_valstore.json"), encoding="utf-8") as f:
        table = json.load(f)
    names = sorted(re.search(r"hg_valstore_\w+?_kernel", k).group(0) for k in table)
    assert names == ["hg_valstore_" + n + "_kernel" for n in ("apply", "long", "lookup", "place", "rehash", "size")]  # (the copy pass is the line gather's)
    for k, v in table.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["Dynamic Stack"] == "False", (k, v)
    for other in ("kernel_resources.json", "kernel_resources_stages.json", "kernel_resources_values.json", "kernel_resources_rank.json"):
        with open(os.path.join(REPO, "hypergrep_amd", "lib", other), encoding="utf-8") as f:
            assert not any("hg_valstore_" in k for k in json.load(f)), other
