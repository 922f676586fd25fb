"""The values stage without a GPU: the scalar rules of hypergrep_amd/csrc/hg_values.h, replayed on the host
(tests/native/valuesim.cpp), against values_ref's plain Python dict; the hashes' agreement; the ABI's names and layouts; the
refusals that need no device; the command line's namespace; the build's resource table."""
from __future__ import annotations

import ctypes
import inspect
import json
import os
import random
import re
import subprocess

import pytest

import values_ref as vr
import valuesim_py as vs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_MAX = 256
SETTINGS = [{"hash_bits": b, "table_log2": t} for b in (64, 8, 2, 1) for t in ("default", "tight")]


def layout(lines_parts, n_patterns=1):
    """A text and its records and parts from [(line bytes, [(from, to, pattern), ...]), ...], all in one file."""
    text, records, parts = b"", [], []
    for no, (line, spans) in enumerate(lines_parts):
        if spans:
            records.append((no, len(text), len(line), 0))
        parts += [(no, f, t, p, 0) for f, t, p in spans]
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


def check(text, records, parts, seg_start=None, by_pattern=(False, True), settings=SETTINGS, **kw):
    starts = {(r[3], r[0]): r[1] for r in records}
    out = None
    for bp in by_pattern:
        want = vr.arrays(vr.groups(text, parts, starts, by_pattern=bp, seg_start=seg_start), segments=seg_start is not None)
        for s in settings:
            log2 = 0 if s["table_log2"] == "default" else max(1, len(parts).bit_length())
            for seed in (0, 5):
                got, info = vs.replay(text, records, parts, by_pattern=bp, seg_start=seg_start, hash_bits=s["hash_bits"], table_log2=log2, order_seed=seed, **kw)
                assert got == want, (bp, s, seed)
        out = out or want
    return out


def test_empty_one_equal_distinct():
    assert check(b"nothing\n", [], [])["off"] == [0]
    one = check(*layout([(b"a=1\n", [(0, 3, 0)])]))
    assert one["bytes"] == b"a=1" and one["count"] == [1] and one["first"] == [0]
    same = check(*layout([(b"a=1 a=1\n", [(0, 3, 0), (4, 7, 0)])] * 40))
    assert same["bytes"] == b"a=1" and same["count"] == [80]
    lines = [(b"id=%04d\n" % i, [(0, 7, 0)]) for i in range(300)]
    distinct = check(*layout(lines))
    assert distinct["count"] == [1] * 300 and distinct["first"] == list(range(300))


def test_prefixes_last_bytes_and_expressions():
    got = check(*layout([(b"ab abc ab\n", [(0, 2, 0), (3, 6, 0), (7, 9, 0)]), (b"abd abc\n", [(0, 3, 0), (4, 7, 0)])]))
    assert got["bytes"] == b"ababcabd" and got["count"] == [2, 2, 1] and got["first"] == [0, 1, 3] and got["line_number"] == [0, 0, 1]
    # equal bytes from different expressions: one group by bytes, two by (expression, bytes)
    text, records, parts = layout([(b"bob bob\n", [(0, 3, 0), (4, 7, 1)]), (b"bob\n", [(0, 3, 1)])])
    plain = check(text, records, parts, by_pattern=(False,))
    keyed = check(text, records, parts, by_pattern=(True,))
    assert plain["count"] == [3] and plain["pattern"] == [0] and keyed["count"] == [1, 2] and keyed["pattern"] == [0, 1] and keyed["bytes"] == b"bobbob"


def test_every_alignment_and_length():
    rows = []
    for pad in range(4):
        for n in range(1, 21):
            word = bytes(97 + (n * 7 + k) % 26 for k in range(n))
            gap = b"." * ((pad + n) % 3 + 1)
            line = b"." * pad + word + gap + word
            line += b"." * (-(len(line) + 1) % 4) + b"\n"  # every line a multiple of 4: the first word starts at alignment `pad`
            rows.append((line, [(pad, pad + n, 0), (pad + n + len(gap), pad + 2 * n + len(gap), 0)]))
    text, records, parts = layout(rows)
    start = {r[0]: r[1] for r in records}
    assert {((start[p[0]] + p[1]) % 4, p[2] - p[1]) for p in parts[::2]} == {(a, n) for a in range(4) for n in range(1, 21)}  # the whole grid, by the first words alone
    got = check(text, records, parts, by_pattern=(False,), tile=64)
    assert got["count"] == [8] * 20  # a word per length: at four pads, twice a line


def test_lengths_around_the_lane_limit_and_long_values():
    assert vs.sizes()["lane_max"] == LANE_MAX
    words = [bytes(97 + (n + k) % 26 for k in range(n)) for n in (LANE_MAX - 1, LANE_MAX, LANE_MAX + 1)]
    rng = random.Random(1)
    big = bytes(rng.randrange(1, 256) for _ in range(3000))
    big = big.replace(b"\n", b" ")
    other = big[:-1] + bytes([big[-1] ^ 1 or 2])
    rows = [(b"." * i + w + b"\n", [(i, i + len(w), 0)]) for i, w in enumerate(words + [big] + words + [big, other])]
    text, records, parts = layout(rows)
    got = check(text, records, parts, by_pattern=(False,), tile=256)
    assert got["count"] == [2, 2, 2, 2, 1] and got["off"] == [0, 255, 511, 768, 3768, 6768]
    _got, info = vs.replay(text, records, parts)
    assert info["n_long"] == 5  # LANE_MAX + 1 and the big ones go the wave's way


def test_the_same_value_in_two_files_is_one_group():
    files = [b"n=1 n=2\nzz\nn=3\n", b"none\n", b"n=9\nn=2 n=1\n"]
    seg_start = [0, 15, 20]
    text = b"".join(files)
    records = [(0, 0, 8, 0), (2, 11, 4, 0), (0, 0, 4, 2), (1, 4, 8, 2)]
    parts = [(0, 0, 3, 0, 0), (0, 4, 7, 0, 0), (2, 0, 3, 0, 0), (0, 0, 3, 0, 2), (1, 0, 3, 0, 2), (1, 4, 7, 0, 2)]
    got = check(text, records, parts, seg_start=seg_start, base=(1 << 32) + 64)
    assert got["bytes"] == b"n=1n=2n=3n=9" and got["count"] == [2, 2, 1, 1] and got["first"] == [0, 1, 2, 3] and got["segment"] == [0, 0, 0, 2]
    # a part whose piece has no record is not counted
    got, _info = vs.replay(text, records[1:], parts, seg_start=seg_start)
    assert got == vr.arrays(vr.groups(text, parts, {(r[3], r[0]): r[1] for r in records[1:]}, seg_start=seg_start), segments=True) and got["first"] == [2, 3, 4, 5]


def test_random_logs_with_collisions():
    rng = random.Random(4)
    words = [b"user=%d" % i for i in range(7)] + [b"ERR%d" % i for i in range(3)] + [b"user=1", b"k"]
    for _ in range(5):
        rows = []
        for _line in range(rng.randrange(1, 120)):
            line = b" ".join(rng.choice(words + [b"lorem", b"-"]) for _ in range(rng.randrange(0, 6))) + b"\n"
            rows.append((line, [(f, t, i % 2) for f, t, i in find_all(line, words)]))
        text, records, parts = layout(rows)
        check(text, records, parts, tile=rng.choice([16, 64, 16384]))
    # a long probe: every key starts at one of two slots of a nearly full table
    text, records, parts = layout([(b"id=%03d\n" % i, [(0, 6, 0)]) for i in range(255)])
    want = vr.arrays(vr.groups(text, parts, {(r[3], r[0]): r[1] for r in records}))
    got_tight, tight = vs.replay(text, records, parts, hash_bits=1, table_log2=8)
    got_loose, loose = vs.replay(text, records, parts)
    assert got_tight == want and got_loose == want and want["count"] == [1] * 255
    assert tight["probes"] > 50 * loose["probes"]


def test_the_three_hashes_agree():
    rng = random.Random(2)
    text = bytes(rng.randrange(256) for _ in range(4099))
    for length in list(range(1, 40)) + [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2000]:
        for s in range(4):
            for start in (s, len(text) - length - s):  # both ends of the text: the last dword may be the text's last
                want = vs.hash_of(text, start, length, 0)
                assert vs.hash_of(text, start, length, 1) == want and vs.hash_of(text, start, length, 2) == want, (start, length)
    # length, expression and cut are part of it
    assert vs.hash_of(b"ab\0", 0, 2, 0) != vs.hash_of(b"ab\0", 0, 3, 0)
    assert vs.hash_of(b"abcd", 0, 4, 0, by_pattern=True, pattern=0) != vs.hash_of(b"abcd", 0, 4, 0, by_pattern=True, pattern=1)
    assert vs.hash_of(b"abcd", 0, 4, 0, pattern=0) == vs.hash_of(b"abcd", 0, 4, 0, pattern=1)
    assert all(vs.hash_of(text, 8, 9, w, hash_bits=b) == vs.hash_of(text, 8, 9, 0) & ((1 << b) - 1) for b in (1, 2, 8, 63) for w in (0, 1))


def test_sanitized_stand_alone_replay(tmp_path):
    """The replay as a program of its own (valuesim.cpp's main), built with AddressSanitizer and UBSan: the text lives in a
    heap block of exactly the readable bytes, and every start carries a base above 2^32."""
    exe = str(tmp_path / "valuesim_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DVALUESIM_MAIN",
                           "-o", exe, vs.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout


def struct_names(header: str, c_name: str):
    body = header[header.index("typedef struct %s {" % c_name):header.index("} %s_t;" % c_name)]
    return re.findall(r"[\s*,](\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_abi_and_python_names():
    import hypergrep_amd
    from hypergrep_amd import device, utils

    header = open(os.path.join(REPO, "include", "hypergrep_amd.h"), encoding="utf-8").read()
    assert "#define HG_VALUES_BY_PATTERN 1u" in header
    lib = ctypes.CDLL(os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so"), mode=os.RTLD_NOW)
    for name in ("hg_count_values", "hg_copy_values", "hg_copy_values_device", "hg_hyperscan_values"):
        assert f"int {name}(" in header and hasattr(lib, name), name
    P, R = device.HgValuesParams, device.HgValuesResult
    assert struct_names(header, "hg_values_params") == [n for n, _ in P._fields_] == [n for n, _ in utils.ValuesParams._fields_]
    assert struct_names(header, "hg_values_result") == [n for n, _ in R._fields_]
    s = vs.sizes()
    assert (s["sizeof_params"], s["sizeof_result"]) == (ctypes.sizeof(P), ctypes.sizeof(R)) == (16, 88) and ctypes.sizeof(utils.ValuesParams) == 16
    assert [s["p." + n] for n, _ in P._fields_] == [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 8, 12]
    assert [s["r." + n] for n, _ in R._fields_] == [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84]
    assert s["by_pattern"] == device.HG_VALUES_BY_PATTERN == 1
    # the existing result structs keep their sizes
    assert (s["sizeof_part_lines_result"], s["sizeof_lines_result"], s["sizeof_counts_result"], s["sizeof_parts_result"]) == (80, 72, 64, 32)
    assert (ctypes.sizeof(device.HgPartLinesResult), ctypes.sizeof(device.HgLinesResult), ctypes.sizeof(device.HgCountsResult), ctypes.sizeof(device.HgPartsResult),
            ctypes.sizeof(device.HgScanResult)) == (80, 72, 64, 32, 80)
    assert list(inspect.signature(device.Scanner.count_values).parameters) == ["self", "d_text", "nbytes", "by_pattern", "stream", "hash_bits", "table_log2"]
    assert [f.name for f in device.ValueStats.__dataclass_fields__.values()] == ["n_values", "n_parts", "n_bytes", "values_us"]
    for name in ("values", "values_arrays", "copy_values_to"):
        assert callable(getattr(device.Scanner, name))
    assert list(inspect.signature(hypergrep_amd.count_values).parameters) == ["file", "patterns", "flags", "ids", "by_pattern", "buffer_size"]
    assert "count_values" in hypergrep_amd.__all__
    from hypergrep_amd import build

    assert "hg_values.hip" in build.HIP_SOURCES and "hg_values.h" in build.HEADERS and "hg_values.hip" not in build.KERNEL_SOURCES + build.STAGE_SOURCES


def test_null_arguments_are_refused_without_a_gpu():
    from hypergrep_amd import device

    l = device.lib()
    res, params = device.HgValuesResult(), device.HgValuesParams()
    assert l.hg_count_values(None, None, 0, ctypes.byref(params), None, ctypes.byref(res)) == -1 and l.hg_count_values(None, None, 0, None, None, None) == -1
    assert l.hg_copy_values(None, None, 0, None, None, None, None, None, None, 0) == -1 and l.hg_copy_values_device(None, None, 0, None) == -1


def test_file_call_on_a_missing_file_and_a_bad_set(tmp_path):
    """Both are answered before any device resource is taken: return codes 6 and 4, no rows."""
    import hypergrep_amd

    missing = str(tmp_path / "missing.txt")
    assert hypergrep_amd.count_values(missing, ["foo", "bar"]) == ([], 6)
    assert hypergrep_amd.count_values(missing, ["foo"], by_pattern=True) == ([], 6)
    assert hypergrep_amd.count_values(missing, ["fo(o"]) == ([], 4)
    engine = hypergrep_amd.utils._get_hyperscanner_lib()  # pylint: disable=protected-access
    engine.hg_hyperscan_values.argtypes = None
    assert engine.hg_hyperscan_values(None, None, None, None, None, 0, 4096, None, None, None) == 5  # HYPERSCANNER_STATE_MEM


def test_command_line_usage_and_namespace(capsys, tmp_path):
    from hypergrep_amd import multiscanner

    plain = multiscanner.parse_args(["-e", "foo", "file"])
    assert not hasattr(plain, "value_counts")  # (the reference's command lines give the reference's namespace)
    given = multiscanner.parse_args(["--value-counts", "-e", "foo", "-e", "bar", "-i", "-H", "-s", "a", "b"])
    assert given.value_counts is True and set(vars(given)) - set(vars(plain)) == {"value_counts"}
    for other in (["--pattern-counts"], ["-v"], ["-o"], ["-c"], ["-l"], ["-L"], ["-q"], ["-A", "1"], ["-B", "1"], ["-C", "0"], ["-m", "3"]):
        with pytest.raises(SystemExit) as stop:
            multiscanner.parse_args(["--value-counts", "-e", "foo", "file"] + other)
        assert stop.value.code == 2, other
    capsys.readouterr()
    names = [str(tmp_path / "a"), str(tmp_path / "b")]
    assert multiscanner.value_counts(names, ["foo"], with_file_name=True) == 2
    assert capsys.readouterr().out == "".join(f"hyperscanner: {n}: No such file or directory\n" for n in names)
    assert multiscanner.value_counts(names[:1], ["foo"], no_messages=True) == 2 and capsys.readouterr().out == ""


def test_kernel_resources():
    """The stage's kernels are in a table of their own, with no scratch, no spills and no dynamic stack."""
    with open(os.path.join(REPO, "hypergrep_amd", "lib", "kernel_resources_values.json"), encoding="utf-8") as f:
        table = json.load(f)
    names = sorted(re.search(r"hg_values_\w+?_kernel", k).group(0) for k in table)
    assert names == ["hg_values_" + n + "_kernel" for n in ("compact", "derive", "hash", "insert", "long", "mark")]  # (the copy pass is the line gather's)
    for k, v in table.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["Dynamic Stack"] == "False", (k, v)
    for other in ("kernel_resources.json", "kernel_resources_stages.json"):
        with open(os.path.join(REPO, "hypergrep_amd", "lib", other), encoding="utf-8") as f:
            assert not any("hg_values_" in k for k in json.load(f)), other
