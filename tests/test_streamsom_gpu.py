"""Start of match in stream mode on the GPU (hg_flow_som_kernel beside hg_flow_scan_kernel): every (id, from, to) of a
stream over random splits equals hs_scan of the concatenation on a block-mode twin with the same flags; batches equal
per-stream calls; the horizons; copy and reset; the Python triples; the kernel's resources."""
from __future__ import annotations

import ctypes
import json
import os
import random
import subprocess
import sys
import zlib

import pytest

from hypergrep_amd import device

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SOM = 256
PAST = device.HS_OFFSET_PAST_HORIZON


class BlockTwin:
    """The same expressions compiled in block mode; scan() = hs_scan's reports [(id, from, to)]."""

    def __init__(self, patterns, flags, ids, ext=None):
        self.h, err = device.hs_compile(patterns, flags, ids, ext, device.HS_MODE_BLOCK)
        assert err is None, err
        self.scratch = ctypes.c_void_p()
        assert device.face_a().hs_alloc_scratch(self.h, ctypes.byref(self.scratch)) == 0

    def scan(self, data: bytes):
        out = []
        cb = device.MATCH_EVENT(lambda i, f, t, fl, c: out.append((i, f, t)) or 0)
        assert device.face_a().hs_scan(self.h, data, len(data), 0, self.scratch, cb, None) == 0
        return out

    def __del__(self):
        device.face_a().hs_free_scratch(self.scratch)
        device.face_a().hs_free_database(self.h)


def stream_calls(sdb, data: bytes, cuts):
    s = sdb.open()
    calls, prev = [], 0
    for c in list(cuts) + [len(data)]:
        calls.append(s.scan(data[prev:c]))
        prev = c
    calls.append(s.close())
    return calls


def check_calls(calls, want):
    got = [r for c in calls for r in c]
    assert sorted(got) == sorted(want)
    assert len({(i, t) for i, _, t in got}) == len(got)
    for c in calls:
        assert c == sorted(c, key=lambda r: (r[2], r[0]))


def random_text(rng, n, alphabet=b"abcdefoxyz \n"):
    return bytes(rng.choice(alphabet) for _ in range(n))


SETS = {
    "one_word": (["foo[0-9]*bar", r"\bba+z", "qu[xy]+", r"o\n", r"ab+$", "x[a-f]*y"], [SOM, SOM, SOM | 1, SOM, SOM, SOM], None),
    "multi_word": (["a[a-f]{40}b", "(ab|cd){12}e", r"\bfo[a-z]{50}\b"], [SOM, SOM | 2, SOM], None),
    "shared_mixed": (["foo[0-9]*bar", "o+bar", r"\bba+z", "qux", "abc$"], [SOM, SOM, 0, SOM, 0], [1, 1, 2, 3, 4]),
}
NEEDLES = [b"foobar", b"foo12bar", b"baaz", b"quxy", b"o\n", b"abb\n", b"xaby", b"abab" * 6 + b"e", b"fo" + b"a" * 50 + b" "]


def _sdb(name, horizon="large"):
    pats, flags, ids = SETS[name]
    ids = ids or [10 + i for i in range(len(pats))]
    return device.StreamDatabase(pats, flags, ids, som_horizon=horizon), BlockTwin(pats, flags, ids)


def _data(rng, n):
    parts = []
    while sum(map(len, parts)) < n:
        parts.append(random_text(rng, rng.randint(1, 30)) if rng.random() < 0.6 else rng.choice(NEEDLES))
    return b"".join(parts)[:n]


def test_first_som_stream_scan_in_child_process():
    """The new kernel's first launches run in a child process under a time limit."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from hypergrep_amd import device\n"
            "db = device.StreamDatabase(['foo', 'b+ar$'], [256, 256], [1, 2], som_horizon='large')\n"
            "s = db.open()\n"
            "a = s.scan(b'xxfo'); b = s.scan(b'o bbar\\n'); c = s.close()\n"
            "assert (a, b, c) == ([], [(1, 2, 5)], [(2, 6, 10)]), (a, b, c)\n"
            "print('ok')\n") % (REPO, HERE)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.parametrize("name", sorted(SETS))
def test_stream_equals_block_som(name):
    rng = random.Random(zlib.crc32(name.encode()))
    sdb, twin = _sdb(name)
    for n in (30, 300, 3000):
        data = _data(rng, n)
        want = twin.scan(data)
        nls = [i for i, b in enumerate(data) if b == 10]
        for cuts in ([], sorted(rng.randint(0, n) for _ in range(5)), sorted(rng.randint(0, n) for _ in range(17)),
                     sorted({c for i in nls[:6] for c in (i, i + 1)}), [0, 0, n // 2, n // 2, n]):
            check_calls(stream_calls(sdb, data, cuts), want)
    data = _data(rng, 200)
    check_calls(stream_calls(sdb, data, list(range(1, len(data)))), twin.scan(data))  # 1-byte writes


def test_long_writes_and_hbm_copy():
    """Writes longer than HG_FLOW_PIECE and a launch above the 1 MiB HBM cut-off."""
    rng = random.Random(4)
    sdb, twin = _sdb("shared_mixed")
    data = _data(rng, (1 << 20) + 70_000)
    want = twin.scan(data)
    assert len(want) > 1000
    for cuts in ([5000, 5001, 1_100_000], [9000]):
        check_calls(stream_calls(sdb, data, cuts), want)


def test_batch_equals_per_stream_calls():
    rng = random.Random(12)
    pats, flags, ids = SETS["shared_mixed"]
    sdb = device.StreamDatabase(pats, flags, ids, som_horizon="medium")
    nstreams = 1100
    batch = [sdb.open() for _ in range(nstreams)]
    single = [sdb.open() for _ in range(nstreams)]
    for rnd in range(3):
        writes = [_data(rng, rng.randint(0, 60)) for _ in range(nstreams)]
        last = [rnd == 2 or rng.random() < 0.1 for _ in range(nstreams)]
        order = list(range(nstreams))
        rng.shuffle(order)
        got = sdb.scan_streams([(batch[i], writes[i]) for i in order], last=[last[i] for i in order])
        for pos, i in enumerate(order):
            want = single[i].scan(writes[i]) + (single[i].reset() if last[i] else [])
            assert got[pos] == want, (rnd, i)
        assert any(got)


@pytest.mark.parametrize("horizon", ["small", "medium", "large"])
def test_horizons(horizon):
    sdb = device.StreamDatabase(["a[^z]*b"], [SOM], [1], som_horizon=horizon)
    for k in (65533, 65534, 70000):  # spans 65535, 65536, 70002
        data = b"a" + b"x" * k + b"b"
        span = k + 2
        frm = PAST if (horizon == "small" and span >= 1 << 16) else 0
        for cuts in ([], [1], [1, 40000], [k + 1]):
            calls = stream_calls(sdb, b"q" + data, [c + 1 for c in cuts])
            assert [r for c in calls for r in c] == [(1, frm + 1 if frm != PAST else PAST, span + 1)], (horizon, k, cuts, calls)


def test_copy_and_reset_carry_the_starts():
    sdb = device.StreamDatabase(["ab+c", "xy"], [SOM, 0], [1, 2], som_horizon="small")
    s = sdb.open()
    assert s.scan(b"zzabb") == []
    t = s.copy()
    assert s.scan(b"bc xy") == [(1, 2, 7), (2, 0, 10)]
    assert t.scan(b"c") == [(1, 2, 6)]
    assert s.reset() == []
    assert s.scan(b"abc") == [(1, 0, 3)]
    s.close()
    t.close()


def test_python_triples_and_pairs():
    sdb = device.StreamDatabase(["foo", "ba+r"], [SOM, SOM], [1, 2], som_horizon="large")
    a, b = sdb.open(), sdb.open()
    out = sdb.scan_streams([(a, b"xfoo baa"), (b, b"bar")], last=[False, True])
    assert out == [[(1, 1, 4)], [(2, 0, 3)]]
    assert sdb.scan_streams([(a, b"ar")], last=[True]) == [[(2, 5, 10)]]
    plain = device.StreamDatabase(["foo"], [0], [1])
    s = plain.open()
    assert s.scan(b"xfoo") == [(1, 4)] and s.close() == []


def test_som_kernel_resources():
    table = json.load(open(os.path.join(REPO, "hypergrep_amd", "lib", "kernel_resources.json"), encoding="utf-8"))
    names = [k for k in table if "hg_flow_som_kernel" in k]
    assert names
    for k in names:
        assert table[k]["ScratchSize [bytes/lane]"] == 0 and table[k]["VGPRs Spill"] == 0, (k, table[k])
