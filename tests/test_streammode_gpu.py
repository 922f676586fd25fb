"""Stream mode on the GPU (hg_flow_scan_kernel): hs_scan_stream over random splits equals hs_scan of the concatenation on a
block-mode twin database; hg_scan_stream_batch equals per-stream calls; mode errors, termination, the Python surface, and
the kernel's resources."""
from __future__ import annotations

import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

import extsim_py
from hypergrep_amd import device

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


class BlockTwin:
    """The same expressions compiled in block mode; scan() = hs_scan's reports [(id, to)]."""

    def __init__(self, patterns, flags, ids, ext=None):
        self.h, err = device.hs_compile(patterns, flags, ids, ext, device.HS_MODE_BLOCK)
        assert err is None, err
        self.scratch = ctypes.c_void_p()
        assert device.face_a().hs_alloc_scratch(self.h, ctypes.byref(self.scratch)) == 0

    def scan(self, data: bytes):
        out = []
        cb = device.MATCH_EVENT(lambda i, f, t, fl, c: out.append((i, t)) or 0)
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
    assert len(set(got)) == len(got)
    last = -1
    for c in calls:
        assert c == sorted(c, key=lambda r: (r[1], r[0]))  # rule 2: (to, id) within a call
        if c:
            assert c[0][1] >= last - 1
            last = max(last, c[-1][1])


def random_text(rng, n, alphabet=b"abcdefoxyz \n"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def random_cuts(rng, n, k):
    return sorted(rng.randint(0, n) for _ in range(k))


SETS = {
    "one_word": (["foo", r"\bbar\b", "ba+z$", "qu[xy]", r"o\n", r"^x"], [0, 0, 0, 1, 0, 4], None),
    "multi_word": (["a[a-f]{40}b", "(ab|cd){12}e", "x[a-z ]{900}y", r"\bfo[a-z]{50}\b"], [0, 2, 2, 0], None),
    "literal": (["hello world", "status=5[0-9][0-9]", "foobar", "xyzzy"], [8, 0, 1 | 8, 0], None),
    "caseless_ext": (["foobar", "abcdef", "zebra"], [1, 0, 1 | 8], [extsim_py.ext(edit=1), extsim_py.ext(min_offset=10, max_offset=5000), extsim_py.ext(hamming=1)]),
}


def _set_case(name, rng, sizes=(40, 300, 3000, 9000)):
    pats, flags, ext = SETS[name]
    ids = [10 + i for i in range(len(pats))]
    sdb = device.StreamDatabase(pats, flags, ids, ext)
    twin = BlockTwin(pats, flags, ids, ext)
    needles = [b"foo", b"bar", b"baz\n", b"qux", b"hello world", b"status=512", b"FooBar", b"xyzzy", b"zebra", b"abcdef", b"abab" * 6 + b"e"]
    for n in sizes:
        parts = []
        while sum(map(len, parts)) < n:
            parts.append(random_text(rng, rng.randint(1, 40)) if rng.random() < 0.7 else rng.choice(needles))
        data = b"".join(parts)[:n]
        for k in (0, 1, 5, 17):
            cuts = random_cuts(rng, len(data), k)
            check_calls(stream_calls(sdb, data, cuts), twin.scan(data))


def test_first_stream_scan_in_child_process():
    """A new kernel's first launches run in a child process under a time limit."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from hypergrep_amd import device\n"
            "db = device.StreamDatabase(['foo', 'bar$'], [0, 0], [1, 2])\n"
            "s = db.open()\n"
            "a = s.scan(b'xxfo'); b = s.scan(b'o bar\\n'); c = s.close()\n"
            "assert (a, b, c) == ([], [(1, 5)], [(2, 9)]), (a, b, c)\n"
            "print('ok')\n") % (REPO, HERE)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.parametrize("name", sorted(SETS))
def test_stream_equals_block_scan(name):
    _set_case(name, random.Random(hash(name) & 0xFFFF))


def test_piece_loop_and_hbm_copy():
    """Writes above HG_FLOW_PIECE (pieces) and a launch above the HBM cut-off (1 MiB x workgroups)."""
    rng = random.Random(3)
    pats, flags, ext = SETS["one_word"]
    ids = list(range(len(pats)))
    sdb = device.StreamDatabase(pats, flags, ids)
    twin = BlockTwin(pats, flags, ids)
    data = random_text(rng, (1 << 20) + 300_000)
    for cuts in ([5000, 5001, 1_100_000], [9000], [100, 200_000]):
        check_calls(stream_calls(sdb, data, cuts), twin.scan(data))


def test_every_split_of_boundary_texts():
    pats = ["foo$", r"foo\Z", r"^x$", r"\bab\b", "foo", r"ab\B"]
    flags = [0, 0, 4, 0, 0, 0]
    ids = [1, 2, 3, 4, 5, 6]
    sdb = device.StreamDatabase(pats, flags, ids)
    twin = BlockTwin(pats, flags, ids)
    for text in (b"foo\n", b"foo\n\n", b"x\nx\n", b"ab ab\n", b"foo\nfoo", b"\nx\n"):
        want = twin.scan(text)
        for c in range(len(text) + 1):
            check_calls(stream_calls(sdb, text, [c]), want)
        check_calls(stream_calls(sdb, text, list(range(1, len(text)))), want)
        check_calls(stream_calls(sdb, text, [0, 0, len(text)]), want)


def test_batch_equals_per_stream_calls():
    rng = random.Random(11)
    pats, flags, ext = SETS["literal"]
    pats = pats + ["foo$", r"\bbar"]
    flags = flags + [0, 0]
    ids = list(range(len(pats)))
    sdb = device.StreamDatabase(pats, flags, ids)
    nstreams = 1200
    batch = [sdb.open() for _ in range(nstreams)]
    single = [sdb.open() for _ in range(nstreams)]
    needles = [b"foo\n", b"bar", b"hello world", b"status=599", b"xyzzy", b"FOOBAR"]
    for rnd in range(3):
        writes = [b"".join(random_text(rng, rng.randint(0, 30)) + (rng.choice(needles) if rng.random() < 0.5 else b"") for _ in range(2)) for _ in range(nstreams)]
        last = [rnd == 2 or rng.random() < 0.1 for _ in range(nstreams)]
        order = list(range(nstreams))
        rng.shuffle(order)  # interleaved: the batch's items are the streams in another order each round
        got = sdb.scan_streams([(batch[i], writes[i]) for i in order], last=[last[i] for i in order])
        for pos, i in enumerate(order):
            want = single[i].scan(writes[i]) + (single[i].reset() if last[i] else [])
            assert got[pos] == want, (rnd, i)


def test_batch_rejects_duplicates_and_terminates_one_item():
    sdb = device.StreamDatabase(["foo", "bar"], [0, 0], [1, 2])
    a, b, c = sdb.open(), sdb.open(), sdb.open()
    l = device.face_a()
    n = 2
    streams = (ctypes.c_void_p * n)(a._h, a._h)
    datas = (ctypes.c_char_p * n)(b"foo", b"foo")
    lengths = (ctypes.c_uint * n)(3, 3)
    seen = []
    cb = device.STREAM_EVENT(lambda it, i, f, t, fl, ctx: seen.append((it, i, t)) or 0)
    assert l.hg_scan_stream_batch(streams, datas, lengths, None, n, sdb._scratch, cb, None) == device.HS_INVALID
    assert seen == []
    # item 1's callback stops it; items 0 and 2 go on
    n = 3
    streams = (ctypes.c_void_p * n)(a._h, b._h, c._h)
    datas = (ctypes.c_char_p * n)(b"foo bar foo", b"foo bar foo", b"foo bar foo")
    lengths = (ctypes.c_uint * n)(11, 11, 11)
    cb = device.STREAM_EVENT(lambda it, i, f, t, fl, ctx: seen.append((it, i, t)) or (1 if it == 1 else 0))
    assert l.hg_scan_stream_batch(streams, datas, lengths, None, n, sdb._scratch, cb, None) == device.HS_SCAN_TERMINATED
    assert [r for r in seen if r[0] == 0] == [(0, 1, 3), (0, 2, 7), (0, 1, 11)] and [r for r in seen if r[0] == 1] == [(1, 1, 3)]
    assert [r for r in seen if r[0] == 2] == [(2, 1, 3), (2, 2, 7), (2, 1, 11)]
    nul = device.MATCH_EVENT(lambda *x: 0)
    assert l.hs_scan_stream(b._h, b"foo", 3, 0, sdb._scratch, nul, None) == device.HS_SCAN_TERMINATED
    assert b.reset() == [] and b.scan(b"xfoo") == [(1, 4)]
    assert a.scan(b"o") == []


def test_mode_errors_and_close_without_callback():
    l = device.face_a()
    sdb = device.StreamDatabase(["foo"], [0], [1])
    bh, err = device.hs_compile(["foo"], [0], [1], None, device.HS_MODE_BLOCK)
    s = ctypes.c_void_p()
    assert l.hs_open_stream(bh, 0, ctypes.byref(s)) == device.HS_DB_MODE_ERROR
    cb = device.MATCH_EVENT(lambda *x: 0)
    assert l.hs_scan(sdb._h, b"foo", 3, 0, sdb._scratch, cb, None) == device.HS_DB_MODE_ERROR
    size = ctypes.c_size_t()
    assert l.hs_stream_size(bh, ctypes.byref(size)) == device.HS_DB_MODE_ERROR
    st = sdb.open()
    assert st.scan(b"fo") == []
    assert l.hs_close_stream(st._h, None, device.MATCH_EVENT(), None) == 0
    st._h = None
    l.hs_free_database(bh)


def test_python_surface_round_trip():
    sdb = device.StreamDatabase(["foo", "bar$", "ab+c"], [0, 0, 8], [1, 2, 3])
    assert sdb.stream_size() > 0
    s = sdb.open()
    assert s.scan(b"xxfo") == []
    t = s.copy()
    assert s.scan(b"o abbbc") == [(1, 5), (3, 11)]
    assert t.scan(b"x bar") == [] and t.close() == [(2, 9)]
    assert s.scan(b"abc foo") == [(1, 18)]       # SINGLEMATCH: id 3 once per stream
    assert s.reset() == []
    assert s.scan(b"abc") == [(3, 3)]
    assert s.close() == []
    a, b = sdb.open(), sdb.open()
    out = sdb.scan_streams([(a, b"foo"), (b, b"bar")], last=[False, True])
    assert out == [[(1, 3)], [(2, 3)]]
    assert sdb.scan_streams([(a, b" bar")], last=[True]) == [[(2, 7)]]


def test_flow_kernel_resources():
    table = json.load(open(os.path.join(REPO, "hypergrep_amd", "lib", "kernel_resources.json"), encoding="utf-8"))
    names = [k for k in table if "hg_flow_scan_kernel" in k]
    assert names
    for k in names:
        assert table[k]["ScratchSize [bytes/lane]"] == 0 and table[k]["VGPRs Spill"] == 0, (k, table[k])


def test_write_cut_over_launches_keeps_call_order():
    """A write longer than one launch takes (64 MiB) is cut over launches; a held '\\n' at the cut must not put a report
    with to = cut - 1 after one with to = cut inside the same call."""
    cut = 64 << 20
    data = b"a" * (cut - 4) + b"foo\n" + b"a" * 100
    pats, flags, ids = [r"foo(?:\Z|\b)", "o\n"], [0, 0], [1, 2]
    sdb = device.StreamDatabase(pats, flags, ids)
    calls = stream_calls(sdb, data, [])
    assert calls[0] == [(1, cut - 1), (2, cut)], calls
    check_calls(calls, BlockTwin(pats, flags, ids).scan(data))
