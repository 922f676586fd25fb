"""The batched block scan on the GPU (hg_block_batch_kernel): BlockDatabase.scan_blocks(items) equals
[hs_scan(x) for x in items] on a block-mode twin through the existing hs_scan, order included: kernel-eligible sets and
lengths, items that fall back one by one, databases that fall back as a whole, growth of the report array, termination,
errors, and the kernel's resources."""
from __future__ import annotations

import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

import extsim_py
import regex_gen
from hypergrep_amd import device

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SOM = device.HS_FLAG_SOM_LEFTMOST

# the four sets of tests/test_streammode_gpu.py (the fourth has offset bounds: it falls back as a whole)
SETS = {
    "one_word": (["foo", r"\bbar\b", "ba+z$", "qu[xy]", r"o\n", r"^x"], [0, 0, 0, 1, 0, 4], None),
    "multi_word": (["a[a-f]{40}b", "(ab|cd){12}e", "x[a-z ]{900}y", r"\bfo[a-z]{50}\b"], [0, 2, 2, 0], None),
    "literal": (["hello world", "status=5[0-9][0-9]", "foobar", "xyzzy"], [8, 0, 1 | 8, 0], None),
    "caseless_ext": (["foobar", "abcdef", "zebra"], [1, 0, 1 | 8], [extsim_py.ext(edit=1), extsim_py.ext(min_offset=10, max_offset=5000), extsim_py.ext(hamming=1)]),
}
FIXED_LENGTHS = [0, 1, 15, 16, 17, 2047, 2048, 8191, 8192]
NEEDLES = [b"foo", b"bar", b"baz\n", b"baz", b"qux", b"hello world", b"status=512", b"FooBar", b"xyzzy", b"zebra", b"abcdef", b"abab" * 6 + b"e", b"o\n", b"\nx"]


class Twin:
    """The same expressions in block mode with a scratch of its own; scan() = the existing hs_scan's reports."""

    def __init__(self, patterns, flags, ids, ext=None):
        self.som = any(f & SOM for f in flags)
        self.h, err = device.hs_compile(patterns, flags, ids, ext, device.HS_MODE_BLOCK)
        assert err is None, err
        self.scratch = ctypes.c_void_p()
        assert device.face_a().hs_alloc_scratch(self.h, ctypes.byref(self.scratch)) == 0

    def scan(self, data: bytes):
        out = []
        som = self.som
        cb = device.MATCH_EVENT(lambda i, f, t, fl, c: out.append((i, f, t) if som else (i, t)) or 0)
        assert device.face_a().hs_scan(self.h, data, len(data), 0, self.scratch, cb, None) == 0
        return out

    def __del__(self):
        device.face_a().hs_free_scratch(self.scratch)
        device.face_a().hs_free_database(self.h)


def text(rng, n, alphabet=b"abcdefoxyz \n\0"):
    parts, size = [], 0
    while size < n:
        p = bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 40))) if rng.random() < 0.7 else rng.choice(NEEDLES)
        parts.append(p)
        size += len(p)
    return b"".join(parts)[:n]


def make_items(rng, lengths):
    items = []
    for n in lengths:
        d = text(rng, n)
        if n and rng.random() < 0.3:
            d = d[:-1] + b"\n"
        if n > 4 and rng.random() < 0.3:
            d = d[:n // 2] + b"\0\n" + d[n // 2 + 2:]
        items.append(d)
        if rng.random() < 0.2:
            items.append(d)  # identical neighbours
    return items


def check(bdb, twin, items):
    got = bdb.scan_blocks(items)
    assert len(got) == len(items)
    for i, d in enumerate(items):
        want = twin.scan(d)
        assert got[i] == want, (i, len(d), got[i][:6], want[:6])
    return got


def test_first_batch_in_child_process():
    """A new kernel's first launches run in a child process under a time limit."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from hypergrep_amd import device\n"
            "db = device.BlockDatabase(['foo', 'bar$'], [0, 0], [1, 2])\n"
            "got = db.scan_blocks([b'xxfoo bar', b'', b'bar\\n', b'foofoo', b'nothing'])\n"
            "assert got == [[(1, 5), (2, 9)], [], [(2, 3)], [(1, 3), (1, 6)], []], got\n"
            "assert db.scan(b'xxfoo bar') == [(1, 5), (2, 9)]\n"
            "print('ok')\n") % (REPO, HERE)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.parametrize("name", sorted(SETS))
def test_sets_and_lengths(name):
    pats, flags, ext = SETS[name]
    ids = [10 + i for i in range(len(pats))]
    bdb = device.BlockDatabase(pats, flags, ids, ext)
    twin = Twin(pats, flags, ids, ext)
    rng = random.Random(len(name) * 131)
    lengths = FIXED_LENGTHS + [rng.randint(1, 300) for _ in range(40)] + [rng.randint(1, 8192) for _ in range(6)] + [8193, 20000]
    rng.shuffle(lengths)
    check(bdb, twin, make_items(rng, lengths))
    check(bdb, twin, make_items(rng, [64] * 40))


def test_large_batch_many_groups_and_shards():
    rng = random.Random(9)
    words = ["w%02dx" % i for i in range(36)]
    pats = words + ["foo", r"\bbar\b", "ba+z$", r"o\n"]  # 40 expressions: two groups
    flags = [0] * 36 + [0, 0, 0, 8]
    ids = list(range(100, 140))
    bdb = device.BlockDatabase(pats, flags, ids)
    twin = Twin(pats, flags, ids)
    items = []
    for _ in range(20500):
        n = rng.randint(0, 96)
        d = bytearray(text(rng, n))
        if n > 12 and rng.random() < 0.5:
            w = rng.choice(words).encode()
            at = rng.randint(0, n - len(w))
            d[at:at + len(w)] = w
        items.append(bytes(d))
    got = check(bdb, twin, items)
    assert sum(map(len, got)) > 5000


def _random_compiled_set(rng, k):
    """k generated expressions that block mode compiles; a rejected one is replaced by the next generated one."""
    pats, flags = [], []
    while len(pats) < k:
        p, f = regex_gen.random_pattern(rng), rng.choice([0, 2, 4, 6, 1, 5]) | (8 if rng.random() < 0.3 else 0)
        h, err = device.hs_compile([p], [f], [1], None, device.HS_MODE_BLOCK)
        if err is None:
            device.face_a().hs_free_database(h)
            pats.append(p)
            flags.append(f)
    return pats, flags


def _regex_item(rng, n):
    return regex_gen.random_text(rng, max(1, n // 10), maxlen=16, final_newline=rng.random() < 0.5)[:n].ljust(n, b"a") if n else b""


RANDOM_SET_SIZES = [3, 9, 20, 32, 40]


def test_random_sets_with_several_passes_per_item():
    """Random regex_gen sets, among them 17 .. 32 expressions in one group and 40 in two, on 1280 items, so that a shard holds
    several (1024 / groups shards: shard s takes items s, s + shards, ...).  Items 0 .. 255 have at most 8 bytes and their
    successors in the shard (items 1024 ..) 600 .. 1024 bytes: a round of eight teams whose first item needs one pass and
    whose second needs more (15 expressions per pass at most).  Items of 4128 .. 8192 bytes sit among short ones: one team,
    16 expressions per pass.  The pass count of a round is the largest of its teams'."""
    rng = random.Random(2025)
    ran = 0
    for k in RANDOM_SET_SIZES:
        pats, flags = _random_compiled_set(rng, k)
        ids = [rng.choice([1, 1, 2, 3, 4, 5]) for _ in pats]
        bdb = device.BlockDatabase(pats, flags, ids)
        twin = Twin(pats, flags, ids)
        lengths = [rng.randint(1, 8) for _ in range(256)]
        lengths += [rng.choice([rng.randint(4128, 8192), 8192, 4128]) if rng.random() < 0.05 else rng.randint(0, 300) for _ in range(768)]
        lengths += [rng.randint(600, 1024) for _ in range(256)]
        check(bdb, twin, [_regex_item(rng, n) for n in lengths])
        ran += 1
    assert ran == len(RANDOM_SET_SIZES)


def test_more_than_2048_expressions_in_groups_of_256():
    """Above 2048 expressions the grouping is 256 per workgroup (tables not staged in LDS, an item's expressions in passes)."""
    rng = random.Random(11)
    words = ["k%04dz" % i for i in range(2060)]
    pats = words + ["foo", r"\bbar\b", "ba+z$", r"o\n"]
    flags = [0] * 2060 + [0, 0, 0, 8]
    ids = list(range(len(pats)))
    bdb = device.BlockDatabase(pats, flags, ids)
    twin = Twin(pats, flags, ids)
    items = []
    for i in range(300):
        n = rng.choice([5000, 8192]) if i % 97 == 5 else rng.randint(0, 200)
        d = bytearray(text(rng, n))
        for _ in range(n // 40):
            w = rng.choice(words).encode()
            at = rng.randint(0, n - len(w))
            d[at:at + len(w)] = w
        items.append(bytes(d))
    got = check(bdb, twin, items)
    assert sum(map(len, got)) > 300


def test_report_array_grows_and_second_call_on_the_same_scratch():
    bdb = device.BlockDatabase([".", "foo"], [2, 0], [1, 2])
    twin = Twin([".", "foo"], [2, 0], [1, 2])
    rng = random.Random(3)
    items = [text(rng, 8192) for _ in range(6)]
    got = check(bdb, twin, items)
    # 6 x 8192 = 49152 reports and more against the 4096 records launch_until_fits (hg_hsface.hip) allocates first and the 512 a
    # workgroup stages per round: the array grew and the launch was repeated.  (Should that first size ever exceed 49152,
    # this batch must grow with it.)
    assert all(len(g) >= 8192 for g in got)
    check(bdb, twin, make_items(rng, [100, 0, 2047, 5]))  # a second call on the grown scratch


def test_som_database_falls_back_with_starts():
    pats, flags, ids = ["fo+", "ba[rz]", "xyz"], [SOM, SOM, 0], [1, 2, 3]
    bdb = device.BlockDatabase(pats, flags, ids)
    twin = Twin(pats, flags, ids)
    rng = random.Random(5)
    items = make_items(rng, [0, 30, 200, 1000, 9000])
    got = check(bdb, twin, items)
    assert any(len(r) == 3 and r[1] > 0 for g in got for r in g)  # (id, from, to) with real starts


def test_combination_quiet_database_falls_back():
    pats = ["foo", "bar", "1 & 2", "1 | 2"]
    flags = [device.HS_FLAG_QUIET, 0, device.HS_FLAG_COMBINATION, device.HS_FLAG_COMBINATION | 8]
    ids = [1, 2, 10, 11]
    bdb = device.BlockDatabase(pats, flags, ids)
    twin = Twin(pats, flags, ids)
    got = check(bdb, twin, make_items(random.Random(6), [0, 40, 300, 300, 2000]) + [b"foo bar", b"bar", b"foo"])
    assert any(g for g in got)


def test_offset_bounds_database_falls_back():
    pats, flags, ids = ["foo", "bar"], [0, 0], [1, 2]
    ext = [extsim_py.ext(min_offset=10, max_offset=200), None]
    bdb = device.BlockDatabase(pats, flags, ids, ext)
    twin = Twin(pats, flags, ids, ext)
    check(bdb, twin, make_items(random.Random(7), [0, 9, 40, 300, 300, 2000]) + [b"foo" * 80])


def test_huge_automaton_falls_back():
    pats, flags, ids = ["foo.{0,3000}bar", "qux"], [2, 0], [1, 2]
    bdb = device.BlockDatabase(pats, flags, ids)
    twin = Twin(pats, flags, ids)
    got = check(bdb, twin, make_items(random.Random(8), [0, 50, 700, 4000]) + [b"foo" + b"x" * 2500 + b"bar qux"])
    assert got[-1]


def _raw_call(bdb, items, cb):
    n = len(items)
    datas = (ctypes.c_char_p * n)(*items)
    lengths = (ctypes.c_uint * n)(*[len(d) for d in items])
    return device.face_a().hg_scan_blocks(bdb._h, datas, lengths, n, bdb._scratch, cb, None)


def test_termination_ends_one_item_only():
    bdb = device.BlockDatabase(["foo"], [0], [1])
    items = [b"foo foo", b"foo foo foo", b"none", b"xfoo foo"]
    want = bdb.scan_blocks(items)
    got = [[] for _ in items]

    def on_event(item, rid, frm, to, fl, ctx):
        got[item].append((rid, to))
        return 1 if item == 1 else 0

    assert _raw_call(bdb, items, device.STREAM_EVENT(on_event)) == device.HS_SCAN_TERMINATED
    assert got[1] == want[1][:1] and len(want[1]) == 3
    assert [got[i] for i in (0, 2, 3)] == [want[i] for i in (0, 2, 3)]
    assert bdb.scan_blocks(items) == want  # items keep no state


def test_errors_and_empty_batches():
    l = device.face_a()
    bdb = device.BlockDatabase(["foo"], [0], [1])
    other = device.BlockDatabase(["bar"], [0], [1])
    cb = device.STREAM_EVENT(lambda *a: 0)
    lengths = (ctypes.c_uint * 2)(3, 3)
    datas = (ctypes.c_char_p * 2)(b"foo", b"foo")
    assert l.hg_scan_blocks(None, datas, lengths, 2, bdb._scratch, cb, None) == device.HS_INVALID
    assert l.hg_scan_blocks(bdb._h, datas, None, 2, bdb._scratch, cb, None) == device.HS_INVALID
    assert l.hg_scan_blocks(bdb._h, None, lengths, 2, bdb._scratch, cb, None) == device.HS_INVALID
    assert l.hg_scan_blocks(bdb._h, datas, lengths, 2, None, cb, None) == device.HS_INVALID
    assert l.hg_scan_blocks(bdb._h, datas, lengths, 2, other._scratch, cb, None) == device.HS_INVALID
    holes = (ctypes.c_char_p * 2)(b"foo", None)
    assert l.hg_scan_blocks(bdb._h, holes, lengths, 2, bdb._scratch, cb, None) == device.HS_INVALID
    sdb = device.StreamDatabase(["foo"], [0], [1])
    assert l.hg_scan_blocks(sdb._h, datas, lengths, 2, sdb._scratch, cb, None) == device.HS_DB_MODE_ERROR
    assert l.hg_scan_blocks(bdb._h, datas, lengths, 0, bdb._scratch, cb, None) == device.HS_SUCCESS
    # only empty items (NULL data allowed), and no callback
    zero = (ctypes.c_uint * 2)(0, 0)
    nothing = (ctypes.c_char_p * 2)(None, None)
    seen = []
    cb2 = device.STREAM_EVENT(lambda *a: seen.append(a) or 0)
    assert l.hg_scan_blocks(bdb._h, nothing, zero, 2, bdb._scratch, cb2, None) == device.HS_SUCCESS and not seen
    assert l.hg_scan_blocks(bdb._h, None, zero, 2, bdb._scratch, cb2, None) == device.HS_SUCCESS and not seen
    assert l.hg_scan_blocks(bdb._h, datas, lengths, 2, bdb._scratch, device.STREAM_EVENT(), None) == device.HS_SUCCESS
    assert bdb.scan_blocks([]) == [] and bdb.scan_blocks([b"", b""]) == [[], []]


def test_kernel_resources():
    table = json.load(open(os.path.join(REPO, "hypergrep_amd", "lib", "kernel_resources.json"), encoding="utf-8"))
    mine = [v for k, v in table.items() if "hg_block_batch_kernel" in k]
    assert len(mine) == 1
    assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0
