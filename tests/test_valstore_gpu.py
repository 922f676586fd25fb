"""Matched values accumulated across scans on the MI355X: hg_accumulate_values and hg_rank_accumulated (the value store,
hypergrep_amd/csrc/hg_valstore.hip) behind hg_scan_device_parts and hg_scan_device_segments_parts.  Every expectation is
valstore_ref's plain Python dict over Scanner.parts(), the starts in Scanner.hits() and the text of every buffer (for one
pattern also Python's re and collections.Counter over the whole text), never anything the stage computes.  Texts are small and
sit at the end of a guarded buffer: a read past them faults."""
from __future__ import annotations

import collections
import random
import re

import pytest

import valstore_ref as sr

pytestmark = pytest.mark.gpu

A = 14  # DOTALL | MULTILINE | SINGLEMATCH
LANE_MAX = 256
SET_KV = (["[a-z]+=[0-9]+", "ERR[0-9]+"], [A, A])
SET_ID = (["id=[0-9a-z]+"], [A])
SET_X = (["x[a-w]*"], [A])
SET_TWO = (["user=[a-z]+", "[a-z]+=bob"], [A, A])  # both match `user=bob`: equal bytes from different expressions
ARRAYS = ("off", "count", "first", "pattern", "line_number")
NOMEM = -2


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 21)
    yield a
    _scanners.clear()  # (before the interpreter takes the module's globals away)
    a.free()


_scanners = {}


def scanner(pset):
    from hypergrep_amd import device

    key = tuple(pset[0])
    if key not in _scanners:
        _scanners[key] = device.Scanner(device.Database(pset[0], flags=pset[1], ids=list(range(1, len(pset[0]) + 1))), 0)
    return _scanners[key]


class Run:
    """A store on the scanner of a pattern set and the reference beside it; add() scans a buffer with the chained line base,
    feeds both and checks the call's numbers."""

    def __init__(self, arena, pset, by_pattern=False, **kw):
        self.arena, self.sc, self.by_pattern, self.kw = arena, scanner(pset), by_pattern, kw
        self.ref = sr.Store(by_pattern)
        self.lines = 0
        self.fresh = True
        self.last = None

    def add(self, text, **kw):
        ptr = self.arena.place(text)
        self.sc.scan(ptr, len(text), parts=True, line_base=self.lines)
        parts = self.sc.parts()
        starts = {(0, h[0]): h[3] for h in self.sc.hits()}
        assert all((0, p[0]) in starts for p in parts)  # every part has a record
        distinct = len(self.ref.table)
        added = self.ref.add(text, parts, starts)
        st = self.sc.accumulate_values(ptr, len(text), by_pattern=self.by_pattern, reset=self.fresh, **dict(self.kw, **kw))
        self.fresh = False
        keys = {(p[3], text[starts[(0, p[0])] + p[1]:starts[(0, p[0])] + p[2]]) if self.by_pattern else text[starts[(0, p[0])] + p[1]:starts[(0, p[0])] + p[2]] for p in parts}
        assert (st.n_added, st.n_distinct, st.n_groups, st.n_parts, st.n_parts_total) == (added, distinct + added, len(keys), len(parts), self.ref.n_parts), st
        assert st.n_bytes == sum(len(k[1] if self.by_pattern else k) for k in self.ref.table)
        self.lines += text.count(b"\n")
        self.last = st
        return st

    def check(self, top=0, order_first=False):
        want_rows = self.ref.rows(top, order_first)
        want = sr.arrays(want_rows)
        st = self.sc.rank_accumulated(top, order_first)
        a = self.sc.accumulated_values_arrays()
        assert (st.n_values, st.n_distinct, st.n_parts, st.n_bytes) == (len(want_rows), len(self.ref.table), self.ref.n_parts, len(want["bytes"])), (top, order_first)
        assert a["bytes"] == want["bytes"], (top, order_first)
        for name in ARRAYS:
            assert a[name].tolist() == want[name], (name, top, order_first)
        assert self.sc.accumulated_values() == [(r["value"], r["count"], r["pattern"], r["line_number"]) for r in want_rows]
        return a


def plain(a):
    return {k: (v if isinstance(v, bytes) else v.tolist()) for k, v in a.items()}


def mix_lines(rng, n):
    vocab = [b"%s=%d" % (rng.choice([b"user", b"code", b"req", b"n"]), rng.randrange(12)) for _ in range(50)] + [b"ERR%d" % rng.randrange(5) for _ in range(5)]
    filler = [b"lorem", b"-", b"GET /index", b"=", b"a=", b"=7"]
    return [b" ".join(rng.choice(vocab + filler) for _ in range(rng.randint(0, 5))) + b"\n" for _ in range(n)]


@pytest.fixture(scope="module")
def log_lines():
    rng = random.Random(21)
    lines = mix_lines(rng, 1400) + [b"lorem - GET /index\n"] * 200 + mix_lines(rng, 1400)
    return lines + [b"tail=77"]  # the last line has no newline: its value ends the text


@pytest.mark.parametrize("hash_bits", [64, 4, 1])
@pytest.mark.parametrize("by_pattern", [False, True])
def test_cut_identity(arena, log_lines, by_pattern, hash_bits):
    """One, two, three and seven buffers (one of the seven holds no part; every buffer ends at the guard, the last with a value)
    leave the same store, first included; two fresh stores agree."""
    n = len(log_lines)
    seen = []
    for cuts in ([], [1700], [900, 2100], [300, 900, 1400, 1600, 2100, 2950], []):
        run = Run(arena, SET_KV, by_pattern=by_pattern, hash_bits=hash_bits)
        bounds = [0] + cuts + [n]
        for lo, hi in zip(bounds, bounds[1:]):
            st = run.add(b"".join(log_lines[lo:hi]))
            if (lo, hi) == (1400, 1600):
                assert st.n_parts == 0 and st.n_added == 0
        got = {(top, of): plain(run.check(top, of)) for top, of in ((0, False), (0, True), (10, False))}
        assert run.ref.n_parts > 5000 and 40 < len(run.ref.table) < 130
        seen.append(got)
    assert all(s == seen[0] for s in seen[1:])
    assert seen[0][(0, True)]["first"] == sorted(seen[0][(0, True)]["first"]) and seen[0][(0, True)]["bytes"].endswith(b"tail=77")


def test_found_or_new(arena):
    run = Run(arena, SET_KV)
    first = b"".join(b"k=%d a=%d\n" % (i, i % 7) for i in range(40)) + b"z=9\n"
    assert run.add(first).n_added == 48  # k=0 .. k=39, a=0 .. a=6, z=9
    st = run.add(b"".join(b"a=%d k=%d\n" % (i % 5, 39 - i) for i in range(30)))  # only values the store has, z=9 not among them
    assert st.n_added == 0 and st.n_groups == 35
    st = run.add(b"z=9 new=1\nz=9\n")  # z=9 again, from buffer 1
    assert st.n_added == 1 and st.n_groups == 2
    st = run.add(b"".join(b"q=%d\n" % i for i in range(300)))  # only new values: more than one workgroup of groups
    assert st.n_added == st.n_groups == 300
    for n in (64, 65, 4096):  # a wave of equal parts, one more, and 16 workgroups, all of a value the store has
        st = run.add(b"a=1 a=1\n" * (n // 2) + (b"a=1\n" if n % 2 else b""))
        assert st.n_parts == n and st.n_groups == 1 and st.n_added == 0
    a = run.check()
    rows = run.ref.rows()
    assert rows[0]["value"] == b"a=1" and rows[0]["count"] == 6 + 6 + 64 + 65 + 4096 and rows[0]["first"] == 3
    z = next(r for r in rows if r["value"] == b"z=9")
    assert z["count"] == 3 and z["first"] == 80 and z["line_number"] == 40
    assert len(a["count"]) == 349
    run.check(5)
    run.check(0, True)


def x_value(rng, n, head=b""):
    return b"x" + head + bytes(rng.randrange(97, 120) for _ in range(n - 1 - len(head)))


@pytest.mark.parametrize("hash_bits", [0, 2])
def test_long_values(arena, hash_bits):
    """Values of 256 bytes (a lane's), 257, 1024 and 1027 (a wave's), repeated across buffers; neighbours that differ in the last
    byte only; a long value whose first bytes are a stored short value."""
    rng = random.Random(6)
    values = [x_value(rng, n) for n in (LANE_MAX, LANE_MAX + 1, 1024, 1027)]
    others = [v[:-1] + (b"b" if v[-1:] == b"a" else b"a") for v in values]
    assert all(o != v and len(o) == len(v) for o, v in zip(others, values))
    short = b"xabc"
    prefixed = x_value(rng, 700, head=b"abc")
    run = Run(arena, SET_X, hash_bits=hash_bits)
    run.add(b"".join(b"." * i + v + b"\n" for i, v in enumerate(values)) + short + b"\n")
    run.add(b"".join(b"." * (3 - i) + o + b" " + v + b"\n" for i, (o, v) in enumerate(zip(others, values))) + b". " + prefixed + b"\n")
    st = run.add(b"".join(v + b" " + o + b"\n" for o, v in zip(others, values)) + prefixed + b" " + short)  # the last value ends the text
    assert st.n_added == 0 and st.n_groups == 10
    rows = run.ref.rows()
    assert len(rows) == 10 and sorted(r["count"] for r in rows) == [2] * 6 + [3] * 4
    run.check()
    run.check(3)
    run.check(0, True)


@pytest.mark.parametrize("long", [False, True])
def test_every_pair_of_alignments(arena, long):
    """A value at text offsets 0 .. 3 (mod 4) against the same value at arena offsets 0 .. 3 (mod 4): values of 1 .. 4 bytes
    stand before it in the store."""
    rng = random.Random(8)
    value = x_value(rng, 301 if long else 9)
    pads = [b"", b"x", b"xa", b"xab", b"xabc"]
    for k, pad in enumerate(pads):
        run = Run(arena, SET_X)
        run.add((pad + b" " if pad else b"") + value + b"\n")
        assert run.ref.rows(0, True)[-1]["value"] == value and sum(len(r["value"]) for r in run.ref.rows(0, True)[:-1]) == k  # its arena offset, by the packing rule
        lines = []
        for t in range(4):  # every line a multiple of 4 bytes: the value starts at t (mod 4)
            line = b"." * t + value
            lines.append(line + b"." * (-(len(line) + 1) % 4) + b"\n")
        text = b"".join(lines)
        st = run.add(text)
        starts = {h[0]: h[3] for h in run.sc.hits()}
        assert sorted((starts[p[0]] + p[1]) % 4 for p in run.sc.parts() if p[2] - p[1] == len(value)) == [0, 1, 2, 3]
        assert st.n_added == 0
        rows = run.check()
        assert rows["count"].tolist()[0] == 5 and rows["bytes"].startswith(value)


def test_growth_and_a_fixed_table(arena):
    """600, 600 and 1500 distinct values: the table grows at every call (a rehash each time the store has values), and a fourth
    buffer finds the values of all three.  A fixed table refuses the call that does not fit and keeps the store."""
    from hypergrep_amd import device

    ids = [b"id=%x\n" % (i * 2654435761 % (1 << 32)) for i in range(2700)]
    bufs = [b"".join(ids[0:600]), b"".join(ids[600:1200]), b"".join(ids[1200:2700]), b"".join(ids[0:2700:7])]
    run = Run(arena, SET_ID)
    assert [run.add(b).store_log2 for b in bufs] == [11, 12, 13, 13]
    assert run.last.n_added == 0 and run.last.n_groups == 386
    a = run.check()
    assert a["count"].tolist().count(2) == 386 and len(a["count"]) == 2700
    run.check(7)
    for fixed, refused in ((11, 2), (10, 1)):  # 2^11 slots hold 1200 values and not 2700; 2^10 hold 600 and not 1200
        run = Run(arena, SET_ID, store_log2=fixed, hash_bits=6)
        for k in range(refused):
            assert run.add(bufs[k]).store_log2 == fixed
        before = plain(run.check())
        ptr = arena.place(bufs[refused])
        run.sc.scan(ptr, len(bufs[refused]), parts=True, line_base=run.lines)
        with pytest.raises(device.DeviceError) as failed:
            run.sc.accumulate_values(ptr, len(bufs[refused]), store_log2=fixed, hash_bits=6)
        assert failed.value.rc == NOMEM and "fit" in str(failed.value)
        assert plain(run.sc.accumulated_values_arrays()) == before  # the last ranking is still there
        assert plain(run.check()) == before and plain(run.check(0, True))["count"] == [1] * (600 * refused)
        st = run.add(b"".join(ids[0:42:7]), store_log2=fixed)  # and the store goes on: values it has
        assert st.n_added == 0 and st.n_distinct == 600 * refused


def test_equal_bytes_from_two_expressions(arena):
    """Without by_pattern equal bytes are one group whatever expression a part carries; with it a group per (expression, bytes)
    pair that occurs among the parts of all buffers."""
    bufs = [b"user=bob x=bob user=bob\nuser=eve\n", b"none\n", b"id=bob user=bob\nuser=al user=bob\nk=bob\n"]
    sizes = {}
    for by_pattern in (False, True):
        run = Run(arena, SET_TWO, by_pattern=by_pattern)
        pairs = set()
        for b in bufs:
            run.add(b)
            starts = {h[0]: h[3] for h in run.sc.hits()}
            pairs |= {(p[3], b[starts[p[0]] + p[1]:starts[p[0]] + p[2]]) for p in run.sc.parts()}
        sizes[by_pattern] = len(run.ref.table)
        assert len(run.ref.table) == (len(pairs) if by_pattern else len({v for _p, v in pairs})) and {p for p, _v in pairs} == {0, 1}
        if not by_pattern:
            assert {k: v[1] for k, v in run.ref.table.items()} == {b"user=bob": 4, b"x=bob": 1, b"user=eve": 1, b"id=bob": 1, b"user=al": 1, b"k=bob": 1}
        run.check()
        run.check(2)
    assert sizes[True] >= sizes[False] == 6


def test_rank_cuts_ties_and_copies(arena):
    import torch

    rng = random.Random(13)
    names = [b"bob", b"alice", b"eve", b"mallory", b"x", b"trent"]
    lines = [b"t=%d user=%s user=%s end\n" % (i, rng.choice(names), rng.choice(names)) if i % 3 else b"no user here\n" for i in range(900)]
    lines += [b"user=tie\n", b"user=knot\n"] * 2 + [b"user=late\n"]
    run = Run(arena, (["user=[a-z]+"], [A]))
    for lo, hi in ((0, 400), (400, 902), (902, len(lines))):  # tie and knot meet in buffer 2 and again in buffer 3: 2 each, tie first
        run.add(b"".join(lines[lo:hi]))
    counter = collections.Counter(re.findall(rb"user=[a-z]+", b"".join(lines)))  # (most_common keeps first occurrence among equals)
    n = len(counter)
    assert n == 9 and counter[b"user=tie"] == counter[b"user=knot"] == 2
    for top in (0, 1, 3, n, n + 1):
        a = run.check(top)
        want = counter.most_common()[:top or None]
        off = a["off"].tolist()
        assert [(a["bytes"][off[j]:off[j + 1]], int(c)) for j, c in enumerate(a["count"])] == want, top
    a = run.check()
    values = [a["bytes"][o:p] for o, p in zip(a["off"].tolist(), a["off"].tolist()[1:])]
    assert values.index(b"user=tie") + 1 == values.index(b"user=knot") and values[-1] == b"user=late"
    a = run.check(0, True)
    assert a["first"].tolist() == sorted(a["first"].tolist()) and a["bytes"].endswith(b"user=tieuser=knotuser=late")
    a = run.check(4)
    dst = torch.zeros(len(a["bytes"]) + 16, dtype=torch.uint8, device="cuda:0")
    assert run.sc.copy_accumulated_to(dst.data_ptr(), len(a["bytes"]) - 2) == len(a["bytes"]) - 2
    torch.cuda.synchronize()
    assert bytes(dst.cpu().numpy()) == a["bytes"][:-2] + bytes(18)


def test_refusals_and_isolation(arena):
    from hypergrep_amd import device

    fresh = device.Scanner(device.Database(["never=[0-9]"], flags=[A], ids=[1]), 0)
    with pytest.raises(ValueError, match="no successful scan"):
        fresh.accumulate_values(0, 0)
    with pytest.raises(ValueError, match="no accumulation"):
        fresh.rank_accumulated()
    fresh.reset_accumulated()
    text = b"a=1 b=2\na=1\nERR7 c=3\n"
    sc = scanner(SET_KV)
    ptr = arena.place(text)
    sc.scan(ptr, len(text))
    with pytest.raises(ValueError, match="not one with parts"):
        sc.accumulate_values(ptr, len(text), reset=True)
    run = Run(arena, SET_KV)
    run.add(text)
    before = plain(run.check())
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    for kw, why in (({"by_pattern": True}, "HG_ACC_BY_PATTERN differs"), ({"hash_bits": 5}, "hash_bits differs"), ({"store_log2": 41}, "store_log2 above 40"),
                    ({"hash_bits": 65}, "hash_bits above 64"), ({"table_log2": 1}, "must exceed"), ({"table_log2": 41}, "table_log2 above 40")):
        with pytest.raises(ValueError, match=why):
            sc.accumulate_values(ptr, len(text), **kw)
    with pytest.raises(ValueError, match="unknown flag bits"):
        sc._accumulate_values(ptr, len(text), device.HgAccParams(flags=4))  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.accumulate_values(ptr, len(text) - 1)
    res = device.HgAccRankResult()
    import ctypes

    assert device.lib().hg_rank_accumulated(sc._h, 0, 2, None, ctypes.byref(res)) == -1  # pylint: disable=protected-access
    assert plain(sc.accumulated_values_arrays()) == before and plain(run.check()) == before  # every refusal left the store and its ranking
    # the other stages' results are not the store's to touch, nor the scan's
    sc.count_values(ptr, len(text))
    sc.rank_values(ptr, len(text), top=2)
    kept = (sc.values(), sc.ranked_values(), sc.parts(), sc.hits())
    sc.accumulate_values(ptr, len(text))
    run.ref.add(text, sc.parts(), {(0, h[0]): h[3] for h in sc.hits()})
    assert (sc.values(), sc.ranked_values(), sc.parts(), sc.hits()) == kept and kept[0][0] == (b"a=1", 2, 0, 0)
    twice = plain(run.check())
    assert twice["count"] == [4, 2, 2, 2] and twice["first"] == [0, 1, 3, 4]  # a scan accumulated twice counts twice
    # a scan between accumulates leaves the store and its last ranking alone
    other = b"zz=5 zz=6\n" * 50
    ptr = arena.place(other)
    sc.scan(ptr, len(other), parts=True)
    assert plain(sc.accumulated_values_arrays()) == twice and plain(run.check()) == twice
    # reset, then reuse: another key rule is accepted, and nothing of the old store is left
    sc.reset_accumulated()
    with pytest.raises(ValueError, match="no accumulation"):
        sc.rank_accumulated()
    with pytest.raises(ValueError):
        sc.accumulated_values_arrays()
    assert device.lib().hg_copy_accumulated(sc._h, None, 0, None, None, None, None, None, 0) == -1  # pylint: disable=protected-access
    again = Run(arena, SET_KV, by_pattern=True, hash_bits=5)
    again.fresh = False  # (after the reset no flag is needed)
    again.add(other)
    assert plain(again.check())["count"] == [50, 50]


def test_after_segment_parts(arena):
    """Files packed in one buffer: equal values in two files are one group, and the ordinals run over the pack."""
    files = [b"n=1 n=2\nzz\nn=3\n", b"none\n", b"n=9\nn=2 n=1\n"]
    more = [b"n=2\n", b"n=7 n=9\n"]
    sc = scanner(SET_KV)
    ref = sr.Store()
    for k, pack in enumerate((files, more)):
        text = b"".join(pack)
        seg_start = [sum(len(f) for f in pack[:i]) for i in range(len(pack))]
        ptr = arena.place(text)
        sc.scan(ptr, len(text), segments=(seg_start, [s + len(f) for s, f in zip(seg_start, pack)]), segment_parts=True)
        parts = [p + (s,) for p, s in zip(sc.parts(), sc.segment_parts()["part_segment"].tolist())]
        starts = {(s, h[0]): h[3] for h, s in zip(sc.hits(), sc.segments()["record_segment"].tolist())}
        ref.add(text, parts, starts, seg_start=seg_start)
        st = sc.accumulate_values(ptr, len(text), reset=k == 0)
        assert (st.n_parts, st.n_parts_total, st.n_distinct) == (len(parts), ref.n_parts, len(ref.table))
    st = sc.rank_accumulated()
    a = sc.accumulated_values_arrays()
    want = sr.arrays(ref.rows())
    assert a["bytes"] == want["bytes"] == b"n=2n=1n=9n=3n=7" and all(a[name].tolist() == want[name] for name in ARRAYS)
    assert a["count"].tolist() == [3, 2, 2, 1, 1] and a["first"].tolist() == [1, 0, 3, 2, 7] and st.n_parts == 9
