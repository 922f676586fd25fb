"""The cells of the value table stages on the MI355X: hg_count_values, hg_rank_values (with the SEG instantiations of the shared
hash, long and insert bodies) and the value store (hg_accumulate_values, hg_rank_accumulated) on every cell of value_cells.py,
through the public calls.  Every expectation is plain Python: values_ref, rank_ref and valstore_ref (a dict, a sort, a slice) over
Scanner.parts(), the starts in Scanner.hits() and the text; the parts themselves are cross-checked with Python's `re` over the
lines.  Nothing the stages compute, and nothing of their headers, enters an expectation: the hashes that aimed some cells chose
inputs only.  Texts sit at the end of a guarded arena: a read past them faults."""
from __future__ import annotations

import pytest

import rank_ref as rr
import value_cells as vc
import values_ref as vr
import valstore_ref as sr

pytestmark = pytest.mark.gpu

ARRAYS = ("off", "count", "first", "pattern", "line_number")
MODES = ((False, False), (False, True), (True, False), (True, True))  # (by_pattern, per_segment)
NOMEM = -2
_scanners: dict = {}
_re_parts: dict = {}  # cell name -> value_cells.re_parts of its text: computed once


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


def scanner(pset, fresh=False):
    from hypergrep_amd import device

    pats, flags = vc.PSETS[pset]
    if fresh:
        return device.Scanner(device.Database(pats, flags=flags, ids=list(range(1, len(pats) + 1))), 0)
    if pset not in _scanners:
        _scanners[pset] = scanner(pset, fresh=True)
    return _scanners[pset]


def in_cells(cells, run):
    failed = []
    for cell in cells:
        try:
            run(cell)
        except AssertionError as e:
            failed.append(f"{cell['name']}: {str(e)[:500]}")
    assert not failed, f"{len(failed)} of {len(cells)} cells failed:\n" + "\n".join(failed[:12])


def same(a, want, segments, where):
    assert a["bytes"] == want["bytes"], where
    for name in ARRAYS:
        assert a[name].tolist() == want[name], (name, where, a[name].tolist()[:8], want[name][:8])
    if segments:
        assert a["segment"].tolist() == want["segment"], where
    else:
        assert a["segment"] is None, where


def scan_text(arena, cell_name, pset, text, line_base=0):
    """scan(parts=True): (scanner, ptr, parts, starts), the parts and the starts held against Python's re over the lines."""
    sc = scanner(pset)
    ptr = arena.place(text)
    st = sc.scan(ptr, len(text), parts=True, line_base=line_base)
    parts = sc.parts()
    starts = {(0, h[0]): h[3] for h in sc.hits()}
    if cell_name not in _re_parts:
        _re_parts[cell_name] = vc.re_parts(pset, text)
    records, rows = _re_parts[cell_name]
    assert parts == [(r[0] + line_base, r[1], r[2], r[3]) for r in rows] and st.n_parts == len(rows), cell_name
    assert starts == {(0, r[0] + line_base): r[1] for r in records}, cell_name
    return sc, ptr, parts, starts


def two_expressions(text, parts, starts, seg_start=None):
    by_bytes = {}
    for p, s in zip(parts, vr.spans(parts, starts, seg_start)):
        by_bytes.setdefault(text[s[0]:s[0] + s[1]], set()).add(p[3])
    return any(len(v) == 2 for v in by_bytes.values())


@pytest.mark.parametrize("group", vc.TEXT_GROUPS)
def test_count_values(arena, group):
    """Scanner.count_values on every one-buffer cell, at each of its settings, by bytes and by (expression, bytes)."""
    def run(cell):
        text = cell["text"]
        sc, ptr, parts, starts = scan_text(arena, cell["name"], cell["pset"], text)
        if ("two_expressions", None, None) in cell["claims"]:
            assert two_expressions(text, parts, starts)
        for bp in cell["by_pattern"]:
            ref = vr.groups(text, parts, starts, by_pattern=bp)
            want = vr.arrays(ref)
            assert sum(want["count"]) == len(parts)  # every part has a record
            for kw in cell["settings"]:
                kw = vc.resolve(kw, len(parts))
                st = sc.count_values(ptr, len(text), by_pattern=bp, **kw)
                assert (st.n_values, st.n_bytes, st.n_parts) == (len(ref), len(want["bytes"]), len(parts)), (bp, kw, st.n_values, len(ref))
                same(sc.values_arrays(), want, False, (bp, kw))
                assert sc.values() == [(r["value"], r["count"], r["pattern"], r["line_number"]) for r in ref], (bp, kw)
        assert sc.parts() == parts

    in_cells(vc.GROUPS[group], run)


def check_rank(sc, st, rows, seg_arrays, n_distinct, n_parts, segments, where):
    want = rr.arrays(rows, segments=segments)
    assert (st.n_values, st.n_distinct, st.n_parts, st.n_bytes) == (len(rows), n_distinct, n_parts, len(want["bytes"])), (where, st.n_values, st.n_distinct)
    same(sc.ranked_values_arrays(), want, segments, where)
    assert sc.ranked_values() == [(r["value"], r["count"], r["pattern"], r["line_number"]) + ((r["segment"],) if segments else ()) for r in rows], where
    if seg_arrays is not None:
        assert {k: v.tolist() for k, v in sc.ranked_segments().items()} == seg_arrays, where


def scan_files(arena, pset, files):
    text = b"".join(files)
    seg_start = [sum(len(f) for f in files[:i]) for i in range(len(files))]
    ends = [s + len(f) for s, f in zip(seg_start, files)]
    sc = scanner(pset)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), segments=(seg_start, ends), segment_parts=True)
    parts = [p + (s,) for p, s in zip(sc.parts(), sc.segment_parts()["part_segment"].tolist())]
    starts = {(s, h[0]): h[3] for h, s in zip(sc.hits(), sc.segments()["record_segment"].tolist())}
    _text, records, rows, _starts = vc.re_files(pset, files)
    assert parts == rows and starts == {(r[3], r[0]): r[1] for r in records}  # Python's re over every file's lines
    return sc, ptr, text, parts, starts, seg_start


@pytest.mark.parametrize("group", vc.TEXT_GROUPS)
def test_rank_values_one_file(arena, group):
    """Every cell as ONE file through rank_values(per_segment=True), the SEG instantiations of the hash, long and insert pass
    (the key word in the hash and in the comparison), and through rank_values without it, uncut."""
    def run(cell):
        if not cell["seg"]:
            return
        sc, ptr, text, parts, starts, seg_start = scan_files(arena, cell["pset"], [cell["text"]])
        for bp in cell["by_pattern"]:
            for ps in (True, False):
                rows, seg_arrays, n_distinct = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=ps, seg_start=seg_start, n_seg=1)
                for kw in cell["settings"] if ps else cell["settings"][:1]:
                    kw = vc.resolve(kw, len(parts))
                    st = sc.rank_values(ptr, len(text), per_segment=ps, by_pattern=bp, **kw)
                    check_rank(sc, st, rows, seg_arrays, n_distinct, len(parts), True, (bp, ps, kw))

    in_cells(vc.GROUPS[group], run)


def test_rank_values_files(arena):
    """The many-file cells: every mode at every cut, the per-file arrays included."""
    def run(cell):
        sc, ptr, text, parts, starts, seg_start = scan_files(arena, cell["pset"], cell["files"])
        n_seg = len(cell["files"])
        if cell["claims"]:  # equal bytes under (file 0, expression 1) and (file 1, expression 0)
            assert two_expressions(text, parts, starts, seg_start) and {(p[4], p[3]) for p in parts} == {(0, 1), (1, 0)}
        for bp, ps in MODES:
            for top in cell["tops"]:
                rows, seg_arrays, n_distinct = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=ps, top=top, seg_start=seg_start, n_seg=n_seg)
                for kw in vc.STD:
                    kw = vc.resolve(kw, len(parts))
                    st = sc.rank_values(ptr, len(text), top=top, per_segment=ps, by_pattern=bp, **kw)
                    check_rank(sc, st, rows, seg_arrays, n_distinct, len(parts), True, (bp, ps, top, kw))
        if cell["claims"]:
            assert n_distinct == 2 and len(rows) == 2  # (both on: the key word's halves do not fold together)

    in_cells(vc.GROUPS["F"], run)


class Run:
    """A store on the pattern set's shared scanner (the first add resets it) and the reference beside it."""

    def __init__(self, arena, cell, by_pattern):
        self.arena, self.cell, self.by_pattern = arena, cell, by_pattern
        self.sc = scanner(cell["pset"])
        self.ref = sr.Store(by_pattern)
        self.lines, self.fresh = 0, True

    def add(self, text, k):
        sc, ptr, parts, starts = scan_text(self.arena, (self.cell["name"], k), self.cell["pset"], text, line_base=self.lines)
        distinct = len(self.ref.table)
        added = self.ref.add(text, parts, starts)
        st = sc.accumulate_values(ptr, len(text), by_pattern=self.by_pattern, reset=self.fresh, store_log2=self.cell.get("store_log2", 0), hash_bits=self.cell.get("hash_bits", 0))
        self.fresh = False
        values = [text[starts[(0, p[0])] + p[1]:starts[(0, p[0])] + p[2]] for p in parts]
        keys = {(p[3], v) if self.by_pattern else v for p, v in zip(parts, values)}
        assert (st.n_added, st.n_distinct, st.n_groups, st.n_parts, st.n_parts_total) == (added, distinct + added, len(keys), len(parts), self.ref.n_parts), (k, st.n_added, added)
        assert st.n_bytes == sum(len(key[1] if self.by_pattern else key) for key in self.ref.table), k
        self.lines += text.count(b"\n")
        return st, parts, values

    def check(self, top=0, order_first=False):
        rows = self.ref.rows(top, order_first)
        want = sr.arrays(rows)
        st = self.sc.rank_accumulated(top, order_first)
        a = self.sc.accumulated_values_arrays()
        assert (st.n_values, st.n_distinct, st.n_parts, st.n_bytes) == (len(rows), len(self.ref.table), self.ref.n_parts, len(want["bytes"])), (top, order_first)
        assert a["bytes"] == want["bytes"], (top, order_first)
        for name in ARRAYS:
            assert a[name].tolist() == want[name], (name, top, order_first)
        assert self.sc.accumulated_values() == [(r["value"], r["count"], r["pattern"], r["line_number"]) for r in rows]


def test_store(arena):
    """The store cells: every call's numbers and, behind the calls, complete rankings."""
    from hypergrep_amd import device

    def run(cell):
        for bp in (False, True):
            run_ = Run(arena, cell, bp)
            for k, text in enumerate(cell["buffers"]):
                st, parts, values = run_.add(text, k)
                if "n_added" in cell:
                    assert st.n_added == cell["n_added"][k]
                if ("two_expressions", None, None) in cell["claims"] and k == 1:  # the value's first part in buffer 2 is expression 1's, and buffer 1 had it under 0
                    v = max(values, key=len)
                    assert parts[values.index(v)][3] == 1 and {p[3] for p, w in zip(parts, values) if w == v} == {0, 1}
                if k + 1 < len(cell["buffers"]):
                    run_.check()
            for top, order_first in cell.get("tops", ((0, False), (0, True), (2, False))):
                run_.check(top, order_first)
            if "refused" in cell:
                sc, ptr, _parts, _starts = scan_text(arena, (cell["name"], "refused"), cell["pset"], cell["refused"], line_base=run_.lines)
                with pytest.raises(device.DeviceError) as failed:  # a 64th value in a table of 64 slots
                    sc.accumulate_values(ptr, len(cell["refused"]), by_pattern=bp, store_log2=cell["store_log2"])
                assert failed.value.rc == NOMEM and "fit" in str(failed.value) and len(run_.ref.table) == 63
                run_.check()  # the store keeps every row
                run_.check(0, True)
            if "counts" in cell:
                assert all(run_.ref.table[(0, v) if bp else v][1] == n for v, n in cell["counts"].items())
            if "then_reset" in cell:
                run_.ref, run_.fresh, run_.lines = sr.Store(bp), True, 0
                for k, text in enumerate(cell["then_reset"]):
                    run_.add(text, ("reset", k))
                run_.check()
                run_.check(0, True)

    in_cells(vc.GROUPS["G"], run)


def test_stale_buffers(arena):
    """One scanner, calls of very different sizes one after the other: 5000 distinct values, 3 values, no part, 70 values by
    (expression, bytes), a ranking, a count again.  Each result is complete: no row, size or table of an earlier call shows."""
    sc = scanner("KV", fresh=True)
    for k, (kind, text, kw) in enumerate(vc.STALE):
        ptr = arena.place(text)
        sc.scan(ptr, len(text), parts=True)
        parts = sc.parts()
        starts = {(0, h[0]): h[3] for h in sc.hits()}
        records, rows = vc.re_parts("KV", text)
        assert parts == [r[:4] for r in rows]
        if kind == "count":
            ref = vr.groups(text, parts, starts, by_pattern=kw.get("by_pattern", False))
            st = sc.count_values(ptr, len(text), **kw)
            want = vr.arrays(ref)
            assert (st.n_values, st.n_bytes, st.n_parts) == (len(ref), len(want["bytes"]), len(parts)), k
            same(sc.values_arrays(), want, False, k)
        else:
            ranked, _seg, n_distinct = rr.ranking(text, parts, starts, top=kw["top"])
            st = sc.rank_values(ptr, len(text), **kw)
            check_rank(sc, st, ranked, None, n_distinct, len(parts), False, k)
    assert [len(vc.re_parts("KV", t)[1]) for _k, t, _kw in vc.STALE] == [5000, 4, 0, 140, 300, 20]


def test_two_calls_are_identical(arena):
    for name in ("A/winner across workgroups", "B/races, 200 equal long values", "C/wrap, a long value among them"):
        cell = next(c for g in vc.TEXT_GROUPS for c in vc.GROUPS[g] if c["name"] == name)
        sc, ptr, _parts, _starts = scan_text(arena, name, cell["pset"], cell["text"])
        runs = []
        for _ in range(2):
            sc.count_values(ptr, len(cell["text"]), **vc.resolve(cell["settings"][-1], len(_parts)))
            a = sc.values_arrays()
            runs.append((a["bytes"],) + tuple(a[k].tolist() for k in ARRAYS))
        assert runs[0] == runs[1], name
