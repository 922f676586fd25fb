"""The cells of the start-of-match and match-length walks on the host (no GPU).  For every cell of som_cells.py:

  * the plain Python reference equals the scalar routines of hg_som.h (hg_hit_som, hg_nfa_minlen through minlensim's piece scan);
  * somsim_walk, the host restatement of the kernel's chunked walk (tests/native/somsim.cpp), equals hg_nfa_som on every `to`
    of every piece of every expression with reverse tables, and in its early mode hg_nfa_minlen for every filtering expression;
  * every tag a cell carries is proved from the compiler's read-out, the reference or the restatement's trace, and the targets
    the suite is for are each tagged somewhere."""
from __future__ import annotations

import pytest

import minlensim_py
import som_cells as sc
import somsim_py
from minlensim_py import exts_for

NONE32 = somsim_py.NONE32
_hosts: dict = {}
_facts: dict = {}   # (database, piece, a mod 64) -> what its walks show
_done: dict = {}    # text name -> per cell facts


def hosts(name):
    """(somsim database, minlensim database) of a cell database"""
    if name not in _hosts:
        d = sc.DBS[name]
        ext = exts_for(d.need) if d.filtering else None
        _hosts[name] = (somsim_py.Db(d.pats, d.flags, d.ids, ext), minlensim_py.Db(d.pats, d.flags, d.ids, ext))
        assert _hosts[name][0].ok() and _hosts[name][1].ok(), (name, _hosts[name][0].error)
    return _hosts[name]


@pytest.mark.parametrize("name", list(sc.DBS))
def test_read_out(name):
    """nw, max_len and literal_only of every expression are the ones the cells state; min_length arrives; the som_next cycle
    of an id runs over exactly its flagged expressions."""
    d = sc.DBS[name]
    h, _m = hosts(name)
    out = [h.pattern(i) for i in range(len(d.pats))]
    for i, r in enumerate(out):
        assert (r["nw"], r["max_len"], r["literal_only"]) == d.shape[i], (name, i, d.pats[i], r)
        assert r["min_length"] == (d.need[i] or 0) and r["flags"] & 0x1FF == d.flags[i], (name, i, r)
        assert bool(r["reverse_tables"]) == bool(d.flags[i] & sc.SOM or d.need[i]), (name, i, r)
        if d.flags[i] & sc.SOM:
            cycle, j = [], i
            while True:
                cycle.append(j)
                j = out[j]["som_next"]
                if j == i:
                    break
                assert len(cycle) <= len(d.pats)
            assert sorted(cycle) == [k for k in range(len(d.pats)) if d.ids[k] == d.ids[i]], (name, i, cycle)
    for rid in set(d.ids):  # an id never mixes flagged and unflagged expressions
        assert len({d.flags[k] & sc.SOM for k in range(len(d.pats)) if d.ids[k] == rid}) == 1


def piece_facts(d, text_bytes, a, piece, want):
    """Everything the host can say about one piece at one place: scalar == reference, restatement == scalar on every `to`,
    loads inside [a & ~15, top | 15]; returns [(top mod 64, exit, nw, rounds, result, mode, at lo)] of the walks the kernels make."""
    key = (d.name, piece, a % 64)
    if key in _facts:
        return _facts[key]
    h, m = hosts(d.name)
    got, n_raw = m.piece(piece)
    assert [g[:3] for g in got] == want, (d.name, piece, got, want)
    if d.filtering:
        assert n_raw == sc.raw_count(d, piece), (d.name, piece, n_raw)
    n = len(piece)
    walks: dict = {}

    def traced(i, to, early, limit):
        w = h.walk(i, text_bytes, a, n, to, early, limit)
        top = a + to - 1
        assert (a & ~15) <= w["lowest"] and w["highest"] <= (top | 15) and w["highest"] >= top, (d.name, piece, i, to, w)
        assert w["rounds"] == (top >> 6) - (w["lowest"] >> 6) + 1, (d.name, piece, i, to, w)
        return w

    for i, pat in enumerate(d.pats):
        nw = d.shape[i][0]
        if d.flags[i] & sc.SOM:
            for to in range(1, n + 1):
                w = traced(i, to, False, 0)
                assert w["result"] == h.nfa_som(i, piece, to), (d.name, pat, piece, to, w)
                assert w["exit"] != "early"
                walks.setdefault((d.ids[i], to), []).append(((a + to - 1) % 64, w["exit"], nw, w["rounds"], w["result"], "som", False))
        if d.need[i]:
            for to in range(d.need[i], n + 1):
                w = traced(i, to, True, to - d.need[i])
                assert (w["result"] != NONE32) == h.nfa_minlen(i, piece, to, d.need[i]), (d.name, pat, piece, to, w)
                assert (w["exit"] == "early") == (w["result"] != NONE32)
                assert w["exit"] != "lo"  # (unreachable in this mode: test_every_target_is_tagged_somewhere says why)
                at_lo = 0 < d.shape[i][1] < to and w["result"] == to - d.shape[i][1]  # the early return taken at the walk's last position
                walks.setdefault(("raw", i, to), []).append(((a + to - 1) % 64, w["exit"], nw, w["rounds"], w["result"], "minlen", at_lo))
    # the walks the kernels make: hg_som_kernel for every delivered report of a flagged id (every member of the cycle, unless
    # the literal shortcut applies), hg_minlen_kernel for every raw report of a filtering expression with to >= need
    made = []
    som_ids = {d.ids[i] for i in range(len(d.pats)) if d.flags[i] & sc.SOM}
    for rid, to, frm in want:
        if rid in som_ids:
            members = [i for i in range(len(d.pats)) if d.ids[i] == rid]
            if len(members) == 1 and d.shape[members[0]][2] and d.shape[members[0]][1] <= to:
                assert frm == to - d.shape[members[0]][1]  # the shortcut's value is the reference's
                continue
            made += walks[(rid, to)]
            counted = [w[4] for i, w in zip(members, walks[(rid, to)]) if w[4] != NONE32 and to - w[4] >= (d.need[i] or 0)]
            assert frm == min(counted), (d.name, piece, rid, to, frm, walks[(rid, to)])
    for i, pat in enumerate(d.pats):
        if d.need[i]:
            for _s, to in minlensim_py.spans(pat, d.flags[i], piece):
                if to >= d.need[i]:
                    made += walks[("raw", i, to)]
    _facts[key] = made
    return made


def run_text(text):
    if text.name in _done:
        return _done[text.name]
    d = sc.DBS[text.db]
    per_cell, whole, _raw = sc.reference(text)
    data = text.data
    assert whole == sorted(whole)
    shown = {c.name: [] for c in text.cells}
    first: dict = {}  # cell -> its first piece (the filler line when it has one)
    for idx, a, piece, c in sc.layout(text):
        want = [r[1:] for r in per_cell[c.name] if r[0] == idx]
        first.setdefault(c.name, idx)
        shown[c.name] += piece_facts(d, data, a, piece, want)
    for c in text.cells:
        rows = per_cell[c.name]
        walks = shown[c.name]
        assert rows or "empty" in c.tags, c.name  # no cell is silently without a report
        for tag in c.tags:
            if tag == "empty":
                assert not rows, (c.name, rows)
            elif tag[0] == "from":
                assert any(r[1:] == tag[1:] for r in rows), (c.name, tag, rows)
            elif tag[0] == "absent":
                assert not any(r[1] == tag[1] for r in rows), (c.name, tag, rows)
            elif tag[0] == "top":
                assert any(w[0] == tag[1] for w in walks), (c.name, tag, walks)
            elif tag[0] in ("exit", "mexit"):
                mode = "som" if tag[0] == "exit" else "minlen"
                assert any(w[1] == tag[1] and w[2] == tag[2] and w[5] == mode for w in walks), (c.name, tag, walks)
            elif tag[0] == "at_lo":
                assert any(w[6] and w[2] == tag[1] and w[1] == "early" for w in walks), (c.name, tag, walks)
            elif tag[0] == "rounds":
                assert any(w[3] >= tag[1] for w in walks), (c.name, tag, walks)
            else:
                raise AssertionError(f"unknown tag {tag!r} of {c.name}")
        if c.planted and text.bs == sc.BIG:  # filler lines hold no report: every report lies in the planted line
            assert all(r[0] == first[c.name] + 1 for r in rows), c.name
    _done[text.name] = shown
    return shown


@pytest.mark.parametrize("group", list(sc.GROUPS))
def test_cells(group):
    cells = reports = 0
    for text in sc.GROUPS[group]:
        run_text(text)
        cells += len(text.cells)
        reports += len(sc.reference(text)[1])
    print(f"group {group}: {len(sc.GROUPS[group])} texts, {cells} cells, {reports} reports")
    assert reports > 0


def test_every_target_is_tagged_somewhere():
    tags = {t for c in sc.CELLS for t in c.tags if isinstance(t, tuple)}
    assert {t[1] for t in tags if t[0] == "top"} == set(range(64))
    for nw in (1, 2, 3, 32):
        for how in ("died", "lo", "start"):  # start-of-match walks
            assert ("exit", how, nw) in tags, (how, nw)
        # match-length walks.  Their `q == lo` return cannot be taken without a start: a node alive max_len bytes before `to`
        # is a first position (anything else would begin a longer match), a first position whose entry condition holds is a
        # start, and lo <= to - need since the compiler refuses need > max_len; so the walk that reaches lo returns there
        # through the early exit ("at_lo").  Every group H cell with to > max_len is of this kind or dies before lo.
        for how in ("early", "died"):
            assert ("mexit", how, nw) in tags, (how, nw)
        assert ("at_lo", nw) in tags, nw
    assert ("mexit", "start", 1) in tags
    assert not any(t[:2] == ("mexit", "lo") for t in tags)
    assert max(t[1] for t in tags if t[0] == "rounds") >= 15
    # group A's grid is the stated one
    by_db = {}
    for t in sc.GROUPS["A"]:
        for c in t.cells:
            by_db.setdefault(t.db, set()).add(([x[1] for x in c.tags if x[0] == "top"][0], [x[2] - 2 for x in c.tags if x[0] == "from"][0]))
    assert by_db["w1"] == {(m, n) for m in range(64) for n in sc.SPANS}
    for name, spans in (("w2", set(sc.SPANS_WIDE) | {52}), ("w3", set(sc.SPANS_WIDE) | {82}), ("w32", set(sc.SPANS_WIDE) | {82, 930})):
        assert by_db[name] == {(m, n) for m in sc.TOPS_FEW for n in spans}, name
    # every must-be-empty cell says so, and the compaction texts have the raw counts and kept sets they name
    for n in sc.COMPACT_COUNTS:
        for which, rule in sc.COMPACT_SETS.items():
            text = [t for t in sc.GROUPS["Hc"] if t.name == f"H/compaction {n} raw, {which} kept"][0]
            per_cell, whole, raw = sc.reference(text)
            assert raw == n and [r[0] for r in whole] == [i for i in range(n) if rule(i, n)]
    singles = [t for t in sc.GROUPS["Hc"] if "only" in t.name]
    assert len(singles) == 65
    for k, text in enumerate(singles):
        _per, whole, raw = sc.reference(text)
        assert raw == 65 and whole == [(k, 0, 11, 0)]


def test_lane_texts_hold_what_they_say():
    """Group F: hit i of a text is lane i % 64 of wave i // 64 (hits are ordered by line, one hit per line here)."""
    texts = {t.name: t for t in sc.GROUPS["F"]}
    for n in sc.F_COUNTS:
        assert len(sc.reference(texts[f"F/{n} hits"])[1]) == n
    for name, nw in (("lane3", 3), ("lane32", 32)):
        whole = sc.reference(texts[f"F/wave of {name}"])[1]
        assert sc.DBS[name].shape[0][0] == nw
        assert whole == [(i, 0, 3 + i, 1) for i in range(64)]  # span 2 + lane behind one filler byte
        walks = run_text(texts[f"F/wave of {name}"])
        assert all(w[2] == nw for ws in walks.values() for w in ws) and sum(len(ws) for ws in walks.values()) == 64
    whole = sc.reference(texts["F/wave of lane32d"])[1]
    assert whole == [(i, 0, 3 + i % 4, 1) for i in range(64)] and sc.DBS["lane32d"].shape[0][0] == 32
    mix = sc.DBS["mix"]
    whole = sc.reference(texts["F/wave of every state home"])[1]
    assert [(r[0], r[1]) for r in whole] == [(i, i % 5) for i in range(130)]
    assert [mix.shape[k][0] for k in range(5)] == [1, 2, 3, 32, 3] and [bool(f & sc.SOM) for f in mix.flags] == [True] * 4 + [False]
    assert all((r[3] == 0) == (r[1] == 4) for r in whole)  # the unflagged expression reports 0, the others 1
    nolds = sc.DBS["nolds"]
    assert max(s[0] for s, f in zip(nolds.shape, nolds.flags) if f & sc.SOM) == 1 and max(s[0] for s in nolds.shape) == 3
    assert len(sc.reference(texts["F/no multi-word expression with the flag"])[1]) == 70
