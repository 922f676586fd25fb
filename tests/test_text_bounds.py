"""The window scans of bounds_cases.py, checked without a GPU: that every window is hostile (the reference on the window
widened by the leak its class is about differs from the reference on the window: a window whose surroundings would not
change the answer proves nothing, and none is allowed), that every class is planted for every tier it makes sense for, that
the compiler places the sets in the routines the cases are named after, and that the host mirrors, given a POINTER INTO the
larger buffer and a length, agree with the reference of the window's bytes alone.  The GPU side: test_text_bounds_gpu.py."""
from __future__ import annotations

import ctypes
import re
from collections import Counter

import numpy as np
import pytest

import bounds_cases as bc
import confirm_cells as cc
import context_ref
import invert_ref

CASES = bc.NAMES


@pytest.mark.parametrize("name", CASES)
def test_placement(name):
    import aosim_py
    import extsim_py

    c = bc.case(name)
    if c.tier == "always_on":
        pl = aosim_py.placement(c.patterns, c.flags)
        assert pl["tiers"] == [1] * len(c.exprs), pl["tiers"]
        units = {(u["kind"], u["ctx"], u["nw"]) for u in pl["units"]}
        want = {"always_on_free": {("group", False, 1), ("single", False, 1), ("single", False, 2)},
                "always_on_ctx": {("group", True, 1), ("single", True, 1), ("single", True, 2)}}[name]
        assert want <= units, units
        if name == "always_on_ctx":
            assert any(u["kind"] == "scalar" and u["nw"] >= 3 for u in pl["units"]), pl["units"]
        return
    db = extsim_py.Db(c.patterns, c.flags, c.ids(False), mode="plain")
    assert db.h, db.error
    for i, e in enumerate(c.exprs):
        p = db.pattern(i)
        assert p["tier"] == 0 and p["mode"] == e.mode, (e.pattern, p)
        if e.mode == 0:
            assert p["literal_only"] and p["max_len"] == len(e.good), (e.pattern, p)
        if e.mode == 4:
            assert p["nw"] > 32, p
    if name == "literal":
        assert {e.mode for e in c.exprs} == {0, 1, 2, 3}
        assert sorted(len(e.good) for e in c.exprs if e.mode == 0 and e.flags == 14) == [8, 16, 17, 32]
        assert any(e.mode == 0 and e.flags & 1 for e in c.exprs)  # one caseless literal
        assert any(db.pattern(i)["nw"] == 2 for i, e in enumerate(c.exprs) if e.mode == 2)  # two state words with boundary conditions


@pytest.mark.parametrize("name", CASES)
def test_every_window_is_hostile(name):
    c = bc.case(name)
    tame = [c.what(w) for w in c.windows if not bc.is_hostile(name, w)]
    assert not tame, f"{len(tame)} of {len(c.windows)} windows would give the same answer with the leak of their class:\n" + "\n".join(tame[:20])


@pytest.mark.parametrize("name", CASES)
def test_the_text_around_the_windows(name):
    c = bc.case(name)
    assert c.body_end <= bc.MAX_BODY and len(c.data) >= c.body_end + bc.FRAME and b"\0" not in c.data
    for w in c.windows:
        assert w.lo % 16 == 0 and w.lo >= 16 and w.hi <= c.body_end, c.what(w)
        if w.cls == "L2":
            assert chr(c.data[w.lo - 1]).isalnum(), c.what(w)
        if w.cls == "L3":
            assert (c.data[w.lo - 1] == 10) == w.tag.endswith("after_newline"), c.what(w)
        if w.cls == "R3":
            nl = w.hi + {"nl-1": 1, "nl": 0, "nl+1": -1}[w.tag.split("/")[1]]
            assert c.data[nl] == 10, c.what(w)
        if w.cls == "R5":  # hi at the edge, and behind it newlines and complete matches of every expression
            edge, d = w.tag.split(":")[0].split("/")[1][:-2], int(w.tag.split(":")[0][-2:])
            assert (w.hi - w.lo - d) % (bc.ROW if edge == "row" else bc.TILE) == 0, c.what(w)
            nxt = c.line_starts[np.searchsorted(c.line_starts, w.hi)]
            rows, _ = bc.reference(name, nxt, w.hi + bc.TILE + bc.ROW)
            assert {int(r[1]) for r in rows} == set(range(len(c.exprs))), c.what(w)
            assert b"\n" in c.data[w.hi:w.hi + bc.ROW - 1] and len(bc.reference(name, nxt, nxt + 2 * bc.ROW)[0]) >= 1, c.what(w)


@pytest.mark.parametrize("name", CASES)
def test_floors(name):
    c = bc.case(name)
    classes = Counter(w.cls for w in c.windows)
    assert set(classes) == set(bc.SENSIBLE[name]), (sorted(classes), bc.SENSIBLE[name])
    assert len(c.windows) >= 60, len(c.windows)
    assert sum(len(bc.window_reference(name, w)[0]) for w in c.windows) >= 200
    edges = {w.tag.split(":")[0] for w in c.windows if w.cls == "R5"}
    assert edges == {f"R5/{e}{d:+d}" for e in ("row", "tile") for d in (-1, 0, 1)}, edges
    assert {w.tag.split("/")[1] for w in c.windows if w.cls == "R3"} == {"nl-1", "nl", "nl+1"}
    if name == "literal":
        for n in (8, 16, 17, 32):  # the 16- and 32-byte compare paths and the byte-compare tail of literal_occurs
            got = {(w.hi - w.lo) % 16 for w in c.windows if w.tag == f"R1/lit{n}"}
            assert got == set(range(16)), (n, sorted(got))
        assert any(w.cls == "R1" and c.exprs[w.expr].flags & 1 for w in c.windows)
        assert any(w.tag == "R2/singlematch" for w in c.windows)
        assert {w.tag for w in c.windows if w.cls == "L2"} == {"L2/^", "L2/\\b", "L2/\\B"}
    if c.tier == "always_on":
        assert any(w.cls == "L4" for w in c.windows)
    if name == "always_on_free":
        assert {"L4/@_before_lo", "L4/digits_before_lo"} <= {w.tag for w in c.windows}


def _view(host: bytearray, lo: int, hi: int):
    """data[lo:hi] as a pointer into the larger buffer: the mirror sees the real neighbourhood, as the GPU does."""
    return (ctypes.c_char * (hi - lo)).from_buffer(host, lo)


@pytest.mark.parametrize("name", CASES)
def test_host_pipeline_mirror_on_windows(name):
    import hgsim_py

    c = bc.case(name)
    host = bytearray(c.data)
    bad = []
    for shared in (False, True):
        db = hgsim_py.Db(c.patterns, c.flags, c.ids(shared))
        assert db.ok(), db.error
        for w in c.windows:
            for bs in bc.SIZES:
                want, nlines = bc.window_reference(name, w, bs, shared)
                hits, stats = db.scan(_view(host, w.lo, w.hi), buffer_size=bs)
                got = cc.sort_hits(hits)
                if stats["pieces"] != nlines:
                    bad.append(f"{c.what(w)} buffer_size {bs}: {stats['pieces']} pieces, want {nlines}")
                if got.shape != want.shape or not (got == want).all():
                    bad.append(f"buffer_size {bs} {'one id' if shared else 'distinct ids'}: {bc.diff_report(c, w, got, want)}")
    tags = sorted(set(re.findall(r" mod 16\) (\S+) ", "\n".join(bad))))
    assert not bad, f"{len(bad)} window scans of the host mirror differ from the reference of the window's own bytes; class tags {tags}\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("name", CASES)
def test_invert_and_context_replays_on_windows(name):
    """The host replays of the invert and context stages (hg_invert.h, hg_context.h) walk the text themselves: pieces, their
    trimmed lengths and the last unterminated piece.  On a pointer into the larger buffer they must stop at hi."""
    c = bc.case(name)
    host = bytearray(c.data)
    bad = []
    for w in c.windows:
        if w.base_cls not in ("R3", "L3", "R2") and w.cls != "R5":
            continue
        for bs in bc.SIZES:
            rows, nlines = bc.window_reference(name, w, bs)
            lines = sorted(int(r[0]) for r in rows)
            data = c.data[w.lo:w.hi]
            got, n_pieces = invert_ref.replay(_view(host, w.lo, w.hi), bc.TILE, bs, lines)
            if got != invert_ref.expected(data, bs, lines) or n_pieces != nlines:
                bad.append(f"invert buffer_size {bs}: {c.what(w)}")
            got = context_ref.replay(_view(host, w.lo, w.hi), bc.TILE, bs, lines, 2, 3, tail=True)
            want = context_ref.expected(data, bs, lines, 2, 3, tail=True)
            if (got[0], got[1], got[2]) != want or got[3] != nlines:
                bad.append(f"context buffer_size {bs}: {c.what(w)}")
    assert not bad, f"{len(bad)} replays differ:\n" + "\n".join(bad[:12])


MIRROR_CLASSES = ("L1", "L2", "L3", "L4", "R2", "R3")
MIN_LENGTHS = {"literal": {"needle_sa_[0-9]+x": 13, "needle_ga_[0-9]*": 12}, "always_on_free": {"[0-9]+x": 4, "[a-z]+@[a-z]+": 8}}
SMALL = tuple(n for n in CASES if n != "huge")  # (start of match, min_length and parts are not offered above HG_MAX_NODES)


def _mirror_windows(c, limit=700):
    return [w for w in c.windows if w.cls in MIRROR_CLASSES and w.hi - w.lo <= limit]


def _pieces_in_place(c, w):
    """(offset in the base text, bytes) of the window's pieces: each has its real neighbours on both sides in the larger
    buffer, the first and the last those the window's class is about."""
    return [(w.lo + a, p) for a, p in invert_ref.pieces(c.data[w.lo:w.hi], bc.DEFAULT_BS) if p]


@pytest.mark.parametrize("name", SMALL)
def test_piece_mirrors_on_windows(name):
    """The mirrors that take one piece as (pointer, length): start of match (somsim: hg_nfa_scan and the walk of hg_som.h),
    min_length (minlensim) and matched parts (partssim: hg_parts.h), given the window's pieces where they lie in the
    larger buffer, against the brute-force references of the piece's bytes alone."""
    import minlensim_py
    import parts_ref
    import partssim_py
    import somsim_py

    c = bc.case(name)
    host = bytearray(c.data)
    ids = c.ids(False)
    som_flags = [(f & ~8) | somsim_py.SOM for f in c.flags]
    som = somsim_py.Db(c.patterns, som_flags, ids)
    parts = partssim_py.Db(c.patterns, c.flags, ids)
    assert som.ok() and parts.ok() and parts.refusal() is None
    need = [MIN_LENGTHS.get(name, {}).get(p) for p in c.patterns]
    minlen = minlensim_py.Db(c.patterns, c.flags, ids, minlensim_py.exts_for(need)) if any(need) else None
    bad, seen, checked = [], set(), 0
    for w in _mirror_windows(c):
        for at, piece in _pieces_in_place(c, w):
            if (at, len(piece)) in seen:
                continue
            seen.add((at, len(piece)))
            view = _view(host, at, at + len(piece))
            want = minlensim_py.expected_piece(c.patterns, som_flags, ids, [None] * len(ids), piece)  # (id, to, from), brute force
            got = som.piece(view)
            checked += len(want)
            if [r[:3] for r in got] != want:
                bad.append(f"{c.what(w)}: somsim piece at {at} ({len(piece)} bytes): {[r[:3] for r in got][:4]}, want {want[:4]}")
            for rid, to, frm, pattern in got:
                brute = somsim_py.start_by_brute_force(c.patterns[pattern], c.flags[pattern], piece, to)
                if som.start(pattern, view, to) != brute:
                    bad.append(f"{c.what(w)}: somsim start of {(pattern, to)} at {at}: {som.start(pattern, view, to)}, want {brute}")
            if parts.piece(view) != parts_ref.piece_parts(c.patterns, c.flags, piece):
                bad.append(f"{c.what(w)}: partssim piece at {at} ({len(piece)} bytes)")
            if minlen is not None:
                want = minlensim_py.expected_piece(c.patterns, c.flags, ids, need, piece)
                if [r[:2] for r in minlen.piece(view)[0]] != [r[:2] for r in want]:
                    bad.append(f"{c.what(w)}: minlensim piece at {at} ({len(piece)} bytes)")
    assert checked >= 100, checked
    tags = sorted(set(re.findall(r" mod 16\) (\S+) ", "\n".join(bad))))
    assert not bad, f"{len(bad)} pieces differ from the reference of the piece's own bytes; class tags {tags}\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("name", CASES)
def test_block_mirrors_on_windows(name):
    """The mirrors of Face A's block scan (flowsim, flowsomsim, batchsim: hg_nfa_scan over one block as (pointer, length)),
    given the window where it lies in the larger buffer, against the block reference of the window's bytes."""
    import batchsim_py
    import flowsim_py
    import flowsomsim_py
    import somsim_py

    c = bc.case(name)
    host = bytearray(c.data)
    every = [f & 7 for f in c.flags]  # every end of every expression: the raw ends the delivery rules start from
    flow, batch = flowsim_py.Db(c.patterns, every), batchsim_py.Db(c.patterns, every)
    assert flow.h and batch.h, (flow.error, batch.error)
    fsom = None
    if name != "huge":
        fsom = flowsomsim_py.Db(c.patterns, [f | somsim_py.SOM for f in every])
        assert fsom.h, fsom.error
    bad, total = [], 0
    for w in _mirror_windows(c, limit=6000):
        data = c.data[w.lo:w.hi]
        view = _view(host, w.lo, w.hi)
        want = sorted(bc.block_reference(c, data, every))
        total += len(want)
        for label, got in (("flowsim", flow.block(view)), ("batchsim", batch.block(view))):
            if sorted(set(got)) != want:
                bad.append(f"{c.what(w)}: {label} block: {len(got)} ends, want {len(want)}")
        if fsom is not None and w.hi - w.lo <= 700:
            if sorted(fsom.block(view)) != sorted(bc.block_reference(c, data, every, som=True)):
                bad.append(f"{c.what(w)}: flowsomsim block")
    assert total >= (30 if name == "huge" else 200), total
    tags = sorted(set(re.findall(r" mod 16\) (\S+) ", "\n".join(bad))))
    assert not bad, f"{len(bad)} block scans differ from the reference of the window's own bytes; class tags {tags}\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("name", CASES)
def test_gather_and_segment_replays_on_windows(name):
    """The host replays that read the text through records: the gather stage (hg_gather.h: bodies copied in aligned dwords,
    every read checked against nbytes rounded up to 4), the segment stage (hg_segments.h walks the pack's pieces) and the
    per-file parts (hg_segparts.h), on a pointer into the larger buffer."""
    import gather_ref
    import parts_ref
    import segments_ref as sr
    import segpartssim_py

    c = bc.case(name)
    host = bytearray(c.data)
    flags = gather_ref.CONTEXT | gather_ref.TERMINATE | gather_ref.NUMBER
    segparts = segpartssim_py.Db(c.patterns, c.flags) if name != "huge" else None
    bad = []
    for w in _mirror_windows(c, limit=6000):
        data = c.data[w.lo:w.hi]
        view = _view(host, w.lo, w.hi)
        rows, _ = bc.window_reference(name, w)
        main = [tuple(int(x) for x in r) for r in rows]
        lines = sorted({r[0] for r in main})
        ctx, _, _ = context_ref.expected(data, bc.DEFAULT_BS, lines, 2, 3, tail=True)
        for tile in (16, 64):
            got = gather_ref.replay(view, tile, main, ctx, flags)
            want, _ = gather_ref.expected(data, bc.DEFAULT_BS, lines, flags, context=(2, 3), tail=True)
            if got["entries"] != want:
                bad.append(f"{c.what(w)}: gather replay, spans of {tile} bytes")
        starts, ends = bc.files_of(c, w)
        per_file = [bc.reference(name, w.lo + a, w.lo + z) for a, z in zip(starts, ends)]
        rep = sr.replay(view, bc.TILE, bc.DEFAULT_BS, main, starts, ends)
        first = rep["first_record"]
        for s, (frows, nlines) in enumerate(per_file):
            mine = sorted(rep["records"][first[s]:first[s + 1]])
            if mine != sorted(tuple(int(x) for x in r) for r in frows) or rep["n_lines"][s] != nlines:
                bad.append(f"{c.what(w)}: segment replay, file {s} of {list(zip(starts, ends))}")
        if segparts is not None and w.hi - w.lo <= 700:
            prow, pseg, pfirst = segparts.run(view, rep["records"], rep["segment"], starts, first)
            for s, ((frows, _), a, z) in enumerate(zip(per_file, starts, ends)):
                want = parts_ref.expected(data[a:z], bc.DEFAULT_BS, c.patterns, c.flags, {int(r[0]) for r in frows})
                if [tuple(int(x) for x in r) for r in prow[pfirst[s]:pfirst[s + 1]]] != want:
                    bad.append(f"{c.what(w)}: segment parts replay, file {s}")
    tags = sorted(set(re.findall(r" mod 16\) (\S+) ", "\n".join(bad))))
    assert not bad, f"{len(bad)} replays differ from the reference of the window's own bytes; class tags {tags}\n" + "\n".join(bad[:12])
