"""The cells of the start-of-match and match-length walks on the MI355X: hg_som_kernel and hg_minlen_kernel (hg_som.hip) on
every cell of som_cells.py.  Every expectation is som_cells.reference: Python `re`, nothing of hg_som.h.  One scan per text; the
complete list of (line, id, to, from) from hits() and hit_starts() must equal the reference, and a difference is named by cell.
Texts sit at the end of a guarded arena: a read past them faults."""
from __future__ import annotations

import pytest

import som_cells as sc
from minlensim_py import exts_for

pytestmark = pytest.mark.gpu

_scanners: dict = {}
_blocks: dict = {}


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 20)
    yield a
    _scanners.clear()  # (before the interpreter takes the module's globals away)
    _blocks.clear()
    a.free()


def scanner(name):
    from hypergrep_amd import device

    if name not in _scanners:
        d = sc.DBS[name]
        ext = exts_for(d.need) if d.filtering else None
        _scanners[name] = device.Scanner(device.Database(list(d.pats), flags=list(d.flags), ids=list(d.ids), ext=ext), 0)
    return _scanners[name]


def scan(arena, text):
    """One scan of the text: ([(line, id, to, from)], stats)."""
    s = scanner(text.db)
    data = text.data
    st = s.scan(arena.place(data), len(data), buffer_size=text.bs)
    hits, starts = s.hits(), s.hit_starts()
    assert len(hits) == len(starts) == st.n_hits
    return [(h[0], h[1], h[2], int(f)) for h, f in zip(hits, starts)], st


def differences(text, got):
    """The cells of the text whose reports differ from the reference, named."""
    per_cell, whole, _raw = sc.reference(text)
    if got == whole:
        return []
    cell_of = {idx: c.name for idx, _a, _p, c in sc.layout(text)}
    mine = {c.name: [] for c in text.cells}
    stray = []
    for r in got:
        (mine[cell_of[r[0]]] if r[0] in cell_of else stray).append(r)
    out = [f"{name}: got {mine[name][:6]} want {want[:6]}" for name, want in per_cell.items() if mine[name] != want]
    if stray:
        out.append(f"{text.name}: reports on lines of no piece {stray[:6]}")
    if not out:
        out.append(f"{text.name}: the same reports in another order")
    return out


def check_text(arena, text):
    got, st = scan(arena, text)
    bad = differences(text, got)
    raw = sc.reference(text)[2]
    # n_raw_hits counts reports before de-duplication.  The databases of group H raise every (expression, end) once, so the
    # count is the reference's; group I's shared ids hold literal-anchored expressions, which may raise a report more than once
    # (I/share_ml: 38 for 36 distinct), so there it is a lower bound
    d = sc.DBS[text.db]
    exact = not any(f & sc.SOM for f in d.flags)
    if d.filtering and (st.n_raw_hits != raw if exact else st.n_raw_hits < raw):
        bad.append(f"{text.name}: n_raw_hits {st.n_raw_hits} for {raw}")
    return bad


@pytest.mark.parametrize("group", [g for g in sc.GROUPS if g != "Hc"])
def test_cells(arena, group):
    failed = []
    for text in sc.GROUPS[group]:
        failed += check_text(arena, text)
    cells = sum(len(t.cells) for t in sc.GROUPS[group])
    assert not failed, f"{len(failed)} of {cells} cells failed:\n" + "\n".join(failed[:12])


@pytest.mark.parametrize("which", list(sc.COMPACT_SETS) + ["one of 65"])
def test_compaction(arena, which):
    """hg_minlen_kernel's ballot, atomic and rank: raw reports of one filtering expression, one per line, with the kept set
    the text's name states; n_raw_hits and the whole delivered list."""
    texts = [t for t in sc.GROUPS["Hc"] if (f", {which} kept" in t.name) or (which == "one of 65" and "only" in t.name)]
    assert len(texts) == (65 if which == "one of 65" else len(sc.COMPACT_COUNTS))
    failed = []
    for text in texts:
        got, st = scan(arena, text)
        _per, whole, raw = sc.reference(text)
        if got != whole or st.n_raw_hits != raw:
            failed.append(f"{text.name}: n_raw_hits {st.n_raw_hits} for {raw}, lines {[r[0] for r in got][:12]} for {[r[0] for r in whole][:12]}")
    assert not failed, f"{len(failed)} of {len(texts)} texts failed:\n" + "\n".join(failed[:12])


def block(name):
    from hypergrep_amd import device

    if name not in _blocks:
        d = sc.DBS[name]
        _blocks[name] = device.BlockDatabase(list(d.pats), list(d.flags), list(d.ids), exts_for(d.need) if d.filtering else None)
    return _blocks[name]


def test_face_a_block_mode(arena):
    """hs_scan, one planted line per call: every cell of group G and every FACE_A_STRIDE-th cell of group A.  The expressions of
    both groups have no assertions, so a block's reports are the line's: (id, from, to) in (to, id) order."""
    failed, n = [], 0
    for group, stride in (("A", sc.FACE_A_STRIDE), ("G", 1)):
        for text in sc.GROUPS[group]:
            d = sc.DBS[text.db]
            for c in text.cells[::stride]:
                line = c.data[c.planted:]
                want = sorted(((rid, frm, to) for rid, to, frm in sc.piece_reports(d, line)), key=lambda r: (r[2], r[0]))
                got = block(text.db).scan(line)
                n += 1
                if got != want:
                    failed.append(f"{c.name}: got {got[:6]} want {want[:6]}")
    assert n > 200
    assert not failed, f"{len(failed)} of {n} cells failed:\n" + "\n".join(failed[:12])


def test_scanner_reuse_and_repeat(arena):
    """One scanner over two different texts and back, and the same text twice: every scan gives the reference's list."""
    first, second = sc.GROUPS["B"][0], [t for t in sc.GROUPS["B"] if t.db == "start"][1]
    assert first.db == second.db == "start" and first.data != second.data
    runs = []
    for text in (first, second, first, first):
        got, _st = scan(arena, text)
        assert not differences(text, got), differences(text, got)[:6]
        runs.append(got)
    assert runs[0] == runs[2] == runs[3] and runs[0] != runs[1]
    ml_a, ml_b = sc.GROUPS["H"][0], [t for t in sc.GROUPS["Hc"] if t.name == "H/compaction 129 raw, every other kept"][0]
    small = sc.compact_text("reuse: three raw reports", [True, False, True])
    for text in (ml_b, small, ml_b, ml_b):  # the match-length pass's arrays shrink and grow on one scanner
        assert not check_text(arena, text), text.name
    assert not check_text(arena, ml_a)
