"""The confirm cells (confirm_cells.py) are sound, without a GPU: the compiler places every cell's expressions in the confirm
routine the cell names, the reference (oracle + piece geometry) agrees with a Python `re` brute force on every short planted
piece, the host replay of the pipeline equals the reference on every text, and every geometry class is planted in numbers
that the reference itself confirms.  The GPU side: test_confirm_cells_gpu.py."""
from __future__ import annotations

import numpy as np
import pytest

import confirm_cells as cc
import hgsim_py
import invert_ref
import regex_gen

BRUTE_MAX = 160  # pieces up to this many bytes meet the brute force; longer ones rely on the oracle (pinned by the same brute force in test_oracle.py)


def _setup(cell):
    info = cc.compiled(cell.name)
    leads = tuple(p["lit_lead"] for p in info)
    return info, leads, cc.cell_texts(cell.name, leads)


@pytest.mark.parametrize("cell", cc.CELLS, ids=lambda c: c.name)
def test_placement(cell):
    """A cell whose expression lands in another routine fails here: it is not quietly re-labelled."""
    info = cc.compiled(cell.name)
    assert 2 <= len(cell.exprs) <= 4 and len({e.lit.lower() for e in cell.exprs}) == len(cell.exprs)
    assert cc.placement_errors(cell, info) == []
    if cell.name == "simple_bounded":  # q in an earlier 16-byte chunk than fs, and in the same one
        assert {e.lead for e in cell.exprs} >= {"lt16", "ge17"}
    if cell.name == "ctx1":  # bounded and unbounded lead, assertions on both sides
        assert {e.lead for e in cell.exprs} >= {"lt16", "unbounded"}
    if cell.modes:
        assert sorted(p["mode"] for p in info) == [0, 1, 2, 3]
    if cell.nw == "huge":  # which routine of hg_huge.hip runs each expression
        import hugesim_py

        pl = hugesim_py.placement(cell.patterns, cell.flags, cell.ids(False))
        assert tuple(pl["exprs"][i]["routine"] for i in range(len(cell.exprs))) == cc.HUGE_ROUTINES[cell.name], pl["exprs"]
        assert [pl["exprs"][i]["ctxfree"] for i in range(len(cell.exprs))] == [True, False]


def test_excluded_classes_name_known_tags():
    known = set(cc.REQUIRED_TAGS) | set(cc.CLASSES) | {"q_sweep"}
    for cell in cc.CELLS:
        assert set(cell.excluded) <= known, (cell.name, set(cell.excluded) - known)
        assert all(isinstance(why, str) and why for why in cell.excluded.values())


_BRUTE: dict = {}


def _brute_reports(cell, piece: bytes):
    """{(expression, to)} of one trimmed piece by Python `re`: every end, or the smallest one under SINGLEMATCH.  An expression
    whose literal (a mandatory part of every cell expression) is not in the piece is not run: it has no match there."""
    out = set()
    for i, e in enumerate(cell.exprs):
        hay, lit = (piece.lower(), e.lit.lower()) if e.flags & 1 else (piece, e.lit)
        if lit not in hay:
            continue
        key = (e.pattern, e.flags, piece)
        if key not in _BRUTE:
            _BRUTE[key] = regex_gen.ends_by_brute_force(e.pattern, e.flags, piece)
        ends = _BRUTE[key]
        out |= {(i, t) for t in (ends[:1] if e.flags & 8 else ends)}
    return out


@pytest.mark.parametrize("cell", cc.CELLS, ids=lambda c: c.name)
def test_reference_agrees_with_brute_force_and_itself(cell):
    _, leads, texts = _setup(cell)
    checked = set()
    for ti, text in enumerate(texts):
        for bs in text.sizes:
            want, nlines, oracle_rows = cc.cell_reference(cell.name, leads, ti, bs, False)
            # the oracle's own (line_off, line_len) are the pieces' (start, len)
            assert want.shape == oracle_rows.shape and (want == oracle_rows).all(), (text.label, bs)
            by_line = {}
            for line, rid, to, _, _ in want.tolist():
                by_line.setdefault(line, set()).add((rid, to))
            planted = np.zeros(len(text.data) + 1, dtype=bool)
            for c in text.cases:
                planted[c.lo:c.hi] = True
            for line, (a, piece) in enumerate(invert_ref.pieces(text.data, bs)):
                if not piece or len(piece) > BRUTE_MAX or not planted[a] or piece in checked:
                    continue
                checked.add(piece)
                assert by_line.get(line, set()) == _brute_reports(cell, piece), (text.label, bs, line, piece)
    assert len(checked) >= 60, len(checked)


@pytest.mark.parametrize("cell", cc.CELLS, ids=lambda c: c.name)
def test_host_mirror_equals_the_reference(cell):
    """hgsim_py.Db.scan replays the pipeline with the host mirrors of the confirm routines (hg_core.h): all five columns."""
    _, leads, texts = _setup(cell)
    for shared in (False, True):
        db = hgsim_py.Db(cell.patterns, cell.flags, cell.ids(shared))
        assert db.ok(), db.error
        for ti, text in enumerate(texts):
            for bs in text.sizes:
                want, _, _ = cc.cell_reference(cell.name, leads, ti, bs, shared)
                got = cc.sort_hits(db.scan(text.data, bs)[0])
                assert got.shape == want.shape and (got == want).all(), f"{cell.name} {text.label} bs {bs} shared {shared}: {cc.diff_report(text, got, want)}"


# tags whose cases must, in every cell that plants them, hold at least one that the reference reports / one that it does not
MUST_REPORT = (
    "align/hit", "tile/line_from_previous_tile", "tile/line_from_two_tiles_back", "tile/line_at_tile_start", "tile/newline_first_byte", "tile/literal_straddles",
    "tile/lead_straddles", "edge/line_at_byte_0", "edge/match_ends_the_text", "nul/leading", "nul/leading17", "nul/leading_in_window", "nul/line_of_nuls_before",
    "break/later_piece", "break/later_piece_leading_nuls", "break/in_prefix", "break/right_after_match", "break/at_piece_start", "break/third_piece",
    "multi/fail_then_match", "multi/overlap", "multi/twice", "multi/far_start", "multi/other_expression",
)
MUST_BE_SILENT = (
    "align/miss", "tile/literal_straddles:miss", "edge/near_miss_ends_the_text", "edge/literal_cut_by_the_end", "nul/blocked", "nul/blocked_far", "nul/in_lead",
    "break/inside_literal", "break/later_piece_nul_blocks", "multi/all_miss",
)
# what the forced-break texts of EVERY buffer size hold (the tile-sized and larger ones included), and how each must end
BREAK_REPORTED = ("break/later_piece", "break/later_piece_leading_nuls", "break/in_prefix", "break/right_after_match", "break/at_piece_start", "break/third_piece")
BREAK_SILENT = ("break/inside_literal", "break/later_piece_nul_blocks", "break/later_piece:miss")
BREAK_PLANTED = BREAK_REPORTED + BREAK_SILENT + ("break/one_byte_before_match_end", "break/one_byte_after_match_end")


@pytest.mark.parametrize("cell", cc.CELLS, ids=lambda c: c.name)
def test_floors(cell):
    """Judged by the reference alone: no test passes by planting nothing."""
    info, leads, texts = _setup(cell)
    planted = {cls: 0 for cls in cc.CLASSES}
    reported = {cls: 0 for cls in cc.CLASSES}
    silent = {cls: 0 for cls in cc.CLASSES}
    by_tag = {}  # tag -> [planted, reported, silent]
    by_break = {bs1: {} for bs1 in cc.BREAK_BS1}  # the same, for the texts of one forced-break size
    longest = {bs1: 0 for bs1 in cc.BREAK_BS1}
    fs_res, q_res, end_res, straddle = set(), set(), set(), set()
    newline_ends = 0
    hits = 0
    for ti, text in enumerate(texts):
        assert 0 < len(text.data) <= cc.MAX_TEXT
        los = [c.lo for c in text.cases]
        assert los == sorted(los) and all(c.lo <= c.line <= c.fs < c.hi for c in text.cases)
        bs1 = text.sizes[0] - 1 if text.label.startswith("break") else None
        for bs in text.sizes:
            want, _, _ = cc.cell_reference(cell.name, leads, ti, bs, False)
            hits += len(want)
            starts, ends = want[:, 3].astype(np.int64), (want[:, 3] + want[:, 2]).astype(np.int64)
            newline_ends += sum(text.data[e - 1] == 10 for e in ends.tolist())
            for c in text.cases:
                cls = c.tag.split("/")[0]
                tag = c.tag.split(":")[0] if c.tag.endswith(":far") else c.tag
                inside = (starts >= c.lo) & (starts < c.hi)
                counts = [by_tag.setdefault(tag, [0, 0, 0])] + ([by_break[bs1].setdefault(tag, [0, 0, 0])] if bs1 is not None else [])
                for n in counts:
                    n[0] += bs == text.sizes[0]
                    n[1 if inside.any() else 2] += 1
                if bs == text.sizes[0]:
                    planted[cls] += 1
                (reported if inside.any() else silent)[cls] += 1
                if bs1 is not None:
                    longest[bs1] = max(longest[bs1], c.hi - c.lo)
                if tag == "tile/literal_straddles" and bs == cc.DEFAULT_BS and inside.any():
                    straddle.add(-c.fs % cc.TILE)  # bytes of the literal in front of the tile edge
                if cls == "align" and bs == cc.DEFAULT_BS and inside.any():
                    fs_res.add(c.fs % 16)
                    end_res |= {int(x) % 16 for x in ends[inside]}
                    lead = leads[c.expr]
                    if 0 < lead < cc.UNBOUNDED and c.fs - c.line > lead:  # (no NUL in these lines: the first scanned byte is the line start)
                        q_res.add((c.fs - lead) % 16)
    tags = set(by_tag)
    for cls in cc.CLASSES:
        assert cls not in cell.excluded
        assert planted[cls] >= 4 and reported[cls] >= 1 and silent[cls] >= 1, (cls, planted[cls], reported[cls], silent[cls])
    for tag in cc.REQUIRED_TAGS:
        assert (tag in tags) != (tag in cell.excluded), (tag, "planted" if tag in tags else "neither planted nor excluded")
    for tag in MUST_REPORT:
        assert tag in cell.excluded or by_tag[tag][1] >= 1, (tag, by_tag[tag])
    for tag in MUST_BE_SILENT:
        assert tag in cell.excluded or by_tag[tag][2] >= 1, (tag, by_tag[tag])
    assert len(straddle) >= 6 and all(0 < x < 24 for x in straddle), straddle  # the literal across a tile edge at six offsets, each one reported
    every = set(range(16))
    assert fs_res == every and end_res == every, (fs_res, end_res)
    if "q_sweep" not in cell.excluded:
        assert q_res == every, q_res
    assert hits >= 300, hits
    if cell.name in ("simple_lead0", "ctx1_nomultiline"):  # matches whose last byte is the line's newline
        assert newline_ends >= 16, newline_ends
    for bs1 in cc.BREAK_BS1:  # no buffer size gets a token check: each holds every kind of break, ending as the kind says
        got = by_break[bs1]
        for tag in BREAK_PLANTED:
            assert tag in cell.excluded or got.get(tag, [0])[0] >= 1, (bs1, tag, "not planted")
        for tag in BREAK_REPORTED:
            assert tag in cell.excluded or got[tag][1] >= 1, (bs1, tag, got[tag])
        for tag in BREAK_SILENT:
            assert tag in cell.excluded or got[tag][2] >= 1, (bs1, tag, got[tag])
        assert longest[bs1] > 2 * bs1, (bs1, longest[bs1])  # a line with an occurrence two breaks in (bs1 20000: 40 KiB)
    assert longest[20000] >= 40000 and min(longest.values()) >= 300


def test_guarded_cases_hold_the_text_edges():
    import gpu_cases

    names = [c[0] for c in gpu_cases.guarded_cases() if c[0].startswith("confirm-")]
    assert 10 <= len(names) <= 16 and {n.split("-")[1] for n in names} == {"ctx1", "simple_bounded", "lit"}, names
