"""The huge-automaton cells (huge_cells.py) are sound, without a GPU: hugesim_py places every expression in the routine of
hg_huge.hip its cell names, every routine label, both condition kinds and every geometry class is present, the reference
(oracle + piece geometry) reports every planted hit and stays silent on every planted miss, the host replay of the pipeline
(hg_huge_scan_slice: it checks the tables and the cells, not the device routines) equals the reference on every text, and the
reference's end offsets agree with a Python `re` brute force on the planted lines that `re` can run.  The GPU side:
test_huge_cells_gpu.py."""
from __future__ import annotations

import re

import numpy as np
import pytest

import hgsim_py
import huge_cells as hc
import hugesim_py
import invert_ref
import regex_gen

BRUTE_MAX_LINE = 12000  # planted lines up to this many bytes meet Python `re`
BRUTE_SHORT = 300  # ... up to this many, regex_gen.ends_by_brute_force (every start against every end)
BRUTE_SHAPES = ("walk", "dense", "loop")  # what `re` runs in reasonable time (the backtracking of (ab?c?){n} and (a?){n}b does not)


def test_every_routine_size_and_condition_kind_is_present():
    have = {}  # routine -> {(nw, ctxfree)}
    for cell in hc.CELLS:
        pl = hc.compiled(cell.name)
        for p in pl["exprs"].values():
            have.setdefault(p["routine"], set()).add((p["nw"], p["ctxfree"]))
    sizes = {r: {nw for nw, _ in v} for r, v in have.items()}
    assert 64 in sizes["reg1"] and {65, 128} <= sizes["reg2"] and {129, 256} <= sizes["reg4"] and 257 in sizes["lds_staged"], sizes
    assert any(nw <= 256 for nw in sizes["lds_l2"]) and any(nw > 256 for nw in sizes["lds_l2"]), sizes
    for r in ("reg2", "reg4", "lds_staged", "lds_l2"):
        assert {c for _, c in have[r]} == {True, False}, (r, have[r])
    shapes = {e.shape for c in hc.CELLS for e in c.exprs}
    assert shapes >= {"walk", "dense", "exc", "loop", "init", "idle"}
    for name in ("ao_restage", "cf_restage"):  # three routines in one set, and single beside all-matches
        cell = hc.BY_NAME[name]
        assert {e.routine for e in cell.exprs} >= {"reg1", "reg4", "lds_staged"} and {e.flags & 8 for e in cell.exprs} == {0, 8}
    assert hc.compiled("ao_restage")["huge_max_nw"] == 12288


@pytest.mark.parametrize("cell", hc.CELLS, ids=lambda c: c.name)
def test_placement(cell):
    """A cell whose expression lands in another routine fails here: it is not quietly re-labelled."""
    pl = hc.compiled(cell.name)
    assert hc.placement_errors(cell, pl) == []
    assert pl["nhuge"] == len(cell.exprs)
    assert pl["nslow_huge"] == sum(p["tier"] == 1 for p in pl["exprs"].values())
    assert pl["cap"] == pl["huge_stage_words"]  # (no set of the suite reaches clamp_stage: see the module)
    assert all(e.short or e.samples for e in cell.exprs) and cell.exprs[cell.short].short[0]


def test_clamp_is_out_of_reach():
    """clamp_stage cuts the cap only above 14304 state words; the program-size bound stops at 12500."""
    assert hugesim_py.clamp_stage(14304, hugesim_py.STAGE_MAX) == hugesim_py.STAGE_MAX > hugesim_py.clamp_stage(14305, hugesim_py.STAGE_MAX)
    assert 400000 // 32 < 14304
    assert hugesim_py.clamp_stage(12288, hugesim_py.STAGE_MAX) == hugesim_py.STAGE_MAX
    assert not hgsim_py.Db([hc.MONSTER + "b" * (400001 - 12 * 32767)]).ok()


def test_excluded_classes_are_named_with_a_reason():
    for cell in hc.CELLS:
        assert set(cell.excluded) <= set(hc.CLASSES) and all(isinstance(w, str) and w for w in cell.excluded.values()), cell.name
        assert ("always_on" in cell.excluded) == (cell.tier == 0) and ("confirm" in cell.excluded) == (cell.tier == 1)
    for cls in hc.CLASSES:  # no class is excluded everywhere
        assert any(cls not in c.excluded for c in hc.CELLS), cls


REQUIRED = {
    "word": ("word/n", "word/n-1:miss", "word/n+1:miss", "word/headless:miss"),
    "slab": ("slab/crosses_63-64", "slab/dies_behind_63-64:miss"),
    "exc": ("exc/beyond_live_words", "exc/higher_slab", "exc/higher_slab:miss"),
    "chunk": tuple(f"chunk/piece_of_{n}_bytes" for n in (63, 64, 65, 127, 128, 129)) + ("chunk/piece_of_1_bytes:miss", "chunk/piece_of_2_bytes:miss", "chunk/match_ends_on_byte_64",
                                                                                         "chunk/match_ends_on_byte_65", "chunk/ends_piece_of_64", "chunk/ends_piece_of_128", "chunk/start_residue_63"),
    "always_on": ("always_on/line_start_residue", "always_on/starts_in_one_group", "always_on/line_at_first_byte_of_tile", "always_on/carried_over_one_tile_edge",
                  "always_on/carried_over_two_tile_edges", "always_on/newline_first_byte_of_tile", "always_on/newline_last_byte_of_tile", "always_on/no_final_newline_last_tile_partial",
                  "always_on/one_byte_text:miss", "always_on/nul_leading", "always_on/nul_ends_the_scanned_bytes:miss", "always_on/piece_of_nuls:miss", "always_on/nuls_then_newline:miss",
                  "always_on/break_match_on_second_piece", "always_on/break_match_on_third_piece", "always_on/break_inside_match:miss", "always_on/break_one_byte_behind_match_end",
                  "always_on/break_at_match_end", "always_on/break_one_byte_before_match_end:miss"),
    "confirm": tuple(f"confirm/literal_{n}_behind_line_start" for n in (1, 63, 64, 65, 200)) + ("confirm/line_from_previous_tile", "confirm/literal_several_times",
                                                                                                "confirm/literal_overlaps_itself", "confirm/piece_k_gt_0"),
}
CTX_KINDS = ("\\b_left", "\\b_right", "\\B_left", "\\B_right", "^", "$")


@pytest.mark.parametrize("cell", hc.CELLS, ids=lambda c: c.name)
def test_classes_are_planted_and_the_reference_judges_them(cell, record_property):
    """Every class the cell does not exclude is planted; every planted hit is in the reference, every planted miss absent."""
    texts = hc.cell_texts(cell.name)
    tags, wrong, reports = {}, [], 0
    residues = set()
    for ti, text in enumerate(texts):
        assert len(text.data) <= hc.MAX_TEXT
        for bs in text.sizes:
            want, _, oracle_rows = hc.cell_reference(cell.name, ti, bs, False)
            assert want.shape == oracle_rows.shape and (want == oracle_rows).all(), (text.label, bs)  # the oracle's own geometry is the pieces'
            reports += len(want)
            for c, expect, reported in hc.judged(cell, text, want):
                n = tags.setdefault(c.tag, [0, 0])
                n[reported] += 1
                if expect != "any" and reported != (expect == "hit") and (bs == text.sizes[0] or c.tag.startswith("confirm/piece_k")):
                    wrong.append((text.label, bs, c.tag, c.expr, c.lo, "reported" if reported else "silent"))
                if c.tag == "always_on/line_start_residue" and reported:
                    residues.add(c.lo % 64)
    assert not wrong, wrong[:10]
    for cls in hc.CLASSES:
        if cls == "block":
            assert cls in cell.excluded or len(hc.cell_blocks(cell.name)) >= 2
            continue
        planted = [t for t in tags if t.startswith(cls + "/")]
        assert (cls in cell.excluded) != bool(planted) or cls in ("slab", "exc", "ctx", "word"), (cls, planted[:3])
        if cls in cell.excluded:
            continue
        assert any(hc.expectation(t) == "hit" for t in planted) and any(hc.expectation(t) == "miss" for t in planted), (cls, planted)
        walks = any(e.shape == "walk" and e.ctxfree for e in cell.exprs)
        for tag in REQUIRED.get(cls, ()) if cls != "word" or walks else ("word/all_live", "word/all_live:miss"):
            assert tag in tags, (cls, tag)
    if "ctx" not in cell.excluded:  # both sides of \b and \B, ^ and $, each with a hit and a miss
        for kind in CTX_KINDS:
            assert any(t.startswith("ctx/") and kind in t and hc.expectation(t) == "hit" for t in tags), kind
            assert any(t.startswith("ctx/") and kind in t and hc.expectation(t) == "miss" for t in tags), kind
        assert any("at_the_end_without_newline" in t for t in tags)
    if cell.tier == 1:
        assert residues == set(range(64)), sorted(set(range(64)) - residues)
        assert {t.sizes[0] - 1 for t in texts if t.label.startswith("break")} == set(hc.BREAK_BS1)
    if cell.name == "ao_reg4_256":
        assert all(f"slab/exc_in_slab{k}" in tags and f"slab/crosses_{64 * k - 1}-{64 * k}" in tags for k in (1, 2, 3))
    if cell.name == "ao_exc":
        assert {"exc/heavy", "exc/lower_word_3", "exc/lower_word_1:miss", "word/every_init"} <= set(tags)
    record_property("reports_distinct_ids", reports)
    assert 2 * reports >= cell.floor > 0, (reports, cell.floor)  # (the GPU test's floor counts both id modes; SINGLEMATCH on one id may merge rows)


@pytest.mark.parametrize("cell", hc.CELLS, ids=lambda c: c.name)
def test_host_mirror_equals_the_reference(cell):
    """hgsim_py.Db.scan replays the pipeline with hg_huge_scan_slice: all five columns, distinct ids and one id."""
    texts = hc.cell_texts(cell.name)
    for shared in (False, True):
        db = hgsim_py.Db(cell.patterns, cell.flags, cell.ids(shared))
        assert db.ok(), db.error
        for ti, text in enumerate(texts):
            for bs in text.sizes:
                want, nlines, _ = hc.cell_reference(cell.name, ti, bs, shared)
                got, stats = db.scan(text.data, bs)
                got = hc.sort_hits(got)
                assert stats["pieces"] == nlines
                assert got.shape == want.shape and (got == want).all(), f"{cell.name} {text.label} bs {bs} shared {shared}: {hc.diff_report(text, got, want)}"


@pytest.mark.parametrize("cell", hc.CELLS, ids=lambda c: c.name)
def test_reference_agrees_with_brute_force(cell):
    """On the planted lines of the sample and chunk texts, for the expressions Python `re` can express and run."""
    texts = hc.cell_texts(cell.name)
    checked = 0
    for ti, text in enumerate(texts):
        if not (text.label.startswith("samples") or text.label == "chunk"):
            continue
        want, _, _ = hc.cell_reference(cell.name, ti, hc.DEFAULT_BS, False)
        by_line = {}
        for line, rid, to, _, _ in want.tolist():
            by_line.setdefault((line, rid), []).append(to)
        pieces = invert_ref.pieces(text.data, hc.DEFAULT_BS)
        starts = {a: ln for ln, (a, _) in enumerate(pieces)}
        for c in text.cases:
            e = cell.exprs[c.expr]
            if e.shape not in BRUTE_SHAPES or c.hi - c.lo > BRUTE_MAX_LINE or c.lo not in starts:
                continue
            ln = starts[c.lo]
            piece = pieces[ln][1]
            if b"\0" in piece:
                continue
            if len(piece) <= BRUTE_SHORT:
                ends = regex_gen.ends_by_brute_force(e.pattern, e.flags, piece)
            elif e.shape == "walk":  # every match of head [a-z]{n} tail has one length: one end per start, which a lookahead finds
                ends = sorted({m.end(1) for m in re.finditer(b"(?=(" + e.pattern.encode() + b"))", piece, regex_gen.py_flags(e.flags))})
            else:
                continue
            assert sorted(by_line.get((ln, c.expr), [])) == (ends[:1] if e.flags & 8 else ends), (text.label, c.tag, c.expr)
            checked += 1
    assert checked >= 20, checked
