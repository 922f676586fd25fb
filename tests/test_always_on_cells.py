"""The always-on cells (always_on_cells.py) are sound, without a GPU: the compiler and the staging rules place every cell's
expressions in the routine the cell names (aosim_py), the reference (oracle + piece geometry) agrees with a Python `re` brute
force on every short planted piece, the host replay of the pipeline equals the reference on every text, and every geometry
class is planted in numbers that the reference itself confirms, in lean and in careful tiles.  The GPU side:
test_always_on_cells_gpu.py."""
from __future__ import annotations

import re

import numpy as np
import pytest

import always_on_cells as ac
import aosim_py
import hgsim_py
import invert_ref
import regex_gen

BRUTE_MAX = 160  # pieces up to this many bytes meet the brute force; longer ones rely on the oracle (pinned by the same brute force in test_oracle.py)


@pytest.mark.parametrize("cell", ac.CELLS, ids=lambda c: c.name)
def test_placement(cell):
    """A cell whose expression lands in another routine fails here: it is not quietly re-labelled."""
    pl = ac.compiled(cell.name)
    assert ac.placement_errors(cell, pl) == []
    assert max((u["nw"] for u in pl["units"]), default=0) == cell.max_nw
    for e in cell.exprs[: cell.n_always_on]:
        assert len(e.plain) >= 2 and e.bad
    assert len(cell.exprs[0].plain[0]) >= 7  # the sample of the split sweeps: six distinct splits and more
    if cell.name == "group_cf":  # SINGLEMATCH and all-matches members mixed
        u = pl["units"][0]
        assert 0 < u["single_mask"] < (1 << len(u["members"])) - 1 and 3 <= len(u["members"]) <= 8
    if cell.name == "group_ctx_riders":  # members without conditions ride along in a group with conditions
        flat = [aosim_py.placement([e.pattern], [e.flags])["units"][0]["ctx"] for e in cell.exprs]
        assert True in flat and False in flat
    if cell.name == "word2_lean_nexc0":  # the optional nodes 30 and 31: M1, M2 and M3 all have a source whose target is in word 1
        M = pl["units"][0]["M"]
        assert all(any((M[k] >> i) & 1 for i in range(32 - k, 32)) for k in (1, 2, 3)), [hex(m) for m in M]
    if cell.name == "word2_lean_nexc1":  # an exception source below bit 32
        assert pl["units"][0]["src"][0] < 32
    if cell.name == "word2_lean_nexc1_high":  # ... the only one at bit 32: taken from the high word
        assert pl["units"][0]["src"] == (32,)
    if cell.name == "word2_lean_back_edge":  # a source above bit 32 whose follow rest is a node of word 0 that the start state does not enter
        u = pl["units"][0]
        assert u["src"][1] >= 32 and u["F"][1] == 1 << 1, (u["src"], [hex(f) for f in u["F"]])
    if cell.name == "word2_lean_nexc2_skip":  # ... one below and one above it
        assert pl["units"][0]["src"][0] < 32 <= pl["units"][0]["src"][1]
    if cell.name == "word2_lean_nexc2":  # ... and a source above it with a follow rest in both words
        u = pl["units"][0]
        assert any(src >= 32 and f & 0xFFFFFFFF and f >> 32 for src, f in zip(u["src"], u["F"])), (u["src"], [hex(f) for f in u["F"]])
    if cell.name == "two_groups_and_singles":
        assert pl["ngroups"] == 2 and len(pl["units"]) == 4
    if cell.name == "mixed_shared_ids":
        assert {u["kind"] for u in pl["units"]} == {"group", "single", "scalar"} and cell.n_literal == 1


# The rows of the routine table: the cells that cover each, and what always_on_stage and hg_always_on_fast_kernel must decide for
# the cell's unit u (of the first unit of that kind) for the row's routine to be the one that runs.
def _word(ctx, nt=None, shift=False):
    return lambda u: u["kind"] == "single" and u["nw"] == 1 and u["ctx"] == ctx and u["shift_form"] == shift and (nt is None or u["nt"] == nt)


ROUTINES = {
    "always_on_word<false, 1>": (("word_cf_nt1", "word_cf_nl"), _word(False, 1)),
    "always_on_word<false, 2>": (("word_cf_nt2", "word_cf_nt2_unbounded"), _word(False, 2)),
    "always_on_word<false, 3>": (("word_cf_nt3",), _word(False, 3)),
    "always_on_word<false, 4>": (("word_cf_nt4",), _word(False, 4)),
    "always_on_word<false, 0>": (("word_cf_shift_nexc0", "word_cf_shift_nexc1", "word_cf_shift_nexc2"), _word(False, shift=True)),
    "always_on_word<true, 1>": (("word_ctx_nt1", "word_ctx_nl"), _word(True, 1)),
    "always_on_word<true, 2>": (("word_ctx_nt2", "word_ctx_nomultiline"), _word(True, 2)),
    "always_on_word<true, 3>": (("word_ctx_nt3",), _word(True, 3)),
    "always_on_word<true, 4>": (("word_ctx_nt4",), _word(True, 4)),
    "always_on_word<true, 0>": (("word_ctx_shift",), _word(True, shift=True)),
    "group, context-free": (("group_cf", "group_unbounded", "two_groups_and_singles", "mixed_shared_ids"), lambda u: u["kind"] == "group" and not u["ctx"]),
    "group with conditions": (("group_ctx_riders",), lambda u: u["kind"] == "group" and u["ctx"]),
    "always_on_word2 lean": (("word2_lean_nexc0", "word2_lean_nexc1", "word2_lean_nexc1_high", "word2_lean_nexc2_skip", "word2_lean_back_edge", "word2_lean_nexc2", "word2_len64"),
                             lambda u: u["kind"] == "single" and u["nw"] == 2 and u["lean2"] and u["nexc"] <= 2),
    "always_on_segment<2, false>": (("word2_ctx", "word2_noshift", "word2_nl"), lambda u: u["kind"] == "single" and u["nw"] == 2 and not u["lean2"]),
    "hg_always_on_kernel": (("scalar_bounded", "scalar_unbounded"), lambda u: u["kind"] == "scalar" and u["nw"] >= 3),
}


def test_every_routine_has_its_cells():
    """Every cell stands in one row, and its unit is what that row's routine takes (ao_exact_dword, the tile prologue and the
    finish kernel run for every cell of the fast kernel: test_floors holds their classes)."""
    listed = [c for cells, _ in ROUTINES.values() for c in cells]
    assert sorted(listed) == sorted(c.name for c in ac.CELLS)
    for routine, (cells, takes) in ROUTINES.items():
        for name in cells:
            units = ac.compiled(name)["units"]
            kind = "group" if routine.startswith("group") else "scalar" if routine == "hg_always_on_kernel" else "single"
            first = next(u for u in units if u["kind"] == kind and (kind != "single" or len(units) == 1))
            assert takes(first), (routine, name, first)


def test_max_len_65_is_out_of_the_fast_kernel():
    """Why there is no `len65` and no `group_len64` cell: a bounded expression is no longer than its node count, the fast kernel
    takes at most 64 nodes and a group member at most 32.  The bound itself, 64, is word2_len64."""
    for pat in ("[0-9a-f]{64}[g-i]", "[0-9a-f]{65}", "[a-c][0-9a-f]{0,64}[g-i]"):
        (u,) = aosim_py.placement([pat], [14])["units"]
        assert u["kind"] == "scalar" and u["nw"] >= 3 and u["max_len"] >= 65, (pat, u)
    (u,) = aosim_py.placement(["[0-9a-f]{63}[g-i]"], [14])["units"]
    assert u["kind"] == "single" and u["nw"] == 2 and u["max_len"] == ac.FAST_MAX_LEN
    for cell in ac.CELLS:
        for u in ac.compiled(cell.name)["units"]:
            if u["kind"] != "scalar":
                assert u["max_len"] <= u["nnodes"] <= 64
            if u["kind"] == "group":
                assert u["max_len"] <= 32


def test_excluded_classes_name_known_tags():
    known = set(REQUIRED_TAGS) | set(ac.CLASSES) | {"lean", "break/63"}
    for cell in ac.CELLS:
        assert set(cell.excluded) <= known, (cell.name, set(cell.excluded) - known)
        assert all(isinstance(why, str) and why for why in cell.excluded.values())


_BRUTE: dict = {}
_SEARCH: dict = {}


def _brute_reports(cell, piece: bytes):
    """{(expression, to)} of one trimmed piece by Python `re`: every end, or the smallest one under SINGLEMATCH.  An expression
    that `re` itself finds nowhere in the piece is not swept end by end: it has no match there."""
    out = set()
    for i, e in enumerate(cell.exprs):
        cre = _SEARCH.get((e.pattern, e.flags))
        if cre is None:
            cre = _SEARCH[(e.pattern, e.flags)] = re.compile(e.pattern.encode(), regex_gen.py_flags(e.flags))
        if not cre.search(piece):
            continue
        key = (e.pattern, e.flags, piece)
        if key not in _BRUTE:
            _BRUTE[key] = regex_gen.ends_by_brute_force(e.pattern, e.flags, piece)
        ends = _BRUTE[key]
        out |= {(i, t) for t in (ends[:1] if e.flags & 8 else ends)}
    return out


@pytest.mark.parametrize("cell", ac.CELLS, ids=lambda c: c.name)
def test_reference_agrees_with_brute_force_and_itself(cell):
    texts = ac.cell_texts(cell.name)
    checked = set()
    for ti, text in enumerate(texts):
        planted = np.zeros(len(text.data) + 1, dtype=bool)
        for c in text.cases:
            planted[c.lo:c.hi] = True
        for bs in text.sizes:
            want, nlines, oracle_rows = ac.cell_reference(cell.name, ti, bs, False)
            # the oracle's own (line_off, line_len) are the pieces' (start, len)
            assert want.shape == oracle_rows.shape and (want == oracle_rows).all(), (text.label, bs)
            by_line = {}
            for line, rid, to, _, _ in want.tolist():
                by_line.setdefault(line, set()).add((rid, to))
            for line, (a, piece) in enumerate(invert_ref.pieces(text.data, bs)):
                if not piece or len(piece) > BRUTE_MAX or not planted[a] or piece in checked:
                    continue
                checked.add(piece)
                assert by_line.get(line, set()) == _brute_reports(cell, piece), (text.label, bs, line, piece)
    assert len(checked) >= 60, len(checked)


@pytest.mark.parametrize("cell", ac.CELLS, ids=lambda c: c.name)
def test_host_mirror_equals_the_reference(cell):
    """hgsim_py.Db.scan replays the pipeline line by line (hg_scan_line_always_on for this tier): all five columns."""
    texts = ac.cell_texts(cell.name)
    for shared in (False, True):
        db = hgsim_py.Db(cell.patterns, cell.flags, cell.ids(shared))
        assert db.ok(), db.error
        for ti, text in enumerate(texts):
            for bs in text.sizes:
                want, _, _ = ac.cell_reference(cell.name, ti, bs, shared)
                got = ac.sort_hits(db.scan(text.data, bs)[0])
                assert got.shape == want.shape and (got == want).all(), f"{cell.name} {text.label} bs {bs} shared {shared}: {ac.diff_report(text, got, want)}"


# every cell plants each of these at least once, unless its `excluded` names the tag (or its class) with the reason
REQUIRED_TAGS = (
    "seg/end_residue", "seg/end_offset", "seg/miss", "seg/split", "seg/split:miss", "seg/full_len_from_q", "seg/over_len",
    "tile/split", "tile/split:miss", "tile/line_from_previous_tile", "tile/line_from_two_tiles_back", "tile/line_at_tile_start", "tile/newline_first_byte",
    "tile/newline_first_byte_of_segment", "tile/newline_last_byte_of_segment", "tile/line_start_residues",
    "edge/match_at_byte_0", "edge/match_ends_the_text", "edge/near_miss_ends_the_text", "edge/match_cut_by_the_end", "edge/len_multiple_of_256", "edge/len_multiple_of_16384",
    "edge/short_text", "edge/short_text:miss", "edge/one_tile",
    "nul/leading", "nul/leading_only", "nul/inside", "nul/blocked", "nul/blocked_far", "nul/after_match", "nul/before_newline", "nul/line_of_nuls_before", "nul/in_leadin",
    "nul/in_leadin_blocked",
    "break/inside_match", "break/right_after_match", "break/on_segment_boundary", "break/in_leadin", "break/at_piece_start", "break/later_piece_leading_nuls",
    "break/later_piece_nul_blocks", "break/later_piece:miss", "break/third_piece",
    "single/same_segment", "single/adjacent_segments", "single/far_apart", "single/both_miss", "single/different_tiles",
    "long/line_700", "long/line_5000", "long/line_40960", "long/line_from_mid_tile", "long/miss",
    "dense/every_byte", "dense/quiet",
)
# tags whose cases must, in every cell that plants them, hold at least one that the reference reports / one that it does not
MUST_REPORT = (
    "seg/end_residue", "seg/end_offset", "seg/split", "seg/full_len_from_q", "tile/split", "tile/line_from_previous_tile", "tile/line_from_two_tiles_back", "tile/line_at_tile_start",
    "tile/newline_first_byte", "tile/newline_first_byte_of_segment", "tile/newline_last_byte_of_segment", "tile/line_start_residues",
    "edge/match_at_byte_0", "edge/match_ends_the_text", "edge/len_multiple_of_256", "edge/len_multiple_of_16384", "edge/short_text", "edge/one_tile",
    "nul/leading", "nul/leading_only", "nul/after_match", "nul/before_newline", "nul/line_of_nuls_before", "nul/in_leadin",
    "single/same_segment", "single/adjacent_segments", "single/far_apart", "single/different_tiles",
    "long/line_700", "long/line_5000", "long/line_40960", "long/line_from_mid_tile", "dense/every_byte",
)
MUST_BE_SILENT = (
    "seg/miss", "seg/split:miss", "seg/over_len", "tile/split:miss", "edge/near_miss_ends_the_text", "edge/match_cut_by_the_end", "edge/short_text:miss",
    "nul/inside", "nul/blocked", "nul/blocked_far", "nul/in_leadin_blocked", "single/both_miss", "long/miss", "dense/quiet",
)
# what the forced-break texts of EVERY buffer size hold (the tile-sized and larger ones included), and how each must end
BREAK_REPORTED = ("break/right_after_match", "break/on_segment_boundary", "break/in_leadin", "break/at_piece_start", "break/later_piece_leading_nuls", "break/third_piece")
BREAK_SILENT = ("break/inside_match", "break/later_piece_nul_blocks", "break/later_piece:miss")


def _excluded(cell, tag):
    return tag in cell.excluded or tag.split("/")[0] in cell.excluded


@pytest.mark.parametrize("cell", ac.CELLS, ids=lambda c: c.name)
def test_floors(cell):
    """Judged by the reference alone: no test passes by planting nothing."""
    texts = ac.cell_texts(cell.name)
    pl = ac.compiled(cell.name)
    planted = {cls: 0 for cls in ac.CLASSES}
    reported = {cls: 0 for cls in ac.CLASSES}
    silent = {cls: 0 for cls in ac.CLASSES}
    by_tag = {}  # tag -> [planted, reported, silent]
    by_break = {bs1: {} for bs1 in ac.BREAK_BS1}  # the same, for the texts of one forced-break size
    longest = {bs1: 0 for bs1 in ac.BREAK_BS1}
    end_res, lane_splits, tile_splits = set(), {}, set()
    mode = {cls: set() for cls in ac.LEAN_CLASSES}  # "lean" / "careful": how the tile of a reported case's match end is walked
    careful = {}
    newline_ends = 0
    hits = {False: 0, True: 0}
    for ti, text in enumerate(texts):
        assert 0 < len(text.data) <= ac.MAX_TEXT
        los = [c.lo for c in text.cases]
        assert los == sorted(los) and all(a.hi <= b.lo for a, b in zip(text.cases, text.cases[1:])), text.label
        bs1 = text.sizes[0] - 1 if text.label.startswith("break") else None
        for bs in text.sizes:
            hits[True] += len(ac.cell_reference(cell.name, ti, bs, True)[0])
            want, _, _ = ac.cell_reference(cell.name, ti, bs, False)
            hits[False] += len(want)
            starts, ends, ids = want[:, 3].astype(np.int64), (want[:, 3] + want[:, 2]).astype(np.int64), want[:, 1].astype(np.int64)
            newline_ends += sum(text.data[e - 1] == 10 for e in ends.tolist())
            for c in text.cases:
                cls = c.tag.split("/")[0]
                inside = (starts >= c.lo) & (starts < c.hi)
                counts = [by_tag.setdefault(c.tag, [0, 0, 0])] + ([by_break[bs1].setdefault(c.tag, [0, 0, 0])] if bs1 is not None else [])
                for n in counts:
                    n[0] += bs == text.sizes[0]
                    n[1 if inside.any() else 2] += 1
                if bs == text.sizes[0]:
                    planted[cls] += 1
                (reported if inside.any() else silent)[cls] += 1
                if bs1 is not None:
                    longest[bs1] = max(longest[bs1], c.hi - c.lo)
                exact = inside & (ends == c.end)  # the sample's own end is reported
                if cls == "seg" and bs == ac.DEFAULT_BS:
                    end_res |= {int(x) % 64 for x in ends[inside]}
                if c.tag == "seg/split" and c.expr == 0 and exact.any():
                    lane_splits.setdefault(bs, set()).add(c.k)
                if c.tag == "tile/split" and bs == ac.DEFAULT_BS and exact.any():
                    assert c.end - (len(cell.exprs[c.expr].plain[0]) - c.k) in range(ac.TILE, len(text.data), ac.TILE)
                    tile_splits.add((c.expr, c.k))
                if cls in mode:
                    for end, rid in zip(ends[inside].tolist(), ids[inside].tolist()):
                        unit = ac.unit_of(pl, rid)
                        if unit is None:
                            continue  # (the literal-anchored expression of the mixed cell)
                        key = (ti, bs, (end - 1) // ac.TILE, rid)
                        if key not in careful:
                            careful[key] = ac.wave_is_careful(unit, text.data, bs, (end - 1) // ac.TILE)
                        mode[cls].add("careful" if careful[key] else "lean")
    tags = set(by_tag)
    assert tags <= set(REQUIRED_TAGS) | {"seg/literal_anchored", "seg/literal_anchored:miss"}, tags - set(REQUIRED_TAGS)
    for cls in ac.CLASSES:
        if cls in cell.excluded:
            assert planted[cls] == 0, cls
            continue
        assert planted[cls] >= 4 and reported[cls] >= 1 and silent[cls] >= 1, (cls, planted[cls], reported[cls], silent[cls])
    for tag in REQUIRED_TAGS:
        assert (tag in tags) != _excluded(cell, tag), (tag, "planted" if tag in tags else "neither planted nor excluded")
    for tag in MUST_REPORT:
        assert _excluded(cell, tag) or by_tag[tag][1] >= 1, (tag, by_tag[tag])
    for tag in MUST_BE_SILENT:
        assert _excluded(cell, tag) or by_tag[tag][2] >= 1, (tag, by_tag[tag])
    assert end_res == set(range(64)), sorted(set(range(64)) - end_res)
    every_split = set(range(1, len(cell.exprs[0].plain[0])))
    assert all(lane_splits.get(bs) == every_split for bs in cell.main_sizes), lane_splits  # (in lean and in careful waves, where the cell has both)
    assert len({k for ei, k in tile_splits if ei == 0}) >= 6, tile_splits
    assert hits[False] >= 300 and hits[True] >= 300, hits
    if "lean" in cell.excluded:
        assert all(m <= {"careful"} for m in mode.values()), mode
    else:
        for cls in ac.LEAN_CLASSES:
            assert mode[cls] == {"lean", "careful"}, (cls, mode[cls])
    if cell.name in ("word_cf_nl", "word_ctx_nl", "word2_nl"):  # matches whose last byte is the line's newline
        assert newline_ends >= 16, newline_ends
    for bs1 in ac.BREAK_BS1:  # no buffer size gets a token check: each holds every kind of break, ending as the kind says
        got = by_break[bs1]
        if f"break/{bs1}" in cell.excluded:
            assert not got
            continue
        for tag in BREAK_REPORTED:
            assert got.get(tag, [0, 0, 0])[1] >= 1, (bs1, tag, got.get(tag))
        for tag in BREAK_SILENT:
            assert got.get(tag, [0, 0, 0])[2] >= 1, (bs1, tag, got.get(tag))
        assert longest[bs1] > 2 * bs1, (bs1, longest[bs1])  # a line with a sample two breaks in (bs1 20000: 40 KiB)
    assert longest[20000] >= 40000


def test_lean_and_careful_tiles_of_one_text():
    """wave_is_careful on the plainest case: short lines, a middle tile and the last one, buffer sizes 262140, 400 and the three
    around the 512 switch; a unit with conditions that takes the newline is careful everywhere."""
    cell = ac.BY_NAME["word_cf_nt1"]
    text = ac.cell_texts(cell.name)[0]
    unit = ac.compiled(cell.name)["units"][0]
    last = (len(text.data) - 1) // ac.TILE
    assert last >= 2
    assert not ac.wave_is_careful(unit, text.data, ac.DEFAULT_BS, 1) and ac.wave_is_careful(unit, text.data, ac.DEFAULT_BS, last)
    assert ac.wave_is_careful(unit, text.data, ac.CAREFUL_BS, 1) and ac.wave_is_careful(unit, text.data, 513, 1) and not ac.wave_is_careful(unit, text.data, 514, 1)
    nl_unit = ac.compiled("word_ctx_nl")["units"][0]
    assert ac.wave_is_careful(nl_unit, text.data, ac.DEFAULT_BS, 1)
    assert not ac.wave_is_careful(ac.compiled("word_cf_nl")["units"][0], text.data, ac.DEFAULT_BS, 1)
    # a long line: the wave whose lanes meet its forced break is careful, the waves of the other tiles are not
    brk = next(t for t in ac.cell_texts(cell.name) if t.label == "break16384_0")
    modes = {ac.wave_is_careful(unit, brk.data, 16385, t) for t in range((len(brk.data) - 1) // ac.TILE)}
    assert modes == {True, False}


def test_guarded_cases_hold_the_text_edges():
    import gpu_cases

    cases = [c for c in gpu_cases.guarded_cases() if c[0].startswith("alwayson-")]
    assert len(cases) == 12 and {c[0].split("-")[1] for c in cases} == set(ac.GUARDED_CELLS), [c[0] for c in cases]
    assert all(len(c[1]) % 16 for c in cases)
