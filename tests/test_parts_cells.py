"""The cells of the parts stage on the host (no GPU): for every cell of parts_cells.py and for the random expressions of
test_parts_host.py, the plain Python reference (parts_ref), the scalar definition (hg_parts_next) and the replay of the kernels'
decomposition (partssim_piece_grouped: groups of 64 starts, the first-byte rule, the ballot / cursor / base loop) agree; and
every claim a cell makes about what it reaches is proved from the compiler's read-out, the replay's trace or the text."""
from __future__ import annotations

import pytest

import accept_rules
import invert_ref
import parts_cells as pc
import parts_ref
import partssim_py
import regex_gen

WORD = set(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_")
_dbs: dict = {}
_done: dict = {}  # cell name -> what run_cell found: computed once


def database(pats, flags):
    key = (tuple(pats), tuple(flags))
    if key not in _dbs:
        _dbs[key] = partssim_py.Db(pats, flags, [0] * len(pats))
    return _dbs[key]


def three_ways(db, pats, flags, piece):
    """One piece: reference == definition == grouped replay.  Returns (parts, ties, trace)."""
    want = parts_ref.piece_parts(pats, flags, piece)
    assert db.piece(piece) == want, (pats, flags, piece, db.piece(piece), want)
    got, ties, trace = db.piece_grouped(piece)
    assert got == want, (pats, flags, piece, got, want, trace)
    assert [t[0] for t in trace] == sorted({t[0] for t in trace}) and all(b < len(piece) for b, _r, _o in trace)
    return want, ties, trace


def context_classes(text: bytes, buffer_size: int, parts_by_piece):
    """The classes of parts_cells.CTX the text's pieces show, read from the bytes alone."""
    found = set()
    pieces = invert_ref.pieces(text, buffer_size)
    for i, (a, piece) in enumerate(pieces):
        line_start = text.rfind(b"\n", 0, a) + 1
        mid_line = a > line_start and text[a - 1] != 0
        if piece and mid_line:
            found.add("after_word" if text[a - 1] in WORD else "after_nonword")
        if piece and a > line_start and text[a - 1] == 0:
            found.add("behind_nuls")
        z = a + len(piece)
        if piece and z < len(text) and text[z] == 0:
            found.add("inner_nul")
        if piece and not piece.endswith(b"\n") and z < len(text) and text[z] != 0:
            found.add("ends_midline")
        if len(piece) == 1 and piece != b"\n":
            found.add("one_byte")
        if len(piece) >= 2 and piece.endswith(b"\n"):
            found.add("dollar_nl")
        if piece and z == len(text) and not piece.endswith(b"\n"):
            found.add("dollar_end")
        if any(b"\n" in piece[f:t] for f, t, _p in parts_by_piece[i]):
            found.add("nl_in_part")
    return found


def selection_shown(db, pats, flags, pieces, per_piece):
    """The expression-selection claims of parts_cells the reference's parts show."""
    found = set()
    words = (db.n_patterns() + 31) // 32
    for piece, parts in zip(pieces, per_piece):
        for f, t, p in parts:
            found.add(("wins", p))
            if p >> 5 == words - 1:
                found.add(("words", words))
            if piece[f] >= 0x80:
                found.add("high_byte")
            if p >= 32 and any(parts_ref.matches_exactly(pats[j], flags[j], piece, f, e) for j in range(32) for e in range(f + 1, t)):
                found.add("higher_longer")
    for j in range(len(pats)):
        firsts = {piece[f:f + 1] for piece, parts in zip(pieces, per_piece) for f, _t, p in parts if p == j}
        if any(c.isupper() and c.lower() in firsts for c in firsts):
            found.add(("caseless", j))
    return found


def run_cell(cell):
    name, pats, flags, text, bs, claims = cell
    if name in _done:
        return _done[name]
    db = database(pats, flags)
    assert db.ok(), (name, db.error)
    assert db.refusal() is None, name
    pieces = invert_ref.pieces(text, bs)
    assert max(len(p) for _a, p in pieces) <= 1100, name
    shown = set()
    per_piece = []
    n_parts = 0
    for _a, piece in pieces:
        parts, ties, trace = three_ways(db, pats, flags, piece)
        per_piece.append(parts)
        n_parts += len(parts)
        bases = [b for b, _r, _o in trace]
        for g, (base, rounds, outrun) in enumerate(trace):
            last = max([t for f, t, _p in parts if f < base + 64 and f >= base], default=0)
            if any(f >= base and f < base + 64 and t == base + 64 for f, t, _p in parts):
                shown.add("edge")
            if last > base + 64:
                shown.add("jump")
                assert g + 1 == len(bases) or bases[g + 1] == last, (name, trace)
            if base % 64:
                shown.add("unaligned")
            if outrun:
                shown.add("outrun")
            if rounds == 64:
                shown.add("rounds64")
        if any(ties):
            shown.add("tie")
    shown |= {("ctx", c) for c in context_classes(text, bs, per_piece)}
    shown |= selection_shown(db, pats, flags, [p for _a, p in pieces], per_piece)
    for claim in claims:
        if claim[0] == "tier":
            info = db.pattern_info(claim[1])
            assert (info["nw"], info["simple"]) == pc.TIERS[claim[2]][2], (name, claim, info)
        else:
            assert claim in shown, (name, claim, sorted(map(str, shown)))
    # what the GPU test will ask for: the reference over the whole text on its matching lines
    lines = parts_ref.matching_lines(text, bs, pats, flags)
    want = parts_ref.expected(text, bs, pats, flags, lines)
    assert want == [(i, f, t, p) for i, parts in enumerate(per_piece) for f, t, p in parts], name
    assert sorted({r[0] for r in want}) == lines, name  # a piece matches somewhere iff it has a part
    _done[name] = (len(pieces), n_parts, len(claims), shown)
    return _done[name]


@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_cells(group):
    pieces = parts = claims = 0
    for cell in pc.GROUPS[group]:
        a, b, c, _shown = run_cell(cell)
        pieces, parts, claims = pieces + a, parts + b, claims + c
    print(f"group {group}: {len(pc.GROUPS[group])} cells, {pieces} pieces, {parts} parts, {claims} claims checked")
    assert parts > 0


def test_every_target_is_claimed_somewhere():
    """The geometry, the tiers, the bitmap sizes and the context classes the suite is for: each is claimed (and so proved) by
    at least one cell, and every cell with parts in group A, B or C that makes no claim is still compared three ways."""
    claimed = {c for cell in pc.CELLS for c in cell[5]}
    for what in ("edge", "jump", "unaligned", "outrun", "rounds64", "tie", "higher_longer", "high_byte", ("caseless", 0)):
        assert what in claimed, what
    assert {c[1] for c in claimed if c[0] == "words"} >= {1, 2, 3, 4}
    assert {c[1] for c in claimed if c[0] == "ctx"} == set(pc.CTX)
    assert {c[2] for c in claimed if c[0] == "tier"} == set(pc.TIERS)
    for group in ("A1", "A2", "A3", "A4", "A5"):  # every tier that can express a group's geometry runs it
        tiers = {c[2].rstrip("s") for cell in pc.GROUPS[group] for c in cell[5] if c[0] == "tier"}  # (L32s: the 32-word walk for long parts)
        assert tiers == ({"L3", "L32"} if group == "A2" else set(pc.ORDER)), group
    # the jump is followed by groups that are not aligned, for the LDS walks of 3 and of 32 words
    for tier in ("L3", "L32s"):
        assert any("unaligned" in cell[5] and ("tier", 0, tier) in cell[5] for cell in pc.GROUPS["A2"])
    for tier in pc.ORDER + ("L32s",):  # a dropped start that outran the accepted end, for every walk
        assert any("outrun" in cell[5] and ("tier", 0, tier) in cell[5] for cell in pc.GROUPS["A3"]), tier
    assert all(cell[5] for cell in pc.GROUPS["C"])  # no cell of group C is without a claim
    chunk = database(*pc.CHUNK_SET)  # the pipeline-chunk test's database walks as it says
    assert chunk.ok() and chunk.refusal() is None
    assert [(chunk.pattern_info(j)["nw"], chunk.pattern_info(j)["simple"]) for j in range(3)] == [pc.TIERS[t][2] for t in pc.CHUNK_TIERS]
    # the mixed database allocates LDS for 32 words while four of its five expressions walk with less
    mixed = [c for c in pc.GROUPS["C"] if c[0] == "C/five tiers in one database"][0]
    db = database(mixed[1], mixed[2])
    assert db.info()["max_nw"] == 32 and [db.pattern_info(j)["nw"] for j in range(5)] == [1, 1, 2, 3, 32]
    want = parts_ref.expected(mixed[3], mixed[4], mixed[1], mixed[2], [1, 2])
    assert {p for _l, _f, _t, p in want} == {0, 1, 2, 3, 4}  # each tier wins once
    four_ends = [(f, t) for _l, f, t, p in want if t - f == 91 and p == 4]
    assert len(four_ends) == 1  # the start where four tiers match with four ends: the longest is the part


@pytest.mark.parametrize("seed", range(20))
def test_random_expressions_three_ways(seed):
    """The random expressions of test_parts_host.py::test_replay_against_reference through the grouped replay as well."""
    tally = accept_rules.Tally()

    def compiles(pat, flags):
        db = partssim_py.Db([pat], [flags])
        return db.ok(), db.error

    parts = 0
    for pat, flags, data, _ in regex_gen.end_offset_cases(seed, accepts=tally.accepts(compiles)):
        db = partssim_py.Db([pat], [flags], [0])
        for _a, piece in invert_ref.pieces(data, 1 << 20):
            parts += len(three_ways(db, [pat], [flags], piece)[0])
    assert parts > 0
