"""The finalize cells (tests/finalize_cells.py) without a GPU: the reference equals the oracle on every cell, record for record
in order, and every cell holds the geometry it is named for: the bucket plan it claims follows from the engine's planning
rule, the per-bucket raw report counts it claims follow from the reference and that plan, and the sorted positions of the
rule cells are where the cell says."""
from __future__ import annotations

import functools

import pytest

import finalize_cells as fc
import oracle_py

CELLS = fc.CELLS
IDS = [c.name for c in CELLS]


@functools.lru_cache(maxsize=4)
def oracle_records(fn, exprs, buffer_size):
    """The oracle's records of a cell text in (line, id, to) order.  (It knows no HS_FLAG_SOM_LEFTMOST; the ends of a literal's
    matches do not depend on it.)"""
    rc, hits, nlines = oracle_py.scan_buffer(fc._text(fn), [e.lit.decode() for e in exprs], flags=fc.flags_of(exprs), ids=[e.id for e in exprs], buffer_size=buffer_size)
    assert rc == 0
    return sorted(hits), nlines


@pytest.mark.parametrize("cell", CELLS, ids=IDS)
def test_reference_equals_the_oracle(cell):
    for which in ("text", "prelude", "second"):
        fn = getattr(cell, which)
        if fn is None:
            continue
        scan = fc.cell_scan(cell, which)
        base = cell.line_base if which == "text" else 0
        want, nlines = oracle_records(fn, tuple(cell.exprs), cell.buffer_size)
        assert nlines == len(scan.starts)
        assert scan.records == [(ln + base, rid, to, off, n) for ln, rid, to, off, n in want]
        assert all(a[:3] < b[:3] for a, b in zip(scan.records, scan.records[1:])), "the reference's list is strictly increasing in (line, id, to)"
        assert len(scan.admissible) == len(scan.records) and all(scan.admissible)
        # the oracle's line_len counts the newline
        assert all(fc._text(fn)[off + n - 1:off + n] == b"\n" or off + n == len(fc._text(fn)) or n == cell.buffer_size - 1 for _, _, _, off, n in scan.records)


def _expect_prev(cell):
    return sum(len(r) for r in fc.cell_scan(cell, "prelude").raw.values()) if cell.prelude else 0


@pytest.mark.parametrize("cell", CELLS, ids=IDS)
def test_claimed_geometry_follows_from_the_reference(cell):
    claim, text, scan = cell.claim, fc.cell_text(cell), fc.cell_scan(cell)
    assert scan.records, "a cell delivers records"
    max_id = max(e.id for e in cell.exprs)
    id_bits, to_bits = fc.bits_for(max_id + 1), fc.bits_for(cell.buffer_size)
    shift, nb, cap = fc.plan_buckets(len(text), _expect_prev(cell), fc.target_of(cell))
    if "first_plan" in claim:  # the pass that overflows; what the repeated pass plans is read from the device
        assert (shift, nb, cap) == claim["first_plan"]
        fill = fc.bucket_fill(scan, shift, nb)
        assert max(fill) == claim["max_fill"] > cap
        assert (claim["max_fill"] > 4096) == claim["left_bucketed"]
        return
    for key, value in (("fin_shift", shift), ("fin_nb", nb), ("fin_cap", cap), ("id_bits", id_bits), ("to_bits", to_bits)):
        if key in claim and (key != "fin_cap" or not cell.prelude):
            assert claim[key] == value, (key, claim[key], value)
    assert claim["path"] == fc.plan_path(shift, max_id, cell.buffer_size, cell.line_base, len(text), len(scan.starts), cell.env)
    if "key_bits" in claim:
        assert shift + id_bits + to_bits + 1 == claim["key_bits"]
    if "bound_bits" in claim:
        assert fc.bits_for(cell.line_base + len(text) + 1) == claim["bound_bits"]
    fill = fc.bucket_fill(scan, shift, nb)
    if claim["path"] == "bucketed" and not cell.prelude:
        assert max(fill) <= cap, "no bucket outgrows its region: the plan stands"
    for b, n in claim.get("fills", {}).items():
        assert fill[b] == n, (b, fill[b], n)
    if "classes" in claim:
        assert set(claim["classes"]) <= set(fill)
    if "fill_class" in claim:
        lo, hi = claim["fill_class"]
        assert all(f == 0 or lo <= f <= hi for f in fill) and any(fill)
    if "positions" in claim:
        claim["positions"](cell)
    if "classes_each_side" in claim:  # buckets of every size class on either side of the settled limit
        lim = claim["classes_each_side"]
        for side in (fill[:lim], fill[lim:]):
            assert any(1 <= f <= 64 for f in side) and any(65 <= f <= 512 for f in side) and any(513 <= f <= 4096 for f in side), (lim, fill)
        # the long line starts on the last byte of a bucket, breaks into pieces, and has records on both pieces, the second
        # of which begins at the last chunk's start, one byte before or one byte behind it
        k = scan.starts.index(fc.RANGES_X)
        assert scan.starts[k + 1] - fc.RANGES_B == cell.buffer_size - 1 - (fc.RANGES_B - fc.RANGES_X) and abs(scan.starts[k + 1] - fc.RANGES_B) <= 1
        assert (fc.RANGES_X + 1) % (1 << shift) == 0 and scan.raw[k] and scan.raw[k + 1]
        assert any(to > cell.buffer_size - 40 for _, to, _, _ in scan.raw[k]), "a report at the far end of the first piece"
    if "neighbour_ids" in claim:  # in each sort class, a line whose neighbouring groups' ids differ in the lowest bit alone, a
        # SINGLEMATCH report in each: one that would be ruled out if the two groups were taken for one
        for b in claim["neighbour_ids"]:
            gs = fc.groups_of(fc.bucket_sorted(scan, shift, b))
            assert any(g[2][0][0] == h[2][0][0] and g[2][0][1] ^ h[2][0][1] == 1 and any(r[3] for r in g[2]) and any(r[3] for r in h[2]) for g, h in zip(gs, gs[1:])), b
    if "kept_buckets" in claim:
        assert sorted({scan.starts[k] >> shift for k in scan.raw}) == claim["kept_buckets"]
        assert {0, nb - 1, 8191, 8192, fc.MANY_SPAN - 1, fc.MANY_SPAN} <= set(claim["kept_buckets"]) and claim["scan_blocks"] == (nb + 8191) // 8192 >= 2


def test_every_path_and_class_has_a_cell():
    paths = {c.claim["path"] for c in CELLS}
    assert paths == {"bucketed", "compact_packed", "compact_wide"}
    assert any(c.claim.get("early_buckets") for c in CELLS) and any(c.claim.get("scan_blocks", 0) > 1 for c in CELLS)
    assert any(c.claim.get("left_bucketed") for c in CELLS) and any(c.claim.get("reruns_min") and not c.claim.get("left_bucketed") for c in CELLS)
    seen = set()
    for c in CELLS:
        seen |= set(c.claim.get("fills", {}).values())
    assert set(fc.CLASS_EDGES) <= seen
    ids = {e.id for c in CELLS for e in c.exprs}
    assert set(fc.WIDE_IDS) <= ids
    # reports of one (line, id) that differ in the lowest bit of `to` alone, in buckets of each of the three sort classes
    classes = set()
    for name in ("fill-one-line", "fill-spread"):
        cell = next(c for c in CELLS if c.name == name)
        for b, n in cell.claim["fills"].items():
            s = fc.bucket_sorted(fc.cell_scan(cell), 16, b)
            if any(x[:2] == y[:2] and x[2] ^ y[2] == 1 for x, y in zip(s, s[1:])):
                classes.add(0 if n <= 64 else 1 if n <= 512 else 2)
    assert classes == {0, 1, 2}

def test_small_groups_are_enumerated_once():
    """Every multiset of up to three (kind, end) reports over three ends is one line of the group cells, and the reference
    gives it what the three rules say."""
    assert len(fc.SMALL_GROUPS) == 6 + 21 + 56 == len(set(fc.SMALL_GROUPS))
    cell = next(c for c in CELLS if c.name == "rule-groups-one-bucket")
    scan = fc.cell_scan(cell)
    assert len(scan.starts) == len(fc.SMALL_GROUPS)
    by_line = {}
    for (ln, _, to, _, _) in scan.records:
        by_line.setdefault(ln, []).append(to)
    for ln, group in enumerate(fc.SMALL_GROUPS):
        words = fc._group_words(group)
        ends, pos = {}, 0
        for w in words:  # the end offset of each planted word
            pos += len(w)
            ends[len(ends)] = pos
            pos += 1
        slots = sorted({e for _, e in group})
        end_of = {e: ends[i] for i, e in enumerate(slots)}
        singles = [end_of[e] for single, e in group if single]
        want = sorted({end_of[e] for single, e in group if not single} | ({min(singles)} if singles else set()))
        assert by_line[ln] == want, (group, by_line[ln], want)
        assert sorted((1 if single else 0, end_of[e]) for single, e in group) == sorted((s, to) for _, to, s, _ in scan.raw[ln])
