"""The verify cells (tests/verify_cells.py) without a GPU: every claim of a cell is proved from the compiler's tables (the
placement read-out of tests/native/hostsim.cpp) or from the engine's sizing rules; the reference is held to the host replay;
and at every probe position of every cell's text three answers are compared: the table-first routine (hg_verify_window), the
buckets-only path the verify kernel takes for a set without `wtab_first` (with the kernel's dword compare under
hg_factor_mask_dword), and a brute force over every window of every literal."""
from __future__ import annotations

import collections
import functools

import pytest

import extsim_py
import hgsim_py
import verify_cells as vc

CELLS = vc.CELLS


@functools.lru_cache(maxsize=None)
def compiled(name):
    cell = next(c for c in CELLS if c.name == name)
    pats, flags, ids = vc.cell_patterns(cell)
    db = hgsim_py.Db(pats, flags=flags, ids=ids)
    assert db.ok(), db.error
    return db, db.selfcheck(), db.windows()


def test_every_class_is_some_cells_tag():
    seen = {t for c in CELLS for t in c.tags}
    assert not set(vc.REQUIRED_TAGS) - seen, sorted(set(vc.REQUIRED_TAGS) - seen)


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_claims_against_the_compiler(cell):
    db, check, windows = compiled(cell.name)
    claim = cell.claim
    assert check["violations"] == 0
    for key in ("table_first", "shared_windows", "byte_windows"):
        if key in claim:
            assert check[key] == claim[key], (key, check[key])
    if "fold_mask" in claim:
        assert db.info()["fold_mask"] == claim["fold_mask"]
    per_literal = collections.Counter(w["factor"] for w in windows)
    if "windows_per_literal" in claim:  # one per residue modulo 4: a literal at ANY text offset is met through exactly one of them
        assert set(per_literal.values()) == {claim["windows_per_literal"]}
        by_factor = collections.defaultdict(set)
        for w in windows:
            by_factor[w["factor"]].add(w["off"] % 4)
        assert all(r == {0, 1, 2, 3} for r in by_factor.values())
    if "buckets" in claim:
        assert set(claim["buckets"]) <= {w["bucket"] for w in windows}
    if "ways" in claim:
        assert set(claim["ways"]) <= {w["way"] for w in windows} and max(w["probes"] for w in windows) >= claim["probes_min"]
    pats, flags, ids = vc.cell_patterns(cell)
    plan = extsim_py.Db(pats, flags, ids, mode="plain")
    modes = collections.Counter(plan.pattern(i)["mode"] for i in range(len(pats)))
    assert all(plan.pattern(i)["tier"] == 0 for i in range(len(pats)))
    if "modes" in claim:
        assert dict(modes) == claim["modes"]
    # hg_verify_kernel (the staging area) runs iff the set has expressions of mode 1 or 2 (HgScanner::launch_side)
    assert claim["kernel"] == ("staged" if modes[1] or modes[2] else "lean")
    if "list_spread" in claim:  # the number written out in the cell against the rule of HgScanner::plan_pass restated in spread_of
        (mode, n), = claim["modes"].items()
        assert vc.spread_of(n) == claim["list_spread"] and claim["list_spread"] in (64, 32, 1)
    # tags that are properties of the tables
    if "table/direct" in cell.tags:
        assert any(w["table"] == "owner" for w in windows) and check["table_first"] == 1
    if "table/shared" in cell.tags:
        assert any(w["table"] == "shared" for w in windows) and check["table_first"] == 1  # both paths in one launch
    if "table/none" in cell.tags:
        assert check["table_first"] == 0
    if "bucket/negative-delta" in cell.tags:
        assert any(w["delta"] < 0 and w["select"] for w in windows)
    if "bucket/aligned-dword" in cell.tags:
        assert check["byte_windows"] == 0 and any(w["select"] and w["table"] == "shared" for w in windows)
    if "bucket/byte-loads" in cell.tags:
        assert check["byte_windows"] != 0


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_three_answers_at_every_position_and_the_reference(cell):
    db, _check, windows = compiled(cell.name)
    claim = cell.claim
    total = collections.Counter()
    for which, (name, text) in enumerate(cell.texts):
        data = vc.text_bytes(text)
        three = db.verify3(data)
        assert three["differing"] == 0, (name, three)
        assert three["table_first"] == three["buckets_only"] == three["brute_force"]
        records, n_lines, verified = vc.cell_reference(cell, which)
        assert three["brute_force"] == verified, name  # every verified pair is a literal occurrence of the reference and vice versa
        for k, v in three.items():
            total[k] += v
        total["largest"] = max(total["largest"], three["largest_bucket"])
        # what the DEVICE's verify pass sees: the positions the filter lets through, and the path each takes
        seen, _classes = db.candidates(data)
        for k, v in seen.items():
            total["cand/" + k] += v
        if len(data) > (4 << 20):
            continue  # (the host replay of the whole pipeline is for the small texts)
        hits, stats = db.scan(data, cell.buffer_size)
        assert hits == records and stats["pieces"] == n_lines and stats["candidates"] == verified, name
        assert seen["candidates"] == stats["level2_hits"], name  # (the read-out's filter is the host replay's)
        if name in claim.get("zero_pair_candidates", {}):
            assert seen["zero_pairs"] >= claim["zero_pair_candidates"][name] and seen["value_mismatch"] >= claim["mismatch_candidates"][name], (name, seen)
            assert seen["candidates"] <= 64  # one verify wave
        if name in claim.get("candidates", {}):
            assert stats["level2_hits"] == claim["candidates"][name], (name, stats)
        if name in claim.get("verified", {}):
            assert verified == claim["verified"][name]
        if name in claim.get("final_flush_only", ()):  # never 384 staged occurrences: only the flush behind the loop runs
            assert verified < vc.STAGE_CAP // 2
        if name in claim.get("false_positives_min", {}):
            # candidates beyond the verified occurrences: windows the filter lets through that belong to no literal
            assert stats["level2_hits"] - stats["candidates"] >= claim["false_positives_min"][name], (name, stats)
        if name in claim.get("verified_min", {}):
            assert verified >= claim["verified_min"][name]
    tags = set(cell.tags)
    if "bucket/value-mismatch" in tags:
        assert total["cand/value_mismatch"] >= cell.claim["value_mismatch_min"]
    if "bucket/zero-pairs" in tags:
        assert total["cand/zero_pairs"] >= cell.claim["zero_pairs_min"]
    if "bucket/select-before-text" in tags:
        assert total["cand/select_before"] > 0
    if "bucket/select-behind-text" in tags:
        assert total["cand/select_behind"] >= 3
    if "bucket/negative-address" in tags:
        assert total["cand/negative_at"] >= cell.claim["negative_at_min"]
    if "table_ends_min" in cell.claim:
        assert total["cand/table_ends"] >= cell.claim["table_ends_min"]
    if "end/byte-compare-tail" in tags:
        assert total["byte_compare_tail"] > 0
    if "end/text-begins-inside-literal" in tags:
        assert total["before_text"] > 0
    if "compare/mask-tail" in tags:
        assert total["mask_tail"] > 0
    if "flatten/bucket-1-2-63-64-65-200" in tags:
        assert total["largest"] == 200


def test_lengths_cell_plants_what_it_says():
    cell = next(c for c in CELLS if c.name == "lengths")
    assert set(range(7, 33)) <= {len(e.lit) for e in cell.exprs}
    lits = [e.lit for e in cell.exprs]
    assert any(a != b and b.startswith(a) for a in lits for b in lits)  # one literal is a prefix of another
    # two literals that overlap in the text so that ONE candidate position verifies both, at different offsets: a window value
    # both hold, at offsets that differ by the literals' displacement
    _db, _check, windows = compiled("lengths")
    a, b = lits.index(b"shared_stem_000"), lits.index(b"hared_stem_0")
    shift = b"shared_stem_000".index(b"hared_stem_0")
    wa = {(w["value"], w["off"]) for w in windows if w["pattern"] == a}
    assert any((w["value"], w["off"] + shift) in wa for w in windows if w["pattern"] == b)
    # every alignment modulo 16 of every literal, the literals taking turns (16 beside 17)
    data = vc.text_bytes(cell.texts[0][1])
    for lit in lits:
        found, pos = set(), data.find(lit)
        while pos >= 0:
            found.add(pos % 16)
            pos = data.find(lit, pos + 1)
        assert found == set(range(16)), lit
    l16, l17 = next(x for x in lits if len(x) == 16), next(x for x in lits if len(x) == 17)
    assert 0 < data.find(l17) - data.find(l16) < 64
    # the near misses: the 32-byte literal with each byte changed
    near = vc.text_bytes(cell.texts[1][1])
    long = next(x for x in lits if len(x) == 32)
    for j in range(32):
        assert long[:j] + bytes([long[j] ^ 1]) + long[j + 1:] in near


def test_staging_and_overflow_bounds_from_the_reference():
    by_name = {c.name: c for c in CELLS}
    # final flush only: these texts of the flatten cell never stage 384 occurrences (the others pass a wave's 4096 pairs)
    flat = by_name["flatten"]
    names = [name for name, _t in flat.texts]
    assert set(flat.claim["final_flush_only"]) == set(names) - {"5000", "mixed"}
    assert vc.cell_reference(flat, names.index("5000"))[2] > 4096
    # mid-loop flush: one pair per candidate, thousands of candidates: a round adds at most 256, so the stage passes 384 and never 768
    assert vc.cell_reference(by_name["stage-mid-flush"], 0)[2] >= 6000
    # direct filing: >= 4 verified pairs per candidate, >= 1 candidate per 64 bytes, >= 16 tiles
    dense = by_name["stage-direct-filing"]
    data = vc.text_bytes(dense.texts[0][1])
    records, n_lines, verified = vc.cell_reference(dense, 0)
    assert len(data) >= dense.claim["tiles_min"] * vc.TILE and n_lines * dense.claim["candidate_every"] == len(data)
    assert verified == n_lines * dense.claim["pairs_per_candidate"] and len(records) == n_lines
    assert 4 * 64 * dense.claim["pairs_per_candidate"] > vc.STAGE_CAP  # a block's round: 4 waves of 64 candidates
    # list overflow: one expression owns more occurrences than a list of a fresh scanner holds
    over = by_name["list-overflow"]
    data = vc.text_bytes(over.texts[0][1])
    assert data.count(vc.OVERFLOW[0].lit) > vc.overflow_capacity() and len(data) < (64 << 20)
    assert vc.spread_of(len(vc.OVERFLOW)) == 1
