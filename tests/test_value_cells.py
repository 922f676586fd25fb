"""The cells of the value table stages on the host (no GPU): every cell of value_cells.py through the replays of the headers'
scalar rules (valuesim, ranksim, valstoresim) against the plain Python references (values_ref, rank_ref, valstore_ref: a dict, a
sort, a slice), with the parts taken from Python's `re` over the lines; and every claim a cell makes about what it reaches is
proved from the replay's read-outs or from the parts."""
from __future__ import annotations

import pytest

import parts_ref
import rank_ref as rr
import ranksim_py as rs
import value_cells as vc
import values_ref as vr
import valstore_ref as sr
import valstoresim_py as ss
import valuesim_py as vs

_parts: dict = {}


def parts_of(cell):
    if cell["name"] not in _parts:
        _parts[cell["name"]] = vc.re_parts(cell["pset"], cell["text"])
    return _parts[cell["name"]]


def values_of(text, parts, starts):
    return [text[starts[(0, p[0])] + p[1]:starts[(0, p[0])] + p[2]] for p in parts]


def prove(cell, claim, text, records, parts):
    what, kw, arg = claim
    starts = {(0, r[0]): r[1] for r in records}
    values = values_of(text, parts, starts)
    if what == "two_expressions":
        by_bytes = {}
        for v, p in zip(values, parts):
            by_bytes.setdefault(v, set()).add(p[3])
        assert any(len(s) == 2 for s in by_bytes.values()), cell["name"]
        return
    if what == "alignments":
        seen, pairs = {}, []
        for v, p in zip(values, parts):
            at = starts[(0, p[0])] + p[1]
            if v in seen:
                pairs.append((seen[v] % 4, at % 4))
            seen[v] = at
        assert tuple(pairs) == arg and {(a, b) for a, b in pairs} == {(a, b) for a in range(4) for b in range(4)}, cell["name"]
        return
    kw = vc.resolve(kw, len(parts))
    _got, info = vs.replay(text, records, parts, trace=True, **kw)
    rows, waves, call = info["parts"], info["waves"], info["call"]
    if what == "path":
        wave, path, leader = arg
        assert (waves[wave]["path"], waves[wave]["leader"]) == (path, leader), (cell["name"], arg, waves[wave])
        assert bin(waves[wave]["mask"]).count("1") == sum(1 for q in range(64 * wave, min(64 * wave + 64, len(parts))) if rows[q]["tier"] == 1)
    elif what == "first_in_wave":
        value, wave = arg
        assert values.index(value) // 64 == wave, (cell["name"], arg)
    elif what == "n_long":
        assert call["n_long"] == arg == sum(r["tier"] == 2 for r in rows) == sum(len(v) > vc.LANE_MAX for v in values), (cell["name"], call)
    elif what == "long_iterations":
        assert call["long_iterations"] == arg and call["long_waves"] == 4096, (cell["name"], call)
    elif what == "wrapped":
        tier, n = arg
        assert sum(r["wrapped"] for r in rows if r["tier"] == tier) >= n, (cell["name"], arg)
        assert all(r["slot"] < r["home"] for r in rows if r["wrapped"])
    elif what == "homes":
        for v, r in zip(values, rows):
            if v in arg:
                assert r["home"] == arg[v], (cell["name"], v, r)
        assert set(arg) <= set(values)
    elif what == "last_slot":
        taken = {r["slot"] for r in rows}
        assert call["last_slot_occupied"] == arg[0] == (call["slots"] - 1 in taken) and (0 in taken) == bool(arg[1]), (cell["name"], call)
    elif what == "n_values":
        assert call["n_values"] == arg == len({r["slot"] for r in rows}) == len(set(values)), (cell["name"], call)
    elif what == "free_slots":
        assert call["slots"] - call["n_values"] == arg, (cell["name"], call)
    elif what == "slots":
        assert call["slots"] == arg, (cell["name"], call)
    elif what == "chain_tags":
        assert any(r["same_tag"] and r["other_tag"] for r in rows), cell["name"]
    elif what == "no_tag":
        assert all(r["other_tag"] == 0 for r in rows) and any(r["same_tag"] for r in rows) or all(r["probes"] == 1 for r in rows), cell["name"]
        assert all(vs.hash_of(v, 0, len(v), which=0, hash_bits=kw["hash_bits"]) >> 40 == 0 for v in set(values))
    elif what == "passes":
        mine, other = rows[values.index(arg[0])], rows[values.index(arg[1])]
        assert mine["probes"] > 1 and (other["slot"] - mine["home"]) % call["slots"] < (mine["slot"] - mine["home"]) % call["slots"], (cell["name"], mine, other)
    elif what == "shared_chain":
        assert any(r["same_tag"] + r["other_tag"] for r in rows), cell["name"]
    elif what == "sort_bits":
        bits, first = arg
        assert call["sort_bits"] == bits == first.bit_length() and first == len(parts) - 1 == values.index(values[-1]), (cell["name"], call)
    else:
        raise AssertionError(f"unknown claim {what}")


@pytest.mark.parametrize("group", vc.TEXT_GROUPS)
def test_text_cells(group):
    """count_values' replay at every setting and in two insertion orders, the SEG form through the rank replay, and the claims."""
    for cell in vc.GROUPS[group]:
        text = cell["text"]
        records, parts = parts_of(cell)
        starts = {(0, r[0]): r[1] for r in records}
        assert all((0, p[0]) in starts for p in parts)
        big = len(parts) > 2000
        for bp in cell["by_pattern"]:
            want = vr.arrays(vr.groups(text, parts, starts, by_pattern=bp))
            assert sum(want["count"]) == len(parts)
            for kw in cell["settings"]:
                for seed in (0,) if big else (0, 5):
                    got, _info = vs.replay(text, records, parts, by_pattern=bp, order_seed=seed, **vc.resolve(kw, len(parts)))
                    assert got == want, (cell["name"], bp, kw, seed)
            if cell["seg"]:
                rows, seg_arrays, n_distinct = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=True, seg_start=[0], n_seg=1)
                for kw in cell["settings"]:
                    got, got_seg, info = rs.replay(text, records, parts, by_pattern=bp, per_segment=True, seg_start=[0], **vc.resolve(kw, len(parts)))
                    assert got == rr.arrays(rows, segments=True) and got_seg == seg_arrays and info["n_distinct"] == n_distinct, (cell["name"], bp, kw)
        for claim in cell["claims"]:
            prove(cell, claim, text, records, parts)


def test_pair_parts_are_what_the_lines_show():
    """The PAIR cells by a second route: a part at a line's start that does not reach its end is expression 0's, one that ends
    the line but does not start it expression 1's, and a part that is the whole line goes to the lower index."""
    for cell in vc.GROUPS["D"]:
        if cell["pset"] != "PAIR":
            continue
        records, parts = parts_of(cell)
        lines = cell["text"].splitlines()
        for no, f, t, p, _s in parts:
            assert lines[no][f:f + 1] == b"x" and p == (0 if f == 0 else 1) and (f == 0 or t == len(lines[no])), (cell["name"], no, f, t, p)
        assert {p[3] for p in parts} == {0, 1}
    assert parts_ref.piece_parts(*vc.PSETS["PAIR"], b"xab xab\n") == [(0, 3, 0), (4, 7, 1)]


def test_file_cells():
    for cell in vc.GROUPS["F"]:
        text, records, parts, seg_start = vc.re_files(cell["pset"], cell["files"])
        starts = {(r[3], r[0]): r[1] for r in records}
        n_seg = len(cell["files"])
        for bp, ps in ((False, False), (False, True), (True, False), (True, True)):
            for top in cell["tops"]:
                rows, seg_arrays, n_distinct = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=ps, top=top, seg_start=seg_start, n_seg=n_seg)
                for kw in vc.STD:
                    kw = vc.resolve(kw, len(parts))
                    got, got_seg, info = rs.replay(text, records, parts, by_pattern=bp, per_segment=ps, top=top, seg_start=seg_start, **kw)
                    assert got == rr.arrays(rows, segments=True) and got_seg == seg_arrays and info["n_distinct"] == n_distinct, (cell["name"], bp, ps, top, kw)
        for bp in (False, True):  # the read-outs of the per-file form: key words, bounds, cuts and both sorts' widths
            for top in cell["tops"]:
                rows, seg_arrays, n_distinct = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=True, top=top, seg_start=seg_start, n_seg=n_seg)
                _got, _seg, info = rs.replay(text, records, parts, by_pattern=bp, per_segment=True, top=top, seg_start=seg_start, trace=True)
                assert [r["key"] for r in info["parts"]] == [((p[4] + 1) << 32) | (p[3] + 1 if bp else 0) for p in parts], cell["name"]
                assert [s["seg_distinct"] for s in info["segs"]] == seg_arrays["seg_distinct"] and [s["seg_parts"] for s in info["segs"]] == seg_arrays["seg_parts"]
                assert [s["kept"] for s in info["segs"]] == [min(top, d) if top else d for d in seg_arrays["seg_distinct"]], (cell["name"], top)
                assert [s["first_group"] for s in info["segs"]] == [sum(seg_arrays["seg_distinct"][:k]) for k in range(n_seg)]
                assert sum(info["placed"]) == len(rows) and len(info["placed"]) == n_distinct and (sum(info["placed"]) < n_distinct) == any(0 < top < d for d in seg_arrays["seg_distinct"])
                assert info["call"]["count_bits"] == max(1, len(parts).bit_length()) and info["call"]["seg_bits"] == max(1, n_seg.bit_length()), (cell["name"], info["call"])
        if cell["name"].startswith("F/count width 2^") and n_seg == 1:
            k = int(cell["name"].split("^")[1])
            assert len(parts) == (2 << k) - 1 and len(parts).bit_length() == k + 1  # the larger count, 2^k, needs all k + 1 bits of the sort's key
        for what, _kw, _arg in cell["claims"]:
            assert what == "two_expressions"
            by_bytes = {}
            for p in parts:
                at = seg_start[p[4]] + starts[(p[4], p[0])]
                by_bytes.setdefault(text[at + p[1]:at + p[2]], set()).add((p[4], p[3]))
            assert {(0, 1), (1, 0)} in by_bytes.values(), cell["name"]  # the crossed pairs
            rows, _a, n = rr.ranking(text, parts, starts, by_pattern=True, per_segment=True, seg_start=seg_start, n_seg=n_seg)
            assert n == 2 and rr.ranking(text, parts, starts, seg_start=seg_start, n_seg=n_seg)[2] == 1


def test_cuts_and_ties_cell_is_what_it_says():
    cell = vc.GROUPS["F"][0]
    text, records, parts, seg_start = vc.re_files(cell["pset"], cell["files"])
    starts = {(r[3], r[0]): r[1] for r in records}
    rows, seg, n = rr.ranking(text, parts, starts, per_segment=True, seg_start=seg_start, n_seg=1)
    assert [(r["value"], r["count"]) for r in rows] == [(b"xe", 3), (b"xc", 2), (b"xb", 2), (b"xa", 2), (b"xd", 1)] and seg["seg_distinct"] == [5] == [n]
    assert [r["first"] for r in rows[1:4]] == sorted(r["first"] for r in rows[1:4])  # the tie by first: xa, the first by bytes, is the last


def store_buffers(cell):
    """[(text, records, parts)] of the cell's buffers, lines numbered on from buffer to buffer."""
    out, lines = [], 0
    for text in cell["buffers"]:
        records, parts = vc.re_parts(cell["pset"], text)
        out.append((text, [(r[0] + lines, r[1], r[2]) for r in records], [(p[0] + lines, p[1], p[2], p[3]) for p in parts]))
        lines += text.count(b"\n")
    return out


def group_values(text, records, parts):
    """The call's distinct values in the order of their first parts: the order of the replay's groups (by bytes)."""
    start = {r[0]: r[1] for r in records}
    return list(dict.fromkeys(text[start[p[0]] + p[1]:start[p[0]] + p[2]] for p in parts))


def prove_store(cell, k, text, records, parts, tr, traces, proved):
    """The claims of a store cell after its call k (by bytes), from valstoresim's read-outs; proved counts them by name."""
    name, call = cell["name"], tr["call"]
    values = group_values(text, records, parts)
    assert len(values) == len(tr["groups"])
    for what, at, arg in cell["claims"]:
        if what == "store_chain" and k == at:
            found, new = (tr["groups"][values.index(v)] for v in arg)
            assert call["log2_old"] == 10 and found["found"] == 1 and found["wrapped"] == 1 and found["probes"] >= 3, (name, found)
            assert new["found"] == 0 and new["wrapped"] == 1 and new["probes"] >= 4, (name, new)  # (the empty slot behind the wrap ends it)
            assert found["tier"] == new["tier"] == (2 if len(arg[0]) > vc.LANE_MAX else 1)
            proved["store_chain"] = proved.get("store_chain", 0) + 1
        if what == "rehash" and k in (1, 2):
            old = (10, 11)[k - 1]
            assert (call["log2_old"], call["log2_new"], call["rehashed"]) == (old, old + 1, 1), (name, call)
            stored = tr["values"][:len(traces[k - 1]["values"])]  # the values the call found in the store
            moves = {v["home_new"] - v["home_old"] for v in stored}
            assert moves == {0, 1 << old} and all(v["home_new"] & ((1 << old) - 1) == v["home_old"] for v in stored), (name, moves)
            if k == 1:
                late = [tr["values"][len(stored) + [v for v in values if v not in set(vc.cand(i) for i in range(100000, 100400))].index(vc.cand(i))] for i in vc.HOME_2047]
                assert {v["home_new"] for v in late} == {2047} and {v["home_old"] for v in late} == {1023}, (name, late)
            proved["rehash"] = proved.get("rehash", 0) + 1
        if what == "rehash" and k == 3:
            assert all(g["found"] for g in tr["groups"]) and len(tr["groups"]) == 1500 and call["rehashed"] == 0 and call["new_bytes"] == 0, name
    if name.startswith("G/arena packing"):
        total = int(name.split(",")[1].split()[0])
        if k == 1:
            assert call["new_bytes"] == total and call["arena_tail"] == 4 and call["tail16"] == 16, (name, call)  # (xa and xq: 4 bytes before)
        if k == 2:
            assert call["arena_tail"] == 16 + total and call["tail16"] == (16 + total + 15) // 16 * 16 and call["new_bytes"] == 3, (name, call)
    if name.startswith("G/long-kernel stride") and k == 1:
        assert call["n_long"] == 4200 and all(g["found"] and g["tier"] == 2 for g in tr["groups"]), name  # (a grid of 4096 waves: two iterations)
    if name.startswith("G/one free slot") and k == 2:
        assert call["log2_new"] == 6 and len(tr["values"]) == 63, name


def test_store_cells():
    proved: dict = {}  # claim name -> how many were proved
    for cell in vc.GROUPS["G"]:
        for bp in (False, True):
            ref, sim = sr.Store(bp), ss.Store(by_pattern=bp, store_log2=cell.get("store_log2", 0), hash_bits=cell.get("hash_bits", 0))
            log2, traces = [], []
            for k, (text, records, parts) in enumerate(store_buffers(cell)):
                added = ref.add(text, parts, {(0, r[0]): r[1] for r in records})
                sim.add(text, records, parts)
                assert sim.info["n_added"] == added and sim.info["n_distinct"] == len(ref.table), (cell["name"], k)
                if "n_added" in cell:
                    assert added == cell["n_added"][k]
                log2.append(sim.info["store_log2"])
                tr = sim.trace()
                traces.append(tr)
                call = tr["call"]
                assert call["tail16"] % 16 == 0 and 0 <= call["tail16"] - call["arena_tail"] < 16 and call["log2_new"] == log2[-1], (cell["name"], call)
                assert call["new_bytes"] == sum(len(key[1] if bp else key) for key in list(ref.table)[len(ref.table) - added:]), (cell["name"], k)
                assert call["sort_bits"] == max(1, ref.n_parts.bit_length()) and len(tr["groups"]) == sim.info["n_groups"] and len(tr["values"]) == len(ref.table)
                assert sum(g["found"] for g in tr["groups"]) == sim.info["n_groups"] - added and call["n_long"] == sum(g["tier"] == 2 for g in tr["groups"])
                if not bp:
                    prove_store(cell, k, text, records, parts, tr, traces, proved)
                if "sort_bits" in cell and k == len(cell["buffers"]) - 1:
                    assert call["sort_bits"] == cell["sort_bits"] == max(ref.table.values(), key=lambda v: v[1])[1].bit_length(), (cell["name"], call)
                for what, at, arg in cell["claims"]:
                    if what == "pattern_decides" and bp and k == at:
                        # the call's groups in the order of first: (1, value) is new; every home is 0 or 1 and the stored values fill
                        # the slots from the smallest home on
                        keys = list(dict.fromkeys((p[3], text[{r[0]: r[1] for r in records}[p[0]] + p[1]:{r[0]: r[1] for r in records}[p[0]] + p[2]]) for p in parts))
                        mine = tr["groups"][keys.index((1, arg))]
                        stored = list(ref.table)[:len(traces[k - 1]["values"])]
                        homes = [v["home_new"] for v in tr["values"][:len(stored)]]
                        at_0 = stored.index((0, arg))
                        assert set(homes) <= {0, 1} and mine["found"] == 0 and mine["probes"] >= len(stored), (cell["name"], homes, mine)
                        # (it read every occupied slot and the empty one behind them, or all but slot 0, which is not (0, value)'s)
                        assert mine["probes"] == len(stored) + 1 or homes[at_0] == 1 or 0 in homes[:at_0], (cell["name"], homes, mine)
                        proved["pattern_decides"] = proved.get("pattern_decides", 0) + 1
                if ("two_expressions", None, None) in cell["claims"] and k == 1:  # the value's first part in buffer 2 is expression 1's, and buffer 1 had it under 0 only
                    values = [text[{r[0]: r[1] for r in records}[p[0]] + p[1]:{r[0]: r[1] for r in records}[p[0]] + p[2]] for p in parts]
                    v = max(values, key=len)
                    assert parts[values.index(v)][3] == 1 and {p[3] for p, w in zip(parts, values) if w == v} == {0, 1}, cell["name"]
                    assert sum((key[1] if bp else key) == v for key in ref.table) == (2 if bp else 1)  # one group by its bytes, two with the expression
            for top, order_first in cell.get("tops", ((0, False), (0, True), (2, False))):
                got, info = sim.rank(top, order_first)
                assert got == sr.arrays(ref.rows(top, order_first)), (cell["name"], bp, top, order_first)
                assert info == {"n_distinct": len(ref.table), "n_parts": ref.n_parts}
            if "refused" in cell:  # a 64th value in a table of 64 slots
                assert len(ref.table) == 63 and log2[-1] == 6
                records, parts = vc.re_parts(cell["pset"], cell["refused"])
                assert sim.add(cell["refused"], [r[:3] for r in records], [p[:4] for p in parts], allow_nomem=True) == ss.Store.NOMEM
                got, _info = sim.rank(0, False)
                assert got == sr.arrays(ref.rows(0, False)), cell["name"]  # the store keeps every row
            if "counts" in cell:
                assert {k: v[1] for k, v in ref.table.items() if (k[1] if bp else k) in cell["counts"]} == {((0, k) if bp else k): v for k, v in cell["counts"].items()}
            if cell["name"] == "G/growth over three calls":
                assert log2 == [11, 12, 12], log2  # 600, 1500 and 1500 values: the least 2^k of at least twice as many
            if "then_reset" in cell:  # a reset empties the store: what follows is a store of its own
                ref, sim, lines = sr.Store(bp), ss.Store(by_pattern=bp), 0
                for text in cell["then_reset"]:
                    records, parts = vc.re_parts(cell["pset"], text)
                    records, parts = [(r[0] + lines, r[1], r[2]) for r in records], [(p[0] + lines, p[1], p[2], p[3]) for p in parts]
                    added = ref.add(text, parts, {(0, r[0]): r[1] for r in records})
                    sim.add(text, records, parts)
                    call = sim.trace()["call"]
                    assert sim.info["n_added"] == added and (call["log2_old"], call["arena_tail"]) == ((0, 0) if not lines else (10, call["arena_tail"])), (cell["name"], call)
                    lines += text.count(b"\n")
                for top, order_first in ((0, False), (0, True)):
                    got, info = sim.rank(top, order_first)
                    assert got == sr.arrays(ref.rows(top, order_first)) and info == {"n_distinct": len(ref.table), "n_parts": ref.n_parts}, cell["name"]
    assert proved == {"store_chain": 2, "rehash": 2, "pattern_decides": 2}, proved


def test_a_part_without_a_record_has_no_value():
    """hg_values_locate returning 0.  No scan produces such a part (every part's piece is a final record: the GPU tests assert
    it for every cell), so the branch is held on the host alone: tier none, not counted, and later parts keep their indices."""
    cell = next(c for c in vc.GROUPS["D"] if c["pset"] == "X")
    text = cell["text"]
    records, parts = parts_of(cell)
    dropped = records[1][0]
    records = records[:1] + records[2:]
    starts = {(0, r[0]): r[1] for r in records}
    for bp in (False, True):
        want = vr.arrays(vr.groups(text, parts, starts, by_pattern=bp))
        for kw in ({}, {"hash_bits": 1}, {"table_log2": vc.tight(len(parts))}):
            got, info = vs.replay(text, records, parts, by_pattern=bp, trace=True, **kw)
            assert got == want and sum(want["count"]) == len(parts) - sum(p[0] == dropped for p in parts)
            assert [r["tier"] == 0 for r in info["parts"]] == [p[0] == dropped for p in parts] and info["call"]["no_value"] == sum(p[0] == dropped for p in parts) > 0
            rows, seg, n = rr.ranking(text, parts, starts, by_pattern=bp, per_segment=True, seg_start=[0], n_seg=1)
            got, got_seg, rinfo = rs.replay(text, records, parts, by_pattern=bp, per_segment=True, seg_start=[0], trace=True, **kw)
            assert got == rr.arrays(rows, segments=True) and got_seg == seg and [r["tier"] == 0 for r in rinfo["parts"]] == [p[0] == dropped for p in parts]


def test_recorded_values_are_what_the_search_finds():
    found = vc.home_search({1023: 3, 1022: 2, 0: 1})
    assert (tuple(found[1023]), tuple(found[1022]), tuple(found[0])) == (vc.HOME_LAST, vc.HOME_BEFORE_LAST, vc.HOME_ZERO)
    assert vc.home_search({1023: 1}, 257)[1023] == [vc.HOME_LAST_LONG]
    assert vc.chain_tag_search() == vc.CHAIN_TAGS
    assert vc.home_search({1023: 4})[1023][3] == vc.HOME_LAST_4TH and tuple(vc.home_search({1023: 4}, 257)[1023]) == vc.HOME_LAST_LONGS

    def low11(h):
        return h & 2047

    low11.keys = {2047: 3}
    assert tuple(vc.search(low11)[2047]) == vc.HOME_2047


def test_every_kind_of_claim_is_made():
    made = {c[0] for g in vc.TEXT_GROUPS for cell in vc.GROUPS[g] for c in cell["claims"]}
    assert made == {"path", "first_in_wave", "n_long", "long_iterations", "wrapped", "homes", "last_slot", "n_values", "free_slots", "slots", "chain_tags", "no_tag", "shared_chain", "passes",
                    "sort_bits", "two_expressions", "alignments"}
    leaders = {c[2][2] for cell in vc.GROUPS["A"] for c in cell["claims"] if c[0] == "path" and c[2][1] == 1}
    assert {0, 1, 31, 32, 63} <= leaders
