"""The stream-mode cells (flow_cells.py) are sound, without a GPU: every coverage claim holds under the restated constants, the
groups are staged or not as their cells say (flowsim's read-out of the kernel's formula), the reference's ends equal the
oracle's hs_scan of the concatenation (no product code), the reference equals the host replay of the kernel's decomposition
(flowsim / flowsomsim with the kernel's piece size and the group's lane count), and no cell compares more reports by a window
of calls than its expressions with assertions have.  The GPU side: test_flow_cells_gpu.py."""
from __future__ import annotations

import ctypes
import os

import pytest

import flow_cells as fc
import flowsim_py
import flowsomsim_py
import oracle_py

HANDLER = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_void_p)


class _HsErr(ctypes.Structure):
    _fields_ = [("message", ctypes.c_char_p), ("expression", ctypes.c_int)]


_oracle = None


def oracle_lib():
    global _oracle
    if _oracle is None:
        oracle_py.lib()  # (builds the oracle if it is missing)
        l = _oracle = ctypes.CDLL(os.path.join(oracle_py.ORACLE_DIR, "_build", "libhs.so.5"))
        vp, u = ctypes.c_void_p, ctypes.c_uint
        l.hs_compile_multi.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(u), ctypes.POINTER(u), u, u, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.POINTER(_HsErr))]
        l.hs_alloc_scratch.argtypes = [vp, ctypes.POINTER(vp)]
        l.hs_scan.argtypes = [vp, ctypes.c_char_p, u, u, vp, HANDLER, vp]
        l.hs_free_scratch.argtypes = [vp]
        l.hs_free_database.argtypes = [vp]
        l.hs_free_compile_error.argtypes = [vp]
    return _oracle


class OracleDb:
    """The cell's expressions in the oracle's block mode (start of match is not asked of it: the flag is taken off)."""

    def __init__(self, cell):
        l = oracle_lib()
        n = len(cell.patterns)
        pa = (ctypes.c_char_p * n)(*[p.encode() for p in cell.patterns])
        fa = (ctypes.c_uint * n)(*[f & ~fc.SOM for f in cell.flags])
        ia = (ctypes.c_uint * n)(*cell.ids)
        self.db, self.scratch = ctypes.c_void_p(), ctypes.c_void_p()
        err = ctypes.POINTER(_HsErr)()
        rc = l.hs_compile_multi(pa, fa, ia, n, 1, None, ctypes.byref(self.db), ctypes.byref(err))
        msg = err.contents.message if err else b""
        assert rc == 0, msg
        assert l.hs_alloc_scratch(self.db, ctypes.byref(self.scratch)) == 0

    def scan(self, data: bytes):
        out = []
        cb = HANDLER(lambda i, f, t, fl, c: out.append((i, t)) or 0)
        assert oracle_lib().hs_scan(self.db, data, len(data), 0, self.scratch, cb, None) == 0
        return out

    def __del__(self):
        oracle_lib().hs_free_scratch(self.scratch)
        oracle_lib().hs_free_database(self.db)


def unique_runs(cell):
    seen, out = set(), []
    for r in cell.runs:
        if id(r) not in seen:
            seen.add(id(r))
            out.append(r)
    return out


CELL_IDS = dict(ids=lambda c: c.name)


def test_every_family_and_shape_is_present():
    names = set(fc.BY_NAME)
    for npat in (1, 2, 3, 7, 8, 31, 32):
        assert any(n.startswith(f"slices-n{npat}-") for n in names)
        have = {p for n in names if n.startswith(f"slices-n{npat}-") for p in fc.BY_NAME[n].patterns}
        assert {"wxyz", "ab+c", "a+b", "st.*us"} <= have
    for n in (1, 32, 33, 64, 65):
        assert f"groups-{n}" in names
    for n in (1, 2, 63, 64, 65, 300):
        assert len(fc.BY_NAME[f"items-{n}"].runs) == n
    for n in (1, 8, 63, 64, 65, 130):
        assert len(fc.BY_NAME[f"som-items-{n}"].runs) == n
    assert all(r.label.startswith("all-alive") for r in fc.BY_NAME["som-items-8"].runs) and 8 * sum(f & fc.SOM != 0 for f in fc.SOM_SET[1]) <= 64
    assert {"contexts", "pieces", "pieces-staged", "shared-ends-3", "shared-ends-two-groups", "held-newline", "singlematch", "singlematch-shared-id-two-groups",
            "hbm-below", "hbm-above", "overflow", "overflow-som", "som-small", "som-medium", "som-large"} <= names
    assert any(c.staged.get(0) is True for c in fc.CELLS) and any(c.staged.get(0) is False for c in fc.CELLS)
    ends = {r.end for c in fc.CELLS for r in c.runs}
    assert ends == {"close", "last"}
    assert any(a == b for c in fc.CELLS for r in c.runs for a, b in r.writes()[:-1])  # a zero-length write that is no close
    assert max(b - a for c in fc.CELLS for r in c.runs for a, b in r.writes()) == 3 * fc.PIECE + 1


def test_restated_constants_are_the_product_s():
    """The coverage claims lean on these; the expectations do not."""
    src = open(os.path.join(flowsim_py.CSRC, "hg_core.h"), encoding="utf-8").read() + open(os.path.join(flowsim_py.CSRC, "hg_engine.h"), encoding="utf-8").read() + \
        open(os.path.join(flowsim_py.CSRC, "hg_flows.h"), encoding="utf-8").read() + open(os.path.join(flowsim_py.CSRC, "hg_flows.hip"), encoding="utf-8").read()
    for text in (f"HG_FLOW_PIECE = {fc.PIECE};", f"HG_FLOW_PPW = {fc.PPW};", f"HG_BLOCK_SMALL_POOL = {fc.POOL};", "HG_FLOW_HBM_MIN_DEFAULT = 1u << 20;",
                 f"__launch_bounds__({fc.LANES}) void hg_flow_scan_kernel", f"max({fc.MIN_SLICE}u, (plen + most - 1) / most)", "dim3(256), 0, stream, args)"):
        assert text in src, text
    face = open(os.path.join(flowsim_py.CSRC, "hg_hsface.hip"), encoding="utf-8").read()
    assert f"std::max<size_t>(st.out.cap(), {fc.FIRST_CAP})" in face and "bytes * f.ngroups >= flow_hbm_min() || !f.som.empty()" in face


@pytest.mark.parametrize("cell", fc.CELLS, **CELL_IDS)
def test_claims_hold(cell):
    bad = [(r.label, text) for r in cell.runs for text, ok in r.claims if not ok] + [text for text, ok in cell.claims if not ok]
    assert not bad, bad[:10]
    assert sum(len(r.claims) for r in cell.runs) + len(cell.claims) > 0
    for r in cell.runs:
        assert r.cuts == sorted(r.cuts) and all(0 <= c <= len(r.data) for c in r.cuts) and r.end in ("close", "last"), r.label
    assert len({r.label for r in unique_runs(cell)}) == len(unique_runs(cell))


@pytest.mark.parametrize("cell", fc.CELLS, **CELL_IDS)
def test_staging_and_state_words(cell):
    db = flowsim_py.Db(cell.patterns, [f & ~fc.SOM for f in cell.flags], cell.ids)
    assert db.h, db.error
    assert set(cell.staged) == set(range(cell.ngroups()))
    for g, staged in cell.staged.items():
        assert (db.group_span(g) <= fc.POOL) == staged, (g, db.group_span(g))
    for e, (lo, hi) in cell.words.items():
        assert lo <= db.words(e) <= hi, (e, db.words(e))


def test_a_full_group_of_one_word_expressions_is_staged():
    """A full group of 32 one-word expressions is NOT over the pool here (the follow table has a row per node, five or six
    for these expressions, not 32): 9532 words.  One expression of 29 words in the group puts it over."""
    cell = fc.BY_NAME["slices-n32-s0"]
    db = flowsim_py.Db(cell.patterns, cell.flags, cell.ids)
    assert all(db.words(e) == 1 for e in range(32))
    assert 32 * (256 + 1 + 16 + 20) < db.group_span(0) <= fc.POOL < 32 * (256 + 32 + 1 + 16 + 20)
    cell = fc.BY_NAME["slices-n32-s0-unstaged"]
    db = flowsim_py.Db(cell.patterns, cell.flags, cell.ids)
    assert db.words(3) >= 28 and db.group_span(0) > fc.POOL


@pytest.mark.parametrize("cell", fc.CELLS, **CELL_IDS)
def test_reference_equals_the_oracle(cell):
    odb = OracleDb(cell)
    reports = 0
    for r in unique_runs(cell):
        want = sorted((w.key[0], w.key[-1]) for w in fc.reference(cell, r))
        assert want == sorted(odb.scan(r.data)), r.label
        reports += len(want)
    assert reports > 0


def replay_calls(cell, db, r):
    """[[report] per call] of the host replay, a "last" run's close folded into its last write."""
    if cell.horizon:
        rows = [(c, (i, f, t)) for c, i, f, t in db.run(r.data, r.cuts, cell.horizon)]
    else:
        raw = []
        for lanes, exprs in fc.cell_lanes(cell).items():
            raw += [x for x in db.run(r.data, r.cuts, piece=fc.PIECE, lanes=lanes, min_slice=fc.MIN_SLICE) if x[1] in exprs]
        rows = [(c, (i, t)) for c, i, t in db.deliver(r.data, r.cuts, sorted(raw))]
    calls = [[] for _ in range(len(r.cuts) + 2)]
    for c, rep in rows:
        calls[c].append(rep)
    if r.end == "last":
        tail = calls.pop()
        calls[-1] = sorted(calls[-1] + tail, key=lambda x: (x[-1], x[0]))
    return calls


@pytest.mark.parametrize("cell", fc.CELLS, **CELL_IDS)
def test_reference_equals_the_replay(cell):
    db = (flowsomsim_py if cell.horizon else flowsim_py).Db(cell.patterns, cell.flags, cell.ids)
    assert db.h, db.error
    for r in unique_runs(cell):
        errors, _ = fc.compare(cell, r, replay_calls(cell, db, r))
        assert not errors, (r.label, errors)


@pytest.mark.parametrize("cell", fc.CELLS, **CELL_IDS)
def test_only_assertions_are_compared_by_window(cell):
    """compare() excludes nothing; the call of a report is left open only inside the window the rules give, and only for
    expressions with assertions (and start-of-match expressions that share an id)."""
    for r in unique_runs(cell):
        want = fc.reference(cell, r)
        windowed = sum(w.lo < w.hi for w in want)
        assert windowed <= fc.windowed_cap(cell, r), r.label
        exact = [[w.key for w in want if w.lo == c] for c in range(r.ncalls())]
        errors, n = fc.compare(cell, r, exact)
        assert not errors and n == windowed, (r.label, errors)
        if want:  # a report one call late, or dropped, or doubled, is an error
            w = want[-1]
            late = [list(c) for c in exact]
            late[w.lo].remove(w.key)
            assert fc.compare(cell, r, late)[0]
            if w.hi + 1 < r.ncalls():
                late[w.hi + 1].append(w.key)
                assert fc.compare(cell, r, late)[0]
            twice = [list(c) for c in exact]
            twice[w.lo].append(w.key)
            assert fc.compare(cell, r, twice)[0]
