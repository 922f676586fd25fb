"""Many files in one scan on the MI355X: hg_scan_device_segments (the segment stage, hypergrep_amd/csrc/hg_segments.hip)
against the SAME device scanning every segment's bytes alone (hg_scan_device / hg_scan_device_invert): records, aux, starts of
match, n_lines and n_selected of every segment of every case of segments_ref.cases, plain and inverted, with and without a
limit.  Texts and segment arrays sit at the end of guarded buffers: a read past them faults."""
from __future__ import annotations

import pytest

import segments_ref as sr

pytestmark = pytest.mark.gpu

TILE = sr.TILE
SOM = 256
# a literal-anchored expression and an always-on one, so that both tiers feed the stage; NL adds one that matches the pad's "\n"
SET_AB = (["abc", "[0-9]+x|q"], [14, 14])
SET_NL = (["abc", "[0-9]+x|q", "\\n"], [14, 14, 14])
SET_SOM = (["a+b", "z"], [6 | SOM, 14])


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 20)
    yield a
    _scanners.clear()  # (before the interpreter takes the module's globals away)
    a.free()


_scanners = {}


def scanner(pset):
    from hypergrep_amd import device

    key = tuple(pset[0])
    if key not in _scanners:
        db = device.Database(pset[0], flags=pset[1], ids=list(range(1, len(pset[0]) + 1)))
        _scanners[key] = (device.Scanner(db, 0), db.info())
    return _scanners[key][0]


def alone(arena, sc, cache, data, bs, invert):
    """(records, starts of match, n_lines) of `data` scanned on its own."""
    key = (data, bs, invert)
    if key not in cache:
        st = sc.scan(arena.place(data), len(data), buffer_size=bs, invert=invert)
        cache[key] = (sc.hits(), sc.hit_starts().tolist(), st.n_lines)
    return cache[key]


def check(arena, pset, files, bs, invert, limits=(0,)):
    sc = scanner(pset)
    data, starts, ends = sr.pack(files)
    assert len(data) <= 1 << 20
    packed_stats = sc.scan(arena.place(data), len(data), buffer_size=bs, invert=invert)
    results = []
    for limit in limits:
        st = sc.scan(arena.place(data), len(data), buffer_size=bs, invert=invert, segments=(starts, ends), max_per_segment=limit)
        results.append((limit, st, sc.hits(), sc.hit_starts().tolist(), sc.segments()))
    cache = {}
    for limit, st, hits, froms, seg in results:
        assert (st.n_lines, st.n_candidates, st.n_raw_hits) == (packed_stats.n_lines, packed_stats.n_candidates, packed_stats.n_raw_hits)
        first = seg["first_record"].tolist()
        assert first[0] == 0 and first[-1] == st.n_hits == len(hits) and len(first) == len(files) + 1
        for s, f in enumerate(files):  # no segment is left out
            want_hits, want_from, want_lines = alone(arena, sc, cache, f, bs, invert)
            if limit:
                keep = len(sr.limited(want_hits, limit))
                want_hits, want_from = want_hits[:keep], want_from[:keep]
            lo, hi = first[s], first[s + 1]
            assert hits[lo:hi] == want_hits, (s, limit, invert, f[-24:])
            assert froms[lo:hi] == want_from, (s, limit)
            assert seg["record_segment"][lo:hi].tolist() == [s] * (hi - lo)
            assert seg["n_lines"][s] == want_lines, (s, f[-24:])
            assert seg["n_selected"][s] == len({h[0] for h in want_hits}), s
    return results


@pytest.mark.parametrize("bs", [8, 64, 262140])
@pytest.mark.parametrize("invert", [False, True])
def test_every_segment_equals_its_own_scan(arena, bs, invert):
    scanner(SET_AB)
    info = _scanners[tuple(SET_AB[0])][1]
    assert info["n_literal_anchored"] > 0 and info["n_always_on"] > 0, info
    # (pieces of 256 KiB: last lines of one piece's length only, the texts of two take seconds to compare)
    for name, files in sr.cases(TILE, bs, multiples=(1, 2) if bs < TILE else (1,)):
        try:
            check(arena, SET_AB, files, bs, invert, limits=(0, 1, 2, 10 ** 6))
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("bs", [8, 64])
def test_the_pads_newline_under_an_expression_that_matches_it(arena, bs):
    bs1 = bs - 1
    files = [(b"abc" * bs1)[:bs1 - 1], b"abc\n", (b"zq" * bs1)[:2 * bs1 - 1], b"", (b"zq" * bs1)[:bs1], b"q\n"]
    sc = scanner(SET_NL)
    data, starts, ends = sr.pack(files)
    sc.scan(arena.place(data), len(data), buffer_size=bs)
    pad_hits = [h for h in sc.hits() if h[1] == 3 and any(e <= h[3] < e + 2 for e, f in zip(ends, files) if f and not f.endswith(b"\n"))]
    assert pad_hits, "the packed scan must report the pads' newlines for this test to mean anything"
    for invert in (False, True):
        check(arena, SET_NL, files, bs, invert, limits=(0, 1, 2))
    for name, files in sr.cases(TILE, bs):  # the NUL-only last pieces among them: their scanned bytes are the pad's newline
        for invert in (False, True):
            try:
                check(arena, SET_NL, files, bs, invert, limits=(0, 2))
            except AssertionError as e:
                raise AssertionError(f"{name} invert={invert}: {e}") from e


def test_starts_of_match_follow_the_compaction(arena):
    files = [b"xaab aab\nab\n", (b"aab " * 9)[:13], b"q\n", b"zaaab\nz\nab ab ab\n", b"", b"ab"]
    for bs in (8, 64):
        results = check(arena, SET_SOM, files, bs, False, limits=(0, 1, 2))
        assert any(any(f > 0 for f in froms) for _, _, _, froms, _ in results)
        assert results[1][1].n_hits < results[0][1].n_hits  # the limit removed records, and the starts moved with the rest


@pytest.mark.parametrize("starts,ends,what", [
    ([0, 6, 3], [3, 9, 6], "ascending"),
    ([0, 3], [6, 9], "ascending"),
    ([0, 6], [7, 9], "ascending"),
    ([0, 6], [3, 13], "past the buffer"),
    ([0, 4], [3, 9], "line start"),
])
def test_malformed_segments_scan_nothing(arena, starts, ends, what):
    sc = scanner(SET_AB)
    data = b"qb\nqb\nqb\nqb\n"
    with pytest.raises(ValueError, match=what):
        sc.scan(arena.place(data), len(data), buffer_size=64, segments=(starts, ends))
    assert sc.hits() == []  # HG_ERR_ARG: nothing was scanned
    with pytest.raises(ValueError):
        sc.segments()
    st = sc.scan(arena.place(data), len(data), buffer_size=64, segments=([0, 6], [6, 12]))  # the scanner is fine afterwards
    assert st.n_hits == 4 and sc.segments()["n_lines"].tolist() == [2, 2]
