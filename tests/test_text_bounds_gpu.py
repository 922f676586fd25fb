"""No stage's result may depend on bytes outside the text (run with `-m gpu`): the window scans of bounds_cases.py on the
MI355X.  Every case's base text is uploaded once into a plain allocation; the GPU scans the window [lo, hi) of it with
d_text = base + lo and nbytes = hi - lo, so the bytes in front of and behind the text are the real continuation of it, and
every stage is held to its existing reference run on data[lo:hi] alone: the plain scan (five columns, hit_patterns, n_lines),
start of match and min_length, invert, context with the tail, matched parts, gathered lines, counts, the three segment stages,
and the plain scan in the second pipeline chunk.  Then the calls that stage the text themselves (Face A's scratch, Face B's
pooled buffers): a long text, a prefix of it, a prefix of that, each against the reference of its own bytes.

That every window is hostile (its answer changes with the leak its class is about), the floors and the placement:
test_text_bounds.py.  A failure names the case, the window and its class tag."""
from __future__ import annotations

import re

import numpy as np
import pytest

import bounds_cases as bc
import confirm_cells as cc
import context_ref
import counts_ref
import gather_ref
import invert_ref

pytestmark = pytest.mark.gpu

CASES = bc.NAMES
QUIET_BYTES = 17 << 20  # in front of the text of the chunked scan: past the first 16 MiB pipeline chunk


@pytest.fixture(scope="module")
def base():
    """name -> (torch uint8 tensor of the whole base text, frame included; uploaded once, never written again)."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    out = {name: torch.frombuffer(bytearray(bc.case(name).data), dtype=torch.uint8).cuda() for name in CASES}
    torch.cuda.synchronize()
    return out


def _fail(stage: str, name: str, bad: list, n: int):
    classes = sorted(set(re.findall(r" mod 16\) (\S+) ", "\n".join(bad))))
    pytest.fail(f"{stage} {name}: {len(bad)} of {n} window scans differ from the reference of the window's own bytes; class tags {classes}\n" + "\n".join(bad[:12]))


def _db(c, shared=False, flags=None, ext=None):
    from hypergrep_amd import device

    return device.Database(c.patterns, flags=flags or c.flags, ids=c.ids(shared), ext=ext)


@pytest.mark.parametrize("shared", (False, True), ids=("distinct_ids", "one_id"))
@pytest.mark.parametrize("name", CASES)
def test_plain_scan(base, name, shared):
    from hypergrep_amd import device

    c = bc.case(name)
    ptr = base[name].data_ptr()
    scanner = device.Scanner(_db(c, shared), 0)
    bad, n = [], 0
    for w in c.windows:
        for bs in bc.SIZES:
            want, nlines = bc.window_reference(name, w, bs, shared)
            stats = scanner.scan(ptr + w.lo, w.hi - w.lo, buffer_size=bs)
            raw = scanner.hits_array()
            got = cc.sort_hits(raw)
            n += 1
            if stats.n_lines != nlines:
                bad.append(f"{c.what(w)} buffer_size {bs}: {stats.n_lines} lines, want {nlines}")
            if got.shape != want.shape or not (got == want).all():
                bad.append(f"{bc.diff_report(c, w, got, want)} (buffer_size {bs})")
            elif not shared and not (scanner.hit_patterns() == raw[:, 1]).all():  # distinct ids: the id names the expression
                bad.append(f"{c.what(w)} buffer_size {bs}: hit_patterns differ from the ids")
            elif shared:  # one id: the expression of every report is one that reports that (line, to) under an id of its own
                own = {(int(r[0]), int(r[2]), int(r[1])) for r in bc.window_reference(name, w, bs, False)[0]}
                named = set(zip(raw[:, 0].tolist(), raw[:, 2].tolist(), scanner.hit_patterns().tolist()))
                if not named <= own:
                    bad.append(f"{c.what(w)} buffer_size {bs}: hit_patterns name {sorted(named - own)[:4]}, which the expression alone does not report")
    if bad:
        _fail("plain scan", name, bad, n)


SOM_CASES = tuple(n for n in CASES if n != "huge")  # (the huge automaton is above HG_MAX_NODES: no start of match, no parts)
# the true start lies before lo (L1, L4); ^ and \b hold at window offset 0 whatever text[lo - 1] is (L2, L3); the match needs
# bytes behind hi (R2)
SOM_CLASSES = ("L1", "L2", "L3", "L4", "R2")


@pytest.mark.parametrize("name", SOM_CASES)
def test_start_of_match(base, name):
    """HS_FLAG_SOM_LEFTMOST (hg_som.hip walks back from the match end): no start before the window, no report from behind it."""
    import somsim_py
    from hypergrep_amd import device

    c = bc.case(name)
    flags = [(f & ~8) | somsim_py.SOM for f in c.flags]  # (start of match is not offered with SINGLEMATCH)
    plain = [f & ~8 for f in c.flags]
    ptr = base[name].data_ptr()
    scanner = device.Scanner(_db(c, flags=flags), 0)
    bad, n, checked = [], 0, 0
    for w in c.windows:
        if w.base_cls not in SOM_CLASSES:
            continue
        data = c.data[w.lo:w.hi]
        want, _ = bc.window_reference(name, w, flags=plain)
        scanner.scan(ptr + w.lo, w.hi - w.lo)
        raw, starts = scanner.hits_array(), scanner.hit_starts()
        order = np.lexsort(tuple(raw[:, col] for col in range(4, -1, -1)))
        got, starts = raw[order], starts[order]
        n += 1
        if got.shape != want.shape or not (got == want).all():
            bad.append(bc.diff_report(c, w, got, want))
            continue
        froms = bc.starts_of(c, lambda r: data[int(r[3]):int(r[3]) + int(r[4])], want)
        checked += len(froms)
        if starts.tolist() != froms:
            k = next(i for i, (a, b) in enumerate(zip(starts.tolist(), froms)) if a != b)
            bad.append(f"{c.what(w)}: start {int(starts[k])} of {tuple(int(x) for x in got[k])}, want {froms[k]}")
    assert checked >= 100, checked
    if bad:
        _fail("start of match", name, bad, n)


MIN_LENGTHS = {
    "literal": {"needle_sa_[0-9]+x": 13, "needle_ga_[0-9]*": 12, r"[a-z]{0,20}needle_cf_11[0-9]{1,20}\b": 16},
    # [0-9]+x: "34x" at the start of an L4 window is too short, "1234x" with the two digits in front of lo would not be
    "always_on_free": {"[0-9]+x": 4, "[a-z]+@[a-z]+": 8, "[X-Z]{2,3}": 3},
}
_MINLEN_PIECE = {}


@pytest.mark.parametrize("name", sorted(MIN_LENGTHS))
def test_min_length(base, name):
    import minlensim_py
    import somsim_py
    from hypergrep_amd import device

    c = bc.case(name)
    need = [MIN_LENGTHS[name].get(p) for p in c.patterns]
    ids = c.ids(False)
    ptr = base[name].data_ptr()
    scanner = device.Scanner(_db(c, ext=minlensim_py.exts_for(need)), 0)
    bad, n, total, plain_total = [], 0, 0, 0
    for w in c.windows:
        if w.base_cls not in SOM_CLASSES or w.hi - w.lo > 600:  # (the brute force runs once per distinct piece)
            continue
        data = c.data[w.lo:w.hi]
        want = []
        for idx, _a, piece in somsim_py.pieces(data, bc.DEFAULT_BS):
            key = (name, piece)
            if key not in _MINLEN_PIECE:
                _MINLEN_PIECE[key] = minlensim_py.expected_piece(c.patterns, c.flags, ids, need, piece)
            want += [(idx, rid, to) for rid, to, _ in _MINLEN_PIECE[key]]
        scanner.scan(ptr + w.lo, w.hi - w.lo)
        got = sorted((h[0], h[1], h[2]) for h in scanner.hits())
        n += 1
        total += len(want)
        plain_total += len(bc.window_reference(name, w)[0])
        if got != sorted(want):
            bad.append(f"{c.what(w)}: missing {sorted(set(want) - set(got))[:4]}; extra {sorted(set(got) - set(want))[:4]}")
    assert 50 <= total < plain_total, (total, plain_total)  # the parameter removes some reports and keeps others
    if bad:
        _fail("min_length", name, bad, n)


CONTEXT = (2, 3)


@pytest.mark.parametrize("name", CASES)
def test_invert_context_gather_counts(base, name):
    """The stages that walk the text's lines themselves: invert (the pieces without a report), context with the tail (context
    after the last hit stops at hi, context before the first hit at lo), the gathered lines byte for byte (no byte from
    behind hi), and the counts per id."""
    from hypergrep_amd import device

    c = bc.case(name)
    ptr = base[name].data_ptr()
    scanner = device.Scanner(_db(c), 0)
    flags = gather_ref.CONTEXT | gather_ref.TERMINATE | gather_ref.NUMBER
    bad, n = [], 0
    for w in c.windows:
        data = c.data[w.lo:w.hi]
        d_text, nbytes = ptr + w.lo, w.hi - w.lo
        for bs in (bc.SIZES if w.base_cls in bc.GEOMETRY else bc.SIZES[:1]):  # (pieces of 63 bytes: where the edge is a line's)
            rows, nlines = bc.window_reference(name, w, bs)
            lines = sorted({int(r[0]) for r in rows})
            what = f"{c.what(w)} buffer_size {bs}"
            n += 1
            stats = scanner.scan(d_text, nbytes, buffer_size=bs, invert=True)
            if scanner.hits() != invert_ref.expected(data, bs, lines) or stats.n_lines != nlines:
                bad.append(f"{what}: invert")
            stats = scanner.scan(d_text, nbytes, buffer_size=bs, context=CONTEXT, tail=True)
            want_ctx, owed, n_tail = context_ref.expected(data, bs, lines, *CONTEXT, tail=True)
            got = cc.sort_hits(scanner.hits_array())
            if got.shape != rows.shape or not (got == rows).all():
                bad.append(f"{what}: the records of the scan with context")
            if scanner.context() != want_ctx or (stats.owed_after, stats.n_tail) != (owed, n_tail):
                bad.append(f"{what}: context ({stats.n_context} records, want {len(want_ctx)}; owed {stats.owed_after}, want {owed}; tail {stats.n_tail}, want {n_tail})")
            scanner.gather(d_text, nbytes, context=True, terminate=True, number=True)
            want_lines, _ = gather_ref.expected(data, bs, lines, flags, context=CONTEXT, tail=True)
            if scanner.lines() != want_lines:
                bad.append(f"{what}: gathered lines with context")
            scanner.scan(d_text, nbytes, buffer_size=bs)
            scanner.gather(d_text, nbytes, terminate=True, number=True)
            want_lines, _ = gather_ref.expected(data, bs, lines, gather_ref.TERMINATE | gather_ref.NUMBER)
            if scanner.lines() != want_lines:
                bad.append(f"{what}: gathered lines")
            scanner.count()
            want_counts = counts_ref.counts((0, int(r[0]), int(r[1])) for r in rows)
            if {k: v for k, v in scanner.counts().items() if v != (0, 0)} != want_counts:
                bad.append(f"{what}: counts")
    if bad:
        _fail("invert / context / gather / counts", name, bad, n)


_PARTS_PIECE = {}


def _parts_expected(c, data: bytes, bs: int, lines) -> list:
    """parts_ref.expected with the parts of a piece computed once per distinct piece."""
    import parts_ref

    wanted, out = set(lines), []
    for i, (_a, piece) in enumerate(invert_ref.pieces(data, bs)):
        if i in wanted:
            key = (c.name, piece)
            if key not in _PARTS_PIECE:
                _PARTS_PIECE[key] = parts_ref.piece_parts(c.patterns, c.flags, piece)
            out += [(i, f, t, p) for f, t, p in _PARTS_PIECE[key]]
    return out


def _parts_windows(c):
    """The windows of the parts stages: the brute force tries every (start, end) pair of a piece, so the windows of a row or
    a tile are left to the other stages."""
    return [w for w in c.windows if w.hi - w.lo <= 800]


@pytest.mark.parametrize("name", SOM_CASES)
def test_matched_parts(base, name):
    from hypergrep_amd import device

    c = bc.case(name)
    ptr = base[name].data_ptr()
    scanner = device.Scanner(_db(c), 0)
    bad, n, total = [], 0, 0
    for w in _parts_windows(c):
        data = c.data[w.lo:w.hi]
        rows, nlines = bc.window_reference(name, w)
        scanner.scan(ptr + w.lo, w.hi - w.lo, parts=True)
        want = _parts_expected(c, data, bc.DEFAULT_BS, {int(r[0]) for r in rows})
        got = cc.sort_hits(scanner.hits_array())
        n += 1
        total += len(want)
        if got.shape != rows.shape or not (got == rows).all():
            bad.append(f"{bc.diff_report(c, w, got, rows)} (the records of the scan with parts)")
        got_parts = scanner.parts()
        if got_parts != want:
            bad.append(f"{c.what(w)}: parts: missing {sorted(set(want) - set(got_parts))[:4]}; extra {sorted(set(got_parts) - set(want))[:4]}")
    assert total >= 200, total
    if bad:
        _fail("matched parts", name, bad, n)


@pytest.mark.parametrize("name", CASES)
def test_segments(base, name):
    """hg_scan_device_segments, _segments_context and _segments_parts: every file's records, context and parts are those of
    the file's own bytes."""
    from hypergrep_amd import device

    c = bc.case(name)
    ptr = base[name].data_ptr()
    scanner = device.Scanner(_db(c), 0)
    with_parts = name in SOM_CASES
    bad, n = [], 0
    for w in c.windows:
        data = c.data[w.lo:w.hi]
        d_text, nbytes = ptr + w.lo, w.hi - w.lo
        starts, ends = bc.files_of(c, w)
        per_file = [bc.reference(name, w.lo + a, w.lo + z) for a, z in zip(starts, ends)]
        n += 1
        what = f"{c.what(w)} files {list(zip(starts, ends))}"
        scanner.scan(d_text, nbytes, segments=(starts, ends))
        got, seg = scanner.hits_array(), scanner.segments()
        first = seg["first_record"].tolist()
        for s, (rows, nlines) in enumerate(per_file):
            mine = cc.sort_hits(got[first[s]:first[s + 1]])
            if mine.shape != rows.shape or not (mine == rows).all() or int(seg["n_lines"][s]) != nlines or int(seg["n_selected"][s]) != len({int(r[0]) for r in rows}):
                bad.append(f"{what}: segment {s}: {len(mine)} records, want {len(rows)}; {int(seg['n_lines'][s])} lines, want {nlines}")
        scanner.scan(d_text, nbytes, segments=(starts, ends), context=CONTEXT)
        ctx, sc = scanner.context(), scanner.segment_context()
        first = sc["first_context"].tolist()
        for s, ((rows, _), a, z) in enumerate(zip(per_file, starts, ends)):
            want, _, _ = context_ref.expected(data[a:z], bc.DEFAULT_BS, sorted({int(r[0]) for r in rows}), *CONTEXT)
            if ctx[first[s]:first[s + 1]] != want:
                bad.append(f"{what}: segment {s}: context {ctx[first[s]:first[s + 1]][:3]}, want {want[:3]}")
        if with_parts and nbytes <= 800:
            scanner.scan(d_text, nbytes, segments=(starts, ends), segment_parts=True)
            parts, sp = scanner.parts(), scanner.segment_parts()
            first = sp["first_part"].tolist()
            for s, ((rows, _), a, z) in enumerate(zip(per_file, starts, ends)):
                want = _parts_expected(c, data[a:z], bc.DEFAULT_BS, {int(r[0]) for r in rows})
                if parts[first[s]:first[s + 1]] != want:
                    bad.append(f"{what}: segment {s}: parts {parts[first[s]:first[s + 1]][:3]}, want {want[:3]}")
    if bad:
        _fail("segments", name, bad, n)


@pytest.mark.parametrize("ahead", (None, "1"), ids=("default", "joiner_ahead_1"))
def test_right_edges_in_the_second_pipeline_chunk(base, monkeypatch, ahead):
    """The literal case behind 17 MiB of quiet lines, in pipeline chunks of 1024 tiles: the window's last, partial tile belongs
    to the second chunk, and with HG_JOINER_AHEAD=1 a joiner instantiation handles it.  Right-edge windows: d_text is the start of
    the allocation, nbytes = 17 MiB + hi."""
    import torch
    from hypergrep_amd import device

    name = "literal"
    c = bc.case(name)
    rng = np.random.default_rng(7)
    quiet = np.frombuffer(bc.FILL, dtype=np.uint8)[rng.integers(0, len(bc.FILL), size=QUIET_BYTES)]
    quiet[rng.random(QUIET_BYTES) < 1 / 100] = 10
    quiet[-1] = 10
    qlines = int((quiet == 10).sum())
    buf = torch.cat([torch.from_numpy(quiet).cuda(), base[name]])
    torch.cuda.synchronize()
    monkeypatch.setenv("HG_CHUNK_TILES", "1024")  # (env knobs are read when the scanner is created)
    if ahead:  # (as test_stream_variants_gpu.py::test_joiner_cell: the joiner streams the tiles of every chunk but the first)
        monkeypatch.setenv("HG_JOINER", "2")
        monkeypatch.setenv("HG_JOINER_AHEAD", ahead)
    scanner = device.Scanner(_db(c), 0)
    shift = np.array([qlines, 0, 0, QUIET_BYTES, 0], dtype=np.uint64)
    bad, n, launches, joined = [], 0, 0, 0
    his = {}
    for w in c.windows:
        if w.side == "R" and w.cls != "R5":  # (rows and tiles count from the allocation's start here: R5 has no meaning)
            his.setdefault(w.hi, w)
    for hi, w in sorted(his.items()):
        want, nlines = bc.reference(name, 0, hi)
        stats = scanner.scan(buf.data_ptr(), QUIET_BYTES + hi)
        got = cc.sort_hits(scanner.hits_array())
        want = want + shift if len(want) else want
        n += 1
        launches = max(launches, stats.stream_launches)
        joined += stats.joiner_tiles
        if stats.n_lines != qlines + nlines:
            bad.append(f"{c.what(w)}: {stats.n_lines} lines, want {qlines + nlines}")
        if got.shape != want.shape or not (got == want).all():
            bad.append(bc.diff_report(c, w, got, want))
    assert launches >= 2 and n >= 60 and (joined > 0 or not ahead), (launches, n, joined)
    if bad:
        _fail("second pipeline chunk", name, bad, n)


# ------------------------------------------------------------------ stale staging: the caller has no device pointer to offset
def _prefix_chains(c, long_blocks: bool, per_tag: int = 2) -> list:
    """(window, [long, prefix, prefix of the prefix]) byte strings: the long text runs on behind hi with the base text's
    matches and newlines, the first prefix ends at the window's hi (cut by its class, R1-R4 or R6), the second at an earlier
    window's hi where one lies inside, else a few bytes in front."""
    his = sorted({w.hi for w in c.windows if w.side == "R"})
    out, taken = [], {}
    for w in c.windows:
        if w.side != "R" or (w.cls == "R5") != long_blocks or (long_blocks and "tile" not in w.tag):
            continue
        key = w.tag.split("/")[0] if not long_blocks else w.tag.split(":")[0]
        if taken.get(key, 0) >= per_tag:
            continue
        taken[key] = taken.get(key, 0) + 1
        inner = [h for h in his if w.lo + 32 < h < w.hi]
        hi2 = inner[-1] if inner else w.hi - 5
        out.append((w, [c.data[w.lo:w.hi + (4096 if long_blocks else 7000 - (w.hi - w.lo))], c.data[w.lo:w.hi], c.data[w.lo:hi2]]))
    return out


@pytest.mark.parametrize("name", CASES)
def test_face_a_scratch_holds_the_longer_text(base, name):
    """hs_scan and hg_scan_blocks stage the caller's bytes in the scratch's own buffers, which are reused: behind a block lies
    what the previous, longer call left there.  What each regime can show (the routing is hg_hsface.hip's, by block length
    and database; no export tells which kernel ran, so it is not asserted here: test_blockbatch_gpu.py and
    test_streammode_gpu.py own it):
      * the general path (block_general: hipMemcpy of `length` bytes into the scratch's device text, then scan_block) leaves
        the stale continuation right behind the block.  Blocks above 8 KiB take it, and every block of a database with
        start of match does: the second database below sends the SHORT chains through it too, so the one-byte leaks of
        R2 / R3 / R4 meet real stale text there.
      * the one-launch paths (blocks of at most 8 KiB through launch_block_small, the items hg_batch_pack packs) write zeros
        into the round-up to 16 behind a block, so a leak inside the round-up meets zeros unless the length is a multiple
        of 16 (the windows of residue 0, where the stale bytes follow at once); what these scans hold is the stale text from
        the next 16-byte boundary on (rows and tiles of matches and newlines behind the block).  In a batch only item 0
        lies where its own longer text lay; the later items lie inside other items' old bytes."""
    import somsim_py
    from hypergrep_amd import device

    c = bc.case(name)
    bdb = device.BlockDatabase(c.patterns, c.flags, c.ids(False))
    som_flags = [(f & ~8) | somsim_py.SOM for f in c.flags]
    bdb_som = device.BlockDatabase(c.patterns, som_flags, c.ids(False)) if name != "huge" else None  # (general path at every length)
    bad, n, total = [], 0, 0
    for long_blocks in (False, True):
        chains = _prefix_chains(c, long_blocks)
        assert len(chains) >= 3, (name, long_blocks)
        assert all((len(t[0]) > 8192) == long_blocks and len(t[0]) > len(t[1]) > len(t[2]) for _, t in chains)
        for w, texts in chains:
            for step, data in enumerate(texts):
                want = bc.block_reference(c, data)
                n += 1
                total += len(want)
                if bdb.scan(data) != want:
                    bad.append(f"{c.what(w)}: hs_scan, step {step} ({len(data)} bytes)")
                if bdb_som is not None and not long_blocks:
                    n += 1
                    if bdb_som.scan(data) != bc.block_reference(c, data, som_flags, som=True):
                        bad.append(f"{c.what(w)}: hs_scan with start of match (general path), step {step} ({len(data)} bytes)")
        for step in range(3):  # one batch per step: item 0 lies where its longer text of the step before lay
            got = bdb.scan_blocks([texts[step] for _, texts in chains])
            for (w, texts), reports in zip(chains, got):
                n += 1
                if reports != bc.block_reference(c, texts[step]):
                    bad.append(f"{c.what(w)}: hg_scan_blocks, step {step} ({len(texts[step])} bytes)")
    assert total >= (30 if name == "huge" else 200), total  # (huge: SINGLEMATCH holds for the block, one report per scan)
    if bad:
        _fail("Face A block scans", name, bad, n)


@pytest.mark.parametrize("som", (False, True), ids=("ends", "som_horizon"))
@pytest.mark.parametrize("name", ("literal", "always_on_free"))
def test_stream_writes_after_a_longer_write(base, name, som):
    """Stream mode (hg_flow_scan_kernel; with a horizon hg_flow_som_kernel): one write per stream, a long one, a prefix of it,
    a prefix of that, on the one scratch of the database.  The staging writes zeros into the round-up to 16 behind a write:
    a leak inside the round-up meets zeros unless the length is a multiple of 16; what is held is the stale text from the
    next 16-byte boundary on."""
    import somsim_py
    from hypergrep_amd import device

    c = bc.case(name)
    flags = [(f & ~8) | somsim_py.SOM for f in c.flags] if som else c.flags
    sdb = device.StreamDatabase(c.patterns, flags, c.ids(False), som_horizon="large" if som else None)
    bad, n, total = [], 0, 0
    for long_blocks in (False, True):
        for w, texts in _prefix_chains(c, long_blocks, per_tag=1 if som else 2):
            for step, data in enumerate(texts):
                s = sdb.open()
                got = s.scan(data) + s.close()
                want = bc.block_reference(c, data, flags, som)
                n += 1
                total += len(want)
                if sorted(got) != sorted(want):
                    bad.append(f"{c.what(w)}: stream write, step {step} ({len(data)} bytes): {len(got)} reports, want {len(want)}")
    assert total >= 200, total
    if bad:
        _fail("stream writes", name, bad, n)


@pytest.mark.parametrize("route", ("per_file", "many_files"))
def test_file_api_pooled_buffers_hold_the_longer_file(base, route, tmp_path):
    """Face B: the pooled device buffers of a context are filled again for every batch and file; behind a short file lies the
    previous, longer one.  A large file, then files that are prefixes of it cut by R1-R4, against the oracle's rows (line
    number, id and the line's bytes) for each file."""
    import hypergrep_amd
    import oracle_py

    name = "literal"
    c = bc.case(name)
    picks, taken = [], {}
    for w in c.windows:
        if w.cls in ("R1", "R2", "R3", "R4") and taken.get(w.tag, 0) < 1:
            taken[w.tag] = 1
            picks.append(w)
    assert {w.cls for w in picks} == {"R1", "R2", "R3", "R4"} and len(picks) >= 12
    picks.sort(key=lambda w: -w.hi)  # every file shorter than the one before it
    files = [("large", c.data)] + [(f"prefix_{i}", c.data[:w.hi]) for i, w in enumerate(picks)]
    paths = []
    for fname, content in files:
        path = str(tmp_path / fname)
        with open(path, "wb") as handle:
            handle.write(content)
        paths.append(path)
    ids = c.ids(False)
    bad = []
    from hypergrep_amd import device

    before = None
    for i, path in enumerate(paths):
        rows = []
        if route == "per_file":
            hypergrep_amd.scan(path, c.patterns, lambda m, k: rows.extend((m[j].line_number, m[j].id, m[j].line) for j in range(k)), flags=c.flags, ids=ids)
        else:
            hypergrep_amd.scan_files([path], c.patterns, lambda _index, m, k: rows.extend((m[j].line_number, m[j].id, m[j].line) for j in range(k)), flags=c.flags, ids=ids)
        stats = device.faceb_stats()
        if before is not None:  # the pooled context of the file before, with its buffers, not a fresh one
            assert stats["contexts_reused"] > before["contexts_reused"] and stats["contexts_created"] == before["contexts_created"], (files[i][0], before, stats)
        before = stats
        rc, want, _ = oracle_py.scan_file(path, c.patterns, flags=c.flags, ids=ids)
        assert rc >= 0 and (i > 0 or len(want) >= 200)
        if sorted(rows) != sorted(want):
            w = picks[i - 1] if i else None
            bad.append(f"{files[i][0]} ({len(files[i][1])} bytes{', ' + c.what(w) if w else ''}): {len(rows)} rows, want {len(want)}; "
                       f"missing {sorted(set(want) - set(rows))[:2]}; extra {sorted(set(rows) - set(want))[:2]}")
    if bad:
        _fail(f"file API ({route})", name, bad, len(paths))
