"""The cells of the parts stage on the MI355X: hg_parts_kernel (hg_scan_device_parts) and its second caller hg_segparts_kernel
(hg_scan_device_segments_parts) on every cell of parts_cells.py, and the launch geometry only a GPU shows (grid stride, head
test, scanner reuse, pipeline chunks).  Every expectation is parts_ref's plain Python reference; nothing of hg_parts.h is used.
Texts sit at the end of a guarded arena: a read past them faults."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest

import chunk_texts
import parts_cells as pc
import parts_ref
import segments_ref as sr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
A = 6
Q_S, Q_L3 = pc.q_db("S")[:2], pc.q_db("L3")[:2]  # the tier's expression with one- and two-byte alternatives, `q\\n`, `^\\n`

_scanners: dict = {}
_want: dict = {}  # (patterns, flags, text, buffer_size) -> (matching lines, parts_ref's rows): computed once, never changed
_line_parts: dict = {}


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


def scanner(pats, flags):
    from hypergrep_amd import device

    key = (tuple(pats), tuple(flags))
    if key not in _scanners:
        _scanners[key] = device.Scanner(device.Database(pats, flags=flags, ids=list(range(len(pats)))), 0)
    return _scanners[key]


def reference(pats, flags, text, bs):
    key = (tuple(pats), tuple(flags), text, bs)
    if key not in _want:
        lines = parts_ref.matching_lines(text, bs, pats, flags)
        _want[key] = (lines, parts_ref.expected(text, bs, pats, flags, lines))
    return _want[key]


def check_parts(arena, pats, flags, text, bs, want_lines, want):
    """scan(parts=True): parts() is `want` in full, n_parts its length, and hits() that of the plain scan."""
    sc = scanner(pats, flags)
    ptr = arena.place(text)
    plain = sc.scan(ptr, len(text), buffer_size=bs)
    plain_hits = sc.hits()
    assert sorted({h[0] for h in plain_hits}) == want_lines
    st = sc.scan(ptr, len(text), buffer_size=bs, parts=True)
    got = sc.parts()
    assert got == want, (len(got), len(want), [(g, w) for g, w in zip(got, want) if g != w][:4], got[len(want):][:4], want[len(got):][:4])
    assert st.n_parts == len(want)
    assert sc.hits() == plain_hits and (st.n_hits, st.n_lines) == (plain.n_hits, plain.n_lines)
    return st, plain_hits


def in_group(group, run):
    failed = []
    for cell in pc.GROUPS[group]:
        try:
            run(cell)
        except AssertionError as e:
            failed.append(f"{cell[0]}: {str(e)[:600]}")
    assert not failed, f"{len(failed)} of {len(pc.GROUPS[group])} cells failed:\n" + "\n".join(failed[:12])


@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_cells(arena, group):
    def run(cell):
        _name, pats, flags, text, bs, _claims = cell
        lines, want = reference(pats, flags, text, bs)
        check_parts(arena, pats, flags, text, bs, lines, want)

    in_group(group, run)


def segment_scan(arena, pats, flags, files, bs):
    """One packed scan with per-file parts: [(kept lines, parts)] per file, the segment beside each part checked."""
    sc = scanner(pats, flags)
    data, starts, ends = sr.pack(files)
    assert len(data) <= 1 << 20
    st = sc.scan(arena.place(data), len(data), buffer_size=bs, segments=(starts, ends), segment_parts=True)
    hits, rows, sp, seg = sc.hits(), sc.parts(), sc.segment_parts(), sc.segments()
    first, first_record = sp["first_part"].tolist(), seg["first_record"].tolist()
    assert len(rows) == st.n_parts and len(first) == len(files) + 1 and first[0] == 0 and first[-1] == st.n_parts
    out = []
    for s in range(len(files)):
        lo, hi = first[s], first[s + 1]
        assert sp["part_segment"][lo:hi].tolist() == [s] * (hi - lo), s
        out.append((sorted({h[0] for h in hits[first_record[s]:first_record[s + 1]]}), rows[lo:hi]))
    return out


@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_second_caller_one_file(arena, group):
    """Every cell as ONE file that covers the text: the parts are the parts scan's, the segment of each is 0."""
    def run(cell):
        _name, pats, flags, text, bs, _claims = cell
        lines, want = reference(pats, flags, text, bs)
        (kept, rows), = segment_scan(arena, pats, flags, [text], bs)
        assert kept == lines and rows == want, (kept, lines, rows[:4], want[:4])

    in_group(group, run)


@pytest.mark.parametrize("family", ["A", "B", "C"])
def test_second_caller_packed(arena, family):
    """The cells of a family that share a database and a buffer size, one file each in one packed scan behind a file of two
    quiet lines: per file parts_ref on that file alone, with file-relative line numbers.  The file in front gives every cell,
    also one whose database no other cell has, a segment and an offset into the packed text that are not 0."""
    packs = {}
    for group, cells in pc.GROUPS.items():
        if group.startswith(family):
            for _name, pats, flags, text, bs, _claims in cells:
                packs.setdefault((tuple(pats), tuple(flags), bs), [pc.QUIET_LINE * 2]).append(text)
    n_cells = 0
    for (pats, flags, bs), files in packs.items():
        assert len(files) >= 2
        got = segment_scan(arena, pats, flags, files, bs)
        for s, f in enumerate(files):
            lines, want = reference(pats, flags, f, bs)
            assert got[s] == (lines, want), (pats, bs, s, f[-24:], got[s][1][:4], want[:4])
        n_cells += len(files) - 1
    assert n_cells == sum(len(c) for g, c in pc.GROUPS.items() if g.startswith(family))


# --- D: launch geometry ----------------------------------------------------------------------------------------------------
def periodic(cycle, n):
    """n lines, line i = cycle[i % len(cycle)] (each ends with a newline): the text and its line list."""
    lines = [cycle[i % len(cycle)] for i in range(n)]
    return b"".join(lines), lines


def periodic_reference(pats, flags, lines):
    """parts_ref on each DISTINCT line once (lines are pieces: they are far shorter than the buffer size): (matching lines, rows)."""
    matching, rows = [], []
    for i, ln in enumerate(lines):
        key = (tuple(pats), tuple(flags), ln)
        if key not in _line_parts:
            hit = bool(parts_ref.matching_lines(ln, 262140, pats, flags))
            _line_parts[key] = (hit, parts_ref.piece_parts(pats, flags, ln) if hit else [])
        hit, parts = _line_parts[key]
        if hit:
            matching.append(i)
            rows += [(i, f, t, p) for f, t, p in parts]
    return matching, rows


def grid():
    import torch

    return 64 * torch.cuda.get_device_properties(0).multi_processor_count


ONE_HIT = [b"q.\n", b".kz\n", b"XY\n", b"..q.\n", b"kaz\n", b"..XY.\n", b"q\n"]  # hit lines of 2 to 6 bytes, one report each (the last: two)
FEW_HITS = [b"q\n", b"kzq\n", b".q.\n", b"kz\n", b"kz.q\n", b"..q\n", b"kzkz\n"]  # ... with 2, 3, 2, 1, 3, 2, 2 reports of D2's two expressions


@pytest.mark.parametrize("pset", [Q_S, Q_L3], ids=["S", "L3"])
@pytest.mark.parametrize("turns", [1, 2])
def test_grid_stride(arena, pset, turns):
    """More hits than the grid has waves: 64 CUs + 1 and 2 * 64 CUs + 3 hit lines, every wave takes a second (and third) hit."""
    g = grid()
    text, lines = periodic(ONE_HIT, turns * g + (1 if turns == 1 else 3))
    matching, want = periodic_reference(*pset, lines)
    assert len(matching) == len(lines) and 2 * len(lines) <= len(text) <= 6 * len(lines)
    st, _hits = check_parts(arena, *pset, text, 262140, matching, want)
    assert st.n_hits > turns * g


def test_head_test_at_arbitrary_hit_indices(arena):
    """Two expressions that report every end: most lines carry 2 or 3 hits, so heads fall on arbitrary hit indices; the hits
    at gridDim.x - 1, gridDim.x and gridDim.x + 1 exist and at least one of them heads no piece."""
    g = grid()
    pats, flags = ["q", "kz|q"], [A, A]
    text, lines = periodic(FEW_HITS, g + 1)
    matching, want = periodic_reference(pats, flags, lines)
    st, hits = check_parts(arena, pats, flags, text, 262140, matching, want)
    assert st.n_hits > g + 1 and len(hits) == st.n_hits
    heads = [hits[i - 1][0] != hits[i][0] for i in (g - 1, g, g + 1)]
    assert not all(heads), heads
    assert sum(1 for i in range(1, len(hits)) if hits[i - 1][0] == hits[i][0]) > len(lines) // 2  # most lines have a second hit


def test_one_scanner_five_scans(arena):
    """Hit counts of about 100, 5 000, 100, 20 000 and 0 on one scanner: the stage's buffers grow, are reused when the next
    scan is smaller, and a scan without hits leaves no part."""
    for n in (100, 5000, 100, 20000):
        text, lines = periodic(ONE_HIT, n)
        matching, want = periodic_reference(*Q_S, lines)
        st, _hits = check_parts(arena, *Q_S, text, 262140, matching, want)
        assert n <= st.n_hits <= n + n // 7 + 1 and st.n_parts == n
    st, hits = check_parts(arena, *Q_S, b"....\n" * 50, 262140, [], [])
    assert st.n_hits == 0 and hits == [] and scanner(*Q_S).parts() == []


CHUNK_SET = pc.CHUNK_SET  # (the S and the L3 walk, read out on the host)


def chunked_text() -> bytes:
    """chunk_texts.build: the last line before the first cut ends in a part that takes in the cut's last byte (its newline),
    the next begins with a part on the cut's first byte, and a three-word part of 66 bytes lies across the second cut."""
    across = b"." * 40 + b"kz " + b"m" + b"a" * 64 + b"z" + b" q" + b"." * 37 + b"\n"  # (the cut falls on its middle byte: inside m...z)
    assert len(across) // 2 in range(44, 44 + 66)
    cluster = [[b"kaz..XY\n", b"..." + pc.word(22) + b"q\n"], [pc.word(20) + b".q\n", b"m" + b"a" * 70 + b"z q\n"], [b"XYXY q.\n", across], [b"maz\n", b"....\n", b"q\n"]]
    fillers = [b"lorem ipsum dolor " * 50 + b"\n", b"." * 700 + b" kz " + b"." * 200 + b"\n", b"12x " * 200 + b"m" + b"a" * 30 + b"z\n"]
    return chunk_texts.build(cluster, fillers)


def chunk_scan(out_path=None):
    """One parts scan of chunked_text() at the end of an arena of its own: (stream launches, hit lines, parts).  As the child
    process (out_path given) it writes them with numpy instead."""
    import numpy as np
    import torch  # noqa: F401  (before the native library)

    from hypergrep_amd import device

    text = chunked_text()
    big = device.GuardedArena(chunk_texts.SIZE + 64)
    try:
        sc = device.Scanner(device.Database(CHUNK_SET[0], flags=CHUNK_SET[1], ids=[0, 1, 2]), 0)
        st = sc.scan(big.place(text), len(text), buffer_size=1000, parts=True)
        lines = sorted({h[0] for h in sc.hits()})
        parts = sc.parts()
        assert st.n_parts == len(parts)
    finally:
        big.free()
    if out_path:
        np.savez(out_path, launches=np.array([st.stream_launches]), lines=np.array(lines, dtype=np.uint64), parts=np.array(parts, dtype=np.uint64).reshape(-1, 4))
    return st.stream_launches, lines, parts


def test_pipeline_chunks(arena, tmp_path):
    """A child process with HG_CHUNK_TILES=1024 scans a text of more than 2048 tiles in three pipeline chunks (the engine
    launched the stream pass more than once); the parts around both cuts and everywhere else are the reference's, evaluated
    once per distinct line.  A control scan in this process runs without the variable."""
    import numpy as np

    text = chunked_text()
    assert text[chunk_texts.CUTS[0] - 2:chunk_texts.CUTS[0] + 2] == b"q\nka"
    mini, which, starts = chunk_texts.distinct(text)
    pats, flags = CHUNK_SET
    mini_lines = parts_ref.matching_lines(mini, 1000, pats, flags)
    mini_parts = parts_ref.expected(mini, 1000, pats, flags, mini_lines)
    by_line = {}
    for ln, f, t, p in mini_parts:
        by_line.setdefault(ln, []).append((f, t, p))
    want = [(i, f, t, p) for i, j in enumerate(which) for f, t, p in by_line.get(j, ())]
    hit = set(mini_lines)
    want_lines = [i for i, j in enumerate(which) if j in hit]
    cut1, cut2 = chunk_texts.CUTS
    line_of = {s: i for i, s in enumerate(starts)}
    last = max(i for i, s in enumerate(starts) if s < cut1)
    assert any(ln == last and starts[ln] + t == cut1 for ln, _f, t, _p in want)  # a part ends on the first cut's last byte
    assert any(ln == line_of[cut1] and f == 0 for ln, f, _t, _p in want)  # ... one begins on its first byte
    assert any(starts[ln] + f < cut2 < starts[ln] + t and p == 1 for ln, f, t, p in want)  # the three-word part across the second
    out = str(tmp_path / "chunked.npz")
    env = dict(os.environ, **chunk_texts.CHUNK_ENV)
    code = f"import sys; sys.path.insert(0, {HERE!r}); import test_parts_cells_gpu as t; t.chunk_scan({out!r})"
    child = subprocess.run([sys.executable, "-c", code], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    got = np.load(out)
    assert int(got["launches"][0]) >= 2  # the buffer went through the engine in several chunks
    assert got["lines"].tolist() == want_lines
    assert [tuple(r) for r in got["parts"].tolist()] == want
    assert not any(k in os.environ for k in chunk_texts.CHUNK_ENV)
    launches, lines, parts = chunk_scan()
    assert launches == 1  # (without the variable the engine cuts a buffer only from 16 GiB on)
    assert lines == want_lines and parts == want
