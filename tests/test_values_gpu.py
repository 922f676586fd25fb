"""Distinct matched parts on the MI355X: hg_count_values (the values stage, hypergrep_amd/csrc/hg_values.hip) behind
hg_scan_device_parts and hg_scan_device_segments_parts.  Every expectation is values_ref's plain Python dict over
Scanner.parts(), the starts in Scanner.hits() and the text (for one pattern also Python's re over the lines), never anything the
stage computes.  Texts are small and sit at the end of guarded buffers: a read past them faults.  The tightest table of any
test still has more slots than parts."""
from __future__ import annotations

import collections
import os
import random
import re
import subprocess
import sys

import pytest

import values_ref as vr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 14  # DOTALL | MULTILINE | SINGLEMATCH
LANE_MAX = 256
SET_KV = (["[a-z]+=[0-9]+", "ERR[0-9]+"], [A, A])
SET_ID = (["id=[0-9a-z]+"], [A])
SET_X = (["x[a-w]*"], [A])
SET_TWO = (["user=[a-z]+", "[a-z]+=bob"], [A, A])  # both match `user=bob`: equal bytes from different expressions


@pytest.fixture(scope="module")
def arena():
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    from hypergrep_amd import device

    a = device.GuardedArena(1 << 21)
    yield a
    _scanners.clear()  # (before the interpreter takes the module's globals away)
    a.free()


_scanners = {}


def scanner(pset):
    from hypergrep_amd import device

    key = tuple(pset[0])
    if key not in _scanners:
        _scanners[key] = device.Scanner(device.Database(pset[0], flags=pset[1], ids=list(range(1, len(pset[0]) + 1))), 0)
    return _scanners[key]


def tight(n_parts: int) -> int:
    """The smallest legal explicit table: 2 ** k > n_parts."""
    return max(1, n_parts.bit_length())


def compare(sc, stats, want, where):
    a = sc.values_arrays()
    assert stats.n_values == len(want["count"]) and stats.n_bytes == len(want["bytes"]), where
    assert a["bytes"] == want["bytes"], where
    for name in ("off", "count", "first", "pattern", "line_number"):
        assert a[name].tolist() == want[name], (name, where)
    if want["segment"] is None:
        assert a["segment"] is None, where
    else:
        assert a["segment"].tolist() == want["segment"], where
    return a


def run(arena, text, pset, settings=({},), by_pattern=(False, True), bs=262140):
    """One scan with parts, then a value count per setting against the reference.  Returns the parts and the rows (by bytes)."""
    sc = scanner(pset)
    ptr = arena.place(text)
    st = sc.scan(ptr, len(text), buffer_size=bs, parts=True)
    parts = sc.parts()
    assert st.n_parts == len(parts)
    starts = {(0, h[0]): h[3] for h in sc.hits()}
    rows = None
    for bp in by_pattern:
        ref = vr.groups(text, parts, starts, by_pattern=bp)
        assert sum(r["count"] for r in ref) == len(parts)  # every part has a record
        rows = ref if not bp or rows is None else rows
        for kw in settings:
            v = sc.count_values(ptr, len(text), by_pattern=bp, **kw)
            assert v.n_parts == len(parts)
            compare(sc, v, vr.arrays(ref), (bp, kw))
            assert sc.values() == [(r["value"], r["count"], r["pattern"], r["line_number"]) for r in ref]
    assert sc.parts() == parts
    return parts, rows


def collision_settings(n_parts):
    return ({}, {"hash_bits": 1}, {"hash_bits": 4}, {"table_log2": tight(n_parts)}, {"hash_bits": 4, "table_log2": tight(n_parts)})


def test_no_parts(arena):
    text = b"nothing here\nnor here\n"
    parts, rows = run(arena, text, SET_KV)
    assert parts == [] and rows == []
    sc = scanner(SET_KV)
    assert sc.values_arrays()["off"].tolist() == [0] and sc.values() == []


@pytest.mark.parametrize("n", [64, 65, 4096])
def test_one_value_many_parts(arena, n):
    """A wave of equal parts adds once; 4096 parts are 16 workgroups."""
    text = b"a=1 a=1\n" * (n // 2) + (b"a=1\n" if n % 2 else b"")
    parts, rows = run(arena, text, SET_KV)
    assert len(parts) == n and len(rows) == 1 and rows[0]["count"] == n and rows[0]["value"] == b"a=1" and rows[0]["first"] == 0


def test_all_distinct(arena):
    text = b"".join(b"id=%x\n" % (i * 2654435761 % (1 << 32)) for i in range(5000))
    parts, rows = run(arena, text, SET_ID, settings=({}, {"table_log2": tight(5000)}), by_pattern=(False,))
    assert len(parts) == 5000 and len(rows) == 5000 and all(r["count"] == 1 for r in rows)  # (an odd multiplier is a bijection mod 2^32)


def mix_text(rng, lines):
    vocab = [b"%s=%d" % (rng.choice([b"user", b"code", b"req", b"n"]), rng.randrange(12)) for _ in range(50)] + [b"ERR%d" % rng.randrange(5) for _ in range(5)]
    filler = [b"lorem", b"-", b"GET /index", b"=", b"a=", b"=7"]
    return b"".join(b" ".join(rng.choice(vocab + filler) for _ in range(rng.randint(0, 5))) + b"\n" for _ in range(lines))


def test_mix_of_few_values(arena):
    text = mix_text(random.Random(5), 20000)
    parts, rows = run(arena, text, SET_KV, settings=({}, {"table_log2": tight(60000)}))
    assert len(parts) > 20000 and 30 < len(rows) < 60 and max(r["count"] for r in rows) > 500


def test_against_python_re(arena):
    rng = random.Random(9)
    names = [b"bob", b"alice", b"eve", b"mallory", b"x"]
    text = b"".join(b"t=%d user=%s user=%s end\n" % (i, rng.choice(names), rng.choice(names)) if i % 3 else b"no user here\n" for i in range(3000))
    sc = scanner((["user=[a-z]+"], [A]))
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    sc.count_values(ptr, len(text))
    want = collections.Counter(m for line in text.split(b"\n") for m in re.findall(rb"user=[a-z]+", line))
    got = {v: c for v, c, _p, _l in sc.values()}
    assert got == dict(want) and len(got) == 5
    order = list(dict.fromkeys(m for line in text.split(b"\n") for m in re.findall(rb"user=[a-z]+", line)))
    assert [v for v, _c, _p, _l in sc.values()] == order  # the order of first occurrence


def test_alignments_and_lengths(arena):
    """Every start alignment 0 .. 3 with every length 1 .. 20, each value twice at different alignments."""
    lines = []
    for pad in range(4):
        for n in range(1, 21):
            body = bytes(97 + (n * 7 + k) % 23 for k in range(n - 1))
            line = b"." * pad + b"x" + body + b" " + b"." * ((pad + n) % 3) + b"x" + body
            lines.append(line + b"." * (-(len(line) + 1) % 4) + b"\n")  # every line a multiple of 4: its first value starts at alignment `pad`
    text = b"".join(lines)
    parts, rows = run(arena, text, SET_X, settings=collision_settings(160), by_pattern=(False,))
    assert len(parts) == 160 and {len(r["value"]) for r in rows} == set(range(1, 21)) and [r["count"] for r in rows] == [8] * 20
    line_start = [sum(len(l) for l in lines[:i]) for i in range(len(lines))]
    assert {((line_start[p[0]] + p[1]) % 4, p[2] - p[1]) for p in parts[::2]} == {(a, n) for a in range(4) for n in range(1, 21)}  # the whole grid, by the first values alone


@pytest.mark.parametrize("tail", [b"", b"\0\0\0", b"zzz"])
def test_value_at_the_unaligned_end_of_the_text(arena, tail):
    """The last value ends at the last byte of a text of 4k + 1 .. 3 bytes; what lies behind nbytes does not matter."""
    for cut in (1, 2, 3):
        text = b"." * cut + b"xab\nxabc\n....xab\n" + b"xabc"
        while len(text) % 4 != cut:
            text = b"\n" + text
        sc = scanner(SET_X)
        ptr = arena.place(text + tail) if tail else arena.place(text)
        sc.scan(ptr, len(text), parts=True)
        parts = sc.parts()
        starts = {(0, h[0]): h[3] for h in sc.hits()}
        v = sc.count_values(ptr, len(text))
        a = compare(sc, v, vr.arrays(vr.groups(text, parts, starts)), (cut, tail))
        assert a["bytes"] == b"xabxabc" and a["count"].tolist() == [2, 2]


def test_long_parts(arena):
    """Parts a wavefront hashes and compares: two equal ones of about 100 KiB and a third that differs in its last byte, and the
    three lengths around the lane limit, each twice."""
    rng = random.Random(3)
    big = b"x" + bytes(97 + rng.randrange(23) for _ in range(100 * 1024))
    other = big[:-1] + (b"a" if big[-1:] != b"a" else b"b")
    around = [b"x" + bytes(97 + (n + k) % 23 for k in range(n - 1)) for n in (LANE_MAX - 1, LANE_MAX, LANE_MAX + 1)]
    text = b"\n".join([big, b"." + around[0], b".." + big, around[1], around[2], b"..." + other, around[0], b"." + around[1], b".." + around[2], b"xq"]) + b"\n"
    parts, rows = run(arena, text, SET_X, settings=({}, {"hash_bits": 1, "table_log2": tight(10)}), by_pattern=(False,))
    assert len(parts) == 10
    assert [(len(r["value"]), r["count"]) for r in rows] == [(len(big), 2), (LANE_MAX - 1, 2), (LANE_MAX, 2), (LANE_MAX + 1, 2), (len(big), 1), (2, 1)]


def test_collisions_and_a_tight_table(arena):
    text = mix_text(random.Random(6), 300)
    sc = scanner(SET_KV)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    n = len(sc.parts())
    assert n > 300
    sc.count_values(ptr, len(text))
    base = sc.values_arrays()
    for kw in collision_settings(n)[1:]:
        sc.count_values(ptr, len(text), **kw)
        a = sc.values_arrays()
        assert a["bytes"] == base["bytes"] and all(a[k].tolist() == base[k].tolist() for k in ("off", "count", "first", "pattern", "line_number")), kw
    run(arena, text, SET_KV, settings=collision_settings(n))


def test_by_pattern(arena):
    text = b"user=bob x=bob user=bob\nuser=al user=bob\nk=bob\n"
    parts, rows = run(arena, text, SET_TWO)
    sc = scanner(SET_TWO)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    plain = sc.count_values(ptr, len(text)).n_values
    keyed = sc.count_values(ptr, len(text), by_pattern=True).n_values
    assert keyed >= plain == len(rows) and len({p[3] for p in parts}) == 2


def test_segments(arena):
    """After segment_parts equal values in different files are one group; segment and line_number are those of `first`."""
    files = [b"n=1 n=2\nzz\nn=3\n", b"none\n", b"n=9\nn=2 n=1\n", b"ERR7 n=3 n=9\n"]
    text = b"".join(files)
    starts = [sum(len(f) for f in files[:i]) for i in range(len(files))]
    ends = [s + len(f) for s, f in zip(starts, files)]
    sc = scanner(SET_KV)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), segments=(starts, ends), segment_parts=True)
    hits, rows, segs = sc.hits(), sc.parts(), sc.segment_parts()["part_segment"].tolist()
    rec_seg = sc.segments()["record_segment"].tolist()
    parts = [p + (s,) for p, s in zip(rows, segs)]
    where = {(s, h[0]): h[3] for h, s in zip(hits, rec_seg)}
    for bp in (False, True):
        ref = vr.groups(text, parts, where, by_pattern=bp, seg_start=starts)
        for kw in collision_settings(len(parts)):
            v = sc.count_values(ptr, len(text), by_pattern=bp, **kw)
            compare(sc, v, vr.arrays(ref, segments=True), (bp, kw))
    a = sc.values_arrays()
    assert a["bytes"] == b"n=1n=2n=3n=9ERR7" and a["count"].tolist() == [2, 2, 2, 2, 1] and a["segment"].tolist() == [0, 0, 0, 2, 3] and a["line_number"].tolist() == [0, 0, 2, 0, 0]
    assert sc.hits() == hits and sc.parts() == rows


def test_two_runs_are_identical(arena):
    text = mix_text(random.Random(8), 5000)
    sc = scanner(SET_KV)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    runs = []
    for _ in range(2):
        sc.count_values(ptr, len(text), by_pattern=True)
        a = sc.values_arrays()
        runs.append((a["bytes"],) + tuple(a[k].tolist() for k in ("off", "count", "first", "pattern", "line_number")))
    assert runs[0] == runs[1]


def test_other_results_untouched(arena):
    text = mix_text(random.Random(10), 500)
    sc = scanner(SET_KV)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    sc.gather_parts(ptr, len(text), number=True, terminate=True)
    sc.count()
    before = (sc.hits(), sc.parts(), sc.part_lines(), sc.counts())
    sc.count_values(ptr, len(text))
    sc.count_values(ptr, len(text), by_pattern=True, hash_bits=3)
    assert (sc.hits(), sc.parts(), sc.part_lines(), sc.counts()) == before
    sc.gather_parts(ptr, len(text))  # and the values are those of the gathered parts
    assert dict(collections.Counter(sc.part_lines())) == {v: c for v, c, _p, _l in sc.values()}


def test_refusals(arena):
    from hypergrep_amd import device

    text = b"a=1 b=2\n"
    sc = device.Scanner(device.Database(SET_KV[0], flags=SET_KV[1], ids=[1, 2]), 0)
    ptr = arena.place(text)
    with pytest.raises(ValueError, match="no successful scan"):
        sc.count_values(ptr, len(text))
    with pytest.raises(ValueError, match="no value count"):
        sc.values_arrays()
    sc.scan(ptr, len(text))
    with pytest.raises(ValueError, match="not one with parts"):
        sc.count_values(ptr, len(text))
    sc.scan(ptr, len(text), parts=True)
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.count_values(ptr, len(text) - 1)
    with pytest.raises(ValueError, match="not those of the last scan"):
        sc.count_values(ptr + 4, len(text))
    with pytest.raises(ValueError, match="hash_bits above 64"):
        sc.count_values(ptr, len(text), hash_bits=65)
    with pytest.raises(ValueError, match="table_log2 above 40"):
        sc.count_values(ptr, len(text), table_log2=41)
    with pytest.raises(ValueError, match="must exceed the number of parts"):
        sc.count_values(ptr, len(text), table_log2=1)  # 2 slots, 2 parts
    with pytest.raises(ValueError, match="unknown flag bits"):
        sc._count_values(ptr, len(text), device.HgValuesParams(flags=2))  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="no value count"):
        sc.values()
    assert sc._count_values(ptr, len(text), None).n_values == 2  # params NULL: the defaults  # pylint: disable=protected-access
    assert sc.count_values(ptr, len(text), table_log2=2).n_values == 2 and sc.values() == [(b"a=1", 1, 0, 0), (b"b=2", 1, 0, 0)]
    # a refused call leaves no earlier count behind in the C ABI either
    import ctypes

    off = (ctypes.c_uint64 * 4)()
    copy = lambda: device.lib().hg_copy_values(sc._h, None, 0, off, None, None, None, None, None, 2)  # noqa: E731  # pylint: disable=protected-access
    assert copy() == 0 and list(off[:3]) == [0, 3, 6]
    with pytest.raises(ValueError, match="hash_bits above 64"):
        sc.count_values(ptr, len(text), hash_bits=65)
    assert copy() == -1
    sc.scan(ptr, len(text), parts=True)
    with pytest.raises(ValueError, match="no value count"):  # a scan forgets the last count
        sc.values()


def test_copy_values_to_device(arena):
    import torch

    text = b"a=1 b=22 a=1\n"
    sc = scanner(SET_KV)
    ptr = arena.place(text)
    sc.scan(ptr, len(text), parts=True)
    v = sc.count_values(ptr, len(text))
    dst = torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert sc.copy_values_to(dst.data_ptr(), 16) == v.n_bytes == 7
    torch.cuda.synchronize()
    assert bytes(dst.cpu().tolist()[:7]) == b"a=1b=22"


def test_file_path_over_several_chunks(tmp_path, monkeypatch):
    """A 2.5 MiB file read in chunks of 1 MiB and pieces of at most 4 KiB: the chunks' values are merged on the host."""
    import hypergrep_amd

    path = tmp_path / "log.txt"
    text = mix_text(random.Random(12), 150000)
    assert len(text) > 2 << 20  # three chunks
    path.write_bytes(text)
    got, rc = hypergrep_amd.grep(str(path), SET_KV[0], matched_parts=True)
    assert rc == 0
    want = collections.Counter(part.rstrip("\n").encode() for _line, part in got)
    one_chunk, rc = hypergrep_amd.count_values(str(path), SET_KV[0], flags=SET_KV[1], by_pattern=True)
    assert rc == 0
    monkeypatch.setenv("HYPERGREP_CHUNK_MB", "1")
    rows, rc = hypergrep_amd.count_values(str(path), SET_KV[0], flags=SET_KV[1], buffer_size=4096)
    assert rc == 0 and rows == sorted(want.items(), key=lambda r: (-r[1], r[0])) and 30 < len(rows) < 60
    keyed, rc = hypergrep_amd.count_values(str(path), SET_KV[0], flags=SET_KV[1], by_pattern=True, buffer_size=4096)
    assert rc == 0 and keyed == one_chunk and {p for _v, p, _c in keyed} == {0, 1}
    merged = collections.Counter()
    for value, _pattern, count in keyed:
        merged[value] += count
    assert merged == want


def test_command_line(tmp_path):
    a, b = tmp_path / "a.log", tmp_path / "b.log"
    a.write_bytes(b"n=1 n=2 n=1\nn=1\n")
    b.write_bytes(b"k=5\n")
    out = subprocess.run([sys.executable, "-m", "hypergrep_amd.multiscanner", "-E", "--value-counts", "-e", "[a-z]+=[0-9]+", str(a), str(b)], capture_output=True, cwd=REPO, check=False)
    assert out.returncode == 0, out.stderr
    assert out.stdout == b"%s:3:n=1\n%s:1:n=2\n%s:1:k=5\n" % (str(a).encode(), str(a).encode(), str(b).encode())
