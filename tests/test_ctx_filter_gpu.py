"""GPU parity of the stream pass's first level with one byte of context (run with `-m gpu`): texts of three full tiles and
a 5-byte partial tile with every literal planted where the context byte comes from somewhere else — the lane's next dword, the
chunk to the right, nowhere (a row's last dword, the end of the text) — against the exact literal reference of
stream_cells.py, and the candidate counts against the host mirror (tests/native/ctxsim.cpp)."""
from __future__ import annotations

import random

import numpy as np
import pytest

import ctxsim_py
import stream_cells as sc

pytestmark = pytest.mark.gpu

NBYTES = 3 * sc.TILE + 5
LAST_ROW = 47 * sc.ROW  # the plants stay below the text's last row, which ends in a literal of its own
MIB = 1 << 20


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    return torch


def _mixed_set():
    """40 case-sensitive literals of 7-16 bytes, among them the short ones whose forced windows end them (7 bytes: the
    window at offset 3 has no byte after it; 8 bytes: the one at offset 4, where the compiler takes it)."""
    rng = random.Random(77)
    lits = []
    for i in range(40):
        n = (7, 8, 9, 11, 12, 16, 7, 8)[i % 8]
        lits.append("".join(rng.choice(sc.ALNUM) for _ in range(n)).encode())
    assert len(set(lits)) == len(lits)
    return lits, [False] * len(lits)


def _set_of(name):
    if name == "mixed":
        return _mixed_set()
    return sc.literal_set(sc.BY_NAME[name])


SETS = {  # name -> how many of its literals are planted (None: all); the cells of stream_cells.py and the mixed set above
    "mixed": None, "dword11": None, "dword12": 64, "dword13": 64, "dword11_fold": 48, "dword12_fold": 48, "dword_expand": None,
}


QUIET = b"-=+.,:;!"  # bytes of no literal


def _quiet_text(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    quiet = np.frombuffer(QUIET, dtype=np.uint8)[rng.integers(0, len(QUIET), size=n)]
    quiet[rng.random(n) < 1 / 100] = 10
    return quiet.tobytes()


def _databases(name, ids, plain=False):
    """The set's database and its host mirror.  plain: both tuned on a sample in which nothing passes the first level, so that
    the tuning turns the context byte down and the scan runs the kernels without it (hg_stream_plain_kernel)."""
    from hypergrep_amd import device

    lits, caseless = _set_of(name)
    pats, flags = sc.patterns_of(lits), sc.flags_of(caseless)
    db = device.Database(pats, flags=flags, ids=ids)
    info = db.info()
    assert info["byte_windows"] == 0 and info["n_always_on"] == 0, info
    mirror = ctxsim_py.Db(pats, flags=flags, ids=ids)
    minfo = mirror.info()
    assert mirror.ok() and minfo["has_ctx"] == 1 and minfo["wide"] == 0 and minfo["dense"] == 0 and minfo["use_ctx"] == 1, minfo
    if plain:
        sample = _quiet_text(MIB, 21)
        db.tune(sample)
        assert mirror.tune(sample) == 0
        tinfo = mirror.info()
        assert tinfo["has_ctx"] == 1 and tinfo["use_ctx"] == 0 and tinfo["wide"] == 0 and tinfo["dense"] == 0, tinfo
        assert db.info()["byte_windows"] == 0, db.info()
    return db, mirror, lits, caseless


def _device_text(torch, data: bytes):
    buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda:0")
    buf[: len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return buf


def _assert_hits(got, want, what):
    if got.shape == want.shape and (got == want).all():
        return
    rows = lambda a: np.ascontiguousarray(a).view([("", np.uint64)] * 5).ravel()  # noqa: E731
    missing, extra = np.setdiff1d(rows(want), rows(got))[:5], np.setdiff1d(rows(got), rows(want))[:5]
    pytest.fail(f"{what}: {len(got)} hits, want {len(want)}; missing {missing}; extra {extra}")


class _Texts:
    """Texts of NBYTES bytes filled with plants (offset in the text, bytes); a plant that does not fit opens the next text."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.done, self.cur, self.used = [], None, None
        self._open()

    def _open(self):
        buf = self.rng.choice(sc.FILLER, size=NBYTES)
        buf[self.rng.random(NBYTES) < 1 / 90] = 10
        self.cur, self.used = bytearray(buf.tobytes()), np.zeros(NBYTES + 64, dtype=bool)

    def _next(self):
        self.done.append(bytes(self.cur))
        self._open()

    def put_at(self, places, b: bytes):
        """At one of these offsets exactly (a geometry plant): the first whose bytes, and one either side, are free in the
        current text, else the first of them in a new text."""
        for fresh in (False, True):
            for at in places:
                assert 0 <= at and at + len(b) <= LAST_ROW
                if not self.used[max(at - 1, 0):at + len(b) + 1].any():
                    self.cur[at:at + len(b)] = b
                    self.used[max(at - 1, 0):at + len(b) + 1] = True
                    return
            assert not fresh, "a fresh text has room"
            self._next()

    def put_residue(self, res: int, b: bytes, mod: int = 16):
        """At the next free offset with this residue (walks forward through the text, then opens the next)."""
        at = getattr(self, "_walk", 0)
        while True:
            at += (res - at) % mod
            if at + len(b) + 1 > LAST_ROW:
                self._next()
                at = 0
                continue
            if not self.used[max(at - 1, 0):at + len(b) + 1].any():
                break
            at += mod
        self.cur[at:at + len(b)] = b
        self.used[max(at - 1, 0):at + len(b) + 1] = True
        self._walk = at + len(b) + 1

    def texts(self):
        return self.done + [bytes(self.cur)]


def _other(b: int) -> int:
    """A byte that differs from b, also under ASCII case folding and under | 0x20."""
    for c in b"#5q":
        if (c | 0x20) != (b | 0x20):
            return c
    raise AssertionError


def _planted_texts(lits, caseless, sample, seed):
    """The issue's plants for the first `sample` literals (all when None); returns (texts, look-alikes planted)."""
    rng = random.Random(seed)
    tx = _Texts(seed)
    chosen = [(l, c) for l, c in zip(lits, caseless) if l != sc.SPACES.encode()][:sample]
    text_form = lambda lit, cl: sc.case_variant(lit, rng) if cl else lit  # noqa: E731
    lookalikes = []
    rows = [r for r in range(1, 46) if r % 16 != 15]  # (a tile's last row is the tile-end plants')
    for li, (lit, cl) in enumerate(chosen):
        n = len(lit)
        # every window offset as a row's last dword, as lane 63's other dwords and (the first literals: a text has two
        # places for it) as a tile's last dword
        for o in range(n - 3):
            rng.shuffle(rows)
            tx.put_at([r * sc.ROW + 1020 - o for r in rows], text_form(lit, cl))
            k = rng.randrange(0, 3)
            tx.put_at([r * sc.ROW + 1008 + 4 * k - o for r in rows], text_form(lit, cl))
            if li < 6:
                tx.put_at([t * sc.TILE - 4 - o for t in (1, 2)], text_form(lit, cl))
        # every residue mod 16
        for res in range(16):
            tx.put_residue(res, text_form(lit, cl))
        # look-alikes: equal through a window (and all before it), another byte after it; mid-row and with the window in
        # lane 63 (as each of its four dwords: the context byte in the lane, or in the next row where the kernel cannot look)
        for o in range(n - 4):
            bad = text_form(lit, cl)[:o + 4] + bytes([_other(lit[o + 4])])
            lookalikes.append(bad)
            tx.put_residue((-o) % 4, bad, mod=4)
            rng.shuffle(rows)
            k = rng.randrange(0, 4)
            tx.put_at([r * sc.ROW + 1008 + 4 * k - o for r in rows], bad)
    texts = tx.texts()
    # the literal ending exactly at the end of the text (the partial tile's 5 bytes hold its tail)
    out = []
    for i, t in enumerate(texts):
        lit, cl = chosen[i % len(chosen)]
        out.append(t[:NBYTES - len(lit)] + text_form(lit, cl))
    return out, lookalikes


@pytest.mark.parametrize("kernels", ["ctx", "plain"])
@pytest.mark.parametrize("ids_kind", ["distinct", "shared"])
@pytest.mark.parametrize("name", list(SETS), ids=list(SETS))
def test_planted_geometry(torch_cuda, name, ids_kind, kernels):
    """For the larger cells the plants are those of a sample of the literals (SETS), and in every set only the first six
    literals are planted as a tile's last dword (a text has two such places); `mixed`, `dword11` and `dword_expand` plant
    every literal at every residue.  kernels = plain: the same texts through the kernels without the context byte."""
    from hypergrep_amd import device

    nlits = len(_set_of(name)[0])
    ids = list(range(nlits)) if ids_kind == "distinct" else [i % 3 for i in range(nlits)]
    db, mirror, lits, caseless = _databases(name, ids, plain=kernels == "plain")
    texts, lookalikes = _planted_texts(lits, caseless, SETS[name], seed=len(name) * 13 + 1)
    assert len(lookalikes) > 0
    scanner = device.Scanner(db, 0)
    rejected = 0
    for k, data in enumerate(texts):
        assert len(data) == NBYTES
        want = sc.reference_hits(data, lits, caseless, ids)
        _nl, nlines = sc.line_table(data)
        buf = _device_text(torch_cuda, data)
        stats = scanner.scan(buf.data_ptr(), len(data))
        got = sc.sort_hits(scanner.hits_array())
        del buf
        assert stats.n_lines == nlines, (name, k, stats.n_lines, nlines)
        _assert_hits(got, want, f"{name} text {k}")  # (a look-alike is no occurrence: reported, it would be an extra hit)
        m = mirror.scan(data)
        assert m["violations"] == 0 and m["cands_new"] == m["cands_old"], (name, k, m)
        assert stats.n_candidates == m["cands_old"], (name, k, stats.n_candidates, m)
        rejected += m["dropped"]
    assert rejected > 0, name  # look-alikes pass the first level on hash C alone and not with the context byte


def test_text_ending_in_a_window(torch_cuda):
    """The window as the text's last dword, the literal ending exactly there: no byte after it, in the text or in the row."""
    from hypergrep_amd import device

    ids = list(range(40))
    db, mirror, lits, caseless = _databases("mixed", ids)
    scanner = device.Scanner(db, 0)
    rng = np.random.default_rng(3)
    for lit in lits:
        for n in (3 * sc.TILE + 4, 3 * sc.TILE + 5, 2 * sc.TILE + sc.ROW, 2 * sc.TILE + 7 * sc.ROW + 16):
            body = rng.choice(sc.FILLER, size=n - len(lit)).tobytes()
            data = body + lit
            buf = _device_text(torch_cuda, data)
            stats = scanner.scan(buf.data_ptr(), len(data))
            got = sc.sort_hits(scanner.hits_array())
            del buf
            _assert_hits(got, sc.reference_hits(data, lits, caseless, ids), f"{lit!r} at the end of {n} bytes")
            m = mirror.scan(data)
            assert m["violations"] == 0 and stats.n_candidates == m["cands_new"] == m["cands_old"], (lit, n, stats.n_candidates, m)


def _repeated(bwant, blines, blen, reps):
    shift = np.zeros((reps, 1, 5), dtype=np.uint64)
    shift[:, 0, 0] = np.arange(reps, dtype=np.uint64) * np.uint64(blines)
    shift[:, 0, 3] = np.arange(reps, dtype=np.uint64) * np.uint64(blen)
    return (bwant[None, :, :] + shift).reshape(-1, 5)


@pytest.mark.parametrize("kernels", ["ctx", "plain"])
@pytest.mark.parametrize("mode", ["two_chunks", "joiner"])
@pytest.mark.parametrize("name", ["mixed", "dword12_fold", "dword13"])
def test_pipeline_and_joiner(torch_cuda, name, mode, kernels, monkeypatch):
    """The planted texts behind each other in 1 MiB blocks: 17 MiB in 16 MiB pipeline chunks (two stream launches, the second
    ending in the partial tile), and 33 MiB with the joiner forced on and put in front of each chunk's stream launch."""
    from hypergrep_amd import device

    nlits = len(_set_of(name)[0])
    ids = list(range(nlits))
    db, mirror, lits, caseless = _databases(name, ids, plain=kernels == "plain")
    texts, _ = _planted_texts(lits, caseless, 6, seed=5)
    head = b"".join(t[:3 * sc.TILE] for t in texts[:4])
    block = head + _quiet_text(MIB, 9)[len(head):MIB - 1] + b"\n"
    assert len(block) == MIB
    tail = texts[0]
    reps = 16 if mode == "two_chunks" else 32
    bwant, blines = sc.reference_hits(block, lits, caseless, ids), sc.line_table(block)[1]
    twant, tlines = sc.reference_hits(tail, lits, caseless, ids), sc.line_table(tail)[1]
    want = np.concatenate([_repeated(bwant, blines, len(block), reps), twant + np.array([reps * blines, 0, 0, reps * len(block), 0], dtype=np.uint64)])
    n = reps * len(block) + len(tail)
    buf = torch_cuda.zeros(n + 32, dtype=torch_cuda.uint8, device="cuda:0")
    dev_block = torch_cuda.frombuffer(bytearray(block), dtype=torch_cuda.uint8).cuda()
    buf[: reps * len(block)].view(reps, len(block)).copy_(dev_block.expand(reps, len(block)))
    buf[reps * len(block):n] = torch_cuda.frombuffer(bytearray(tail), dtype=torch_cuda.uint8).cuda()
    torch_cuda.cuda.synchronize()
    monkeypatch.setenv("HG_CHUNK_TILES", "1024")
    if mode == "joiner":
        monkeypatch.setenv("HG_JOINER", "2")
        monkeypatch.setenv("HG_JOINER_AHEAD", "1")
    else:
        monkeypatch.setenv("HG_STREAM_WGS_PER_CU", "1")
    scanner = device.Scanner(db, 0)  # (env knobs are read when the scanner is created)
    stats = scanner.scan(buf.data_ptr(), n)
    got = sc.sort_hits(scanner.hits_array())
    assert stats.n_lines == reps * blines + tlines
    if mode == "joiner":
        assert stats.stream_launches == 3 and stats.joiner_launches == 2 and stats.joiner_tiles > 0, stats
    else:
        assert stats.stream_launches == 2, stats
    _assert_hits(got, sc.sort_hits(want), f"{name} {mode}")
    cands = reps * mirror.scan(block)["cands_old"] + mirror.scan(tail)["cands_old"]
    assert stats.n_candidates == cands, (stats.n_candidates, cands)
