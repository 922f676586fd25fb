"""GPU parity for the stream pass's bookkeeping (run with `-m gpu`): the per-chunk queue entries, the newline prefix they
carry, the first / last newline of a tile and the drain at tile and launch ends.  Each text is built to stress one of
them and the hits must equal the oracle's."""
from __future__ import annotations

import random

import pytest

import gpu_cases
import oracle_py

pytestmark = pytest.mark.gpu

# literals long enough for the dword-aligned single-probe filter (the variant the headline workload runs)
LITERALS = ["abcdefgh", "qwertyuio", "lit0042x", "status=503", "zzkeyzz1"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    return torch


def _scan(torch, data: bytes, patterns, **kw):
    from hypergrep_amd import device

    n = len(data)
    buf = torch.zeros(n + 32, dtype=torch.uint8, device="cuda:0")
    if n:
        buf[:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    ids = list(range(len(patterns)))
    sc = device.Scanner(device.Database(patterns, ids=ids), 0)
    stats = sc.scan(buf.data_ptr(), n, **kw)
    return gpu_cases.ordered_hits(sc), stats


def _check(torch, data: bytes, patterns=LITERALS, min_hits=1):
    ids = list(range(len(patterns)))
    rc, want, nlines = oracle_py.scan_buffer(data, patterns, ids=ids)
    assert rc == 0
    got, stats = _scan(torch, data, patterns)
    assert stats.n_lines == nlines
    assert got == sorted(want)
    assert len(want) >= min_hits
    return stats


def _words(rng, n):
    return "".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789 =") for _ in range(n))


def test_every_chunk_queued(torch_cuda):
    """Every 16-byte chunk holds a window of a literal: the queue fills every iteration and drains every iteration."""
    line = b"abcdefgh" * 15 + b"\n"  # 121 bytes: the literal at every dword offset over the text
    data = line * 9000 + b"tail abcdefgh"
    _check(torch_cuda, data, min_hits=9000)


def test_several_newlines_per_chunk(torch_cuda):
    """Short lines: most 16-byte chunks hold several newlines (the wave scan path for the newline prefix)."""
    rng = random.Random(7)
    parts = []
    for _ in range(60000):
        r = rng.random()
        if r < 0.05:
            parts.append(rng.choice(LITERALS) + _words(rng, rng.randrange(0, 3)))
        elif r < 0.5:
            parts.append("")
        else:
            parts.append(_words(rng, rng.randrange(1, 7)))
    data = ("\n".join(parts) + "\n").encode()
    _check(torch_cuda, data, min_hits=1000)


def test_sparse_newlines_and_mixed_chunks(torch_cuda):
    """Long stretches without a newline next to stretches with several per chunk; queued chunks from many tiles in one
    batch."""
    rng = random.Random(11)
    out = []
    for _ in range(400):
        if rng.random() < 0.5:
            out.append(_words(rng, rng.randrange(2000, 30000)) + rng.choice(LITERALS) + _words(rng, rng.randrange(0, 100)) + "\n")
        else:
            out.append("\n".join(_words(rng, rng.randrange(0, 4)) for _ in range(rng.randrange(10, 400))) + "\n")
        if rng.random() < 0.3:
            out.append(rng.choice(LITERALS) + "\n\n" + rng.choice(LITERALS) + "\n")
    data = "".join(out).encode()
    _check(torch_cuda, data, min_hits=100)


def test_lines_crossing_tiles(torch_cuda):
    """Lines of 20-60 KiB with literals anywhere in them: a line's pieces and its hits lie in several tiles."""
    rng = random.Random(3)
    out = []
    for _ in range(60):
        body = bytearray(_words(rng, rng.randrange(20000, 60000)).encode())
        for _ in range(rng.randrange(1, 6)):
            lit = rng.choice(LITERALS).encode()
            at = rng.randrange(0, len(body) - len(lit))
            body[at:at + len(lit)] = lit
        out.append(bytes(body) + b"\n")
    _check(torch_cuda, b"".join(out), min_hits=30)


@pytest.mark.parametrize("extra", [0, 1, 15, 16, 17, 1023, 1024, 1025, 16383])
def test_last_partial_tile(torch_cuda, extra):
    """The text ends inside a tile (at every kind of boundary) with a literal and newlines in the last bytes."""
    rng = random.Random(extra)
    head = ("\n".join(_words(rng, rng.randrange(0, 60)) for _ in range(900)) + "\n").encode()
    head = (head * 3)[: 3 * 16384]
    tail = bytearray(_words(rng, extra).encode())
    lit = b"abcdefgh"
    if extra >= len(lit):
        tail[-len(lit):] = lit
    if extra >= 2:
        tail[extra // 2] = 0x0A
    data = head + bytes(tail)
    _check(torch_cuda, data, min_hits=0)


def test_pipeline_joiner_and_segments(torch_cuda, monkeypatch):
    """A 40 MiB text in 16 MiB pipeline chunks (joiner launches behind the side passes), then in several segments with the
    hit limit lowered: the queue drains at every launch end."""
    from hypergrep_amd import benchspec, device

    torch = torch_cuda
    patterns, needles, hpm = benchspec.c3_spec(n_literals=12, n_classes=8, n_anchored=8)
    nbytes = (40 << 20) + 777
    text = torch.empty(nbytes + 32, dtype=torch.uint8, device="cuda:0")
    device.synth_device(text.data_ptr(), nbytes, seed=99, needles=needles, hit_per_million=hpm * 3)
    host = bytes(text[:nbytes].cpu().numpy())
    ids = list(range(len(patterns)))
    rc, want, nlines = oracle_py.scan_buffer(host, patterns, ids=ids)
    assert rc == 0
    want = sorted(want)
    monkeypatch.setenv("HG_CHUNK_TILES", "1024")
    db = device.Database(patterns, ids=ids)
    db.tune(host[: 1 << 20])
    sc = device.Scanner(db, 0)
    stats = sc.scan(text.data_ptr(), nbytes)
    assert stats.n_lines == nlines and stats.joiner_launches >= 1
    assert sorted(sc.hits()) == want and len(want) > 1000
    monkeypatch.setenv("HG_HIT_LIMIT", str(int(stats.n_raw_hits * 0.4)))
    sc_seg = device.Scanner(db, 0)
    st_seg = sc_seg.scan(text.data_ptr(), nbytes)
    assert st_seg.n_lines == nlines and st_seg.stream_launches >= 4
    assert sc_seg.hits() == want
