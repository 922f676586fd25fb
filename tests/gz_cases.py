"""Compressed input files beyond the toy fixtures, generated at test time (nothing large is committed): gzip members cut
mid-line, trailing bytes, truncated streams, an empty member, a plain file that starts with the gzip magic, concatenated
zstd frames.  Shared by the host test of the oracle's two splitters (test_oracle.py) and the GPU Face B test
(test_gpu_parity.py).  No zstd compressor is at hand (neither a Python module nor the CLI), so the only zstd case is the
committed frame concatenated with itself — a valid stream of many frames that still fits one ingest chunk."""
from __future__ import annotations

import gzip
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")
CHUNK = 1 << 20  # HYPERGREP_CHUNK_MB=1


def large_text():
    """(text, patterns): about 5 MiB of synthetic log for benchspec.c3_spec(), no newline on the last line, with lines of
    3000 and 300000 bytes (longer than both scan buffers of the tests) laid across the 1 MiB and 3 MiB ingest chunk cuts."""
    from hypergrep_amd import benchspec, device

    patterns, needles, hpm = benchspec.c3_spec()
    nbytes = 5 << 20
    text = bytearray(device.synth_host(nbytes, 9, needles, hpm * 3)[: nbytes - 777])
    for at, n in ((CHUNK - 1500, 3000), (3 * CHUNK - 150000, 300000)):
        for i in range(at, at + n):
            if text[i] == 10:
                text[i] = 32
    assert text[-1] != 10
    return bytes(text), patterns


def _mid_line(text: bytes, at: int) -> int:
    while text[at - 1] == 10 or text[at] == 10:
        at += 1
    return at


def build(tmp_dir, text: bytes):
    """[(name, path, decoded, large)]: `decoded` = the bytes a reader delivers where that is defined by the format alone (None
    for damaged streams: there the oracle's zlib path is the only definition); `large`: spans several ingest chunks."""
    out = []

    def add(name, raw, decoded, large, suffix=".gz"):
        path = os.path.join(str(tmp_dir), name + suffix)
        with open(path, "wb") as f:
            f.write(raw)
        out.append((name, path, decoded, large))

    whole = gzip.compress(text, 1)
    add("one_member", whole, text, True)
    # member cuts inside the long lines that also cross the ingest chunk cuts at 1 MiB and 3 MiB
    a, b = _mid_line(text, CHUNK + 700), _mid_line(text, 3 * CHUNK + 70000)
    assert b"\n" not in text[CHUNK - 1000:a + 1] and b"\n" not in text[3 * CHUNK - 1000:b + 1]
    add("three_members_cut_mid_line", gzip.compress(text[:a], 1) + gzip.compress(text[a:b], 6) + gzip.compress(text[b:], 1), text, True)
    add("trailing_garbage", whole + b"this is not gzip\n" * 3, text, True)
    add("truncated_in_deflate", whole[: len(whole) // 2], None, True)
    add("truncated_in_trailer", whole[:-3], None, True)
    add("empty_member", gzip.compress(b""), b"", False)
    add("empty_member_then_text", gzip.compress(b"") + gzip.compress(text[:5000]), text[:5000], False)
    add("magic_then_text", b"\x1f\x8b" + text[:5000], None, False, suffix=".txt")
    with open(os.path.join(FILES, "samplefile.txt.zst"), "rb") as f:
        frame = f.read()
    with open(os.path.join(FILES, "samplefile.txt"), "rb") as f:
        sample = f.read()
    add("zstd_frames", frame * 2000, sample * 2000, False, suffix=".zst")
    return out


EXTRA_PATTERN, EXTRA_ID = "fo+d?", 999  # (matches the committed sample file's lines, which no benchspec pattern does)


def oracle_job(job):
    """(rc, rows, batches) of the oracle's file path for one (path, patterns, ids, buffer_size, buffer_count): a picklable
    unit, so that a test can spread the oracle's slow single-threaded scans over worker processes."""
    import oracle_py

    path, patterns, ids, buffer_size, buffer_count = job
    return oracle_py.scan_file(path, patterns, ids=ids, buffer_size=buffer_size, buffer_count=buffer_count)


def runs(large: bool):
    """(buffer_size, buffer_count) per case: the large files with both scan buffer sizes and batch sizes 1, 16 and 64."""
    return [(bs, count) for bs in (262140, 1000) for count in (1, 16, 64)] if large else [(262140, 16), (1000, 1)]
