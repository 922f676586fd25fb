"""The most frequent matched values of a file of many chunks on the MI355X: hg_hyperscan_values_top
(hypergrep_amd.count_values_top), the value store behind every chunk's scan and one ranking at the end.  The expectations are
Python's re and collections.Counter over the file's lines, hypergrep_amd.count_values_files over the file alone, and
hypergrep_amd.count_values for the totals.  A fresh child process reads the files with HYPERGREP_CHUNK_MB=1: 2.5 MiB are three
chunks."""
from __future__ import annotations

import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "files")
A = 14  # DOTALL | MULTILINE | SINGLEMATCH

CHILD = """
import collections, gzip, re, sys
import torch  # one HIP runtime per process: torch's
import hypergrep_amd
path, pattern, least = sys.argv[1], sys.argv[2], int(sys.argv[3])
data = gzip.open(path).read() if path.endswith(".gz") else open(path, "rb").read()
parts = [m for line in data.split(b"\\n") for m in re.findall(pattern.encode(), line)]
counts = collections.Counter(parts)  # (in the order of first occurrence)
shown = lambda rows: sorted(rows, key=lambda r: (-r[1], r[0]))
whole = hypergrep_amd.count_values(path, [pattern], flags=[14])
assert whole == (shown(counts.items()), 0) and len(counts) >= least, (len(whole[0]), len(counts))
for top in (1, 5, 10 ** 6):
    totals = []
    got = hypergrep_amd.count_values_top(path, [pattern], top, flags=[14], totals=totals)
    assert got == (shown(counts.most_common()[:top]), 0), (top, got[0][:8])
    assert got == hypergrep_amd.count_values_files([path], [pattern], flags=[14], top=top)[0], top
    assert totals == [(len(whole[0]), sum(r[1] for r in whole[0]))] == [(len(counts), len(parts))], (top, totals)
    keyed = hypergrep_amd.count_values_top(path, [pattern], top, flags=[14], by_pattern=True)
    assert keyed == ([(v, 0, c) for v, c in got[0]], 0), top
assert hypergrep_amd.count_values_top(path, [pattern], 0, flags=[14]) == whole
print("done", len(counts), len(parts))
"""


def run_child(path, pattern, least):
    env = dict(os.environ, HYPERGREP_CHUNK_MB="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    done = subprocess.run([sys.executable, "-c", CHILD, str(path), pattern, str(least)], env=env, capture_output=True, text=True, timeout=120, check=False)
    assert done.returncode == 0 and done.stdout.startswith("done "), done.stderr[-2000:]
    return [int(v) for v in done.stdout.split()[1:3]]


def test_three_chunks(tmp_path):
    """Values that tie in count across chunk borders: the cut goes by first occurrence in the file, whatever chunk it is in."""
    rng = random.Random(31)
    vocab = [b"%s=%d" % (rng.choice([b"user", b"code", b"req", b"n"]), rng.randrange(40)) for _ in range(120)]
    filler = [b"lorem", b"-", b"GET /index", b"=", b"a=", b"=7"]
    lines = [b" ".join(rng.choice(vocab + filler) for _ in range(rng.randint(0, 5))) + b"\n" for _ in range(180000)]
    # rare values on both sides of the chunk borders: counts of 1 and 2 tie at every cut below the vocabulary
    for k in range(60):
        lines[(k * 2477) % len(lines)] += b"rare=%d x\n" % (k % 45)
    data = b"".join(lines)
    nbytes = (5 << 20) // 2
    assert len(data) > nbytes
    path = tmp_path / "log.txt"
    path.write_bytes(data[:nbytes - 333])  # (a cut line: the last line has no newline)
    n_values, n_parts = run_child(path, "[a-z]+=[0-9]+", 100)
    assert n_parts > 100000


def test_gzip_fixture():
    assert run_child(os.path.join(GOLDEN, "samplefile.txt.gz"), "foo[a-z]*", 3) == [3, 4]
