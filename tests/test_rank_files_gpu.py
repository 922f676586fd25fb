"""Ranked matched values of many files on the MI355X: hg_hyperscan_files_values (hypergrep_amd.count_values_files) and
hyperscanner --value-counts over several files, with and without --top.  The expectations are hypergrep_amd.count_values and
hypergrep_amd.grep(matched_parts=True) over each file alone, and the stated rule (count descending, then first occurrence in the
file) applied in Python to the parts in their order."""
from __future__ import annotations

import collections
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "files")
A = 14  # DOTALL | MULTILINE | SINGLEMATCH
PATTERNS = ["[a-z]+=[0-9]+", "ERR[0-9]+", "foo[a-z]*"]
FLAGS = [A, A, A]


def mix_text(rng, lines):
    vocab = [b"%s=%d" % (rng.choice([b"user", b"code", b"req", b"n"]), rng.randrange(12)) for _ in range(50)] + [b"ERR%d" % rng.randrange(5) for _ in range(5)]
    filler = [b"lorem", b"-", b"GET /index", b"=", b"a=", b"=7"]
    return b"".join(b" ".join(rng.choice(vocab + filler) for _ in range(rng.randint(0, 5))) + b"\n" for _ in range(lines))


@pytest.fixture(scope="module")
def six(tmp_path_factory):
    """Six files: three small text files, one of them empty; a gzip fixture; a file of three chunks (HYPERGREP_CHUNK_MB=1 makes a
    pack 1 MiB, so it also takes the per-file route); a missing file.  With them, per file, the parts in their order (None for the
    missing file) from grep(matched_parts=True)."""
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    import hypergrep_amd

    root = tmp_path_factory.mktemp("rank_files")
    rng = random.Random(17)
    contents = {"a.log": b"n=1 n=2 n=1\nfood n=1\nERR3 n=2 k=9\n", "empty.log": b"", "b.log": b"k=5 foo\nk=5 n=1\nnothing\nfoo k=6 k=7 foo\n", "big.log": mix_text(rng, 150000)}
    assert len(contents["big.log"]) > 2 << 20
    for name, data in contents.items():
        (root / name).write_bytes(data)
    names = [str(root / "a.log"), str(root / "empty.log"), os.path.join(GOLDEN, "samplefile.txt.gz"), str(root / "big.log"), str(root / "missing.log"), str(root / "b.log")]
    old = os.environ.get("HYPERGREP_CHUNK_MB")
    os.environ["HYPERGREP_CHUNK_MB"] = "1"
    parts = []
    for name in names:
        got, rc = hypergrep_amd.grep(name, PATTERNS, matched_parts=True) if os.path.exists(name) else (None, 6)
        parts.append(None if rc else [part.rstrip("\n").encode() for _line, part in got])
    yield names, parts
    if old is None:
        del os.environ["HYPERGREP_CHUNK_MB"]
    else:
        os.environ["HYPERGREP_CHUNK_MB"] = old


def ranking(parts, top=0):
    """The stated rule over a file's parts in their order: (value, count) by count descending, then first occurrence; the cut."""
    counts = collections.Counter(parts)
    first = {}
    for q, v in enumerate(parts):
        first.setdefault(v, q)
    rows = sorted(counts.items(), key=lambda r: (-r[1], first[r[0]]))
    return rows[:top] if top else rows


def shown(rows):
    """As count_values() sorts its rows: count descending, then value."""
    return sorted(rows, key=lambda r: (-r[1], r[0]))


def test_top_zero_equals_the_loop_over_count_values(six):
    import hypergrep_amd

    names, parts = six
    totals = []
    got = hypergrep_amd.count_values_files(names, PATTERNS, flags=FLAGS, totals=totals)
    loop = [hypergrep_amd.count_values(n, PATTERNS, flags=FLAGS) for n in names]
    assert got == loop
    assert [rc for _rows, rc in got] == [0, 0, 0, 0, 6, 0] and got[1] == ([], 0) and got[4] == ([], 6)
    for (rows, _rc), mine in zip(got, parts):
        assert rows == (shown(ranking(mine)) if mine is not None else [])
    assert got[2][0] == [(b"foo", 2), (b"foobar", 1), (b"food", 1)] and 30 < len(got[3][0]) < 70
    # the callback sees the distinct values and the counted parts before the cut
    assert totals == [(len(set(p)), len(p)) if p is not None else (0, 0) for p in parts]
    keyed = hypergrep_amd.count_values_files(names, PATTERNS, flags=FLAGS, by_pattern=True)
    assert keyed == [hypergrep_amd.count_values(n, PATTERNS, flags=FLAGS, by_pattern=True) for n in names]


@pytest.mark.parametrize("buffer_size", [262140, 4096])
def test_top_two_whichever_route_a_file_took(six, buffer_size):
    """The small files are packed, the gzip file and the big one take the per-file route; 4096 cuts the big file's chunks into
    small pieces."""
    import hypergrep_amd

    names, parts = six
    totals = []
    got = hypergrep_amd.count_values_files(names, PATTERNS, flags=FLAGS, top=2, buffer_size=buffer_size, totals=totals)
    for name, (rows, rc), mine in zip(names, got, parts):
        assert (rows, rc) == ((shown(ranking(mine, top=2)), 0) if mine is not None else ([], 6)), name
    assert got[0][0] == [(b"n=1", 3), (b"n=2", 2)] and got[5][0] == [(b"foo", 3), (b"k=5", 2)] and got[2][0] == [(b"foo", 2), (b"foobar", 1)]  # (foobar before food: it occurs first)
    assert totals == [(len(set(p)), len(p)) if p is not None else (0, 0) for p in parts]  # before the cut


def test_a_tie_at_the_cut_goes_to_the_first_occurrence_not_to_the_value(six, tmp_path):
    import hypergrep_amd

    import gzip

    data = b"z=1 b=1 a=1\nz=1\n"
    (tmp_path / "tie.log").write_bytes(data)  # packed
    with gzip.open(tmp_path / "tie.log.gz", "wb") as f:  # the per-file route
        f.write(data)
    names = [str(tmp_path / "tie.log"), str(tmp_path / "tie.log.gz")]
    assert hypergrep_amd.count_values_files(names, PATTERNS, flags=FLAGS, top=2) == [([(b"z=1", 2), (b"b=1", 1)], 0)] * 2


def run_cli(args, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    return subprocess.run([sys.executable, "-m", "hypergrep_amd.multiscanner", "-E", "--value-counts", "-e", "[a-z]+=[0-9]+", "-e", "foo[a-z]*"] + args, capture_output=True, cwd=REPO,
                          check=False, env=env)


def test_command_line_recursive_and_top(tmp_path):
    d = tmp_path / "logs"
    (d / "sub").mkdir(parents=True)
    (d / "a.log").write_bytes(b"n=1 n=2 n=1\nn=1\n")
    (d / "b.log").write_bytes(b"k=5\nzz=1 food k=5\n")
    (d / "sub" / "c.log").write_bytes(b"nothing\n")
    batched, loop = run_cli(["-r", str(d)]), run_cli(["-r", str(d)], {"HYPERGREP_BATCH_FILES": "0"})
    assert batched.returncode == 0 and batched.stdout == loop.stdout and batched.stdout.count(b"\n") == 5, batched.stderr
    a, b = str(d / "a.log").encode(), str(d / "b.log").encode()
    assert set(batched.stdout.splitlines()) == {a + b":3:n=1", a + b":1:n=2", b + b":2:k=5", b + b":1:food", b + b":1:zz=1"}
    top, top_loop = run_cli(["--top", "1", "-r", str(d)]), run_cli(["--top", "1", "-r", str(d)], {"HYPERGREP_BATCH_FILES": "0"})
    assert top.returncode == 0 and top.stdout == top_loop.stdout and set(top.stdout.splitlines()) == {a + b":3:n=1", b + b":2:k=5"}, top.stderr
    one = run_cli(["--top", "2", str(d / "b.log")])
    assert one.returncode == 0 and one.stdout == b"2:k=5\n1:zz=1\n", one.stderr  # (zz=1 occurs before food)
    refused = subprocess.run([sys.executable, "-m", "hypergrep_amd.multiscanner", "-E", "--top", "2", "-e", "foo", str(d / "a.log")], capture_output=True, cwd=REPO, check=False)
    assert refused.returncode == 2 and b"--top is only valid with --value-counts" in refused.stderr
