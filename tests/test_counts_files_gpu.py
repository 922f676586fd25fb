"""Counts per report id for files on the MI355X: hypergrep_amd.count / count_files (hg_hyperscan_counts,
hg_hyperscan_files_counts) and `hyperscanner --pattern-counts`.  The yardstick is counts_ref's plain count of the rows scan()
delivers for the same file, whose parity with the oracle the file tests hold."""
from __future__ import annotations

import gzip
import os
import subprocess
import sys

import pytest

import counts_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")
M = 6  # DOTALL | MULTILINE: every match end is a report
PATTERNS, FLAGS, IDS = ["foo", "ba[rz]", "o", "never-there"], [M, 14, M, 14], [7, 2, 7, 40]  # "foo" and "o" share id 7: their ends at one offset are one report


def from_rows(path, patterns=PATTERNS, flags=FLAGS, ids=IDS):
    """({id: (lines, reports)} over every id, rc) from scan()'s callback rows."""
    import hypergrep_amd

    rows = []

    def on_match(matches, n):
        rows.extend((0, matches[k].line_number, matches[k].id) for k in range(n))

    rc = hypergrep_amd.scan(path, patterns, on_match, flags=flags, ids=ids)
    ref = counts_ref.counts(rows)
    return {i: ref.get(i, (0, 0)) for i in sorted(set(ids))}, rc


@pytest.mark.parametrize("name", ["samplefile.txt", "samplefile.txt.gz", "samplefile.txt.zst"])
def test_count_equals_the_rows_of_scan(name):
    import hypergrep_amd

    path = os.path.join(FILES, name)
    want = from_rows(path)
    assert want[1] == 0 and want[0][7][1] > want[0][7][0] > 0 and want[0][40] == (0, 0)
    assert hypergrep_amd.count(path, PATTERNS, flags=FLAGS, ids=IDS) == want


CHILD = """
import sys
import torch  # one HIP runtime per process: torch's
import hypergrep_amd
import test_counts_files_gpu as t
path = sys.argv[1]
want = t.from_rows(path)
got = hypergrep_amd.count(path, t.PATTERNS, flags=t.FLAGS, ids=t.IDS)
assert want[1] == 0 and got == want, (got, want)
print("done", sum(v[1] for v in got[0].values()))
"""


def test_three_chunks_accumulate(tmp_path):
    """A 2.5 MiB file under HYPERGREP_CHUNK_MB=1 (a fresh child process reads it): three chunks add up to the file's counts."""
    from hypergrep_amd import benchspec, device

    _patterns, needles, hpm = benchspec.c3_spec()
    nbytes = (5 << 20) // 2
    path = tmp_path / "log.txt"
    path.write_bytes(device.synth_host(nbytes, 9, needles, hpm * 3)[: nbytes - 333])  # the last line has no newline
    env = dict(os.environ, HYPERGREP_CHUNK_MB="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    done = subprocess.run([sys.executable, "-c", CHILD, str(path)], env=env, capture_output=True, text=True, timeout=120, check=False)
    assert done.returncode == 0 and done.stdout.startswith("done "), done.stderr[-2000:]
    assert int(done.stdout.split()[1]) > 1000


@pytest.fixture()
def tree(tmp_path):
    names = {"a.txt": b"foo\nq\nbar foo\n", "b.txt": b"foo\nbaz\n", "empty.txt": b"", "c.txt": b"q\nq\nboo", "none.txt": b"q\n"}
    for name, data in names.items():
        (tmp_path / name).write_bytes(data)
    with gzip.open(tmp_path / "z.txt.gz", "wb") as f:
        f.write(b"foo foo\nbar\n" * 30)
    files = [str(tmp_path / n) for n in ("a.txt", "b.txt", "empty.txt", "z.txt.gz", "c.txt", "none.txt")]
    return files[:3] + [str(tmp_path / "missing.txt")] + files[3:]


def test_count_files_equals_count_per_file(tree):
    import hypergrep_amd

    got = hypergrep_amd.count_files(tree, PATTERNS, flags=FLAGS, ids=IDS)
    assert got == [hypergrep_amd.count(f, PATTERNS, flags=FLAGS, ids=IDS) for f in tree]
    assert [rc for _c, rc in got] == [s[0] for s in hypergrep_amd.scan_files(tree, PATTERNS, None, flags=FLAGS, ids=IDS)] == [0, 0, 0, 6, 0, 0, 0]
    # a.txt and b.txt both match on their line 0: the same file-relative line in two files of one pack stays two lines
    assert got[0][0] == {2: (1, 1), 7: (2, 4), 40: (0, 0)} and got[1][0] == {2: (1, 1), 7: (1, 2), 40: (0, 0)}
    assert got[2][0] == got[3][0] == got[6][0] == {2: (0, 0), 7: (0, 0), 40: (0, 0)}
    assert got[4][0] == {2: (30, 30), 7: (30, 120), 40: (0, 0)} and got[5][0][7] == (1, 2)
    for f, (counts, rc) in zip(tree, got):
        if rc == 0:
            assert (counts, rc) == from_rows(f), f


def test_pattern_counts_command_line(monkeypatch, capsys):
    from hypergrep_amd import multiscanner

    one, two = os.path.join(FILES, "greptest1.txt"), os.path.join(FILES, "greptest2.txt")
    monkeypatch.setattr("sys.argv", ["hyperscanner", "--pattern-counts", "-e", "foo", "-e", "bar", "-e", "absent", one, two])
    with pytest.raises(SystemExit) as stop:
        multiscanner.main()
    # what `grep -c -e foo` and `grep -c -e bar` print for the two files, pattern by pattern
    assert capsys.readouterr().out == f"{one}:16:foo\n{one}:9:bar\n{two}:16:foo\n{two}:9:bar\n"
    assert stop.value.code == 0
    monkeypatch.setattr("sys.argv", ["hyperscanner", "--pattern-counts", "-E", "-h", "-e", "bar", "-e", "fo+d", one])
    with pytest.raises(SystemExit) as stop:
        multiscanner.main()
    assert capsys.readouterr().out == "9:bar\n1:fo+d\n" and stop.value.code == 0
    monkeypatch.setattr("sys.argv", ["hyperscanner", "--pattern-counts", "-e", "absent", one])
    with pytest.raises(SystemExit) as stop:
        multiscanner.main()
    assert capsys.readouterr().out == "" and stop.value.code == 1
