"""Many files in one native call on the MI355X: hg_hyperscan_files through scan_files() / grep_files() and the batch route of
the command line.  The contract is equivalence with the per-file route: grep_files(files) == [grep(f) for f in files], and
the command line prints byte for byte what it prints with HYPERGREP_BATCH_FILES=0."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

import pytest

import invert_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")
PATTERNS = ["foo", "ba[rz]"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    root = str(tmp_path_factory.mktemp("tree"))
    names = []

    def put(rel, content):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as handle:
            handle.write(content)
        names.append(path)

    golden = {name: open(os.path.join(FILES, name), "rb").read() for name in ("greptest1.txt", "greptest2.txt", "samplefile.txt")}
    for i in range(10):  # 30 copies of the golden files, some cut to an unterminated last line
        for name, content in golden.items():
            put(f"d{i % 3}/{i}_{name}", content if i % 2 else content[:len(content) - 1 - i])
    put("gen/empty", b"")
    put("gen/unterminated", b"no match\nfoo at the end")
    put("gen/one_byte", b"f")
    put("gen/only_newlines", b"\n\n\n")
    put("gen/nul_inside", b"foo\0bar\n\0\0foo\nbar\0\n")
    put("gen/nul_tail", b"foo\n\0\0\0")
    put("gen/nul_only", b"\0")
    put("gen/big_line", b"x" * 300000 + b" foo\nbar\n")  # a line longer than buffer_size - 1: cut into pieces
    put("gen/large", (b"lorem ipsum foo dolor\nsit amet\nbaz\n" * 40000)[:1300000])  # larger than a 1 MiB pack
    for i in range(4):
        put(f"gen/medium{i}", b"medium foo line\nnothing\n" * 12000 + b"bar without newline")  # ~290 KiB each: several packs of 1 MiB
    for source in ("samplefile.txt.gz", "samplefile.txt.zst"):
        shutil.copy(os.path.join(FILES, source), os.path.join(root, "gen", source))
        names.append(os.path.join(root, "gen", source))
    names.sort()
    missing = os.path.join(root, "gen", "missing-name")
    return root, names, missing


KWARGS = [{}, {"invert": True}, {"count_only": True}, {"max_match_count": 2}, {"only_matching": True}, {"ignore_case": True, "invert": True, "max_match_count": 3},
          {"count_only": True, "invert": True}]


@pytest.mark.parametrize("chunk_mb", [None, "1"])
@pytest.mark.parametrize("kwargs", KWARGS)
def test_grep_files_equals_grep_per_file(tree, monkeypatch, kwargs, chunk_mb):
    import hypergrep_amd

    if chunk_mb:
        monkeypatch.setenv("HYPERGREP_CHUNK_MB", chunk_mb)  # packs of 1 MiB: several packs, and a file that fits none
    _root, names, missing = tree
    files = names[:20] + [missing] + names[20:]
    want = [hypergrep_amd.grep(f, PATTERNS, no_messages=True, **kwargs) for f in files]
    assert hypergrep_amd.grep_files(files, PATTERNS, no_messages=True, **kwargs) == want
    assert want[20][1] == hypergrep_amd.RC_INVALID_FILE and any(w[0] for w in want)
    with pytest.raises(FileNotFoundError):
        hypergrep_amd.grep_files(files, PATTERNS, **kwargs)


def test_scan_files_summaries_and_batches(tree):
    import hypergrep_amd

    _root, names, missing = tree
    files = [missing] + names
    seen = []

    def on_match(index, matches, count):
        assert 1 <= count <= 4
        seen.append((index, [(matches[i].line_number, matches[i].id, matches[i].line) for i in range(count)]))

    flags = [hypergrep_amd.HS_FLAG_DOTALL | hypergrep_amd.HS_FLAG_MULTILINE] * 2  # every match end is a report
    got = hypergrep_amd.scan_files(files, PATTERNS, on_match, flags=flags, ids=[1, 2], buffer_count=4)
    assert [index for index, _ in seen] == sorted(index for index, _ in seen)  # file order, no batch mixes files
    counts_only = hypergrep_amd.scan_files(files, PATTERNS, None, flags=flags, ids=[1, 2])
    assert got[0][0] == 6 and counts_only[0][0] == 6
    for index, name in enumerate(files[1:], start=1):
        rows = []
        rc = hypergrep_amd.scan(name, PATTERNS, lambda m, c: rows.extend((m[i].line_number, m[i].id, m[i].line) for i in range(c)), flags=flags, ids=[1, 2])
        assert [r for i, batch in seen if i == index for r in batch] == rows, name
        assert got[index][0] == rc == counts_only[index][0], name
        assert got[index][2] == counts_only[index][2] == len({r[0] for r in rows}), name
        assert got[index][1] == counts_only[index][1], name
        if not name.endswith((".gz", ".zst")):  # the file's line pieces, counted in Python from its bytes
            assert got[index][1] == len(invert_ref.pieces(open(name, "rb").read(), 262140)), name


def run(monkeypatch, capsys, argv):
    from hypergrep_amd import multiscanner

    monkeypatch.setattr("sys.argv", ["hyperscanner"] + argv)
    with pytest.raises(SystemExit) as exit_info:
        multiscanner.main()
    return capsys.readouterr().out, exit_info.value.code


@pytest.mark.parametrize("options", [["-rn"], ["-r", "-c"], ["-r", "-l"], ["-r", "-L"], ["-r", "-v"], ["-r", "-o"], ["-r", "-m", "2", "-n"], ["-r", "-t"],
                                     ["-r", "-vc", "-i"], ["-rs", "-n"]])
def test_command_line_batch_route_prints_what_the_per_file_route_prints(tree, monkeypatch, capsys, options):
    root, _names, missing = tree
    argv = options + ["-e", "foo", "-e", "ba[rz]", root, missing]
    monkeypatch.setenv("HYPERGREP_BATCH_FILES", "0")
    want = run(monkeypatch, capsys, argv)
    monkeypatch.delenv("HYPERGREP_BATCH_FILES")
    got = run(monkeypatch, capsys, argv)
    assert got == want
    assert want[1] == 2 and (want[0] or "-q" in options)  # (the missing name: exit code 2)


def test_quiet_stops_at_the_first_match_on_both_routes(tree, monkeypatch, capsys):
    root, _names, _missing = tree
    monkeypatch.setenv("HYPERGREP_BATCH_FILES", "0")
    want = run(monkeypatch, capsys, ["-rq", "foo", root])
    monkeypatch.delenv("HYPERGREP_BATCH_FILES")
    assert run(monkeypatch, capsys, ["-rq", "foo", root]) == want == ("", 0)


def test_only_empty_files(tree, tmp_path):
    import hypergrep_amd

    files = []
    for i in range(3):
        files.append(str(tmp_path / f"empty{i}"))
        open(files[-1], "wb").close()
    assert hypergrep_amd.scan_files(files, PATTERNS, None) == [(0, 0, 0)] * 3
    assert hypergrep_amd.grep_files(files, PATTERNS, invert=True) == [([], 0)] * 3 == [hypergrep_amd.grep(f, PATTERNS, invert=True) for f in files]


CHILD = """
import sys
import torch  # one HIP runtime per process: torch's
import hypergrep_amd
files = sys.argv[1:]
for kwargs in ({}, {"invert": True, "max_match_count": 2}):
    got = hypergrep_amd.grep_files(files, ["foo", "ba[rz]"], no_messages=True, **kwargs)
    assert got == [hypergrep_amd.grep(f, ["foo", "ba[rz]"], no_messages=True, **kwargs) for f in files]
print("done", len(files))
"""


def test_one_pooled_context_is_enough(tree):
    """HYPERGREP_POOL=1: the call must never hold its pack's context while a file of the per-file route (compressed, oversized)
    takes one, or it waits for ever.  A child process, so that the pool's size is read afresh; the limit only ends a hang."""
    _root, names, missing = tree
    files = names + [missing]
    assert any(n.endswith(".gz") for n in files[1:]) and any(n.endswith("empty") for n in files)
    env = dict(os.environ, HYPERGREP_POOL="1", HYPERGREP_CHUNK_MB="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    done = subprocess.run([sys.executable, "-c", CHILD] + files, env=env, capture_output=True, text=True, timeout=120, check=False)
    assert done.returncode == 0 and done.stdout.strip() == f"done {len(files)}", done.stderr[-2000:]
