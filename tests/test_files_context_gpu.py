"""Context lines for many files in one native call on the MI355X: hg_hyperscan_files_context through scan_files() /
grep_files() and the batch route of the command line (-r with -A / -B / -C).  The contract is equivalence with the per-file
route: grep_files(files, **kw) == [grep(f, **kw) for f in files], every file's rows from scan_files() are scan()'s for the
file alone, and the command line prints byte for byte what it prints with HYPERGREP_BATCH_FILES=0 (and what GNU grep
prints, where there is one).  The tree is built as tests/test_files_gpu.py builds its own."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")
PATTERNS = ["foo", "ba[rz]"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    root = str(tmp_path_factory.mktemp("ctxtree"))
    names = []

    def put(rel, content):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as handle:
            handle.write(content)
        names.append(path)

    golden = {name: open(os.path.join(FILES, name), "rb").read() for name in ("greptest1.txt", "greptest2.txt", "samplefile.txt")}
    for i in range(10):  # 30 copies of the golden files, half of them cut to an unterminated last line
        for name, content in golden.items():
            put(f"d{i % 3}/{i}_{name}", content if i % 2 else content[:len(content) - 1 - i])
    put("gen/empty", b"")
    put("gen/empty2", b"")
    put("gen/last_line_matches", b"one\ntwo\nthree\nfoo")        # its after-context must not reach the next file ...
    put("gen/last_line_matches_next", b"bar\ntwo\nthree\nfour\n")  # ... nor this one's before-context the previous
    put("gen/one_byte", b"f")
    put("gen/only_newlines", b"\n\n\n")
    put("gen/nul_inside", b"foo\0bar\nx\n\0\0foo\ny\nbar\0\n")
    put("gen/nul_tail", b"foo\n\0\0\0")
    put("gen/nul_only", b"\0")
    put("gen/dense", b"foo\nfoo\nx\nfoo\ny\nz\nbar\n" * 20)
    put("gen/big_line", b"head\n" + b"x" * 300000 + b" foo\nbar\nafter\n")  # a line longer than buffer_size - 1: cut into pieces
    put("gen/large", (b"lorem ipsum foo dolor\nsit amet\nconsectetur\nadipiscing\nbaz\n" * 30000)[:1300000])  # larger than a 1 MiB pack
    for i in range(3):
        put(f"gen/medium{i}", b"medium foo line\nnothing\nat all\n" * 9000 + b"bar without newline")  # ~290 KiB each: several packs of 1 MiB
    for source in ("samplefile.txt.gz", "samplefile.txt.zst"):
        shutil.copy(os.path.join(FILES, source), os.path.join(root, "gen", source))
        names.append(os.path.join(root, "gen", source))
    names.sort()
    missing = os.path.join(root, "gen", "missing-name")
    return root, names, missing


CONTEXTS = [{"after_context": 1}, {"before_context": 2}, {"before_context": 1, "after_context": 2}]
EXTRAS = [{}, {"invert": True}, {"max_match_count": 2}, {"only_matching": True}, {"ignore_case": True}]
KWARGS = [dict(c, **e) for c in CONTEXTS for e in EXTRAS]


@pytest.mark.parametrize("chunk_mb", [None, "1"])
@pytest.mark.parametrize("kwargs", KWARGS, ids=lambda kw: "-".join(f"{k[:3]}{v}" for k, v in kw.items()))
def test_grep_files_equals_grep_per_file(tree, monkeypatch, kwargs, chunk_mb):
    import hypergrep_amd

    if chunk_mb:
        monkeypatch.setenv("HYPERGREP_CHUNK_MB", chunk_mb)  # packs of 1 MiB: several packs, and a file that fits none
    _root, names, missing = tree
    files = names[:20] + [missing] + names[20:]
    want = [hypergrep_amd.grep(f, PATTERNS, no_messages=True, **kwargs) for f in files]
    got = hypergrep_amd.grep_files(files, PATTERNS, no_messages=True, **kwargs)
    for f, g, w in zip(files, got, want):
        assert g == w, f
    assert want[20][1] == hypergrep_amd.RC_INVALID_FILE and any(w[0] for w in want)
    assert any(any(not row[2] for row in w[0]) for w in want), "some file must have context rows for this test to mean anything"
    with pytest.raises(FileNotFoundError):
        hypergrep_amd.grep_files(files, PATTERNS, **kwargs)


def test_count_only_with_context(tree):
    import hypergrep_amd

    _root, names, _missing = tree
    kwargs = {"count_only": True, "before_context": 1, "after_context": 1, "max_match_count": 3}
    assert hypergrep_amd.grep_files(names, PATTERNS, **kwargs) == [hypergrep_amd.grep(f, PATTERNS, **kwargs) for f in names]


@pytest.mark.parametrize("kwargs", [{"before_context": 2, "after_context": 1}, {"after_context": 3, "max_match_count": 2}, {"before_context": 1, "invert": True}],
                         ids=["B2A1", "A3m2", "B1v"])
def test_scan_files_rows_batches_and_summaries(tree, kwargs):
    import hypergrep_amd

    _root, names, missing = tree
    files = [missing] + names
    seen = []

    def on_match(index, matches, count):
        assert 1 <= count <= 4
        seen.append((index, [(matches[i].line_number, matches[i].id, matches[i].line) for i in range(count)]))

    flags = [hypergrep_amd.HS_FLAG_DOTALL | hypergrep_amd.HS_FLAG_MULTILINE] * 2  # every match end is a report
    got = hypergrep_amd.scan_files(files, PATTERNS, on_match, flags=flags, ids=[1, 2], buffer_count=4, **kwargs)
    assert [index for index, _ in seen] == sorted(index for index, _ in seen)  # file order, no batch mixes files
    plain = {k: v for k, v in kwargs.items() if k not in ("before_context", "after_context")}
    without = hypergrep_amd.scan_files(files, PATTERNS, lambda *_: None, flags=flags, ids=[1, 2], **plain)
    counts_only = hypergrep_amd.scan_files(files, PATTERNS, None, flags=flags, ids=[1, 2], **kwargs)
    assert got[0][0] == 6
    context_rows = 0
    for index, name in enumerate(files[1:], start=1):
        rows = []
        rc = hypergrep_amd.scan(name, PATTERNS, lambda m, c: rows.extend((m[i].line_number, m[i].id, m[i].line) for i in range(c)), flags=flags, ids=[1, 2], **kwargs)
        assert [r for i, batch in seen if i == index for r in batch] == rows, name
        context_rows += sum(1 for r in rows if r[1] == hypergrep_amd.utils.HG_ID_CONTEXT)
        assert got[index][0] == rc, name
        if name.endswith(("gen/large", ".gz", ".zst")) and "max_match_count" in kwargs:
            continue  # (the per-file route counts the pieces it scanned before the limit stopped it: with context it reads on)
        assert got[index] == without[index] == counts_only[index], name  # the summaries are those of the call without context
    assert context_rows > 0


def run(monkeypatch, capsys, argv):
    from hypergrep_amd import multiscanner

    monkeypatch.setattr("sys.argv", ["hyperscanner"] + argv)
    with pytest.raises(SystemExit) as exit_info:
        multiscanner.main()
    return capsys.readouterr().out, exit_info.value.code


@pytest.mark.parametrize("options", [["-rn", "-C1"], ["-r", "-A2", "-m2", "-n"], ["-r", "-v", "-B1"], ["-r", "-H", "-A1"], ["-r", "-c", "-C2"]],
                         ids=lambda o: "".join(o))
def test_command_line_batch_route_prints_what_the_per_file_route_prints(tree, monkeypatch, capsys, options):
    root, _names, missing = tree
    argv = options + ["-e", "foo", "-e", "ba[rz]", root, missing]
    monkeypatch.setenv("HYPERGREP_BATCH_FILES", "0")
    want = run(monkeypatch, capsys, argv)
    monkeypatch.delenv("HYPERGREP_BATCH_FILES")
    got = run(monkeypatch, capsys, argv)
    assert got == want
    assert want[1] == 2 and want[0]  # (the missing name: exit code 2)
    if "-c" not in options:
        assert "\n--\n" in want[0]


def test_command_line_takes_the_batch_route_with_context(tree, monkeypatch, capsys):
    from hypergrep_amd import utils

    root, _names, _missing = tree
    calls = []
    real = utils.grep_files_outcomes
    monkeypatch.setattr(utils, "grep_files_outcomes", lambda files, patterns, **kw: calls.append(kw) or real(files, patterns, **kw))
    out, code = run(monkeypatch, capsys, ["-rn", "-C2", "foo", root])
    assert code == 0 and out and len(calls) == 1 and calls[0]["before_context"] == calls[0]["after_context"] == 2


def test_two_files_print_what_gnu_grep_prints(tree, monkeypatch, capsys):
    """The two golden files in one batch, every context and mode of the command line cases: GNU grep's bytes and exit code
    where this machine has a grep, the per-file route's otherwise."""
    import context_cli_cases as cli

    names = cli.FILE_SETS[1]
    assert len(names) == 2
    paths = [os.path.join(cli.FILES, n) for n in names]
    for pattern in cli.PATTERNS:
        for context in cli.CONTEXTS:
            for mode in cli.MODES:
                options = context + mode
                got = run(monkeypatch, capsys, options + ["-e", pattern] + paths)
                if cli.GREP is not None:
                    want = cli.grep_run(pattern, options, paths)
                else:
                    monkeypatch.setenv("HYPERGREP_BATCH_FILES", "0")
                    want = run(monkeypatch, capsys, options + ["-e", pattern] + paths)
                    monkeypatch.delenv("HYPERGREP_BATCH_FILES")
                assert got == want, (pattern, options)


def test_a_context_id_is_refused(tree):
    import hypergrep_amd

    _root, names, _missing = tree
    called = []
    got = hypergrep_amd.scan_files(names[:3], ["bar"], lambda *a: called.append(a), ids=[0xFFFFFFFD], after_context=1)
    assert got == [(4, 0, 0)] * 3 and not called
    assert hypergrep_amd.scan_files(names[:3], ["bar"], None, ids=[0xFFFFFFFD], after_context=1) == hypergrep_amd.scan_files(names[:3], ["bar"], None, ids=[0xFFFFFFFD])


CHILD = """
import sys
import torch  # one HIP runtime per process: torch's
import hypergrep_amd
files = sys.argv[1:]
for kwargs in ({"before_context": 1, "after_context": 1}, {"invert": True, "max_match_count": 2, "after_context": 2}):
    got = hypergrep_amd.grep_files(files, ["foo", "ba[rz]"], no_messages=True, **kwargs)
    assert got == [hypergrep_amd.grep(f, ["foo", "ba[rz]"], no_messages=True, **kwargs) for f in files]
print("done", len(files))
"""


def test_one_pooled_context_is_enough(tree):
    """HYPERGREP_POOL=1 with the gzip file in the middle: the call must never hold its pack's context while a file of the
    per-file route takes one, or it waits for ever.  A child process, so that the pool's size is read afresh; the limit only
    ends a hang."""
    _root, names, missing = tree
    files = names + [missing]
    at = next(i for i, n in enumerate(files) if n.endswith(".gz"))
    assert 0 < at < len(files) - 2
    env = dict(os.environ, HYPERGREP_POOL="1", HYPERGREP_CHUNK_MB="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    done = subprocess.run([sys.executable, "-c", CHILD] + files, env=env, capture_output=True, text=True, timeout=120, check=False)
    assert done.returncode == 0 and done.stdout.strip() == f"done {len(files)}", done.stderr[-2000:]
