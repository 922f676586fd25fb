"""Matched parts of many files in one native call on the MI355X: hg_hyperscan_files_parts through scan_files(parts=True),
grep_files(matched_parts=True) and the batch route of the command line (-r -o --gnu-parts).  The contract is equivalence with
the per-file route: grep_files(files, matched_parts=True) == [grep(f, matched_parts=True) for f in files], every file's rows
from scan_files(parts=True) are scan(parts=True)'s for the file alone, and the command line prints byte for byte what it
prints with HYPERGREP_BATCH_FILES=0."""
from __future__ import annotations

import os
import shutil

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")
PATTERNS = ["foo", "ba[rz]", "o+ b"]


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
    for i in range(4):  # copies of the golden files, some cut to an unterminated last line
        for name, content in golden.items():
            put(f"d{i % 2}/{i}_{name}", content if i % 2 else content[:len(content) - 1 - i])
    put("gen/empty", b"")
    put("gen/unterminated", b"no match\nfoo bar foo at the end")
    put("gen/one_line_a", b"foo bar\n")
    put("gen/one_line_b", b"foo baz\n")
    put("gen/nul_inside", b"foo\0bar\n\0\0foo\nbar\0\n")
    put("gen/nul_tail", b"foo\n\0\0\0")
    put("gen/big_line", b"x" * 300000 + b" foo\nbar\n")  # a line longer than buffer_size - 1: cut into pieces
    for source in ("samplefile.txt.gz", "samplefile.txt.zst"):  # the per-file route inside the call
        shutil.copy(os.path.join(FILES, source), os.path.join(root, "gen", source))
        names.append(os.path.join(root, "gen", source))
    names.sort()
    return root, names, os.path.join(root, "gen", "missing-name")


@pytest.mark.parametrize("kwargs", [{}, {"ignore_case": True}, {"max_match_count": 1}, {"count_only": True}, {"invert": True}],
                         ids=["plain", "ignore_case", "max_1", "count_only", "invert"])
def test_grep_files_equals_grep_per_file(tree, kwargs):
    import hypergrep_amd

    root, names, missing = tree
    files = names[:5] + [missing, root] + names[5:]  # a missing file and a directory among them
    want = [hypergrep_amd.grep(f, PATTERNS, matched_parts=True, no_messages=True, **kwargs) for f in files]
    assert hypergrep_amd.grep_files(files, PATTERNS, matched_parts=True, no_messages=True, **kwargs) == want
    assert want[5][1] == want[6][1] == hypergrep_amd.RC_INVALID_FILE
    if "invert" not in kwargs:
        assert any(w[0] for w in want)
    with pytest.raises(FileNotFoundError):
        hypergrep_amd.grep_files(files, PATTERNS, matched_parts=True, **kwargs)


def test_scan_files_rows_batches_and_summaries(tree):
    import hypergrep_amd

    _root, names, missing = tree
    files = [missing] + names
    seen = []

    def on_match(index, matches, count):
        assert 1 <= count <= 4
        seen.append((index, [(matches[i].line_number, matches[i].id, matches[i].line) for i in range(count)]))

    flags = [hypergrep_amd.HS_FLAG_DOTALL | hypergrep_amd.HS_FLAG_MULTILINE] * 3
    ids = [1, 2, 3]
    got = hypergrep_amd.scan_files(files, PATTERNS, on_match, flags=flags, ids=ids, buffer_count=4, parts=True)
    assert [index for index, _ in seen] == sorted(index for index, _ in seen)  # file order, no batch mixes files
    plain = hypergrep_amd.scan_files(files, PATTERNS, None, flags=flags, ids=ids)
    assert got == plain and got[0][0] == 6  # the summaries are those without parts
    for index, name in enumerate(files[1:], start=1):
        rows = []
        rc = hypergrep_amd.scan(name, PATTERNS, lambda m, c: rows.extend((m[i].line_number, m[i].id, m[i].line) for i in range(c)), flags=flags, ids=ids, parts=True)
        assert [r for i, batch in seen if i == index for r in batch] == rows, name
        assert got[index][0] == rc, name
    assert any(len(batch) > 1 for _i, batch in seen)
    # with a limit: the reports decide the lines, every part of a kept line goes out
    seen.clear()
    hypergrep_amd.scan_files(names, PATTERNS, on_match, flags=flags, ids=ids, buffer_count=4, max_match_count=2, parts=True)
    for index, name in enumerate(names):
        rows = []
        hypergrep_amd.scan(name, PATTERNS, lambda m, c: rows.extend((m[i].line_number, m[i].id, m[i].line) for i in range(c)), flags=flags, ids=ids, max_match_count=2,
                           parts=True)
        assert [r for i, batch in seen if i == index for r in batch] == rows, name


def test_a_refused_set_fails_the_whole_call(tree):
    import hypergrep_amd
    from hypergrep_amd import utils

    _root, names, _missing = tree
    seen = []
    got = hypergrep_amd.scan_files(names[:3], ["foo", "bar"], lambda i, m, c: seen.append(i), flags=[6, 6], ids=[1, 2], ext=[None, utils.ExprExt(flags=1, min_offset=2)],
                                   parts=True)
    assert got == [(4, 0, 0)] * 3 and not seen


def run(monkeypatch, capsys, argv):
    from hypergrep_amd import multiscanner

    monkeypatch.setattr("sys.argv", ["hyperscanner"] + argv)
    with pytest.raises(SystemExit) as exit_info:
        multiscanner.main()
    return capsys.readouterr().out, exit_info.value.code


@pytest.mark.parametrize("options", [["-rn", "-o", "--gnu-parts"], ["-r", "-o", "--gnu-parts", "-i"], ["-rn", "-o", "--gnu-parts", "-m", "1"]])
def test_command_line_batch_route_prints_what_the_per_file_route_prints(tree, monkeypatch, capsys, options):
    root, _names, _missing = tree
    argv = options + ["-e", "foo", "-e", "ba[rz]", root]
    monkeypatch.setenv("HYPERGREP_BATCH_FILES", "0")
    want = run(monkeypatch, capsys, argv)
    monkeypatch.delenv("HYPERGREP_BATCH_FILES")
    got = run(monkeypatch, capsys, argv)
    assert got == want and want[0] and want[1] == 0
