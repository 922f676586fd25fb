"""hyperscanner -r on the MI355X: a directory tree prints what the same files named one by one print."""
from __future__ import annotations

import os
import shutil

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")


def run(monkeypatch, capsys, argv):
    from hypergrep_amd import multiscanner

    monkeypatch.setattr("sys.argv", ["hyperscanner"] + argv)
    with pytest.raises(SystemExit) as exit_info:
        multiscanner.main()
    return capsys.readouterr().out, exit_info.value.code


@pytest.fixture()
def tree(tmp_path):
    import torch  # before the native library: a process must have ONE HIP runtime, torch's (__graft_entry__.build)

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU path to fall back to")
    root = str(tmp_path / "tree")
    names = []
    for rel, source in (("a/greptest1.txt", "greptest1.txt"), ("a/b/greptest2.txt", "greptest2.txt"), ("sample.txt", "samplefile.txt"),
                        ("z/sample.txt.gz", "samplefile.txt.gz"), ("z/sample.txt.zst", "samplefile.txt.zst")):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        shutil.copy(os.path.join(FILES, source), path)
        names.append(path)
    for rel, content in (("a/empty", b""), ("a/unterminated", b"no match\nfoo at the end"), ("m/nul", b"foo\0bar\n\0\0foo\n")):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as handle:
            handle.write(content)
        names.append(path)
    os.makedirs(os.path.join(root, "hollow"))
    return root, sorted(names)


@pytest.mark.parametrize("options", [["-n"], ["-c"], ["-l"], ["-L"], ["-v"], ["-o"], ["-m", "2"]])
def test_a_tree_prints_what_its_files_print(tree, monkeypatch, capsys, options):
    root, names = tree
    want, want_code = run(monkeypatch, capsys, ["-H"] + options + ["foo"] + names)
    got, code = run(monkeypatch, capsys, ["-r"] + options + ["foo", root])
    assert want and (got, code) == (want, want_code)
    assert run(monkeypatch, capsys, ["-R"] + options + ["foo", root]) == (want, want_code)


def test_without_the_option_a_directory_is_an_error(tree, monkeypatch, capsys):
    root, _names = tree
    out, code = run(monkeypatch, capsys, ["foo", root])
    assert code == 2 and "directory" in out.lower()
