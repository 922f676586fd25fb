"""hyperscanner -r / -R: the directory walk and the option's place in the command line's namespace (no GPU needed)."""
from __future__ import annotations

import os

from hypergrep_amd import multiscanner


def make_tree(root):
    for rel in ("b/2.txt", "b/1.txt", "a.txt", "b/c/deep.log", "z/only.txt"):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w", encoding="utf-8") as handle:
            handle.write("foo\n")
    os.makedirs(os.path.join(root, "empty"))
    os.symlink(os.path.join(root, "nowhere"), os.path.join(root, "dangling"))


def test_directories_become_their_regular_files_sorted(tmp_path):
    root = str(tmp_path)
    make_tree(root)
    lone = os.path.join(root, "a.txt")
    got = multiscanner.expand_directories([lone, os.path.join(root, "b"), "missing-name", root])
    below_b = [os.path.join(root, "b", name) for name in ("1.txt", "2.txt", "c/deep.log")]
    everything = sorted([lone] + below_b + [os.path.join(root, "z", "only.txt")])
    assert got == [lone] + below_b + ["missing-name"] + everything  # a missing name stays, to be reported in its place
    unsorted = multiscanner.expand_directories([root], sort_files=False)
    assert sorted(unsorted) == everything


def test_the_option_exists_only_when_given():
    plain = multiscanner.parse_args(["foo", "x"])
    assert not hasattr(plain, "recursive")
    for flag in ("-r", "-R", "--recursive"):
        args = multiscanner.parse_args([flag, "-n", "foo", "dir"])
        assert args.recursive is True and args.line_number and args.files == ["dir"]
    assert multiscanner.parse_args(["-rn", "foo", "dir"]).recursive is True
