"""Command-line cases of the context options, shared by the host formatting test and the GPU end-to-end test: the argument
lists, what the local GNU grep prints for them on the golden files, and the rows grep() has to deliver, worked out with `re`."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, "golden", "files")
GREP = shutil.which("grep")

FILE_SETS = [["greptest1.txt"], ["greptest1.txt", "greptest2.txt"], ["samplefile.txt"]]
CONTEXTS = [["-A", "1"], ["-B", "2"], ["-C", "1"], ["-A", "2", "-B", "1"], ["-C", "3"]]
MODES = [[], ["-n"], ["-H"], ["-v", "-n"], ["-m", "2", "-n"], ["-m", "2", "-v"], ["-o", "-n"], ["-i", "-n", "-h"]]
PATTERNS = ["bar", "foo"]


def cases():
    """(pattern, option list, file paths) of every case."""
    for pattern in PATTERNS:
        for names in FILE_SETS:
            for context in CONTEXTS:
                for mode in MODES:
                    yield pattern, context + mode, [os.path.join(FILES, n) for n in names]


def grep_run(pattern: str, options: list[str], paths: list[str]) -> tuple[str, int]:
    """What GNU grep prints (file names as given) and its exit code: 0 with a selected line, 1 without."""
    done = subprocess.run([GREP] + options + ["-e", pattern] + paths, capture_output=True, text=True, check=False)
    assert done.returncode in (0, 1), done.stderr
    return done.stdout, done.returncode


def grep_output(pattern: str, options: list[str], paths: list[str]) -> str:
    return grep_run(pattern, options, paths)[0]


def parse(options: list[str]) -> dict:
    opt = {"before": 0, "after": 0, "n": "-n" in options, "H": "-H" in options, "h": "-h" in options, "v": "-v" in options, "o": "-o" in options,
           "i": "-i" in options, "m": 0}
    for i, o in enumerate(options):
        if o == "-A":
            opt["after"] = int(options[i + 1])
        elif o == "-B":
            opt["before"] = int(options[i + 1])
        elif o == "-C":
            opt["before"] = opt["after"] = int(options[i + 1])
        elif o == "-m":
            opt["m"] = int(options[i + 1])
    return opt


def rows_for(path: str, pattern: str, opt: dict):
    """[(1-based line number, text, is_match)]: what grep(path, [pattern], ..., before_context, after_context) returns."""
    with open(path, encoding="utf-8") as f:
        lines = f.read().splitlines(keepends=True)
    finder = re.compile(pattern, re.IGNORECASE if opt["i"] else 0)
    matching = [i for i, line in enumerate(lines) if bool(finder.search(line)) != opt["v"]]
    kept = matching[:opt["m"]] if opt["m"] else matching
    context = set()
    for m in kept:
        context.update(range(max(0, m - opt["before"]), m))
        context.update(range(m + 1, min(len(lines), m + opt["after"] + 1)))
    if len(kept) == len(matching):
        context -= set(matching)
    else:  # under -m the trailing lines of the last counted line are context, matching or not (GNU grep 3.5 and later)
        context -= set(kept)
        context = {q for q in context if q <= kept[-1] + opt["after"]}
    return _rows(lines, kept, context, finder, opt)


def _rows(lines, kept, context, finder, opt):
    rows = []
    for i, line in enumerate(lines):
        if i in kept and i not in context:
            if opt["o"] and not opt["v"]:
                rows.extend((i + 1, part.group() + "\n", True) for part in finder.finditer(line))
            else:
                rows.append((i + 1, line, True))
        elif i in context:
            rows.append((i + 1, line, False))
    return rows
