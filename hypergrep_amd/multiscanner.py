#! /usr/bin/env python3
"""GNU-grep style front end over hypergrep_amd.grep(): many files, one pattern set, results replayed in file order.

Counterpart of the reference's hypergrep/multiscanner.py (same function names, arguments, output lines and exit
codes: parallel_grep :86-223, print_results :226-255, read_stdin :258-270, to_basic_regular_expressions :273-305,
to_gnu_regular_expressions :308-328, parse_args :331-548, main :551-606), written for this engine:

* the scan of each file is one `hyperscan()` call of the native library, which streams the file into HBM and hands
  files to the node's GPUs round-robin — the pool here only has to keep a few calls in flight, it does no matching;
* finished files are reported by the calling thread as their futures complete (no pool callbacks), a file that
  finishes early waits in `parked` until every file before it has been printed;
* `--mp` uses spawned (not forked) worker processes: a forked child must not inherit an initialised HIP runtime.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import multiprocessing
import os
import re
import sys
import textwrap
from typing import Any, Generator, Iterable

import hypergrep_amd

_BRE_LITERALS = "+?(){}|"  # regex operators in ERE / PCRE, ordinary characters in a POSIX basic regular expression


def _grep_with_index(index: int, args: Iterable, kwargs: dict[str, Any]) -> tuple[int, Any]:
    """One job: grep a file, hand back (job index, result or the exception it raised)."""
    try:
        return index, hypergrep_amd.grep(*args, **kwargs)
    except Exception as error:  # pylint: disable=broad-except
        return index, error


def get_argparse_files(args: argparse.Namespace) -> list[str]:
    """Files named on the command line.  As in GNU grep, once -e / -f supplies patterns the first positional is a file."""
    named = list(args.files or [])
    if args.pattern and (args.patterns or args.pattern_files):
        named.insert(0, args.pattern)
    return named


def expand_directories(names: list[str], sort_files: bool = True) -> list[str]:
    """-r / -R: every directory among `names` is replaced by the regular files below it (walked top down; sorted by path unless
    sort_files is False, then in the order the directory listing gives them).  Other names stay as they are."""
    found: list[str] = []
    for name in names:
        if not os.path.isdir(name):
            found.append(name)
            continue
        below = []
        for root, directories, members in os.walk(name):
            if sort_files:
                directories.sort()
                members = sorted(members)
            below.extend(path for path in (os.path.join(root, member) for member in members) if os.path.isfile(path))
        found.extend(sorted(below) if sort_files else below)
    return found


def get_argparse_patterns(args: argparse.Namespace) -> list[str]:
    """Patterns from -e, -f FILE (one per line) or, without either, the first positional.

    Raises ValueError (message in grep's style) for a pattern Python's `re` rejects or the engine cannot compile.
    """
    found: list[str] = list(args.patterns or [])
    if not found and not args.pattern_files and args.pattern:
        found.append(args.pattern)
    for name in args.pattern_files or []:
        with open(name, "rt", encoding="utf-8") as handle:
            found.extend(line.rstrip("\n") for line in handle.readlines())
    for pattern in found:  # cheap syntax check with a readable message before the engine's yes / no answer
        try:
            re.compile(pattern)
        except Exception as error:
            raise ValueError(f"hyperscanner: invalid regex: {error}") from error
    if hypergrep_amd.check_compatibility(found):
        raise ValueError(
            "hyperscanner: incompatible regex: for more information visit "
            "https://intel.github.io/hyperscan/dev-reference/compilation.html#unsupported-constructs"
        )
    return found


class _Replay:
    """Turns finished grep jobs into output lines, in file order when asked to, and keeps the exit-code facts."""

    def __init__(self, files: list, options: dict[str, Any]):
        self.files = files
        self.opt = options
        self.parked: dict[int, Any] = {}
        self.due = 0  # index of the next file to report in ordered mode
        self.total = 0
        self.matched = False
        self.errored = False
        self.context_state = {"printed": False}  # context output: something was printed, so the next group is set off by "--"

    def accept(self, index: int, outcome: Any) -> None:
        if self.opt["ordered_results"] and index != self.due:
            self.parked[index] = outcome
            return
        self._report(index, outcome)
        while self.due in self.parked:
            self._report(self.due, self.parked.pop(self.due))

    def _report(self, index: int, outcome: Any) -> None:
        name = self.files[index]
        opt = self.opt
        if isinstance(outcome, Exception):
            print(f"hyperscanner: {name}: {outcome}")  # grep's message shape
            self.errored = True
            self.due += 1
            return
        found, return_code = outcome
        if return_code:
            self.errored = True
        if found:
            self.matched = True
            if opt["quiet"]:
                return  # first match ends a quiet run; nothing is printed and the order no longer matters
        if opt["files_without_match"]:
            if not found:
                print(name)
        elif opt["files_with_matches"]:
            if found:
                print(name)
        elif opt["total_results"]:
            self.total += found
        elif opt["count_results"]:
            print(f"{name}:{found}" if opt["with_file_name"] else f"{found}")
        elif not opt["rows_unprinted"]:  # (-o -v: the selected lines decide the exit code, and none has a matched part to print)
            try:
                if opt["context"]:
                    print(format_context_results(found, name, opt["with_file_name"], opt["with_line_number"], opt["only_matching"], self.context_state), end="")
                else:
                    print_results(found, name, with_file_name=opt["with_file_name"], with_line_number=opt["with_line_number"])
            except BrokenPipeError:
                pass  # `| head` closed stdout: keep draining jobs quietly
        self.due += 1


def parallel_grep(  # pylint: disable=too-many-arguments,too-many-locals
    files: list,
    patterns: list[str],
    ignore_case: bool = False,
    ordered_results: bool = True,
    count_results: bool = False,
    total_results: bool = False,
    with_file_name: bool = False,
    with_line_number: bool = False,
    use_multithreading: bool = True,
    only_matching: bool = False,
    no_messages: bool = False,
    max_match_count: int = 0,
    files_without_match: bool = False,
    files_with_matches: bool = False,
    quiet: bool = False,
    invert_match: bool = False,
    gnu_parts: bool = False,
    before_context: int = 0,
    after_context: int = 0,
) -> int:
    """Search files for the patterns and print what grep would print.

    Args:
        files: files to scan (plain, gzip or zstd).
        patterns: regular expressions the engine accepts.
        ignore_case: case-insensitive matching.
        ordered_results: print a file's results only after those of every earlier file.
        count_results: print the number of matching lines per file instead of the lines.
        total_results: print one number, the matching lines of all files together.
        with_file_name / with_line_number: output prefixes.
        use_multithreading: threads (default) or, if False, spawned worker processes.
        only_matching: print each matched part on its own line.
        no_messages: no error text for missing / unreadable files.
        max_match_count: stop reading a file after that many matching lines (0: no limit).
        files_without_match / files_with_matches: print file names only; reading stops at the first match.
        quiet: print nothing and stop everything at the first match.
        invert_match: select the lines NO pattern matches (grep -v).  Counts, totals, -l / -L / -q and max_match_count then
            go by the selected lines; with only_matching nothing is printed, and the exit code still goes by the selected lines.
        gnu_parts: with only_matching, print the parts the GPU computes (grep(matched_parts=True)): GNU grep's -o over all
            patterns at once, leftmost-longest.  Without only_matching, with invert_match or with context lines it changes nothing.
        before_context / after_context: also print that many lines before / after each selected line (grep -B / -A), in GNU
            grep's format: "-" instead of ":" after the prefixes of a context line, "--" between groups that are not adjacent.
            They change nothing where lines are only counted or files only listed.

    Returns:
        grep's exit code: 2 after any error, else 1 without a match, else 0.
    """
    if files_without_match or files_with_matches or quiet:
        max_match_count = 1  # these modes only ask "is there a match"
    listing = count_results or total_results or files_without_match or files_with_matches or quiet
    context = bool(before_context or after_context) and not listing
    replay = _Replay(
        files,
        {"ordered_results": ordered_results, "count_results": count_results, "total_results": total_results, "with_file_name": with_file_name,
         "with_line_number": with_line_number, "files_without_match": files_without_match, "files_with_matches": files_with_matches, "quiet": quiet,
         "rows_unprinted": only_matching and invert_match, "context": context, "only_matching": only_matching},
    )
    job_kwargs = {
        "ignore_case": ignore_case,
        "count_only": count_results or total_results,
        "only_matching": only_matching and not invert_match,  # (-o -v: the jobs still report the selected lines, GNU grep's exit code)
        "no_messages": no_messages,
        "max_match_count": max_match_count,
        "invert": invert_match,
    }
    if context:
        job_kwargs.update(before_context=before_context, after_context=after_context)
    elif gnu_parts and only_matching and not invert_match:
        job_kwargs["matched_parts"] = True
    # More than one file, threads: the batch route, with or without context lines.  The files share one native call, small ones
    # one GPU scan (hypergrep_amd.grep_files); the outcomes are replayed exactly as the per-file jobs' are.
    # HYPERGREP_BATCH_FILES=0 keeps the per-file route (A/B runs).
    if len(files) > 1 and use_multithreading and os.environ.get("HYPERGREP_BATCH_FILES", "1") != "0":
        try:
            outcomes = hypergrep_amd.utils.grep_files_outcomes(files, patterns, **job_kwargs)
        except Exception as error:  # pylint: disable=broad-except
            outcomes = [error] * len(files)  # (what every per-file job would have raised: a pattern `re` rejects)
        for index, outcome in enumerate(outcomes):
            replay.accept(index, outcome)
            if quiet and replay.matched:
                break
        if total_results:
            print(replay.total)
        return 2 if replay.errored else (0 if replay.matched else 1)
    # the reference runs one job per core; here a job is a GPU scan with its own reader threads and pinned buffers, so a
    # handful in flight already keeps every GPU of the node busy
    workers = max(1, min(len(files), max((os.cpu_count() or 2) - 1, 1), 16))
    if use_multithreading:
        pool: concurrent.futures.Executor = concurrent.futures.ThreadPoolExecutor(max_workers=workers)
    else:
        pool = concurrent.futures.ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("spawn"))
    try:
        jobs = [pool.submit(_grep_with_index, index, (name, patterns), job_kwargs) for index, name in enumerate(files)]
        for done in concurrent.futures.as_completed(jobs):
            replay.accept(*done.result())
            if quiet and replay.matched:
                for job in jobs:
                    job.cancel()
                break
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
    if total_results:
        print(replay.total)
    return 2 if replay.errored else (0 if replay.matched else 1)


def pattern_counts(files: list, patterns: list[str], shown: list[str] | None = None, ignore_case: bool = False, with_file_name: bool = False,
                   no_messages: bool = False) -> int:
    """--pattern-counts: for every file one line "[file:]count:pattern" per pattern that matched, in pattern order, `count`
    being the file's matching lines for that pattern (what grep -c -e pattern prints).  The counts are taken on the GPU
    (hypergrep_amd.count_files; count for one file): the patterns get the ids 0..n-1 and no line leaves the device.
    shown: the patterns as the user wrote them (default: as compiled).  Returns grep's exit code."""
    shown = shown if shown is not None else patterns
    flags = hypergrep_amd.utils.HS_FLAG_DOTALL | hypergrep_amd.utils.HS_FLAG_MULTILINE | hypergrep_amd.utils.HS_FLAG_SINGLEMATCH
    flags |= hypergrep_amd.utils.HS_FLAG_CASELESS if ignore_case else 0
    kwargs = {"flags": [flags] * len(patterns), "ids": list(range(len(patterns)))}
    outcomes = [hypergrep_amd.count(files[0], patterns, **kwargs)] if len(files) == 1 else hypergrep_amd.count_files(files, patterns, **kwargs)
    matched = errored = False
    for name, (counts, return_code) in zip(files, outcomes):
        if return_code:
            errored = True
            if not no_messages:
                problem = "No such file or directory" if not os.path.exists(name) else ("is a directory" if os.path.isdir(name) else f"scan failed ({return_code})")
                print(f"hyperscanner: {name}: {problem}")
            continue
        for index, pattern in enumerate(shown):
            lines = counts.get(index, (0, 0))[0]
            if lines:
                matched = True
                print(f"{name}:{lines}:{pattern}" if with_file_name else f"{lines}:{pattern}")
    return 2 if errored else (0 if matched else 1)


def value_counts(files: list, patterns: list[str], ignore_case: bool = False, with_file_name: bool = False, no_messages: bool = False, top: int = 0) -> int:
    """--value-counts: for every file, one after another, one line "[file:]count:value" per distinct matched part (what grep -o
    prints), by count descending, then value ascending: grep -o | sort | uniq -c | sort -rn.  The parts are grouped on the GPU;
    only the distinct values leave the device.  Several files, or any with --top, go through one native call
    (hypergrep_amd.count_values_files: small files share a scan, and with top only every file's `top` most frequent values
    leave the device; measured 5.7 to 30 times faster than a call per file at 1024 and 16384 files of 1, 16 and 256 KiB,
    profiles/rank_bench.txt); HYPERGREP_BATCH_FILES=0 keeps a call per file.  Returns grep's exit code."""
    flags = hypergrep_amd.utils.HS_FLAG_DOTALL | hypergrep_amd.utils.HS_FLAG_MULTILINE | hypergrep_amd.utils.HS_FLAG_SINGLEMATCH
    flags |= hypergrep_amd.utils.HS_FLAG_CASELESS if ignore_case else 0
    matched = errored = False
    given = {"flags": [flags] * len(patterns), "ids": list(range(len(patterns)))}
    batched = None
    if (len(files) > 1 or top) and os.environ.get("HYPERGREP_BATCH_FILES", "1") != "0":
        batched = hypergrep_amd.count_values_files(files, patterns, top=top, **given)
    for index, name in enumerate(files):
        if batched is not None:
            rows, return_code = batched[index]
        elif top:  # (the cut is the native call's: a tie at it goes to the value that occurs first)
            rows, return_code = hypergrep_amd.count_values_files([name], patterns, top=top, **given)[0]
        else:
            rows, return_code = hypergrep_amd.count_values(name, patterns, **given)
        if return_code:
            errored = True
            if not no_messages:
                problem = "No such file or directory" if not os.path.exists(name) else ("is a directory" if os.path.isdir(name) else f"scan failed ({return_code})")
                print(f"hyperscanner: {name}: {problem}")
            continue
        head = f"{name}:".encode() if with_file_name else b""
        sys.stdout.flush()
        for value, count in rows:
            matched = True
            sys.stdout.buffer.write(head + str(count).encode() + b":" + value + b"\n")  # (the value as it was counted, byte for byte)
        sys.stdout.buffer.flush()
    return 2 if errored else (0 if matched else 1)


def print_results(results: list, file_name: str, with_file_name: bool = False, with_line_number: bool = False) -> None:
    """Print (line number, line) results with the requested prefixes; lines keep their own newline."""
    head = f"{file_name}:" if with_file_name else ""
    if with_line_number:
        chunks = [f"{head}{number}:{line}" for number, line in results]
    else:
        chunks = [f"{head}{line}" for _number, line in results]
    if chunks:
        print("".join(chunks), end="")


def format_context_results(results: list, file_name: str, with_file_name: bool = False, with_line_number: bool = False, only_matching: bool = False,
                           state: dict | None = None) -> str:
    """GNU grep's output for (line number, line, is_match) rows in line order (grep() with context): a context line has "-" where
    a matching line has ":" after the file name and the line number, and a "--" line stands between groups whose line numbers
    are not adjacent, also from one file to the next.  only_matching: the context lines are not printed (they still make the
    groups).  state: {"printed": bool}, carried from file to file."""
    state = state if state is not None else {"printed": False}
    out = []
    previous = None
    for number, line, is_match in results:
        if previous is not None and number > previous + 1 or previous is None and state["printed"]:
            out.append("--\n")
        previous = number
        state["printed"] = True
        if only_matching and not is_match:
            continue
        mark = ":" if is_match else "-"
        out.append((f"{file_name}{mark}" if with_file_name else "") + (f"{number}{mark}" if with_line_number else "") + line)
    return "".join(out)


def read_stdin() -> Generator[str, None, None]:
    """File names from standard input, one per line, up to the first empty line or end of input."""
    for raw in iter(sys.stdin.readline, ""):
        name = raw.strip()
        if not name:
            return
        yield name


def to_basic_regular_expressions(patterns: list[str]) -> list[str]:
    """Read the patterns as POSIX basic regular expressions and return their ERE / PCRE spelling.

    In a BRE the characters + ? ( ) { } | are literals and become operators when escaped, the opposite of ERE / PCRE:
    every one of them swaps its escaping.  Raises ValueError when the result no longer compiles.
    """
    converted = []
    for pattern in patterns:
        out: list[str] = []
        for position, char in enumerate(pattern):
            if char in _BRE_LITERALS:
                if position and pattern[position - 1] == "\\":
                    out[-1] = char  # escaped in the BRE: an operator, spelled bare
                else:
                    out.append("\\" + char)  # bare in the BRE: a literal, spelled escaped
            else:
                out.append(char)
        text = "".join(out)
        try:
            re.compile(text)
        except Exception as error:
            raise ValueError(f"hyperscanner: invalid regex: {error}") from error
        converted.append(text)
    return converted


def to_gnu_regular_expressions(patterns: list[str]) -> list[str]:
    """GNU's word-edge operators \\< and \\> become \\b (not for PCRE input, which is taken as written).

    An operator whose backslash directly follows another backslash is left alone.
    """
    converted = []
    for pattern in patterns:
        out: list[str] = []
        position = 0
        while position < len(pattern):
            char = pattern[position]
            if char == "\\" and pattern[position + 1 : position + 2] in ("<", ">") and (position == 0 or pattern[position - 1] != "\\"):
                out.append("\\b")
                position += 2
            else:
                out.append(char)
                position += 1
        converted.append("".join(out))
    return converted


def _top_count(text: str) -> int:
    """--top takes a positive number; anything else ends the command with exit code 2."""
    try:
        value = int(text)
    except ValueError:
        value = 0
    if value < 1:
        raise argparse.ArgumentTypeError(f"{text}: invalid number of values")
    return value


def _context_length(text: str) -> int:
    """-A / -B / -C take a non-negative number; anything else ends the command with exit code 2, as in GNU grep."""
    try:
        value = int(text)
    except ValueError:
        value = -1
    if value < 0:
        raise argparse.ArgumentTypeError(f"{text}: invalid context length argument")
    return value


def parse_args(args: list = None) -> argparse.Namespace:
    """Command line of the `hyperscanner` command: grep's option letters where grep has them."""
    parser = argparse.ArgumentParser(
        formatter_class=argparse.RawTextHelpFormatter,
        add_help=False,  # -h is grep's --no-filename
        description=textwrap.dedent(
            """\
            grep over many files with one multi-pattern scan per file on the GPU.
              hyperscanner <regex> <file(s)>
              find <args> | hyperscanner <regex>
            Patterns are limited to what the engine compiles (no look-around, no back-references); plain, gzip and
            zstd files are read; only the options listed here exist (nothing is passed on to a grep process)."""
        ),
    )
    parser.add_argument("pattern", nargs="?", help="Regex pattern to use.")
    parser.add_argument("files", nargs="*", help="Files to scan.")
    parser.add_argument_group("Generic Program Information").add_argument(
        "--help", action="help", default=argparse.SUPPRESS, help="show this help message and exit"
    )

    syntax = parser.add_argument_group("Pattern Syntax").add_mutually_exclusive_group()
    syntax.set_defaults(regexp="bre")
    syntax.add_argument("-E", "--extended-regexp", dest="regexp", action="store_const", const="ere", help="PATTERNS are extended regular expressions.")
    syntax.add_argument("-G", "--basic-regexp", dest="regexp", action="store_const", const="bre", help="PATTERNS are basic regular expressions (default).")
    syntax.add_argument("-P", "--perl-regexp", dest="regexp", action="store_const", const="pcre", help="PATTERNS are Perl-compatible regular expressions.")

    matching = parser.add_argument_group("Matching Control")
    matching.add_argument("-e", "--regexp", action="append", dest="patterns", metavar="pattern", help="A pattern; may be repeated and combined with -f.")
    matching.add_argument("-f", "--file", action="append", dest="pattern_files", metavar="file", help="Read patterns from FILE, one per line; may be repeated.")
    matching.add_argument("-i", "--ignore-case", action="store_true", help="Case-insensitive matching.")
    # (no attribute unless given: tests/test_multiscanner.py compares the whole namespace of the reference's command lines)
    matching.add_argument("-v", "--invert-match", action="store_true", default=argparse.SUPPRESS, help="Select the lines that match NO pattern.")

    context = parser.add_argument_group("Context Line Control")
    context.add_argument("-A", "--after-context", type=_context_length, metavar="NUM", default=argparse.SUPPRESS, help="Print NUM lines of trailing context after matching lines.")
    context.add_argument("-B", "--before-context", type=_context_length, metavar="NUM", default=argparse.SUPPRESS, help="Print NUM lines of leading context before matching lines.")
    context.add_argument("-C", "--context", type=_context_length, metavar="NUM", default=argparse.SUPPRESS, help="Print NUM lines of output context.")

    output = parser.add_argument_group("General Output Control")
    output.add_argument("-c", "--count", action="store_true", help="Print the number of matching lines per file.")
    output.add_argument("-L", "--files-without-match", action="store_true", help="Print only the names of files without a match.")
    output.add_argument("-l", "--files-with-matches", action="store_true", help="Print only the names of files with a match.")
    output.add_argument("-m", "--max-count", type=int, default=0, help="Stop reading a file after NUM matching lines.")
    output.add_argument("-o", "--only-matching", action="store_true", help="Print only the matched parts, one per line.")
    output.add_argument("-q", "--quiet", "--silent", action="store_true", help="Print nothing; exit 0 at the first match.")
    output.add_argument("-s", "--no-messages", action="store_true", help="No messages about missing or unreadable files.")

    prefix = parser.add_argument_group("Output Line Prefix Control")
    names = prefix.add_mutually_exclusive_group()
    names.add_argument("-H", "--with-filename", action="store_true", default=None, help="Prefix lines with the file name (default with several files).")
    names.add_argument("-h", "--no-filename", action="store_true", default=None, help="No file name prefix (default with one file).")
    prefix.add_argument("-n", "--line-number", action="store_true", help="Prefix lines with their 1-based line number.")

    selection = parser.add_argument_group("File and Directory Selection")
    selection.add_argument("-a", "--text", action="store_true", help="Accepted for grep compatibility; files are always read as bytes.")
    # (no attribute unless given, like -v)
    selection.add_argument("-r", "-R", "--recursive", dest="recursive", action="store_true", default=argparse.SUPPRESS,
                           help="Read all regular files under each directory; -H becomes the default.  -R is a synonym: symbolic links to\n"
                                "directories are not followed, symbolic links to files are read.")

    own = parser.add_argument_group("Unique arguments to hyperscanner")
    own.add_argument("-t", "--total", action="store_true", help="Print one count of matching lines over all files.")
    own.add_argument("--no-gnu", dest="gnu_regexp", action="store_false", help="Keep GNU operators such as \\< as written (BRE / ERE input only).")
    own.add_argument("--no-order", dest="ordered", action="store_false", help="Print each file's results as soon as it finishes.")
    own.add_argument("--no-sort", dest="sort_files", action="store_false", help="Keep the given file order instead of sorting the names.")
    own.add_argument("--mp", action="store_false", dest="use_multithreading", help="Worker processes instead of threads.")
    # (no attribute unless given, like -v)
    own.add_argument("--gnu-parts", dest="gnu_parts", action="store_true", default=argparse.SUPPRESS,
                     help="With -o: print the matched parts of ALL patterns, leftmost-longest, computed on the GPU (GNU grep's -o\n"
                          "output for several patterns and alternations).  Without -o it has no effect.")
    # (no attribute unless given, like -v)
    own.add_argument("--pattern-counts", dest="pattern_counts", action="store_true", default=argparse.SUPPRESS,
                     help="For every file print one line [file:]count:pattern per pattern that matched, count being the matching\n"
                          "lines, counted on the GPU.  Not combined with -v, -o, -c, -l, -L, -q, -A / -B / -C or -m.")
    # (no attribute unless given, like -v)
    own.add_argument("--value-counts", dest="value_counts", action="store_true", default=argparse.SUPPRESS,
                     help="For every file print one line [file:]count:value per distinct matched part (grep -o | sort | uniq -c |\n"
                          "sort -rn), grouped on the GPU; a value is printed byte for byte as it was counted.  Not combined with --pattern-counts, -v, -o, -c, -l, -L, -q, -A / -B / -C or -m.")
    own.add_argument("--top", dest="top", type=_top_count, metavar="NUM", default=argparse.SUPPRESS,
                     help="With --value-counts: print only each file's NUM most frequent values (cut on the GPU; a tie at the cut goes to the\n"
                          "value that occurs first in the file).")
    parser.set_defaults(parser=parser)
    parsed = parser.parse_intermixed_args(args=args)
    if hasattr(parsed, "top") and not getattr(parsed, "value_counts", False):
        parser.error("--top is only valid with --value-counts")  # (exit code 2)
    if getattr(parsed, "value_counts", False):
        others = (getattr(parsed, "pattern_counts", False) or getattr(parsed, "invert_match", False) or parsed.only_matching or parsed.count or parsed.files_with_matches or
                  parsed.files_without_match or parsed.quiet or parsed.max_count or any(hasattr(parsed, name) for name in ("after_context", "before_context", "context")))
        if others:
            parser.error("--value-counts is not combined with --pattern-counts, -v, -o, -c, -l, -L, -q, -A, -B, -C or -m")  # (exit code 2)
    if getattr(parsed, "pattern_counts", False):
        others = (getattr(parsed, "invert_match", False) or parsed.only_matching or parsed.count or parsed.files_with_matches or parsed.files_without_match or parsed.quiet or
                  parsed.max_count or any(hasattr(parsed, name) for name in ("after_context", "before_context", "context")))
        if others:
            parser.error("--pattern-counts is not combined with -v, -o, -c, -l, -L, -q, -A, -B, -C or -m")  # (exit code 2)
    return parsed


def main() -> None:
    """The `hyperscanner` command."""
    args = parse_args()
    try:
        patterns = get_argparse_patterns(args)
        if not patterns:
            args.parser.print_usage()
            raise SystemExit(2)
        patterns_as_written = list(patterns)
        if args.regexp == "bre":
            patterns = to_basic_regular_expressions(patterns)
    except ValueError as error:
        print(error)
        raise SystemExit(2) from error
    if args.gnu_regexp and args.regexp != "pcre":
        patterns = to_gnu_regular_expressions(patterns)
    files = get_argparse_files(args) or list(read_stdin())
    recursive = getattr(args, "recursive", False)
    if recursive:  # (without -r a directory stays an error of its own, reported in its place)
        files = expand_directories(files, args.sort_files)
    if args.sort_files:
        files = sorted(files)
    if not files:
        args.parser.print_usage()
        raise SystemExit(2)
    if args.no_filename is not None:
        with_file_name = False
    elif args.with_filename is not None:
        with_file_name = True
    else:
        with_file_name = recursive or len(files) > 1
    if getattr(args, "value_counts", False):
        raise SystemExit(value_counts(files, patterns, args.ignore_case, with_file_name, args.no_messages, getattr(args, "top", 0)))
    if getattr(args, "pattern_counts", False):
        raise SystemExit(pattern_counts(files, patterns, patterns_as_written, args.ignore_case, with_file_name, args.no_messages))
    raise SystemExit(
        parallel_grep(
            files=files,
            patterns=patterns,
            ignore_case=args.ignore_case,
            ordered_results=args.ordered,
            count_results=args.count,
            total_results=args.total,
            with_file_name=with_file_name,
            with_line_number=args.line_number,
            use_multithreading=args.use_multithreading,
            only_matching=args.only_matching,
            no_messages=args.no_messages,
            max_match_count=args.max_count,
            quiet=args.quiet,
            files_without_match=args.files_without_match,
            files_with_matches=args.files_with_matches,
            invert_match=getattr(args, "invert_match", False),
            gnu_parts=getattr(args, "gnu_parts", False),
            before_context=getattr(args, "before_context", getattr(args, "context", 0)),
            after_context=getattr(args, "after_context", getattr(args, "context", 0)),
        )
    )


if __name__ == "__main__":
    try:
        main()
    except KeyboardInterrupt as user_interrupt:
        raise SystemExit(130) from user_interrupt
