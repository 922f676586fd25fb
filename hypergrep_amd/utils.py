"""hypergrep-compatible Python API on top of the MI355X scan engine.

The public surface of the reference's hypergrep/utils.py, name for name and default for default:

    Result / CALLBACK_TYPE          utils.py:25-51      batched-match C struct and callback type
    check_compatibility()           utils.py:97-122     compile-only probe, 0 or 4
    configure_libraries()           utils.py:125-144    library path override, ValueError once loaded
    grep()                          utils.py:147-231    (1-based line number, decoded line) tuples + return code
    prepare_patterns()              utils.py:234-289    str -> C arrays, default flags 14, default ids all 0
    scan()                          utils.py:292-358    FFI call on a daemon thread, 130 on Ctrl-C

The native side is ONE shared object, hypergrep_amd/lib/libhyperscanner.so, exporting the reference shim's
`hyperscan` / `check_patterns` ABI (include/hypergrep_amd.h, Face B).  It replaces both libraries of the
reference bundle (libhs + libhyperscanner); gzip comes from the system zlib and zstd from the system
libzstd, so `configure_libraries(libzstd=...)` only preloads an alternative libzstd.

There is no CPU scan path: on a machine without a usable GPU `scan()` returns 3 (HYPERSCANNER_SCRATCH)
and the native library prints the reason.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading
from typing import Callable, Sequence

# Hyperscan's compile flags, the values the reference passes through (utils.py:10-13).
HS_FLAG_CASELESS, HS_FLAG_DOTALL, HS_FLAG_MULTILINE, HS_FLAG_SINGLEMATCH = 1, 2, 4, 8
# Logical combinations: a formula over other expressions' report ids, and reports that only feed combinations
# (include/hypergrep_amd.h has the contract).
HS_FLAG_COMBINATION, HS_FLAG_QUIET = 512, 1024
HG_ID_INVERT = 0xFFFFFFFF  # Result.id of an inverted scan (scan(invert=True)): no expression
HG_ID_CONTEXT = 0xFFFFFFFE  # Result.id of a context line (scan(before_context=, after_context=)); a context record of the device API
HG_ID_CONTEXT_TAIL = 0xFFFFFFFD  # device API: a tail record (the next buffer's before-context, maybe)
_GREP_FLAGS = HS_FLAG_DOTALL | HS_FLAG_MULTILINE | HS_FLAG_SINGLEMATCH  # what grep() and the default of scan() use

RC_INVALID_FILE = 101  # grep(): the path is missing or a directory (utils.py:16)
_RC_INTERRUPTED = 130
_JOIN_TIMEOUT_S = 3600


class Result(ctypes.Structure):
    """One match as the shim lays it out (hyperscanner.c:42-46): report id, 0-based line index, the line's bytes."""

    _fields_ = [("id", ctypes.c_uint), ("line_number", ctypes.c_ulonglong), ("line", ctypes.c_char_p)]


class ExprExt(ctypes.Structure):
    """Extended parameters of one expression: Hyperscan's hs_expr_ext_t (include/hypergrep_amd.h has the contract).  Set the
    fields you use and their HS_EXT_FLAG_* bits in `flags`, e.g. ExprExt(flags=HS_EXT_FLAG_EDIT_DISTANCE, edit_distance=1) or
    ExprExt(flags=HS_EXT_FLAG_MIN_LENGTH, min_length=12): only reports of matches of at least 12 bytes."""

    _fields_ = [("flags", ctypes.c_ulonglong), ("min_offset", ctypes.c_ulonglong), ("max_offset", ctypes.c_ulonglong),
                ("min_length", ctypes.c_ulonglong), ("edit_distance", ctypes.c_uint), ("hamming_distance", ctypes.c_uint)]


HS_EXT_FLAG_MIN_OFFSET, HS_EXT_FLAG_MAX_OFFSET, HS_EXT_FLAG_MIN_LENGTH = 1, 2, 4
HS_EXT_FLAG_EDIT_DISTANCE, HS_EXT_FLAG_HAMMING_DISTANCE = 8, 16


def ext_array(ext, count: int):
    """One ExprExt or None per pattern -> a C array of hs_expr_ext_t pointers (NULL for None).  ValueError if the count is
    not one per pattern."""
    entries = list(ext)
    if len(entries) != count:
        raise ValueError(f"Found {len(entries)} ext entries, expecting {count}: one ExprExt or None per pattern.")
    for entry in entries:
        if entry is not None and not isinstance(entry, ExprExt):
            raise TypeError(f"ext entries must be ExprExt or None, not {type(entry).__name__}")
    return (ctypes.POINTER(ExprExt) * count)(*[ctypes.pointer(e) if e is not None else None for e in entries])


def _bind_ext(engine: ctypes.CDLL) -> None:
    engine.hg_check_patterns_ext.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                          ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint]


# void on_event(Result *batch, int count)  (hyperscanner.c:54)
CALLBACK_TYPE = ctypes.CFUNCTYPE(None, ctypes.POINTER(Result), ctypes.c_int, use_errno=False, use_last_error=False)


class _Libraries:
    """Paths chosen through configure_libraries() and the handles once loaded (loading is lazy: a forked worker must
    initialise the GPU runtime itself)."""

    engine_path = ""
    zstd_path = ""
    engine = None
    zstd = None

    @staticmethod
    def default_engine() -> str:
        return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libhyperscanner.so")


def _get_hyperscanner_lib() -> ctypes.CDLL:
    if _Libraries.zstd is None and _Libraries.zstd_path:
        _Libraries.zstd = ctypes.CDLL(_Libraries.zstd_path, mode=ctypes.RTLD_GLOBAL)
    if _Libraries.engine is None:
        path = _Libraries.engine_path or _Libraries.default_engine()
        if not os.path.exists(path):
            raise OSError(
                f"{path}: native library not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(needs hipcc); hypergrep_amd has no pure-Python or CPU fallback."
            )
        _Libraries.engine = ctypes.cdll.LoadLibrary(path)
    return _Libraries.engine


def configure_libraries(libhs: str | None = None, libzstd: str | None = None) -> None:
    """Choose other library files; only possible before the first scan / check loads them.

    libhs: the engine library (default: this package's libhyperscanner.so).  libzstd: a libzstd to preload for .zst input.
    """
    in_use = _Libraries.engine is not None  # the engine opens its libzstd itself, so both are fixed once it is loaded
    for name, wanted, slot in (("libhs", libhs, "engine_path"), ("libzstd", libzstd, "zstd_path")):
        if not wanted:
            continue
        if in_use:
            raise ValueError(f"{name} already loaded, configuration overrides must be called before library usage")
        setattr(_Libraries, slot, wanted)


def _one_per_pattern(kind: str, values: Sequence[int], default: int, count: int) -> list[int]:
    chosen = list(values) if values else [default] * count
    if len(chosen) != count:
        raise ValueError(
            f"Found {len(chosen)} {kind}, expecting {count}. Hyperscan {kind} must be provided for each regex to compile the database."
        )
    return chosen


def prepare_patterns(patterns: list[str], flags: list[int] = (), ids: list[int] = ()) -> tuple[ctypes.Array, ctypes.Array, ctypes.Array]:
    """Patterns, per-pattern flags (default DOTALL | MULTILINE | SINGLEMATCH) and report ids (default all 0) as C arrays.

    ValueError for an empty pattern or when flags / ids are given but not one per pattern.
    """
    count = len(patterns)
    flag_values = _one_per_pattern("flags", flags, _GREP_FLAGS, count)
    id_values = _one_per_pattern("ids", ids, 0, count)
    for pattern in patterns:
        if not pattern:
            raise ValueError(f'Invalid pattern "{pattern}" found. Please provide a valid regex for Intel Hyperscan.')
    return (
        (ctypes.c_char_p * count)(*[pattern.encode() for pattern in patterns]),
        (ctypes.c_uint * count)(*flag_values),
        (ctypes.c_uint * count)(*id_values),
    )


def check_compatibility(patterns: list, flags: list[int] = (), ids: list[int] = (), ext=None) -> int:
    """Compile the patterns without scanning anything: 0 if the engine accepts them all, else 4.  `ids` (default all 0)
    matter for sets with HS_FLAG_COMBINATION, whose formulas name report ids.  `ext`: one ExprExt or None per pattern."""
    c_patterns, c_flags, c_ids = prepare_patterns(patterns, flags=flags, ids=ids)
    engine = _get_hyperscanner_lib()
    if ext is None:
        return engine.check_patterns(c_patterns, c_flags, c_ids, len(c_patterns))
    c_ext = ext_array(ext, len(c_patterns))
    _bind_ext(engine)
    return engine.hg_check_patterns_ext(c_patterns, c_flags, c_ids, c_ext, len(c_patterns))


def scan(  # pylint: disable=too-many-arguments
    path: str,
    patterns: list[str],
    callback: Callable,
    flags: list[int] = (),
    ids: list[int] = (),
    buffer_size: int = 262140,
    buffer_count: int = 16,
    max_match_count: int = 0,
    ext=None,
    invert: bool = False,
    before_context: int = 0,
    after_context: int = 0,
    parts: bool = False,
) -> int:
    """Scan a plain / gzip / zstd text file; `callback(matches, count)` receives the hits in batches of `buffer_count`.
    `ext`: one ExprExt (extended parameters: approximate matching, offset bounds, min_length) or None per pattern.
    `invert` (grep -v): the callback receives the lines NO pattern matches instead, one Result with id HG_ID_INVERT each, in
    line order; `max_match_count` then bounds those lines.
    `before_context` / `after_context` (grep -B / -A, in line pieces): the callback also receives the lines around the delivered
    ones, one Result with id HG_ID_CONTEXT each, merged in line order (hg_hyperscan_context); `max_match_count` does not count
    them, and pattern ids of 0xFFFFFFFD and above are refused (return code 4).
    `parts` (grep -o over all patterns, hg_hyperscan_parts): the callback receives, for every line it would receive, the
    line's matched parts instead: one Result per part with the id of the part's pattern and the part's bytes as `line`, in
    (line, offset) order; `max_match_count` still goes by the reports.  Not combined with `invert` or context (ValueError);
    pattern sets with `ext`, combinations, QUIET or automata above 1024 nodes are refused (return code 4).

    The native call runs on a daemon thread so that Ctrl-C reaches Python (return code 130); otherwise the shim's
    return code (0 = fine, 1-7 as in hyperscanner.c:25-33) comes back.
    """
    if parts and (invert or before_context or after_context):
        raise ValueError("parts: not combined with invert or context lines")
    c_patterns, c_flags, c_ids = prepare_patterns(patterns, flags=flags, ids=ids)
    c_ext = None if ext is None else ext_array(ext, len(c_patterns))
    c_callback = CALLBACK_TYPE(callback)  # referenced until the call is over
    engine = _get_hyperscanner_lib()
    outcome = [0]

    def native_call() -> None:
        if parts:
            engine.hg_hyperscan_parts.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                                  ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, CALLBACK_TYPE, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_ulonglong]
            outcome[0] = engine.hg_hyperscan_parts(path.encode(), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), c_callback, buffer_size,
                                                   buffer_count, max_match_count)
        elif before_context or after_context:
            engine.hg_hyperscan_context.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                                    ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, CALLBACK_TYPE, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_uint, ctypes.c_int]
            outcome[0] = engine.hg_hyperscan_context(path.encode(), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), c_callback, buffer_size,
                                                     buffer_count, max_match_count, before_context, after_context, 1 if invert else 0)
        elif invert:
            engine.hg_hyperscan_invert.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                                   ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, CALLBACK_TYPE, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_ulonglong]
            outcome[0] = engine.hg_hyperscan_invert(path.encode(), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), c_callback, buffer_size,
                                                    buffer_count, max_match_count)
        elif c_ext is None:
            outcome[0] = engine.hyperscan(path.encode(), c_patterns, c_flags, c_ids, len(c_patterns), c_callback, buffer_size, buffer_count,
                                          ctypes.c_ulonglong(max_match_count))
        else:
            outcome[0] = engine.hg_hyperscan_ext(path.encode(), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), c_callback, buffer_size,
                                              buffer_count, ctypes.c_ulonglong(max_match_count))

    worker = threading.Thread(target=native_call, daemon=True)
    worker.start()
    try:
        worker.join(timeout=_JOIN_TIMEOUT_S)
    except KeyboardInterrupt:
        return _RC_INTERRUPTED
    return outcome[0]


# void on_event(unsigned file_index, Result *batch, int count, void *context)  (hg_files_event)
FILES_CALLBACK_TYPE = ctypes.CFUNCTYPE(None, ctypes.c_uint, ctypes.POINTER(Result), ctypes.c_int, ctypes.c_void_p, use_errno=False, use_last_error=False)


class FileSummary(ctypes.Structure):
    """hg_file_summary_t: a file's return code (scan()'s), its line pieces and the distinct lines among its results."""

    _fields_ = [("rc", ctypes.c_int), ("n_lines", ctypes.c_uint64), ("n_selected", ctypes.c_uint64)]


def scan_files(  # pylint: disable=too-many-arguments
    files: Sequence[str],
    patterns: list[str],
    on_match: Callable | None,
    flags: list[int] = (),
    ids: list[int] = (),
    buffer_size: int = 262140,
    buffer_count: int = 16,
    max_match_count: int = 0,
    ext=None,
    invert: bool = False,
    before_context: int = 0,
    after_context: int = 0,
    parts: bool = False,
) -> list[tuple[int, int, int]]:
    """scan() for many files in ONE native call (hg_hyperscan_files): small files are packed into one buffer and share one GPU
    scan.  `on_match(file_index, matches, count)` receives each file's results in batches of `buffer_count`, in file order, no
    batch mixing files; every file's results are those scan() gives for it alone (`max_match_count` bounds each file).  Without
    a callback (None) only the per-file summaries are produced.  Returns one (return code, line pieces, distinct result lines)
    per file; a missing or unreadable file has return code 6 and does not disturb the others.
    `before_context` / `after_context` (hg_hyperscan_files_context): each file's batches also hold the lines around its results,
    one Result with id HG_ID_CONTEXT each, merged in line order, exactly as scan() with the same arguments gives them for the
    file alone; the context stays inside the file, the summaries do not count it, and pattern ids of 0xFFFFFFFD and above are
    refused (return code 4).
    `parts` (grep -r -o, hg_hyperscan_files_parts): each file's batches hold its matched parts instead, one Result per part with
    the id of the part's pattern and the part's bytes as `line`, exactly as scan(parts=True) gives them for the file alone; the
    summaries are those without parts.  Not combined with `invert` or context (ValueError); a pattern set scan(parts=True)
    refuses fails the whole call (return code 4 for every file)."""
    if parts and (invert or before_context or after_context):
        raise ValueError("parts: not combined with invert or context lines")
    names = [os.fspath(name) for name in files]
    c_patterns, c_flags, c_ids = prepare_patterns(patterns, flags=flags, ids=ids)
    c_ext = None if ext is None else ext_array(ext, len(c_patterns))
    c_names = (ctypes.c_char_p * max(len(names), 1))(*[name.encode() for name in names])
    summaries = (FileSummary * max(len(names), 1))()
    if on_match is None:
        c_callback = ctypes.cast(None, FILES_CALLBACK_TYPE)
    else:
        c_callback = FILES_CALLBACK_TYPE(lambda index, matches, count, _context: on_match(index, matches, count))  # referenced until the call is over
    engine = _get_hyperscanner_lib()
    engine.hg_hyperscan_files.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint),
                                          ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, FILES_CALLBACK_TYPE,
                                          ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, ctypes.POINTER(FileSummary)]
    outcome = [0]

    def native_call() -> None:
        if parts:
            argtypes = engine.hg_hyperscan_files.argtypes
            engine.hg_hyperscan_files_parts.argtypes = argtypes[:12] + argtypes[13:]  # (no `invert`)
            outcome[0] = engine.hg_hyperscan_files_parts(c_names, len(names), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), c_callback, None, buffer_size,
                                                         buffer_count, max_match_count, summaries)
            return
        if before_context or after_context:
            engine.hg_hyperscan_files_context.argtypes = engine.hg_hyperscan_files.argtypes + [ctypes.c_uint, ctypes.c_uint]
            outcome[0] = engine.hg_hyperscan_files_context(c_names, len(names), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), c_callback, None, buffer_size,
                                                           buffer_count, max_match_count, 1 if invert else 0, summaries, before_context, after_context)
            return
        outcome[0] = engine.hg_hyperscan_files(c_names, len(names), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), c_callback, None, buffer_size,
                                               buffer_count, max_match_count, 1 if invert else 0, summaries)

    worker = threading.Thread(target=native_call, daemon=True)
    worker.start()
    try:
        worker.join(timeout=_JOIN_TIMEOUT_S)
    except KeyboardInterrupt:
        return [(_RC_INTERRUPTED, 0, 0)] * len(names)
    if outcome[0]:  # a failure of the whole call (the expressions do not compile): every file reports it, as scan() would
        return [(outcome[0], 0, 0)] * len(names)
    return [(summaries[i].rc, summaries[i].n_lines, summaries[i].n_selected) for i in range(len(names))]


class IdCount(ctypes.Structure):
    """hg_id_count_t: a report id with the matching lines and the reports of that id."""

    _fields_ = [("id", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("n_lines", ctypes.c_uint64), ("n_reports", ctypes.c_uint64)]


def _run_native(native_call: Callable) -> bool:
    """The native call on a daemon thread, so that Ctrl-C reaches Python; False when it was interrupted."""
    worker = threading.Thread(target=native_call, daemon=True)
    worker.start()
    try:
        worker.join(timeout=_JOIN_TIMEOUT_S)
    except KeyboardInterrupt:
        return False
    return True


def count(file: str, patterns: list[str], flags: list[int] = (), ids: list[int] = (), ext=None, buffer_size: int = 262140) -> tuple[dict, int]:
    """Which patterns fired in a plain / gzip / zstd text file, and how often (hg_hyperscan_counts): ({id: (matching lines,
    reports)}, return code) with one entry per distinct report id, zeroes included.  The counts are taken on the GPU behind
    every chunk's scan; no hit record and no line leaves it.  There is no max_match_count: counts describe the whole file."""
    c_patterns, c_flags, c_ids = prepare_patterns(patterns, flags=flags, ids=ids)
    c_ext = None if ext is None else ext_array(ext, len(c_patterns))
    max_counts = len(set(c_ids))
    rows = (IdCount * max_counts)()
    n_counts, n_lines = ctypes.c_uint(), ctypes.c_uint64()
    engine = _get_hyperscanner_lib()
    engine.hg_hyperscan_counts.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                           ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_int, ctypes.POINTER(IdCount), ctypes.c_uint,
                                           ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint64)]
    outcome = [0]

    def native_call() -> None:
        outcome[0] = engine.hg_hyperscan_counts(os.fspath(file).encode(), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), buffer_size, rows, max_counts,
                                                ctypes.byref(n_counts), ctypes.byref(n_lines))

    if not _run_native(native_call):
        return {}, _RC_INTERRUPTED
    return {rows[b].id: (rows[b].n_lines, rows[b].n_reports) for b in range(min(n_counts.value, max_counts))}, outcome[0]


class ValuesParams(ctypes.Structure):
    """hg_values_params_t (include/hypergrep_amd.h)."""

    _fields_ = [("flags", ctypes.c_uint32), ("hash_bits", ctypes.c_uint32), ("table_log2", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


_VALUES_EVENT = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                 ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64)


def count_values(file: str, patterns: list[str], flags: list[int] = (), ids: list[int] = (), by_pattern: bool = False, buffer_size: int = 262140) -> tuple[list, int]:
    """The distinct matched parts of a plain / gzip / zstd text file and how often each occurs (hg_hyperscan_values; grep -o |
    sort | uniq -c | sort -rn): (rows, return code).  The rows are (value bytes, count), with by_pattern (value bytes, pattern
    index, count) and the pattern index part of the key; sorted by count descending, then value ascending.  The parts are
    grouped on the GPU behind every chunk's scan; only each chunk's distinct values come back, and the chunks are merged here."""
    c_patterns, c_flags, c_ids = prepare_patterns(patterns, flags=flags, ids=ids)
    params = ValuesParams(flags=1 if by_pattern else 0)
    rows: list = []

    def on_values(_context, data, off, counts, pattern, n_values) -> None:
        blob = ctypes.string_at(data, off[n_values]) if n_values else b""
        for j in range(n_values):
            value = blob[off[j]:off[j + 1]]
            rows.append((value, pattern[j], counts[j]) if by_pattern else (value, counts[j]))

    callback = _VALUES_EVENT(on_values)
    engine = _get_hyperscanner_lib()
    engine.hg_hyperscan_values.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                           ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_int, ctypes.POINTER(ValuesParams), _VALUES_EVENT, ctypes.c_void_p]
    outcome = [0]

    def native_call() -> None:
        outcome[0] = engine.hg_hyperscan_values(os.fspath(file).encode(), c_patterns, c_flags, c_ids, None, len(c_patterns), buffer_size, ctypes.byref(params), callback, None)

    if not _run_native(native_call):
        return [], _RC_INTERRUPTED
    rows.sort(key=(lambda r: (-r[2], r[0], r[1])) if by_pattern else (lambda r: (-r[1], r[0])))
    return rows, outcome[0]


def count_values_top(file: str, patterns: list[str], top: int, flags: list[int] = (), ids: list[int] = (), by_pattern: bool = False, buffer_size: int = 262140,
                     totals: list | None = None) -> tuple[list, int]:
    """count_values() cut to the `top` most frequent values, with the whole file's values accumulated on the GPU
    (hg_hyperscan_values_top; grep -o | sort | uniq -c | sort -rn | head): (rows, return code).  A value store on the device
    takes every chunk's parts behind its scan and is ranked once at the end, so only the kept rows come back, however many
    chunks the file has.  The rows are shaped and sorted as count_values() gives them; the cut is count_values_files()': the
    most frequent values, a tie at the cut going to the value that occurs first in the file, so that
    count_values_top(f, p, N) == count_values_files([f], p, top=N)[0].  top=0 keeps every value.  totals: a list that
    receives (distinct values, parts), both before the cut."""
    if top < 0:
        raise ValueError("top must not be negative")
    c_patterns, c_flags, c_ids = prepare_patterns(patterns, flags=flags, ids=ids)
    params = ValuesParams(flags=1 if by_pattern else 0)
    rows: list = []

    def on_values(_context, data, off, counts, pattern, n_values) -> None:
        blob = ctypes.string_at(data, off[n_values]) if n_values else b""
        for j in range(n_values):
            value = blob[off[j]:off[j + 1]]
            rows.append((value, pattern[j], counts[j]) if by_pattern else (value, counts[j]))

    callback = _VALUES_EVENT(on_values)
    engine = _get_hyperscanner_lib()
    engine.hg_hyperscan_values_top.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                               ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_int, ctypes.POINTER(ValuesParams), ctypes.c_uint64, _VALUES_EVENT,
                                               ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    outcome = [0]
    n_distinct, n_parts = ctypes.c_uint64(), ctypes.c_uint64()

    def native_call() -> None:
        outcome[0] = engine.hg_hyperscan_values_top(os.fspath(file).encode(), c_patterns, c_flags, c_ids, None, len(c_patterns), buffer_size, ctypes.byref(params), top, callback, None,
                                                    ctypes.byref(n_distinct), ctypes.byref(n_parts))

    if not _run_native(native_call):
        return [], _RC_INTERRUPTED
    if totals is not None:
        totals[:] = [(n_distinct.value, n_parts.value)]
    rows.sort(key=(lambda r: (-r[2], r[0], r[1])) if by_pattern else (lambda r: (-r[1], r[0])))
    return rows, outcome[0]


class RankParams(ctypes.Structure):
    """hg_rank_params_t (include/hypergrep_amd.h)."""

    _fields_ = [("flags", ctypes.c_uint32), ("hash_bits", ctypes.c_uint32), ("table_log2", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("top", ctypes.c_uint64)]


_FILE_VALUES_EVENT = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64)


def count_values_files(files: Sequence[str], patterns: list[str], flags: list[int] = (), ids: list[int] = (), by_pattern: bool = False, top: int = 0,
                       buffer_size: int = 262140, totals: list | None = None) -> list[tuple[list, int]]:
    """count_values() for many files in ONE native call (hg_hyperscan_files_values): small files are packed into one buffer and
    share one GPU scan, with the values grouped per file, ordered by count and cut to the `top` most frequent of every file on
    the GPU behind it (top=0: all of them).  One (rows, return code) per file, the rows shaped and sorted as count_values()
    gives them (count descending, then value); the cut keeps the most frequent values, a tie at the cut going to the value
    that occurs first in the file.  With top=0 it equals [count_values(f, ...) for f in files]; a missing or unreadable file
    has return code 6 and no rows.  totals: a list that receives one (distinct values, counted parts) per file, both before
    the cut."""
    if top < 0:
        raise ValueError("top must not be negative")
    names = [os.fspath(name) for name in files]
    c_patterns, c_flags, c_ids = prepare_patterns(patterns, flags=flags, ids=ids)
    params = RankParams(flags=1 if by_pattern else 0, top=top)
    rows: list = [[] for _ in names]
    seen: list = [(0, 0)] * len(names)

    def on_file(_context, index, data, off, counts, pattern, n_values, n_distinct, n_parts) -> None:
        seen[index] = (n_distinct, n_parts)
        if not n_values:
            return
        base = off[0]
        blob = ctypes.string_at(ctypes.addressof(data.contents) + base, off[n_values] - base)
        for j in range(n_values):
            value = blob[off[j] - base:off[j + 1] - base]
            rows[index].append((value, pattern[j], counts[j]) if by_pattern else (value, counts[j]))

    callback = _FILE_VALUES_EVENT(on_file)
    c_names = (ctypes.c_char_p * max(len(names), 1))(*[name.encode() for name in names])
    summaries = (FileSummary * max(len(names), 1))()
    engine = _get_hyperscanner_lib()
    engine.hg_hyperscan_files_values.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint),
                                                 ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_int, ctypes.POINTER(RankParams),
                                                 _FILE_VALUES_EVENT, ctypes.c_void_p, ctypes.POINTER(FileSummary)]
    outcome = [0]

    def native_call() -> None:
        outcome[0] = engine.hg_hyperscan_files_values(c_names, len(names), c_patterns, c_flags, c_ids, None, len(c_patterns), buffer_size, ctypes.byref(params), callback, None,
                                                      summaries)

    if not _run_native(native_call):
        return [([], _RC_INTERRUPTED)] * len(names)
    if totals is not None:
        totals[:] = seen
    if outcome[0]:  # a failure of the whole call (the expressions do not compile): every file reports it, as count_values() would
        return [([], outcome[0])] * len(names)
    order = (lambda r: (-r[2], r[0], r[1])) if by_pattern else (lambda r: (-r[1], r[0]))
    return [(sorted(rows[i], key=order) if not summaries[i].rc else [], summaries[i].rc) for i in range(len(names))]


def count_files(files: Sequence[str], patterns: list[str], flags: list[int] = (), ids: list[int] = (), ext=None, buffer_size: int = 262140) -> list[tuple[dict, int]]:
    """count() for many files in ONE native call (hg_hyperscan_files_counts): small files are packed into one buffer and share
    one GPU scan, with the per-file counts taken behind it.  One ({id: (matching lines, reports)}, return code) per file, what
    count() gives for it alone; a missing or unreadable file has return code 6 and zero counts."""
    names = [os.fspath(name) for name in files]
    c_patterns, c_flags, c_ids = prepare_patterns(patterns, flags=flags, ids=ids)
    c_ext = None if ext is None else ext_array(ext, len(c_patterns))
    c_names = (ctypes.c_char_p * max(len(names), 1))(*[name.encode() for name in names])
    summaries = (FileSummary * max(len(names), 1))()
    max_ids = len(set(c_ids))
    c_report_ids = (ctypes.c_uint32 * max_ids)()
    n_ids = ctypes.c_uint()
    file_lines, file_reports = (ctypes.c_uint64 * max(len(names) * max_ids, 1))(), (ctypes.c_uint64 * max(len(names) * max_ids, 1))()
    engine = _get_hyperscanner_lib()
    engine.hg_hyperscan_files_counts.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint),
                                                 ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.POINTER(ExprExt)), ctypes.c_uint, ctypes.c_int,
                                                 ctypes.POINTER(FileSummary), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint, ctypes.POINTER(ctypes.c_uint),
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    outcome = [0]

    def native_call() -> None:
        outcome[0] = engine.hg_hyperscan_files_counts(c_names, len(names), c_patterns, c_flags, c_ids, c_ext, len(c_patterns), buffer_size, summaries, c_report_ids,
                                                      max_ids, ctypes.byref(n_ids), file_lines, file_reports)

    if not _run_native(native_call):
        return [({}, _RC_INTERRUPTED)] * len(names)
    if outcome[0]:  # a failure of the whole call (the expressions do not compile): every file reports it, as count() would
        return [({}, outcome[0])] * len(names)
    n = min(n_ids.value, max_ids)
    return [({c_report_ids[b]: (file_lines[f * max_ids + b], file_reports[f * max_ids + b]) for b in range(n)}, summaries[f].rc) for f in range(len(names))]


class _GrepSink:
    """on_match for grep(): counts, keeps whole lines, or keeps the matched parts (`re.finditer` of the pattern whose
    id the hit carries — with grep()'s all-zero ids that is the first pattern, as in the reference)."""

    def __init__(self, patterns: list[str], count_only: bool, only_matching: bool, errors: str, invert: bool = False, context: bool = False,
                 limit: int = 0, after: int = 0, parts: bool = False):
        self.parts = parts  # the hits are matched parts already (scan(parts=True)): one trailing newline off, a bare newline dropped
        self.invert = invert  # the hits are the lines without a match: no matched parts to show
        self.context = context  # rows are (line number, line, is_match); context lines (id HG_ID_CONTEXT) are rows, not counted
        # GNU grep's -m NUM with -A NUM (3.5 and later): after the NUM-th selected line the next `after` lines still go out, all of
        # them as context, selected or not.  The file API ends that trailing context before the next selected piece, so grep()
        # asks it for `after` selected lines more (grep()) and draws the line here.
        self.limit = limit if context and after else 0
        self.after = after
        self.selected = 0  # selected lines seen
        self.last_line = -1  # the line number of the limit-th selected line
        self.count = 0
        self.rows: list[tuple[int, str]] = []
        self.count_only = count_only
        self.errors = errors
        self.finders = [re.compile(pattern) for pattern in patterns] if only_matching else None

    def __call__(self, matches, count: int) -> None:
        if self.count_only:
            self.count += sum(1 for i in range(count) if matches[i].id != HG_ID_CONTEXT) if self.context else count
            return
        for hit in (matches[i] for i in range(count)):
            text = hit.line.decode(errors=self.errors)
            if self.parts:
                text = text[:-1] if text.endswith("\n") else text
                if text:
                    self.rows.append((hit.line_number + 1, text + "\n"))
                continue
            if self.context:
                if self.limit and self.selected >= self.limit:  # behind the limit: trailing context only, whatever the line is
                    if hit.line_number <= self.last_line + self.after:
                        self.rows.append((hit.line_number + 1, text, False))
                    continue
                if hit.id != HG_ID_CONTEXT:
                    self.selected += 1
                    self.last_line = hit.line_number
                if hit.id == HG_ID_CONTEXT:
                    self.rows.append((hit.line_number + 1, text, False))
                elif self.finders is None:
                    self.rows.append((hit.line_number + 1, text, True))
                elif not self.invert:
                    self.rows.extend((hit.line_number + 1, f"{part.group()}\n", True) for part in self.finders[hit.id].finditer(text))
            elif self.finders is None:
                self.rows.append((hit.line_number + 1, text))
            elif not self.invert:
                self.rows.extend((hit.line_number + 1, f"{part.group()}\n") for part in self.finders[hit.id].finditer(text))

    def result(self):
        return self.count if self.count_only else self.rows


def grep(  # pylint: disable=too-many-arguments
    file: str,
    patterns: list[str],
    ignore_case: bool = False,
    count_only: bool = False,
    only_matching: bool = False,
    no_messages: bool = False,
    errors: str = "ignore",
    max_match_count: int = 0,
    invert: bool = False,
    before_context: int = 0,
    after_context: int = 0,
    matched_parts: bool = False,
) -> tuple[int | list[tuple[int, str]], int]:
    """grep for Python: (number of matching lines | [(1-based line number, line)], return code).

    `invert` (grep -v): the lines no pattern matches are selected instead: counted, listed, and bounded by `max_match_count`;
    with `only_matching` nothing is listed (a line without a match has no matched part): the result is [] even where lines
    were selected, so a caller that needs to know whether any were asks without `only_matching`, as multiscanner does.
    `before_context` / `after_context` (grep -B / -A): with either, the rows are (1-based line number, line, is_match) in line
    order, the context lines among them with is_match False (also with `only_matching`, where the matching rows are the matched
    parts); counts (`count_only`) and `max_match_count` go by the matching lines only.  Without them rows are as ever.
    With `max_match_count` and `after_context` the rows end as GNU grep's output (3.5 and later) does: the `after_context` lines
    behind the last counted line are all rows with is_match False, matching or not.  (scan() / hg_hyperscan_context end that
    trailing context before the next matching line instead, as the file API's contract states.)
    `matched_parts`: the rows are [(1-based line number, part + "\\n")] with the parts the GPU computes (scan(parts=True)): GNU
    grep's -o over ALL patterns at once, leftmost-longest, honouring `ignore_case`; one trailing "\\n" of a part is stripped
    first and a part that was only "\\n" is dropped.  It takes precedence over `only_matching`, which alone stays the
    reference's route (`re.finditer` of the first pattern).  With `invert` the result is [], with `count_only` lines are
    counted as ever, with context arguments it raises ValueError.

    A missing path raises FileNotFoundError and a directory ValueError — or, with `no_messages`, comes back as
    (nothing found, 101).  Invalid regexes raise `re.error` before anything is scanned.
    """
    if matched_parts:
        if before_context or after_context:
            raise ValueError("matched_parts: context lines are not supported")
        only_matching = False
    with_parts = matched_parts and not invert and not count_only
    sink = _GrepSink(patterns, count_only, only_matching, errors, invert, bool(before_context or after_context), max_match_count, after_context, with_parts)
    if max_match_count and after_context and not count_only:
        max_match_count += after_context  # (the trailing `after_context` lines hold that many selected lines at most: _GrepSink)
    if not only_matching:
        for pattern in patterns:  # the reference compiles them for -o in every mode: same early failure for bad syntax
            re.compile(pattern)
    problem = None
    if not os.path.exists(file):
        problem = FileNotFoundError("No such file or directory")
    elif os.path.isdir(file):
        problem = ValueError("is a directory")
    if problem is not None:
        if not no_messages:
            raise problem
        return sink.result(), RC_INVALID_FILE
    flags = _GREP_FLAGS | (HS_FLAG_CASELESS if ignore_case else 0)
    if with_parts:
        return_code = scan(file, patterns, sink, flags=[flags] * len(patterns), max_match_count=max_match_count, parts=True)
    else:
        return_code = scan(file, patterns, sink, flags=[flags] * len(patterns), max_match_count=max_match_count, invert=invert,
                           before_context=before_context, after_context=after_context)
    if matched_parts and invert and not count_only:
        return [], return_code  # (a line without a match has no matched part)
    return sink.result(), return_code


def grep_files_outcomes(files: Sequence[str], patterns: list[str], **grep_kwargs) -> list:
    """What grep(file, patterns, **grep_kwargs) gives for every file, in order: its result, or the exception it raises (not
    raised here).  The files share one native call (scan_files), with context lines too (every file has a sink built as grep()
    builds it), and with matched_parts when two or more files can be scanned (scan_files(parts=True); one file has nothing to
    share and takes grep())."""
    names = list(files)
    outcomes: list = [None] * len(names)
    known = {"ignore_case", "count_only", "only_matching", "no_messages", "errors", "max_match_count", "invert", "before_context", "after_context", "matched_parts"}
    matched_parts = grep_kwargs.get("matched_parts", False)
    # (context arguments, which grep() refuses for every file, and unknown ones: grep() raises what it raises)
    if matched_parts and (sum(1 for name in names if os.path.exists(name) and not os.path.isdir(name)) < 2 or grep_kwargs.get("before_context") or
                          grep_kwargs.get("after_context") or set(grep_kwargs) - known):
        for index, name in enumerate(names):
            try:
                outcomes[index] = grep(name, patterns, **grep_kwargs)
            except Exception as error:  # pylint: disable=broad-except
                outcomes[index] = error
        return outcomes
    ignore_case = grep_kwargs.get("ignore_case", False)
    count_only = grep_kwargs.get("count_only", False)
    only_matching = grep_kwargs.get("only_matching", False)
    no_messages = grep_kwargs.get("no_messages", False)
    invert = grep_kwargs.get("invert", False)
    max_match_count = grep_kwargs.get("max_match_count", 0)
    before_context, after_context = grep_kwargs.get("before_context", 0), grep_kwargs.get("after_context", 0)
    unknown = set(grep_kwargs) - known
    if matched_parts:
        only_matching = False  # (as in grep(): matched_parts takes precedence)
    with_parts = matched_parts and not invert and not count_only
    if unknown:
        raise TypeError(f"grep_files() got unexpected keyword arguments {sorted(unknown)}")
    # (exactly grep()'s sink and its limit: the trailing rule of GNU grep 3.5 and later is the sink's)
    sinks = [_GrepSink(patterns, count_only, only_matching, grep_kwargs.get("errors", "ignore"), invert, bool(before_context or after_context), max_match_count,
                       after_context, with_parts) for _name in names]
    if max_match_count and after_context and not count_only:
        max_match_count += after_context
    if not only_matching:
        for pattern in patterns:  # (grep()'s early failure for bad syntax)
            re.compile(pattern)
    scanned = []
    for index, name in enumerate(names):
        problem = None
        if not os.path.exists(name):
            problem = FileNotFoundError("No such file or directory")
        elif os.path.isdir(name):
            problem = ValueError("is a directory")
        if problem is None:
            scanned.append(index)
        else:
            outcomes[index] = problem if not no_messages else (sinks[index].result(), RC_INVALID_FILE)
    if scanned:
        flags = _GREP_FLAGS | (HS_FLAG_CASELESS if ignore_case else 0)
        summaries = scan_files([names[i] for i in scanned], patterns, lambda which, matches, count: sinks[scanned[which]](matches, count),
                               flags=[flags] * len(patterns), max_match_count=max_match_count, invert=invert, before_context=before_context,
                               after_context=after_context, **({"parts": True} if with_parts else {}))
        for which, index in enumerate(scanned):
            # (matched_parts with invert: a line without a match has no matched part, as in grep())
            outcomes[index] = ([] if matched_parts and invert and not count_only else sinks[index].result(), summaries[which][0])
    return outcomes


def grep_files(files: Sequence[str], patterns: list[str], **grep_kwargs) -> list:
    """[grep(file, patterns, **grep_kwargs) for file in files], with the files sharing one native call and small files one
    GPU scan (scan_files).  Raises what the first failing grep() of that list raises."""
    outcomes = grep_files_outcomes(files, patterns, **grep_kwargs)
    for outcome in outcomes:
        if isinstance(outcome, Exception):
            raise outcome
    return outcomes
