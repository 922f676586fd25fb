"""Cost of the most frequent matched values of a file of many chunks: the value store's route (hg_hyperscan_values_top,
csrc/hg_valstore.hip: every chunk's parts accumulated on the GPU, one ranking, only the kept rows downloaded) against the only
route without it (hg_hyperscan_values: every chunk's distinct values downloaded and merged in a std::map, then a host sort and
cut), both in one process on the same file.

usage: python tools/valstore_bench.py [--gib 8] [--distinct-gib 0.5] [--reps 3] [--top 100] [--configs 3,5,d] [--dir DIR] [--out FILE]
(the record: profiles/valstore_bench.txt)
File: the benchmark's synthetic log (hg_synth_device), --gib GiB of it written to --dir and read back in 256 MiB chunks, with
config 3's expression set and needles (256 expressions) and with config 5's (4096 literals); and, as `d`, --distinct-gib GiB of
it with one expression that matches every line's timestamp and host, so that nearly every value is distinct.  Per config one
warm run of either route (database compile, window tuning, buffers, page cache), then --reps timed runs of either, alternating;
wall time around the native call, whose callback only takes the arrays (the old route's sort and cut by numpy: a stable argsort
by descending count over the rows, which come in the order of first occurrence).  Reported: median, minimum and maximum per
route, the old route's spread (max - min) and the difference of the medians.  Both routes must agree on the kept rows.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = [r"[0-9:]+\.[0-9]+Z host-[0-9]+"]


def emit(lines, line) -> None:
    """One line of the report: shown at once (a long run stays visibly alive), kept for --out."""
    lines.append(line)
    print(line, flush=True)


def main() -> None:
    import numpy as np
    import torch

    from hypergrep_amd import benchspec, device, utils

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--distinct-gib", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--configs", default="3,5,d")
    ap.add_argument("--dir", default="", help="where the file is written (default: the system's temporary directory)")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("valstore_bench needs a GPU: there is nothing to measure without one")
    lines = []
    emit(lines, f"# tools/valstore_bench.py --gib {args.gib:g} --distinct-gib {args.distinct_gib:g} --reps {args.reps} --top {args.top} --configs {args.configs}: one MI355X, "
                "synthetic log in a file, 256 MiB chunks, buffer_size 262140")
    emit(lines, "# config | file bytes | distinct values | parts | kept rows | old route s (median, min, max) | store route s (median, min, max) | old spread s | "
                "store - old s (medians) | old / store")
    full = int(args.gib * (1 << 30)) & ~15
    text = torch.empty(full + 16, dtype=torch.uint8, device="cuda:0")
    engine = utils._get_hyperscanner_lib()  # pylint: disable=protected-access
    event = utils._VALUES_EVENT  # pylint: disable=protected-access
    head = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.POINTER(utils.ExprExt)), ctypes.c_uint,
            ctypes.c_int, ctypes.POINTER(utils.ValuesParams)]
    engine.hg_hyperscan_values.argtypes = head + [event, ctypes.c_void_p]
    engine.hg_hyperscan_values_top.argtypes = head + [ctypes.c_uint64, event, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    with tempfile.TemporaryDirectory(dir=args.dir or None) as root:
        path = os.path.join(root, "valstore_bench.log")
        for config in args.configs.split(","):
            if config == "d":
                pats, needles, hpm = DISTINCT, benchspec.c3_spec()[1], 0  # (no line carries a needle)
                nbytes = min(full, int(args.distinct_gib * (1 << 30)) & ~15)
            else:
                pats, needles, hpm = {"3": benchspec.c3_spec, "5": benchspec.c5_spec}[config]()
                nbytes = full
            device.synth_device(text.data_ptr(), nbytes, seed=23, needles=needles, hit_per_million=hpm)
            torch.cuda.synchronize()
            with open(path, "wb") as f:
                for lo in range(0, nbytes, 256 << 20):
                    f.write(memoryview(text[lo:min(lo + (256 << 20), nbytes)].cpu().numpy()))
            c_patterns, c_flags, c_ids = utils.prepare_patterns(pats, flags=[14] * len(pats), ids=list(range(len(pats))))
            params = utils.ValuesParams()
            kept = {}

            def take(which, top):
                def on_values(_context, data, off, counts, _pattern, n_values) -> None:
                    c = np.ctypeslib.as_array(counts, shape=(max(n_values, 1),))[:n_values]
                    o = np.ctypeslib.as_array(off, shape=(n_values + 1,))
                    order = np.argsort(-c.astype(np.int64), kind="stable")[:top] if which == "old" else np.arange(n_values)
                    blob = ctypes.string_at(data, int(o[n_values])) if n_values else b""
                    kept[which] = ([(blob[int(o[j]):int(o[j + 1])], int(c[j])) for j in order], n_values)
                return event(on_values)

            def old_route() -> float:
                cb = take("old", args.top)
                t0 = time.perf_counter()
                rc = engine.hg_hyperscan_values(path.encode(), c_patterns, c_flags, c_ids, None, len(c_patterns), 262140, ctypes.byref(params), cb, None)
                dt = time.perf_counter() - t0
                if rc:
                    raise SystemExit(f"c{config}: hg_hyperscan_values returned {rc}")
                return dt

            totals = [ctypes.c_uint64(), ctypes.c_uint64()]

            def store_route() -> float:
                cb = take("store", args.top)
                t0 = time.perf_counter()
                rc = engine.hg_hyperscan_values_top(path.encode(), c_patterns, c_flags, c_ids, None, len(c_patterns), 262140, ctypes.byref(params), args.top, cb, None,
                                                    ctypes.byref(totals[0]), ctypes.byref(totals[1]))
                dt = time.perf_counter() - t0
                if rc:
                    raise SystemExit(f"c{config}: hg_hyperscan_values_top returned {rc}")
                return dt

            old_route()
            store_route()  # warm: the database, the tuned windows, the buffers and the page cache are there for both
            old, new = [], []
            for _rep in range(args.reps):
                old.append(old_route())
                new.append(store_route())
            if kept["old"][0] != kept["store"][0] or kept["old"][1] != totals[0].value:
                raise SystemExit(f"c{config}: the routes disagree ({kept['old'][1]} and {totals[0].value} distinct values)")
            mo, mn = statistics.median(old), statistics.median(new)
            emit(lines, f"c{config} | {nbytes} | {totals[0].value} | {totals[1].value} | {len(kept['store'][0])} | {mo:.3f}, {min(old):.3f}, {max(old):.3f} | "
                        f"{mn:.3f}, {min(new):.3f}, {max(new):.3f} | {max(old) - min(old):.3f} | {mn - mo:+.3f} | {mo / mn:.2f}")
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
