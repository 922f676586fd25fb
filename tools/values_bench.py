"""Cost of counting the distinct matched parts on the GPU (hg_count_values, csrc/hg_values.hip) for text resident in HBM.

usage: python tools/values_bench.py [--gib 8] [--reps 5] [--configs 3,5,d] [--distinct-gib 0.5] [--out FILE]
(the record: profiles/values_bench.txt)
Text: the benchmark's synthetic log (hg_synth_device), --gib GiB of it in one buffer, with config 3's expression set and
needles (256 expressions, three tiers) and with config 5's (4096 literals); and, as `d`, --distinct-gib GiB of it with one
expression that matches every line's timestamp and host (`[0-9:]+\\.[0-9]+Z host-[0-9]+`), so that nearly every value is
distinct.  Per config, after one scan with parts:
  values_us   the whole stage, median and minimum of --reps calls (HIP events around everything the call queues, its two host
              synchronisations included), keyed by bytes and keyed by (expression, bytes);
  download    the distinct values to the host (Scanner.values_arrays), milliseconds;
  host route  the only route without the stage: hg_gather_parts with flags 0, its bytes and offsets to the host
              (Scanner.part_lines_arrays), and a dictionary over the slices (collections.Counter); timed in the same run, the
              gather and download alone and with the dictionary.  Both routes must agree on every count.
The passes' kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -- python tools/values_bench.py
--configs <one> --reps 3, whose kernel statistics name the hg_values_* kernels.
"""
from __future__ import annotations

import argparse
import collections
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = [r"[0-9:]+\.[0-9]+Z host-[0-9]+"]


def emit(lines, line) -> None:
    """One line of the report: shown at once (a long run stays visibly alive), kept for --out."""
    lines.append(line)
    print(line, flush=True)


def host_route(sc, d_text: int, nbytes: int):
    """Gather the parts, download bytes and offsets, count in a dictionary.  Returns (gather + download ms, all ms, the Counter)."""
    t0 = time.perf_counter()
    sc.gather_parts(d_text, nbytes)
    a = sc.part_lines_arrays()
    t1 = time.perf_counter()
    blob, off = a["bytes"], a["entry_off"].tolist()
    table = collections.Counter(blob[off[j]:off[j + 1]] for j in range(len(off) - 1))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3, table


def main() -> None:
    import torch

    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--distinct-gib", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="3,5,d")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("values_bench needs a GPU: there is nothing to measure without one")
    lines = []
    emit(lines, f"# tools/values_bench.py --gib {args.gib:g} --distinct-gib {args.distinct_gib:g} --reps {args.reps} --configs {args.configs}: one MI355X, synthetic log resident, buffer_size 262140")
    emit(lines, "# config | text bytes | lines | parts | parts_us | key | values | value bytes | table 2^k | values_us (median, min) | download ms | "
         "host route ms: gather + download, + dictionary | host / stage")
    full = int(args.gib * (1 << 30)) & ~15
    text = torch.empty(full + 16, dtype=torch.uint8, device="cuda:0")
    for config in args.configs.split(","):
        if config == "d":
            pats, needles, hpm = DISTINCT, benchspec.c3_spec()[1], 0  # (no line carries a needle)
            nbytes = min(full, int(args.distinct_gib * (1 << 30)) & ~15)
        else:
            pats, needles, hpm = {"3": benchspec.c3_spec, "5": benchspec.c5_spec}[config]()
            nbytes = full
        device.synth_device(text.data_ptr(), nbytes, seed=23, needles=needles, hit_per_million=hpm)
        torch.cuda.synchronize()
        sc = device.Scanner(device.Database(pats, ids=list(range(len(pats)))), 0)
        try:
            st = sc.scan(text.data_ptr(), nbytes, parts=True)
        except ValueError as e:  # a set the parts stage is not offered for
            emit(lines, f"c{config} | no parts: {e}")
            continue
        down_ms, host_ms, table = host_route(sc, text.data_ptr(), nbytes)
        for key, by_pattern in (("bytes", False), ("pattern+bytes", True)):
            us = []
            for rep in range(args.reps + 1):
                v = sc.count_values(text.data_ptr(), nbytes, by_pattern=by_pattern)
                if rep:  # (the first call allocates the stage's buffers)
                    us.append(v.values_us)
            t0 = time.perf_counter()
            rows = sc.values()
            got_ms = (time.perf_counter() - t0) * 1e3
            merged = collections.Counter()
            for value, count, _pattern, _line in rows:
                merged[value] += count
            if merged != table:  # the two routes agree on what the values are and how often they occur
                raise SystemExit(f"c{config} ({key}): the stage and the host route disagree ({len(merged)} and {len(table)} values)")
            med = statistics.median(us)
            emit(lines, f"c{config} | {nbytes} | {st.n_lines} | {st.n_parts} | {st.parts_us} | {key} | {v.n_values} | {v.n_bytes} | {sc._last_values.table_log2} | "  # pylint: disable=protected-access
                 f"{med:.0f}, {min(us)} | {got_ms:.1f} | {down_ms:.0f}, {host_ms:.0f} | {host_ms * 1e3 / max(med, 1):.0f}")
        del sc
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
