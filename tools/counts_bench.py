"""Cost of counting reports and matching lines per report id on the GPU (hg_count_records, csrc/hg_counts.hip) for text
resident in HBM, against the route that existed before it.

usage: python tools/counts_bench.py [--gib 8] [--reps 5] [--shapes c3,c5,hot] [--out FILE]
(the record: profiles/counts_bench.txt)
Text: the benchmark's synthetic log (hg_synth_device), --gib GiB of it in one buffer.  Shapes: c3, config 3's 256 expressions
at their usual hit rate (a few hundred lukewarm bins); c5, config 5's 4096 literals with 10 % of the lines hit (thousands of
lukewarm bins, the most a workgroup counts in LDS); hot, one expression that every line matches (every record in one bin).
Per shape, after one scan, one warm-up and then --reps repetitions each of
  (a) counts_us   the stage (HIP events: zeroing the totals, the one kernel);
  (b) host route  what a caller did before, in the same process on the same build: hg_copy_hits of all records (16 B each,
                  no aux) and numpy.unique over the ids, with the head rule for the lines, timed with perf_counter;
median and spread (min .. max) of each, and the stage's traffic bound: 16 bytes per record over 6646 GB/s, the rate a read-only
kernel reaches on this part (profiles/r03_bw_ceiling.txt).  The two routes' results are compared; a difference ends the run.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_RATE = 6.646e12  # bytes per second (profiles/r03_bw_ceiling.txt, default loads)


def emit(lines, line) -> None:
    """One line of the report: shown at once (a long run stays visibly alive), kept for --out."""
    lines.append(line)
    print(line, flush=True)


def host_route(sc, device):
    """(ids, n_lines, n_reports) from the downloaded records."""
    import numpy as np

    n = sc._last.n_hits  # pylint: disable=protected-access
    hits = np.zeros(n, dtype=[("line_number", "<u8"), ("id", "<u4"), ("to", "<u4")])
    if n and device.lib().hg_copy_hits(sc._h, hits.ctypes.data_as(ctypes.POINTER(device.HgHit)), None, n) != 0:  # pylint: disable=protected-access
        raise SystemExit("hg_copy_hits failed")
    rid, line = hits["id"], hits["line_number"]
    ids, inverse, reports = np.unique(rid, return_inverse=True, return_counts=True)
    head = np.ones(n, dtype=bool)
    head[1:] = (line[1:] != line[:-1]) | (rid[1:] != rid[:-1])
    return ids, np.bincount(inverse[head], minlength=len(ids)), reports


def main() -> None:
    import numpy as np
    import torch

    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c3,c5,hot")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("counts_bench needs a GPU: there is nothing to measure without one")
    nbytes = int(args.gib * (1 << 30)) & ~15
    lines = []
    emit(lines, f"# tools/counts_bench.py --gib {args.gib:g} --reps {args.reps} --shapes {args.shapes}: one MI355X, {nbytes} bytes of synthetic log resident, buffer_size 262140")
    emit(lines, "# shape | bins | bins hit | lines | records | (a) counts_us median (min .. max) | bound us at 16 B/record, 6646 GB/s | (a) / bound | records GB/s | "
         "(b) copy_hits + numpy.unique ms median (min .. max) | (b) / (a)")
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    c3, c5 = benchspec.c3_spec(), benchspec.c5_spec()
    shapes = {"c3": (c3[0], list(range(len(c3[0]))), c3[1], c3[2]), "c5": (c5[0], list(range(len(c5[0]))), c5[1], c5[2]), "hot": (["."], [0], c3[1], c3[2])}
    for name in args.shapes.split(","):
        patterns, ids, needles, hpm = shapes[name]
        device.synth_device(text.data_ptr(), nbytes, seed=23, needles=needles, hit_per_million=hpm)
        torch.cuda.synchronize()
        sc = device.Scanner(device.Database(patterns, ids=ids), 0)
        st = sc.scan(text.data_ptr(), nbytes)
        us = []
        for rep in range(args.reps + 1):
            c = sc.count()
            if rep:  # (the first count allocates the stage's buffers)
                us.append(c.counts_us)
        got = sc.counts_arrays()
        ms = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            want = host_route(sc, device)
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3)
        hit = got[2] != 0
        if not (np.array_equal(got[0][hit], want[0]) and np.array_equal(got[1][hit], want[1]) and np.array_equal(got[2][hit], want[2])):
            raise SystemExit(f"{name}: the stage and the host route disagree")
        med, bound = statistics.median(us), st.n_hits * 16 / READ_RATE * 1e6
        emit(lines, f"{name} | {c.n_bins} | {int(hit.sum())} | {st.n_lines} | {st.n_hits} | {med:.0f} ({min(us)} .. {max(us)}) | {bound:.1f} | {med / max(bound, 1e-9):.1f} | "
             f"{st.n_hits * 16 / max(med, 1) / 1e3:.0f} | {statistics.median(ms):.1f} ({min(ms):.1f} .. {max(ms):.1f}) | {statistics.median(ms) * 1e3 / max(med, 1):.0f}")
        del sc
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
