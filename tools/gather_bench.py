"""Cost of gathering the selected lines on the GPU (hg_gather_lines, csrc/hg_gather.hip) for text resident in HBM.

usage: python tools/gather_bench.py [--gib 8] [--reps 5] [--cases 1000,10000,100000,invert] [--out FILE]
(the record: profiles/gather_bench.txt)
Text: the benchmark's synthetic log (hg_synth_device), --gib GiB of it in one buffer, one 8-byte literal as the expression and
as the needle.  Cases: needle rates per million lines (about 0.1 %, 1 % and 10 % of the lines match), and `invert`: the
inverted scan at the lowest rate, where nearly every line is selected and the output is nearly the whole text.
Per case, after one scan, medians of --reps gathers each with flags 0 and with TERMINATE | NUMBER | SEPARATOR:
  gather_us   the whole stage (HIP events: flags, scan, entries, scan, the host synchronisation that sizes the output, copy);
  bound       the stage's traffic over the HBM rate: the bodies read and the output written (2 x n_bytes at flags 0), plus the
              records and per-entry arrays the index passes move, over 8.0 TB/s (the part's peak) and 6.29 TB/s (the rate a
              float4 copy reaches on it);
  whole text  what a caller had to do before: a device-to-host copy of the whole text, through a pinned buffer of 1 GiB,
              timed in the same run.
The three steps' kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -- python tools/gather_bench.py
--cases <one case> --reps 3, whose kernel statistics name hg_gather_flag_kernel, hg_gather_entry_kernel, hg_gather_first_kernel
and hg_gather_copy_kernel.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_SPEC, PEAK_COPY = 8.0e12, 6.29e12  # bytes per second: the part's HBM peak, and what a float4 copy reaches
PRINT_READY = 2 | 4 | 8  # HG_LINES_TERMINATE | HG_LINES_NUMBER | HG_LINES_SEPARATOR


def emit(lines, line) -> None:
    """One line of the report: shown at once (a long run stays visibly alive), kept for --out."""
    lines.append(line)
    print(line, flush=True)


def traffic(n_records: int, n_entries: int, n_bytes: int, body_bytes: int) -> int:
    """Bytes the stage moves: bodies read, output written, and the index passes: each record's 32 bytes read by the flag and the
    entry pass with 8 + 8 bytes of flag and scan written and read, and per entry the 24-byte descriptor, size, offset, line
    number and kind written and the descriptor and offset read again by the copy pass."""
    return body_bytes + n_bytes + n_records * (2 * 32 + 4 * 8) + n_entries * (24 + 8 + 8 + 8 + 4 + 24 + 8 + 8)


def main() -> None:
    import torch

    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="1000,10000,100000,invert")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gather_bench needs a GPU: there is nothing to measure without one")
    nbytes = int(args.gib * (1 << 30)) & ~15
    pats, needles, _hpm = benchspec.c1_spec()
    lines = []
    emit(lines, f"# tools/gather_bench.py --gib {args.gib:g} --reps {args.reps} --cases {args.cases}: one MI355X, {nbytes} bytes of synthetic log resident, buffer_size 262140")
    emit(lines, "# case | lines | records | entries | flags | n_bytes | gather_us (median, min) | output GB/s | traffic bound us at 8.0 / 6.29 TB/s | gather / bound(6.29) | "
         "whole-text D2H ms | D2H / gather")
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    bounce = torch.empty(min(nbytes, 1 << 30), dtype=torch.uint8, pin_memory=True)
    sc = device.Scanner(device.Database(pats, ids=[0]), 0)
    made = None
    for case in args.cases.split(","):
        invert = case == "invert"
        rate = 1000 if invert else int(case)
        if rate != made:
            device.synth_device(text.data_ptr(), nbytes, seed=23, needles=needles, hit_per_million=rate)
            torch.cuda.synchronize()
            made = rate
        st = sc.scan(text.data_ptr(), nbytes, invert=invert)
        # the route a caller has without the stage: the whole text to the host
        t0 = time.perf_counter()
        for at in range(0, nbytes, bounce.numel()):
            n = min(bounce.numel(), nbytes - at)
            bounce[:n].copy_(text[at:at + n], non_blocking=True)
        torch.cuda.synchronize()
        d2h_ms = (time.perf_counter() - t0) * 1e3
        body = None
        for flags in (0, PRINT_READY):
            us = []
            for rep in range(args.reps + 1):
                g = sc._gather(text.data_ptr(), nbytes, flags)  # pylint: disable=protected-access
                if rep:  # (the first gather allocates the stage's buffers)
                    us.append(g.gather_us)
            if flags == 0:
                body = g.n_bytes
            bytes_moved = traffic(st.n_hits, g.n_entries, g.n_bytes, body)
            med = statistics.median(us)
            emit(lines, f"{case} | {st.n_lines} | {st.n_hits} | {g.n_entries} | {flags} | {g.n_bytes} | {med:.0f}, {min(us)} | {g.n_bytes / max(med, 1) / 1e3:.1f} | "
                 f"{bytes_moved / PEAK_SPEC * 1e6:.0f} / {bytes_moved / PEAK_COPY * 1e6:.0f} | {med / max(bytes_moved / PEAK_COPY * 1e6, 1e-9):.1f} | {d2h_ms:.0f} | "
                 f"{d2h_ms * 1e3 / max(med, 1):.0f}")
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
