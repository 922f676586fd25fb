"""Cost of the parts stage (hg_scan_device_parts, csrc/hg_parts.hip) and of grep(matched_parts=True).

usage: python tools/parts_bench.py [--mib 64] [--reps 5] [--file-mib 8] [--skip resident,e2e,worst] [--out FILE]
(the record: profiles/parts_bench.txt)
Resident.  hg_scan_device and hg_scan_device_parts alternate in one process on one scanner over the same synthetic text
(csrc/hg_synth.h), for one literal expression (benchspec.c1_spec), 64 and 256 expressions of config 3 (benchspec.c3_spec, sized
down for 64), each with its own needles at per-line needle rates 1e-3, 0.1 and 1 (every line carries a needle; config 3's
needles include about 20 % look-alikes that must not match).  Per cell: the scans' ms_total (HIP events, the same launches in
both), the stage's parts_us (HIP events around count, scan, the host synchronisation that sizes the output, and write), parts
per second of stage time, and the stage's text bytes (the scanned bytes of the distinct hit lines) over its time.
End to end.  grep(matched_parts=True) against grep(only_matching=True), the route through Python's `re`, on the same file with
one literal expression, for which both give the same rows (asserted), at the same three rates; medians of the wall time.
Worst case.  One line of 16 KiB and one of 64 KiB of `a` under a.*b|a: every anchored walk runs to the line's end, so the
stage is quadratic in the line's length; measured once each (the second is skipped when the first predicts minutes).  And
one line of 2 KiB of `q` under [a-z]{1000}x, the multi-word walk (32 state words per lane in LDS) at its longest.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATES = ((1000, "1e-3"), (100000, "0.1"), (1000000, "every line"))


def resident(args, lines) -> None:
    import numpy as np
    import torch

    from hypergrep_amd import benchspec, device

    nbytes = args.mib << 20
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    sets = (("1 literal (simple)", benchspec.c1_spec()), ("64 of config 3", benchspec.c3_spec(48, 12, 4)), ("256 of config 3", benchspec.c3_spec()))
    lines += [f"## resident: {nbytes} bytes of synthetic log text, one MI355X, {args.reps} alternating pairs, medians",
              f"{'set':20s} {'needle rate':>11s} {'hit lines':>9s} {'parts':>9s} {'scan ms_total':>13s} {'parts scan ms_total':>19s} {'parts_us':>9s} {'Mparts/s':>9s} {'stage text GB/s':>15s}"]
    for name, (pats, needles, _hpm) in sets:
        flags = [6] * len(pats)  # DOTALL | MULTILINE: every match end is a report
        sc = device.Scanner(device.Database(pats, flags=flags, ids=list(range(len(pats)))), 0)
        for hpm, label in RATES:
            device.synth_device(text.data_ptr(), nbytes, seed=17, needles=needles, hit_per_million=hpm)
            torch.cuda.synchronize()
            for parts in (False, True):  # warm-up: workspace sizing, the stage's buffers
                sc.scan(text.data_ptr(), nbytes, parts=parts)
            total = {False: [], True: []}
            stage = []
            st = None
            for _ in range(args.reps):
                for parts in (False, True):
                    st = sc.scan(text.data_ptr(), nbytes, parts=parts)
                    total[parts].append(st.ms_total)
                    if parts:
                        stage.append(st.parts_us)
            rows = sc.hits_array()
            _, first = np.unique(rows[:, 0], return_index=True) if len(rows) else ([], [])
            text_bytes = int(rows[first, 4].sum()) if len(rows) else 0
            us = statistics.median(stage)
            lines.append(f"{name:20s} {label:>11s} {len(first):9d} {st.n_parts:9d} {statistics.median(total[False]):13.3f} {statistics.median(total[True]):19.3f} {us:9.0f} "
                         f"{st.n_parts / us if us else 0:9.2f} {text_bytes / us / 1e3 if us else 0:15.3f}")
        del sc


def end_to_end(args, lines) -> None:
    import hypergrep_amd
    from hypergrep_amd import benchspec, device

    pats, needles, _hpm = benchspec.c1_spec()
    nbytes = args.file_mib << 20
    lines += [f"## end to end: grep() on a file of {nbytes} bytes, one literal expression, {args.reps} runs each, median wall seconds",
              f"{'needle rate':>11s} {'rows':>8s} {'only_matching (re)':>18s} {'matched_parts (GPU)':>19s} {'re / GPU':>9s}"]
    with tempfile.TemporaryDirectory() as tmp:
        for hpm, label in RATES:
            path = os.path.join(tmp, f"text_{hpm}")
            data = device.synth_host(nbytes, 23, needles, hpm)
            with open(path, "wb") as f:
                f.write(data[:data.rfind(b"\n") + 1])
            wall = {"only_matching": [], "matched_parts": []}
            rows = {}
            for _ in range(args.reps + 1):  # (the first pair warms the database cache and the pooled context)
                for mode in wall:
                    t0 = time.perf_counter()
                    rows[mode], rc = hypergrep_amd.grep(path, pats, **{mode: True})
                    wall[mode].append(time.perf_counter() - t0)
                    assert rc == 0
            assert rows["only_matching"] == rows["matched_parts"], "the two routes disagree on a literal"
            old, new = statistics.median(wall["only_matching"][1:]), statistics.median(wall["matched_parts"][1:])
            lines.append(f"{label:>11s} {len(rows['matched_parts']):8d} {old:18.4f} {new:19.4f} {old / new:9.2f}")


def worst_case(_args, lines) -> None:
    import torch

    from hypergrep_amd import device

    sc = device.Scanner(device.Database(["a.*b|a"], flags=[6]), 0)
    lines.append("## worst case: a.*b|a on ONE line of `a` (every anchored walk runs to the line's end), measured once")
    last_ms = 0.0
    for kib in (16, 64):
        if kib == 64 and last_ms * 16 > 120000:
            lines.append(f"  64 KiB: skipped, the 16 KiB line predicts {last_ms * 16 / 1000:.0f} s")
            break
        n = kib << 10
        text = torch.full((n + 16,), ord("a"), dtype=torch.uint8, device="cuda:0")
        text[n - 1] = 10
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = sc.scan(text.data_ptr(), n, parts=True)
        wall = (time.perf_counter() - t0) * 1e3
        last_ms = st.parts_us / 1e3
        lines.append(f"  {kib} KiB: {st.n_parts} parts, parts stage {last_ms:.1f} ms (count and write: two walks), call {wall:.1f} ms")
    # the multi-word walk (32 state words in LDS per lane): no part, every start walks until the line or the repeat ends
    sc = device.Scanner(device.Database(["[a-z]{1000}x", "Q"], flags=[6, 6], ids=[0, 1]), 0)
    n = 2048
    text = torch.full((n + 16,), ord("q"), dtype=torch.uint8, device="cuda:0")
    text[n - 2] = ord("Q")  # (the line needs a hit to be walked)
    text[n - 1] = 10
    torch.cuda.synchronize()
    st = sc.scan(text.data_ptr(), n, parts=True)
    lines.append(f"  [a-z]{{1000}}x (32 state words) on one line of 2 KiB of q: {st.n_parts} part, parts stage {st.parts_us / 1e3:.1f} ms")


def main() -> None:
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--file-mib", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("parts_bench needs a GPU: there is nothing to measure without one")
    lines = [f"# tools/parts_bench.py --mib {args.mib} --file-mib {args.file_mib} --reps {args.reps}"]
    skip = set(args.skip.split(","))
    shown = 0
    for name, fn in (("resident", resident), ("e2e", end_to_end), ("worst", worst_case)):
        if name not in skip:
            fn(args, lines)
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
    report = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(report)


if __name__ == "__main__":
    main()
