"""Cost of the context stage (hg_scan_device_context, csrc/hg_context.hip) on bench.py's config-3 text, sized down.

usage: python tools/context_bench.py [--gib 2] [--reps 7] [--before 2] [--after 2] [--lib OTHER.so] [--out FILE]
(the record: profiles/context_bench.txt)
Two sets on the same synthetic text (benchspec.c3_spec, 1e-3 of the lines carry a needle): config 3's 256 expressions, where
about (before + after) / 1000 of the lines are context, and the same plus one expression every line matches, where no line is
(no context record: the count pass only).  hg_scan_device and hg_scan_device_context alternate in one process on one scanner;
per call the host wall time around the blocking call, the scan's own ms_total (HIP events, the same launches in both) and,
for calls with context, the stage's time (context_us: HIP events around its count launch, scan and write launch, with the
one host synchronisation between them that sizes the output).
--lib: another build of the library (hypergrep_amd/build.py HG_BUILD_OUT), e.g. one of the parent commit, which has no
context stage: then only hg_scan_device is timed, on the same text and sets.  Runs of the two builds are alternated by the
caller, one process each (a process loads one library).
The stage's traffic bound: one read of the tiles that hold a context record (an upper estimate from the records' starts)
plus 32 bytes written per record, at the HBM read rate of profiles/r03_bw_ceiling.txt (default loads, as the stage uses).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_READ_GBPS = 6645.8  # profiles/r03_bw_ceiling.txt: default loads, best occupancy
TILE = 16384


def main() -> None:
    import torch

    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--before", type=int, default=2)
    ap.add_argument("--after", type=int, default=2)
    ap.add_argument("--out", default="", help="append the report to this file")
    ap.add_argument("--lib", default="", help="scan with this build of the library instead of the package's")
    args = ap.parse_args()
    if args.lib:
        import hypergrep_amd

        hypergrep_amd.configure_libraries(libhs=os.path.abspath(args.lib))
    if not torch.cuda.is_available():
        raise SystemExit("context_bench needs a GPU: there is nothing to measure without one")
    nbytes = int(args.gib * (1 << 30))
    pats, needles, _hpm = benchspec.c3_spec()
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    device.synth_device(text.data_ptr(), nbytes, seed=17, needles=needles, hit_per_million=1000)
    torch.cuda.synchronize()
    can_context = hasattr(device.lib(), "hg_scan_device_context")
    ctx = (args.before, args.after)
    lines = [f"# tools/context_bench.py --gib {args.gib} --reps {args.reps} --before {ctx[0]} --after {ctx[1]}{' --lib ' + args.lib if args.lib else ''}: {nbytes} bytes of config-3 text, hit rate 1e-3, one MI355X",
             "# per call: host wall ms (median / min) and the scan's ms_total (median); context stage: context_us (median), HIP events",
             f"# bound = (16 KiB x tiles with a context record + 32 B x records) / {HBM_READ_GBPS} GB/s (profiles/r03_bw_ceiling.txt, default loads)"]
    sets = (("config 3, 1e-3 of the lines match", pats, [14] * len(pats)), ("config 3 + an expression every line matches", pats + ["^."], [14] * len(pats) + [14]))
    for name, p, flags in sets:
        sc = device.Scanner(device.Database(p, flags=flags, ids=list(range(len(p)))), 0)
        modes = (None, ctx) if can_context else (None,)
        for mode in modes + modes:  # warm-up: workspace sizing, the stage's buffers
            sc.scan(text.data_ptr(), nbytes, context=mode)
        wall = {None: [], ctx: []}
        total = {None: [], ctx: []}
        stage = []
        last = {}
        for _ in range(args.reps):
            for mode in modes:
                t0 = time.perf_counter()
                st = sc.scan(text.data_ptr(), nbytes, context=mode)
                wall[mode].append((time.perf_counter() - t0) * 1e3)
                total[mode].append(st.ms_total)
                last[mode] = st
                if mode:
                    stage.append(st.context_us / 1e3)
        med = statistics.median
        lines += [f"{name}: {len(p)} expressions, {last[None].n_lines} lines, {last[None].n_hits} hits",
                  f"  hg_scan_device          wall {med(wall[None]):8.3f} / {min(wall[None]):8.3f} ms   ms_total {med(total[None]):8.3f}"]
        if can_context:
            n_context = last[ctx].n_context
            tiles = len({row[3] // TILE for row in sc.context()}) if n_context else 0  # (a piece belongs to the tile its first byte lies in; start >= that byte)
            bound_ms = (tiles * TILE + 32 * n_context) / (HBM_READ_GBPS * 1e9) * 1e3
            stage_ms = med(stage)
            lines += [
                f"  hg_scan_device_context  wall {med(wall[ctx]):8.3f} / {min(wall[ctx]):8.3f} ms   ms_total {med(total[ctx]):8.3f}   context stage {stage_ms:8.3f} ms (min {min(stage):.3f})",
                f"  {n_context} context records in {tiles} tiles; traffic bound of the stage {bound_ms:8.3f} ms; stage / bound = {stage_ms / bound_ms if bound_ms else float('nan'):6.2f}",
            ]
        del sc
    report = "\n".join(lines) + "\n"
    print(report, end="")
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(report)


if __name__ == "__main__":
    main()
