"""Cost of the invert stage (hg_scan_device_invert, csrc/hg_invert.hip) on bench.py's config-3 text, sized down.

usage: python tools/invert_bench.py [--gib 2] [--reps 7] [--lib OTHER.so] [--out FILE]   (the record: profiles/invert_bench.txt)
Two sets on the same synthetic text (benchspec.c3_spec, 1e-3 of the lines carry a needle): config 3's 256 expressions, where
nearly every line is selected, and the same plus one expression every line matches, where nothing is.  hg_scan_device and
hg_scan_device_invert alternate in one process on one scanner; per call the host wall time around the blocking call, the
scan's own ms_total (HIP events, the same launches in both) and, for inverted calls, the stage's time (invert_us: HIP events
around its count launch, scan and write launch, with the one host synchronisation between them that sizes the output).
--lib: another build of the library (hypergrep_amd/build.py HG_BUILD_OUT), e.g. one of the parent commit, which has no
inverted scan: then only hg_scan_device is timed, on the same text and sets.  Runs of the two builds are alternated by the
caller, one process each (a process loads one library).
The stage's traffic bound: one read of the text plus 32 bytes written per selected piece, at the HBM read rate of
profiles/r03_bw_ceiling.txt (default loads, as the stage uses).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_READ_GBPS = 6645.8  # profiles/r03_bw_ceiling.txt: default loads, best occupancy


def main() -> None:
    import torch

    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="", help="append the report to this file")
    ap.add_argument("--lib", default="", help="scan with this build of the library instead of the package's")
    args = ap.parse_args()
    if args.lib:
        import hypergrep_amd

        hypergrep_amd.configure_libraries(libhs=os.path.abspath(args.lib))
    if not torch.cuda.is_available():
        raise SystemExit("invert_bench needs a GPU: there is nothing to measure without one")
    nbytes = int(args.gib * (1 << 30))
    pats, needles, _hpm = benchspec.c3_spec()
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    device.synth_device(text.data_ptr(), nbytes, seed=17, needles=needles, hit_per_million=1000)
    torch.cuda.synchronize()
    can_invert = hasattr(device.lib(), "hg_scan_device_invert")
    lines = [f"# tools/invert_bench.py --gib {args.gib} --reps {args.reps}{' --lib ' + args.lib if args.lib else ''}: {nbytes} bytes of config-3 text, hit rate 1e-3, one MI355X",
             "# per call: host wall ms (median / min) and the scan's ms_total (median); invert stage: invert_us (median), HIP events",
             f"# bound = (text bytes + 32 B x selected pieces) / {HBM_READ_GBPS} GB/s (profiles/r03_bw_ceiling.txt, default loads)"]
    sets = (("config 3, 1e-3 of the lines match", pats, [14] * len(pats)), ("config 3 + an expression every line matches", pats + ["^."], [14] * len(pats) + [14]))
    for name, p, flags in sets:
        sc = device.Scanner(device.Database(p, flags=flags, ids=list(range(len(p)))), 0)
        modes = (False, True) if can_invert else (False,)
        for inv in modes + modes:  # warm-up: workspace sizing, the stage's buffers
            sc.scan(text.data_ptr(), nbytes, invert=inv)
        wall = {False: [], True: []}
        total = {False: [], True: []}
        stage = []
        last = {}
        for _ in range(args.reps):
            for inv in modes:
                t0 = time.perf_counter()
                st = sc.scan(text.data_ptr(), nbytes, invert=inv)
                wall[inv].append((time.perf_counter() - t0) * 1e3)
                total[inv].append(st.ms_total)
                last[inv] = st
                if inv:
                    stage.append(st.invert_us / 1e3)
        med = statistics.median
        if not can_invert:
            lines += [f"{name}: {len(p)} expressions, {last[False].n_lines} lines, {last[False].n_hits} hits",
                      f"  hg_scan_device         wall {med(wall[False]):8.3f} / {min(wall[False]):8.3f} ms   ms_total {med(total[False]):8.3f}"]
            del sc
            continue
        selected, n_lines = last[True].n_hits, last[True].n_lines
        bound_ms = (nbytes + 32 * selected) / (HBM_READ_GBPS * 1e9) * 1e3
        stage_ms = med(stage)
        lines += [
            f"{name}: {len(p)} expressions, {n_lines} lines, {last[False].n_hits} hits, {selected} selected",
            f"  hg_scan_device         wall {med(wall[False]):8.3f} / {min(wall[False]):8.3f} ms   ms_total {med(total[False]):8.3f}",
            f"  hg_scan_device_invert  wall {med(wall[True]):8.3f} / {min(wall[True]):8.3f} ms   ms_total {med(total[True]):8.3f}   invert stage {stage_ms:8.3f} ms (min {min(stage):.3f})",
            f"  traffic bound of the stage {bound_ms:8.3f} ms; stage / bound = {stage_ms / bound_ms:6.2f}; text rate of the stage {nbytes / stage_ms / 1e6:8.1f} GB/s",
        ]
        del sc
    report = "\n".join(lines) + "\n"
    print(report, end="")
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(report)


if __name__ == "__main__":
    main()
