"""Cost of the start-of-match pass (HS_FLAG_SOM_LEFTMOST, hg_som.hip) on synthetic text resident in HBM.

usage: python tools/som_bench.py [--gib 1] [--reps 5]
Two sets: literal-anchored (benchspec config 3's literal expressions, about 1 % of lines hit) and always-on (short class
expressions with no usable literal).  For each: the whole scan (hg_scan_device, wall time and ms_total) with and without
the flag, and the match span per hit (to - from, computed on the host from the hits): the walk reads at least that many
bytes per hit, and at most up to the expression's max_len.  The kernel time itself: run this under
rocprofv3 --kernel-trace --stats (hg_som_kernel).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOM = 256
ALWAYS_ON = [r"[0-9]{3}x", r"a[b-d]{2}e", r"\b[a-c]{2}_[0-9]\b", r"([a-f][0-9]){6}"]


def main() -> None:
    import numpy as np
    import torch

    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    nbytes = int(args.gib * (1 << 30))
    pats3, needles, hpm = benchspec.c3_spec()
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    device.synth_device(text.data_ptr(), nbytes, seed=17, needles=needles, hit_per_million=hpm)
    torch.cuda.synchronize()
    sets = {"anchored": pats3[:192], "always_on": ALWAYS_ON}
    for name, pats in sets.items():
        ids = list(range(len(pats)))
        for flag in (0, SOM):
            sc = device.Scanner(device.Database(pats, flags=[6 | flag] * len(pats), ids=ids), 0)
            st = sc.scan(text.data_ptr(), nbytes)  # warm-up (workspace sizing)
            walls, totals = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                st = sc.scan(text.data_ptr(), nbytes)
                walls.append((time.perf_counter() - t0) * 1e3)
                totals.append(st.ms_total)
            line = f"{name:9s} flag={flag:3d} hits={st.n_hits:9d} lines={st.n_lines:9d} wall_ms(min/med)={min(walls):8.2f}/{sorted(walls)[len(walls) // 2]:8.2f}"
            if flag:
                hits = sc.hits_array()
                starts = sc.hit_starts().astype(np.int64)
                span = hits[:, 2].astype(np.int64) - starts
                line += f" span_per_hit(mean/max)={span.mean():.2f}/{span.max()}"
            print(line, flush=True)
            del sc


if __name__ == "__main__":
    main()
