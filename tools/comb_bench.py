"""Cost of the combination pass (HS_FLAG_COMBINATION / HS_FLAG_QUIET, hg_comb.hip) on synthetic text resident in HBM.

usage: python tools/comb_bench.py [--gib 1] [--reps 5]
Two sets of 8 sub-expressions (report ids 0..7) and 4 combinations over them (ids 100..103):
  low:  benchspec config 3's 192 literal expressions, id = index % 8 (about 1 % of lines hit);
  high: ^[^\\n]{k}, k = 1..8: every line of at least k bytes reports id k - 1 once (about 100 % of lines hit).
Grep's flags (DOTALL | MULTILINE | SINGLEMATCH), the combinations with SINGLEMATCH.  For each: the whole scan (wall time,
ms_total) of the sub-expressions alone ("plain"), and of the set with the sub-expressions QUIET plus the 4 combinations
("comb").  The kernels themselves: run this under
rocprofv3 --kernel-trace --stats (hg_comb_kernel, the rocprim scan and the compact finalize it feeds).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COMB, QUIET = 512, 1024
FORMULAS = ["0 & 1", "2 & !3", "(4 | 5) & !6", "7 | 0 & 2"]


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
    sets = {"low": pats3[:192], "high": [f"^[^\\n]{{{k}}}" for k in range(1, 9)]}
    for name, subs in sets.items():
        ids = [i % 8 for i in range(len(subs))]
        variants = {
            "plain": (subs, [14] * len(subs), ids),
            "comb": (subs + FORMULAS, [14 | QUIET] * len(subs) + [COMB | 8] * len(FORMULAS), ids + [100 + k for k in range(len(FORMULAS))]),
        }
        for label, (pats, flags, all_ids) in variants.items():
            sc = device.Scanner(device.Database(pats, flags=flags, ids=all_ids), 0)
            st = sc.scan(text.data_ptr(), nbytes)  # warm-up (workspace sizing)
            walls, totals = [], []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = sc.scan(text.data_ptr(), nbytes)
                walls.append((time.perf_counter() - t0) * 1e3)
                totals.append(st.ms_total)
            lines_hit = np.unique(sc.hits_array()[:, 0]).size if st.n_hits and label == "comb" else 0  # (lines with a delivered report)
            print(f"{name:4s} {label:5s} raw={st.n_raw_hits:10d} delivered={st.n_hits:10d} lines={st.n_lines:9d} lines_hit={lines_hit / max(st.n_lines, 1) * 100:6.2f}% "
                  f"wall_ms(min/med)={min(walls):8.2f}/{sorted(walls)[len(walls) // 2]:8.2f} ms_total(min)={min(totals):8.2f}", flush=True)
            del sc


if __name__ == "__main__":
    main()
