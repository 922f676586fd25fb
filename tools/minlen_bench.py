"""Cost of the match-length pass (hs_expr_ext_t min_length, hg_minlen_kernel in hg_som.hip) on synthetic text resident in HBM.

usage: python tools/minlen_bench.py [--gib 1] [--reps 5]
Two sets of variable-width expressions: literal-anchored (benchspec config 3's class expressions of variable width) and
always-on (short class expressions with no usable literal).  For each: the whole scan (hg_scan_device wall time) plain,
with a min_length on every expression, and with HS_FLAG_SOM_LEFTMOST instead (the start-of-match pass on the same set, for
comparison), with the raw reports (n_raw_hits: what the match-length pass walks) and the delivered ones.  The kernel times
themselves: run this under rocprofv3 --kernel-trace --stats (hg_minlen_kernel, hg_som_kernel) and divide by the counts.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOM = 256
# (expression, min_length): above the shortest match, at most the longest
ALWAYS_ON = [(r"[0-9]{2,4}x", 4), (r"a[b-d]{1,3}e", 4), (r"\b[a-c]{1,3}_[0-9]\b", 4), (r"([a-f][0-9]){4,6}", 10)]
ANCHORED_LENGTHS = {"user=": 25, "retry_": 32, "blk_": 16}  # config 3's variable-width families, by their first bytes


def main() -> None:
    import torch

    from hypergrep_amd import benchspec, device, utils

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    nbytes = int(args.gib * (1 << 30))
    pats3, needles, hpm = benchspec.c3_spec()
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    device.synth_device(text.data_ptr(), nbytes, seed=17, needles=needles, hit_per_million=hpm)
    torch.cuda.synchronize()
    anchored = [(p, n) for p in pats3 for k, n in ANCHORED_LENGTHS.items() if p.startswith(k)]
    for name, pairs in (("anchored", anchored), ("always_on", ALWAYS_ON)):
        pats = [p for p, _ in pairs]
        ids = list(range(len(pats)))
        exts = [utils.ExprExt(flags=utils.HS_EXT_FLAG_MIN_LENGTH, min_length=n) for _, n in pairs]
        for mode, flag, ext in (("plain", 0, None), ("min_length", 0, exts), ("som", SOM, None)):
            sc = device.Scanner(device.Database(pats, flags=[6 | flag] * len(pats), ids=ids, ext=ext), 0)
            st = sc.scan(text.data_ptr(), nbytes)  # warm-up (workspace sizing)
            walls = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                st = sc.scan(text.data_ptr(), nbytes)
                walls.append((time.perf_counter() - t0) * 1e3)
            print(f"{name:9s} {mode:10s} exprs={len(pats):3d} raw={st.n_raw_hits:9d} hits={st.n_hits:9d} lines={st.n_lines:9d} "
                  f"wall_ms(min/med)={min(walls):8.2f}/{sorted(walls)[len(walls) // 2]:8.2f}", flush=True)
            del sc


if __name__ == "__main__":
    main()
