"""Cost of the segment stage (hg_scan_device_segments, csrc/hg_segments.hip): N files of about S bytes packed into one
resident buffer and scanned once, against the same files scanned one by one.

usage: python tools/segments_bench.py [--reps 7] [--sample 256] [--out FILE]      (the record: profiles/segments_bench.txt)
The text is bench.py's config-3 synthetic log (benchspec.c3_spec, 1e-3 of the lines carry a needle) made on the device and
read back once to place the file boundaries at the line starts nearest to multiples of S.  Shapes: N = 1024 and 16384,
S = 1 KiB, 16 KiB and 256 KiB, as far as N * S fits the 256 MiB a pack of the file path may hold.
Per shape, alternating in one process on one scanner:
  packed    one hg_scan_device_segments call over the whole buffer: host wall time around the blocking call, the scan's own
            ms_total and the stage's segments_us (HIP events; the stage's two host synchronisations included);
  plain     one hg_scan_device call over the same buffer (what the packed call adds to);
  per file  for a sample of the files (--sample, evenly spread): a device-to-device copy of the file to an aligned buffer
            and one hg_scan_device call each, the way a per-file route must scan them; wall time per file, scaled to N.
This measures the RESIDENT stage only.  Nothing here opens, reads or uploads a file, and no line bytes are delivered.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PACK = 256 << 20


def main() -> None:
    import numpy as np
    import torch

    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segments_bench needs a GPU: there is nothing to measure without one")
    pats, needles, _hpm = benchspec.c3_spec()
    sc = device.Scanner(device.Database(pats, ids=list(range(len(pats)))), 0)
    text = torch.empty(PACK + 16, dtype=torch.uint8, device="cuda:0")
    device.synth_device(text.data_ptr(), PACK, seed=23, needles=needles, hit_per_million=1000)
    torch.cuda.synchronize()
    host = text[:PACK].cpu().numpy()
    line_starts = np.concatenate(([0], np.flatnonzero(host == 10) + 1)).astype(np.int64)
    stage_buf = torch.empty((1 << 20) + 16, dtype=torch.uint8, device="cuda:0")
    lines = [f"# tools/segments_bench.py --reps {args.reps} --sample {args.sample}: config-3 text, hit rate 1e-3, one MI355X, buffer_size 262140",
             "# wall: host ms around the blocking call (median / min); ms_total, segments_us: HIP events (median)",
             "# N x S | bytes | packed wall | packed ms_total | segments_us | plain wall | per file wall (sample) | per file x N | packed / (per file x N)"]
    for n_files in (1024, 16384):
        for size in (1 << 10, 16 << 10, 256 << 10):
            if n_files * size > PACK:
                lines.append(f"{n_files} x {size} | does not fit one pack of {PACK} bytes: not measured")
                continue
            wanted = np.arange(n_files + 1, dtype=np.int64) * size
            bounds = line_starts[np.searchsorted(line_starts, wanted, side="right") - 1]
            bounds = np.unique(bounds)  # (a line longer than S would give an empty file: none in this text)
            starts, ends = bounds[:-1].tolist(), bounds[1:].tolist()
            nbytes = int(bounds[-1])
            n = len(starts)
            d_bounds = torch.from_numpy(np.concatenate((bounds[:-1], bounds[1:])).astype(np.uint64).view(np.int64)).to("cuda:0")
            seg = (d_bounds.data_ptr(), d_bounds.data_ptr() + 8 * n, n)
            sample = [int(i) for i in np.linspace(0, n - 1, min(args.sample, n)).astype(np.int64)]
            packed_wall, packed_total, seg_us, plain_wall, file_wall = [], [], [], [], []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                st = sc.scan(text.data_ptr(), nbytes, segments=seg)
                t1 = time.perf_counter()
                n_packed = st.n_hits
                plain = sc.scan(text.data_ptr(), nbytes)
                t2 = time.perf_counter()
                found = 0
                for i in sample:
                    ln = ends[i] - starts[i]
                    stage_buf[:ln].copy_(text[starts[i]:ends[i]])
                    found += sc.scan(stage_buf.data_ptr(), ln).n_hits
                t3 = time.perf_counter()
                if rep == 0:  # warm-up (workspace growth, first launches)
                    assert n_packed == plain.n_hits, (n_packed, plain.n_hits)  # no pad in this text: every record survives
                    continue
                packed_wall.append((t1 - t0) * 1e3)
                packed_total.append(st.ms_total)
                seg_us.append(st.segments_us)
                plain_wall.append((t2 - t1) * 1e3)
                file_wall.append((t3 - t2) * 1e3 / len(sample))
            med = statistics.median
            loop_ms = med(file_wall) * n
            lines.append(f"{n} x {size} | {nbytes} | {med(packed_wall):.3f} / {min(packed_wall):.3f} ms | {med(packed_total):.3f} ms | {med(seg_us):.0f} us | "
                         f"{med(plain_wall):.3f} / {min(plain_wall):.3f} ms | {med(file_wall):.4f} ms ({len(sample)} files) | {loop_ms:.1f} ms | {med(packed_wall) / loop_ms:.4f}")
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(report)


if __name__ == "__main__":
    main()
