"""Cost of matched parts in many-file scans (hg_scan_device_segments_parts, csrc/hg_segparts.hip), resident and end to end.

usage: python tools/segparts_bench.py [--reps 7] [--file-reps 3] [--shapes 1024x1024,...] [--skip-files] [--out FILE]
(the record: profiles/segparts_bench.txt)
Shapes: N files of about S bytes, default 1024 x 1 KiB, 1024 x 16 KiB, 16384 x 1 KiB and 1024 x 256 KiB.  Sets: one literal,
and the first 64 expressions of config 3 (literals); the needles are the sets' own literals.  Needle rates per line: 1e-3 and 0.1.
Resident (tools/segments_bench.py's text and boundaries; nothing is read, uploaded or delivered), alternating in one process
on one scanner, medians of --reps:
  packed  hg_scan_device_segments_parts: segments_us and parts_us (the new stage: count, scan, write, offsets, two host
          synchronisations), host wall time around the blocking call;
  plain   hg_scan_device_parts over the SAME buffer without segments: its parts_us.  The existing stage is the yardstick: it
          walks the same pieces (the pads aside) and writes the same parts.
End to end (tools/manyfiles_bench.py's files), alternating in one process, median and minimum of --file-reps:
  grep_files(files, patterns, matched_parts=True) against [grep(f, patterns, matched_parts=True) for f in files], the route
  matched parts took before the batch route offered them; the two results are compared.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PACK = 256 << 20
RATES = (1000, 100000)  # needle lines per million: 1e-3 and 0.1


def emit(lines, line) -> None:
    """One line of the report: shown at once (a long run stays visibly alive), kept for --out."""
    lines.append(line)
    print(line, flush=True)


def sets():
    from hypergrep_amd import benchspec

    pats, _needles, _hpm = benchspec.c3_spec()
    return (("1 literal", pats[:1]), ("64 of config 3", pats[:64]))


def resident(shapes, reps, lines) -> None:
    import numpy as np
    import torch

    from hypergrep_amd import device

    emit(lines, "# resident: set | rate | N x S | bytes | records / parts | packed: segments_us, parts_us, wall ms | plain (no segments): parts_us, parts | "
         "packed parts_us / plain parts_us")
    text = torch.empty(PACK + 16, dtype=torch.uint8, device="cuda:0")
    for name, pats in sets():
        sc = device.Scanner(device.Database(pats, ids=list(range(len(pats)))), 0)
        for rate in RATES:
            device.synth_device(text.data_ptr(), PACK, seed=23, needles=[p.encode() for p in pats], hit_per_million=rate)
            torch.cuda.synchronize()
            host = text[:PACK].cpu().numpy()
            line_starts = np.concatenate(([0], np.flatnonzero(host == 10) + 1)).astype(np.int64)
            for n_files, size in shapes:
                if n_files * size > PACK:
                    emit(lines, f"{name} | {rate / 1e6:g} | {n_files} x {size} | does not fit one pack of {PACK} bytes: not measured")
                    continue
                wanted = np.arange(n_files + 1, dtype=np.int64) * size
                bounds = np.unique(line_starts[np.searchsorted(line_starts, wanted, side="right") - 1])
                nbytes, n = int(bounds[-1]), len(bounds) - 1
                d_bounds = torch.from_numpy(np.concatenate((bounds[:-1], bounds[1:])).astype(np.uint64).view(np.int64)).to("cuda:0")
                seg = (d_bounds.data_ptr(), d_bounds.data_ptr() + 8 * n, n)
                seg_us, packed_us, wall, plain_us = [], [], [], []
                for rep in range(reps + 1):
                    t0 = time.perf_counter()
                    b = sc.scan(text.data_ptr(), nbytes, segments=seg, segment_parts=True)
                    t1 = time.perf_counter()
                    c = sc.scan(text.data_ptr(), nbytes, parts=True)
                    if rep == 0:  # warm-up (workspace growth, first launches)
                        assert b.n_hits == c.n_hits and b.n_parts == c.n_parts > 0
                        continue
                    seg_us.append(b.segments_us)
                    packed_us.append(b.parts_us)
                    wall.append((t1 - t0) * 1e3)
                    plain_us.append(c.parts_us)
                med = statistics.median
                emit(lines, f"{name} | {rate / 1e6:g} | {n} x {size} | {nbytes} | {b.n_hits} / {b.n_parts} | {med(seg_us):.0f} us, {med(packed_us):.0f} us, {med(wall):.3f} ms | "
                     f"{med(plain_us):.0f} us, {c.n_parts} | {med(packed_us) / max(med(plain_us), 1):.2f}")


def end_to_end(shapes, reps, lines) -> None:
    import hypergrep_amd
    from hypergrep_amd import device

    emit(lines, "# end to end: set | rate | N x S | grep_files matched_parts wall ms (median / min) | loop over grep() matched_parts wall ms (median / min / max) | loop / grep_files")
    for name, pats in sets():
        for rate in RATES:
            for n_files, size in shapes:
                with tempfile.TemporaryDirectory() as root:
                    text = device.synth_host(n_files * size + 4096, 29, [p.encode() for p in pats], rate)
                    files, pos = [], 0
                    for i in range(n_files):
                        end = text.find(b"\n", pos + size - 1)
                        end = len(text) if end < 0 else end + 1
                        os.makedirs(os.path.join(root, f"{i % 64:02d}"), exist_ok=True)
                        path = os.path.join(root, f"{i % 64:02d}", f"f{i:06d}.log")
                        with open(path, "wb") as handle:
                            handle.write(text[pos:end])
                        files.append(path)
                        pos = end
                    batch, loop = [], []
                    for rep in range(reps + 1):
                        t0 = time.perf_counter()
                        got = hypergrep_amd.grep_files(files, pats, matched_parts=True)
                        t1 = time.perf_counter()
                        want = [hypergrep_amd.grep(f, pats, matched_parts=True) for f in files]
                        t2 = time.perf_counter()
                        assert got == want
                        if rep:
                            batch.append((t1 - t0) * 1e3)
                            loop.append((t2 - t1) * 1e3)
                    med = statistics.median
                    emit(lines, f"{name} | {rate / 1e6:g} | {n_files} x {size} | {med(batch):.1f} / {min(batch):.1f} | {med(loop):.1f} / {min(loop):.1f} / {max(loop):.1f} | "
                         f"{med(loop) / med(batch):.2f}")


def main() -> None:
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1024,1024x16384,16384x1024,1024x262144")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--file-reps", type=int, default=3)
    ap.add_argument("--skip-files", action="store_true", help="the resident part only")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segparts_bench needs a GPU: there is nothing to measure without one")
    shapes = [tuple(int(v) for v in shape.split("x")) for shape in args.shapes.split(",")]
    lines = []
    emit(lines, f"# tools/segparts_bench.py --shapes {args.shapes} --reps {args.reps} --file-reps {args.file_reps}: one MI355X, buffer_size 262140")
    resident(shapes, args.reps, lines)
    if not args.skip_files:
        end_to_end(shapes, args.file_reps, lines)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
