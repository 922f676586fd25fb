"""Cost of context lines in many-file scans (hg_scan_device_segments_context, csrc/hg_segctx.hip), resident and end to end.

usage: python tools/segctx_bench.py [--reps 7] [--file-reps 3] [--shapes 1024x1024,...] [--skip-files] [--out FILE]
(the record: profiles/segctx_bench.txt)
Shapes: N files of about S bytes, default 1024 x 1 KiB, 1024 x 16 KiB, 16384 x 1 KiB and 1024 x 256 KiB; config 3's expressions,
hit rate 1e-3, before = after = 2 (-C2).
Resident (tools/segments_bench.py's text and boundaries; nothing is read, uploaded or delivered), alternating in one process
on one scanner, medians of --reps:
  segments   hg_scan_device_segments: the stage's segments_us;
  packed -C2 hg_scan_device_segments_context: segments_us and context_us (the new stage: its launches, scan and two host
             synchronisations), host wall time around the blocking call;
  plain -C2  hg_scan_device_context over the SAME buffer without segments: its context_us.  An existing stage, the baseline for
             what the windows cost: it writes nearly the same records (context may cross the boundaries there).
End to end (tools/manyfiles_bench.py's files, 64 expressions), alternating in one process, medians of --file-reps:
  grep_files(files, patterns, before_context=2, after_context=2) against [grep(f, ...) for f in files], the route context took
  before the batch route offered it; the two results are compared.
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


def resident(shapes, reps, lines) -> None:
    import numpy as np
    import torch

    from hypergrep_amd import benchspec, device

    pats, needles, _hpm = benchspec.c3_spec()
    sc = device.Scanner(device.Database(pats, ids=list(range(len(pats)))), 0)
    text = torch.empty(PACK + 16, dtype=torch.uint8, device="cuda:0")
    device.synth_device(text.data_ptr(), PACK, seed=23, needles=needles, hit_per_million=1000)
    torch.cuda.synchronize()
    host = text[:PACK].cpu().numpy()
    line_starts = np.concatenate(([0], np.flatnonzero(host == 10) + 1)).astype(np.int64)
    lines += ["# resident: N x S | bytes | records / context records | segments_us (no context) | packed -C2: segments_us, context_us, wall ms | "
              "plain -C2 (no segments): context_us, context records | packed context_us / plain context_us"]
    for n_files, size in shapes:
        if n_files * size > PACK:
            lines.append(f"{n_files} x {size} | does not fit one pack of {PACK} bytes: not measured")
            continue
        wanted = np.arange(n_files + 1, dtype=np.int64) * size
        bounds = np.unique(line_starts[np.searchsorted(line_starts, wanted, side="right") - 1])
        nbytes, n = int(bounds[-1]), len(bounds) - 1
        d_bounds = torch.from_numpy(np.concatenate((bounds[:-1], bounds[1:])).astype(np.uint64).view(np.int64)).to("cuda:0")
        seg = (d_bounds.data_ptr(), d_bounds.data_ptr() + 8 * n, n)
        seg_only, seg_ctx, ctx_us, wall, plain_us = [], [], [], [], []
        for rep in range(reps + 1):
            a = sc.scan(text.data_ptr(), nbytes, segments=seg)
            t0 = time.perf_counter()
            b = sc.scan(text.data_ptr(), nbytes, segments=seg, context=(2, 2))
            t1 = time.perf_counter()
            c = sc.scan(text.data_ptr(), nbytes, context=(2, 2))
            if rep == 0:  # warm-up (workspace growth, first launches)
                assert a.n_hits == b.n_hits == c.n_hits and 0 < b.n_context <= c.n_context
                continue
            seg_only.append(a.segments_us)
            seg_ctx.append(b.segments_us)
            ctx_us.append(b.context_us)
            wall.append((t1 - t0) * 1e3)
            plain_us.append(c.context_us)
        med = statistics.median
        lines.append(f"{n} x {size} | {nbytes} | {b.n_hits} / {b.n_context} | {med(seg_only):.0f} us | {med(seg_ctx):.0f} us, {med(ctx_us):.0f} us, {med(wall):.3f} ms | "
                     f"{med(plain_us):.0f} us, {c.n_context} | {med(ctx_us) / max(med(plain_us), 1):.2f}")


def end_to_end(shapes, reps, lines) -> None:
    import hypergrep_amd
    from hypergrep_amd import benchspec, device

    pats, needles, _hpm = benchspec.c3_spec()
    pats = pats[:64]
    kwargs = {"before_context": 2, "after_context": 2}
    lines += [f"# end to end: {len(pats)} expressions | N x S | grep_files -C2 wall ms (median / min) | loop over grep() -C2 wall ms (median / min) | loop / grep_files"]
    for n_files, size in shapes:
        with tempfile.TemporaryDirectory() as root:
            text = device.synth_host(n_files * size + 4096, 29, needles, 1000)
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
                got = hypergrep_amd.grep_files(files, pats, **kwargs)
                t1 = time.perf_counter()
                want = [hypergrep_amd.grep(f, pats, **kwargs) for f in files]
                t2 = time.perf_counter()
                assert got == want
                if rep:
                    batch.append((t1 - t0) * 1e3)
                    loop.append((t2 - t1) * 1e3)
            med = statistics.median
            lines.append(f"{n_files} x {size} | {med(batch):.1f} / {min(batch):.1f} | {med(loop):.1f} / {min(loop):.1f} | {med(loop) / med(batch):.2f}")


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
        raise SystemExit("segctx_bench needs a GPU: there is nothing to measure without one")
    shapes = [tuple(int(v) for v in shape.split("x")) for shape in args.shapes.split(",")]
    lines = [f"# tools/segctx_bench.py --shapes {args.shapes} --reps {args.reps} --file-reps {args.file_reps}: config 3, hit rate 1e-3, -C2, one MI355X, buffer_size 262140"]
    resident(shapes, args.reps, lines)
    if not args.skip_files:
        end_to_end(shapes, args.file_reps, lines)
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(report)


if __name__ == "__main__":
    main()
