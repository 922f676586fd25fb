"""grep over many small files: grep_files() (one native call, small files packed into one GPU scan) against the loop over
grep(), end to end: open, read, upload, scan, result copy, delivery into Python.

usage: python tools/manyfiles_bench.py [--shapes 1024x1024,1024x16384,...] [--reps 3] [--out FILE]
(the record: profiles/manyfiles_bench.txt)
Writes N files of S bytes each (hg_synth_host's config-3 log, hit rate 1e-3, cut at line ends) into a temporary directory and
times, alternating in one process, grep_files(files, patterns) and [grep(f, patterns) for f in files], with count_only and
with delivered lines.  Per shape it also reports, for one pack scanned through Scanner.scan(segments=...), the stage's
segments_us against the scan's ms_total.  Default shapes: N = 1024 and 16384 with S = 1 KiB, 16 KiB and 256 KiB.
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


def main() -> None:
    import torch

    import hypergrep_amd
    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1024,1024x16384,1024x262144,16384x1024,16384x16384,16384x262144")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("manyfiles_bench needs a GPU: there is nothing to measure without one")
    pats, needles, _hpm = benchspec.c3_spec()
    pats = pats[:64]
    lines = [f"# tools/manyfiles_bench.py --shapes {args.shapes} --reps {args.reps}: {len(pats)} expressions of config 3, hit rate 1e-3, one MI355X",
             "# N x S | mode | grep_files wall ms (median / min) | loop over grep() wall ms (median / min) | loop / grep_files | one pack: segments_us / ms_total"]
    for shape in args.shapes.split(","):
        n_files, size = (int(v) for v in shape.split("x"))
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
            packed = text[:min(pos, PACK)]
            packed = packed[:packed.rfind(b"\n") + 1]
            d_text = torch.frombuffer(bytearray(packed + b"\0" * 16), dtype=torch.uint8).to("cuda:0")
            sc = device.Scanner(device.Database(pats), 0)
            cuts = [0]
            while cuts[-1] < len(packed):
                nl = packed.find(b"\n", min(cuts[-1] + size - 1, len(packed) - 1))
                cuts.append(nl + 1)
            stage = []
            for _ in range(args.reps + 1):
                st = sc.scan(d_text.data_ptr(), len(packed), segments=(cuts[:-1], cuts[1:]))
                stage.append((st.segments_us, st.ms_total))
            seg_us, ms_total = statistics.median(s[0] for s in stage[1:]), statistics.median(s[1] for s in stage[1:])
            del sc
            for mode, kwargs in (("count_only", {"count_only": True}), ("lines", {})):
                batch, loop = [], []
                for rep in range(args.reps + 1):
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
                lines.append(f"{n_files} x {size} | {mode} | {med(batch):.1f} / {min(batch):.1f} | {med(loop):.1f} / {min(loop):.1f} | {med(loop) / med(batch):.2f} | "
                             f"{seg_us:.0f} us / {ms_total:.3f} ms")
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(report)


if __name__ == "__main__":
    main()
