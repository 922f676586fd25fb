#!/usr/bin/env python3
"""Batched block scan on the GPU (hg_scan_blocks) against the two routes that exist without it.

    python tools/block_batch_bench.py [--rounds N] [--legs A,B,C] [--lib PATH] [--only SET,BYTES,ITEMS]

One process, the legs alternated round by round, one line per measurement.  Reports are not delivered to Python (NULL
callback), so the numbers are the library's.
  leg A  a loop of hs_scan over the items (the baseline)
  leg B  hg_scan_stream_batch on a stream-mode twin with HG_STREAM_ITEM_LAST on every item
  leg C  hg_scan_blocks
Grid: the 4-expression and 256-expression sets of tools/stream_bench.py; items of 64 B, 256 B, 4 KiB; batches of 1, 64, 1024
and 16384.  --lib: another build of the library (--legs A with a build of the parent commit records the baseline's code
path before this change).
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hypergrep_amd import device  # noqa: E402
from stream_bench import sets, text  # noqa: E402

SIZES = (64, 256, 4096)
COUNTS = (1, 64, 1024, 16384)


def reps_for(n: int, size: int, leg: str) -> int:
    if leg == "A":  # (leg_a sizes its own loop from a timed warm-up: 256 expressions on 4 KiB cost milliseconds per call)
        return 0
    return max(2, min(50, (8 << 20) // (n * size)))


class Block:
    def __init__(self, pats, flags):
        self.h, err = device.hs_compile(pats, flags, list(range(len(pats))), None, device.HS_MODE_BLOCK)
        assert err is None, err
        self.scratch = ctypes.c_void_p()
        assert device.face_a().hs_alloc_scratch(self.h, ctypes.byref(self.scratch)) == 0


def leg_a(blk, data, la, n, reps):
    l = device.face_a()
    cb = device.MATCH_EVENT()
    t0 = time.perf_counter()
    for d in data[:4]:
        assert l.hs_scan(blk.h, d, len(d), 0, blk.scratch, cb, None) == 0
    per_item = (time.perf_counter() - t0) / min(4, n)
    reps = max(1, min(200, int(0.4 / (per_item * n))))  # about 0.4 s per measurement, one pass over the items at least
    t0 = time.perf_counter()
    for _ in range(reps):
        for d in data:
            l.hs_scan(blk.h, d, len(d), 0, blk.scratch, cb, None)
    return (time.perf_counter() - t0) / reps


def leg_b(sdb, streams, da, la, n, reps):
    l = device.face_a()
    sa = (ctypes.c_void_p * n)(*[s._h for s in streams[:n]])
    last = (ctypes.c_uint * n)(*[device.HG_STREAM_ITEM_LAST] * n)
    cb = device.STREAM_EVENT()
    for _ in range(2):
        assert l.hg_scan_stream_batch(sa, da, la, last, n, sdb._scratch, cb, None) == 0
    t0 = time.perf_counter()
    for _ in range(reps):
        assert l.hg_scan_stream_batch(sa, da, la, last, n, sdb._scratch, cb, None) == 0
    return (time.perf_counter() - t0) / reps


def leg_c(blk, da, la, n, reps):
    l = device.face_a()
    cb = device.STREAM_EVENT()
    for _ in range(2):
        assert l.hg_scan_blocks(blk.h, da, la, n, blk.scratch, cb, None) == 0
    t0 = time.perf_counter()
    for _ in range(reps):
        assert l.hg_scan_blocks(blk.h, da, la, n, blk.scratch, cb, None) == 0
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--legs", default="A,B,C")
    ap.add_argument("--lib", help="another build of libhyperscanner.so")
    ap.add_argument("--only", help="one cell of the grid: SET,BYTES,ITEMS (e.g. 256expr,4096,16384; for a kernel trace)")
    args = ap.parse_args()
    legs = args.legs.split(",")
    import torch  # noqa: F401  (one HIP runtime: torch's)

    if args.lib:
        import hypergrep_amd

        hypergrep_amd.configure_libraries(libhs=os.path.abspath(args.lib))
    print(f"device: {torch.cuda.get_device_name(0)} lib: {args.lib or 'this build'} legs: {','.join(legs)}", flush=True)
    only = args.only.split(",") if args.only else None
    for name, (pats, flags) in sets().items():
        if only and name != only[0]:
            continue
        blk = Block(pats, flags)
        sdb = device.StreamDatabase(pats, flags, list(range(len(pats)))) if "B" in legs else None
        streams = [sdb.open() for _ in range(max(COUNTS))] if sdb else []
        for size in SIZES:
            for n in COUNTS:
                if only and (size, n) != (int(only[1]), int(only[2])):
                    continue
                data = [text(size, seed=i % 64) for i in range(n)]
                da = (ctypes.c_char_p * n)(*data)
                la = (ctypes.c_uint * n)(*[size] * n)
                for r in range(args.rounds):
                    for leg in legs:
                        reps = reps_for(n, size, leg)
                        dt = leg_a(blk, data, la, n, reps) if leg == "A" else leg_b(sdb, streams, da, la, n, reps) if leg == "B" else leg_c(blk, da, la, n, reps)
                        print(f"set={name} bytes={size} items={n} round={r} leg={leg} ms_per_call={dt * 1e3:.3f} us_per_item={dt * 1e6 / n:.3f} "
                              f"items/s={n / dt:.0f} MiB/s={n * size / dt / 2**20:.1f}", flush=True)
        for s in streams:
            s.close()


if __name__ == "__main__":
    main()
