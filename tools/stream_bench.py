#!/usr/bin/env python3
"""Stream mode on the GPU (hs_scan_stream / hg_scan_stream_batch): per-call latency, batch throughput and the HBM cut-off.

    python tools/stream_bench.py [--quick] [--lib PATH] [--hbm-child MODE]
    python tools/stream_bench.py --som [--rounds N]

Prints one line per measurement.  Reports are not delivered to Python (NULL callback), so the numbers are the library's.
--lib: another build of the library (e.g. one of the parent commit), as tools/block_batch_bench.py's.
The HBM cut-off (HG_FLOW_HBM_MIN: bytes x workgroups per item from which a launch's writes are copied to HBM first) is
measured by running the batch legs in child processes with the copy always on (0) and always off (2^62).
--som: the 4-expression set without the SOM flag and with it (horizons LARGE and SMALL), alternated round by round in one
process: hs_scan_stream on a 64-byte and on a 1 MiB write, batches of 1024 and 16384 streams with 256 B and 4 KiB writes.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from hypergrep_amd import benchspec, device  # noqa: E402

FOUR = (["foobar", r"\bstatus=5[0-9][0-9]\b", "err(or)?$", "user=[a-z]+"], [0, 0, 4, 1])


def text(n: int, seed: int = 1) -> bytes:
    import random

    rng = random.Random(seed)
    words = [b"alpha", b"beta", b"status=200", b"status=503", b"user=bob", b"error", b"foobar", b"x", b"\n"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
    return bytes(out[:n])


def latency(sdb, size: int, reps: int) -> float:
    l = device.face_a()
    s = sdb.open()
    data = text(size)
    cb = device.MATCH_EVENT()
    for _ in range(3):
        l.hs_scan_stream(s._h, data, len(data), 0, sdb._scratch, cb, None)
    t0 = time.perf_counter()
    for _ in range(reps):
        l.hs_scan_stream(s._h, data, len(data), 0, sdb._scratch, cb, None)
    dt = (time.perf_counter() - t0) / reps
    s.close()
    return dt


def batch(sdb, nstreams: int, size: int, reps: int) -> float:
    l = device.face_a()
    streams = [sdb.open() for _ in range(nstreams)]
    data = [text(size, seed=i % 64) for i in range(nstreams)]
    sa = (ctypes.c_void_p * nstreams)(*[s._h for s in streams])
    da = (ctypes.c_char_p * nstreams)(*data)
    la = (ctypes.c_uint * nstreams)(*[size] * nstreams)
    cb = device.STREAM_EVENT()
    for _ in range(2):
        assert l.hg_scan_stream_batch(sa, da, la, None, nstreams, sdb._scratch, cb, None) == 0
    t0 = time.perf_counter()
    for _ in range(reps):
        assert l.hg_scan_stream_batch(sa, da, la, None, nstreams, sdb._scratch, cb, None) == 0
    dt = (time.perf_counter() - t0) / reps
    for s in streams:
        s.close()
    return dt


def sets():
    pats, _, _ = benchspec.c3_spec()
    return {"4expr": FOUR, "256expr": (list(pats), [0] * len(pats))}


def run_batches(quick: bool, only=None):
    for name, (pats, flags) in sets().items():
        if only and name not in only:
            continue
        sdb = device.StreamDatabase(pats, flags, list(range(len(pats))))
        counts = [1, 64, 1024, 16384] if quick else [1, 16, 256, 1024, 4096, 16384]
        for size in (256, 4096):
            for n in counts:
                if n * size > (64 << 20):
                    continue
                reps = max(2, min(50, (8 << 20) // (n * size)))
                dt = batch(sdb, n, size, reps)
                print(f"batch set={name} streams={n} bytes={size} ms_per_call={dt * 1e3:.3f} MiB/s={n * size / dt / 2**20:.1f} "
                      f"writes/s={n / dt:.0f}", flush=True)


def run_som(rounds: int):
    pats, flags = FOUR
    ids = list(range(len(pats)))
    dbs = {"plain": device.StreamDatabase(pats, flags, ids),
           "som_large": device.StreamDatabase(pats, [f | 256 for f in flags], ids, som_horizon="large"),
           "som_small": device.StreamDatabase(pats, [f | 256 for f in flags], ids, som_horizon="small")}
    for r in range(rounds):
        for name, sdb in dbs.items():
            for size, reps in ((64, 200), (1 << 20, 3)):
                dt = latency(sdb, size, reps)
                print(f"som round={r} db={name} latency write={size} us_per_call={dt * 1e6:.1f}", flush=True)
            for n in (1024, 16384):
                for size in (256, 4096):
                    reps = max(2, min(20, (8 << 20) // (n * size)))
                    dt = batch(sdb, n, size, reps)
                    print(f"som round={r} db={name} batch streams={n} bytes={size} ms_per_call={dt * 1e3:.3f} "
                          f"MiB/s={n * size / dt / 2**20:.1f} writes/s={n / dt:.0f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--som", action="store_true", help="start of match: plain against SOM LARGE / SMALL, alternated")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--hbm-child", choices=["on", "off"], help="(internal) batch legs with the HBM copy forced on / off")
    ap.add_argument("--lib", help="another build of libhyperscanner.so")
    args = ap.parse_args()
    if args.lib:
        import hypergrep_amd

        hypergrep_amd.configure_libraries(libhs=os.path.abspath(args.lib))
    if args.hbm_child:
        run_batches(True)
        return
    import torch  # noqa: F401  (one HIP runtime: torch's)

    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if args.som:
        run_som(args.rounds)
        return
    pats, flags = FOUR
    sdb = device.StreamDatabase(pats, flags, list(range(len(pats))))
    for size in (64, 1024, 8192, 1 << 20):
        dt = latency(sdb, size, 200 if size < (1 << 20) else 20)
        print(f"latency set=4expr write={size} us_per_call={dt * 1e6:.1f}", flush=True)
    del sdb
    for mode, value in (("on", "0"), ("off", str(1 << 62))):
        env = dict(os.environ, HG_FLOW_HBM_MIN=value)
        print(f"-- HBM copy forced {mode} (HG_FLOW_HBM_MIN={value})", flush=True)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--hbm-child", mode] + (["--lib", args.lib] if args.lib else []), env=env, capture_output=True, text=True, timeout=900)
        sys.stdout.write(out.stdout)
        if out.returncode:
            sys.stdout.write(out.stderr[-3000:])
            sys.exit(out.returncode)
    print("-- default cut-off", flush=True)
    run_batches(args.quick)


if __name__ == "__main__":
    main()
