"""Cost of ranking the matched values on the GPU (hg_rank_values, csrc/hg_rank.hip) against the routes there were before it.

usage: python tools/rank_bench.py [--gib 8] [--distinct-gib 0.5] [--reps 5] [--configs 3,5,d] [--files 1024x1,1024x16,1024x256] [--old-call] [--out FILE]
(the record: profiles/rank_bench.txt)
1. The cut.  Text resident in HBM as in tools/values_bench.py: config 3's and config 5's expression sets over --gib GiB (top 20)
and, as `d`, --distinct-gib GiB with one expression whose values are nearly all distinct (top 100).  After one scan with parts:
  old route   count_values + values() + a host sort by (count descending, first occurrence): stage us, download + sort ms;
  ranked      rank_values(top) + ranked_values(): stage us, download ms.
  One warm-up, then the median and the minimum of --reps calls.  Both routes must give the same rows or the tool stops.
2. Many files.  --files takes shapes NxK: N files of K KiB of a small synthetic log in a temporary directory.  Per shape
count_values_files(top=0) in one native call against the loop over count_values, both in this process, one warm-up, median
and minimum of --reps; they must agree on every row.  The files' bodies are drawn from a pool of at most 64, written in turn.
3. The old call (--old-call, and nothing else then).  values_us of hg_count_values on config 3 and config 5 over --gib GiB, one
warm-up, median and minimum of --reps.  With HG_LIB set the library at that path is loaded (as bench.py does), so that a job
can alternate this build and another commit's library, a process each.
"""
from __future__ import annotations

import argparse
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = [r"[0-9:]+\.[0-9]+Z host-[0-9]+"]
FILE_PATTERNS = ["[a-z]+=[0-9]+", "ERR[0-9]+"]


def emit(lines, line) -> None:
    """One line of the report: shown at once (a long run stays visibly alive), kept for --out."""
    lines.append(line)
    print(line, flush=True)


def timed(call, reps):
    """(median ms, minimum ms, last result) of `reps` calls after one warm-up."""
    call()
    ms, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), out


def the_cut(lines, args) -> None:
    import torch

    from hypergrep_amd import benchspec, device

    emit(lines, "# 1. the cut | config | text bytes | parts | distinct | top | old: values_us (median, min), values() + sort ms (median, min) | ranked: rank_us (median, min), "
         "ranked_values() ms (median, min) | kept bytes")
    full = int(args.gib * (1 << 30)) & ~15
    text = torch.empty(full + 16, dtype=torch.uint8, device="cuda:0")
    for config in [c for c in args.configs.split(",") if c]:
        if config == "d":
            pats, needles, hpm, top = DISTINCT, benchspec.c3_spec()[1], 0, 100
            nbytes = min(full, int(args.distinct_gib * (1 << 30)) & ~15)
        else:
            pats, needles, hpm = {"3": benchspec.c3_spec, "5": benchspec.c5_spec}[config]()
            nbytes, top = full, 20
        device.synth_device(text.data_ptr(), nbytes, seed=23, needles=needles, hit_per_million=hpm)
        torch.cuda.synchronize()
        sc = device.Scanner(device.Database(pats, ids=list(range(len(pats)))), 0)
        st = sc.scan(text.data_ptr(), nbytes, parts=True)
        ptr = text.data_ptr()

        def old_download():
            a = sc.values_arrays()
            off, count, first = a["off"].tolist(), a["count"].tolist(), a["first"].tolist()
            order = sorted(range(len(count)), key=lambda j: (-count[j], first[j]))[:top]
            return [(a["bytes"][off[j]:off[j + 1]], count[j]) for j in order]

        old_us = [sc.count_values(ptr, nbytes).values_us for _ in range(args.reps + 1)][1:]
        old_ms = timed(old_download, args.reps)
        ranked = [sc.rank_values(ptr, nbytes, top=top) for _ in range(args.reps + 1)][1:]
        new_us, r = [v.rank_us for v in ranked], ranked[-1]
        new_ms = timed(lambda: [(v, c) for v, c, _p, _l in sc.ranked_values()], args.reps)
        if old_ms[2] != new_ms[2]:
            raise SystemExit(f"c{config}: the two routes disagree")
        emit(lines, f"c{config} | {nbytes} | {st.n_parts} | {r.n_distinct} | {top} | {statistics.median(old_us):.0f}, {min(old_us)}, {old_ms[0]:.1f}, {old_ms[1]:.1f} | "
             f"{statistics.median(new_us):.0f}, {min(new_us)}, {new_ms[0]:.2f}, {new_ms[1]:.2f} | {r.n_bytes}")
        del sc


def many_files(lines, args) -> None:
    import hypergrep_amd

    emit(lines, "# 2. many files | files x KiB | count_values_files ms (median, min) | loop over count_values ms (median, min) | loop / one call")
    rng = random.Random(7)
    vocab = [b"%s=%d" % (rng.choice([b"user", b"code", b"req", b"n"]), rng.randrange(40)) for _ in range(200)] + [b"ERR%d" % k for k in range(8)] + [b"lorem", b"GET /index", b"-"]
    for shape in [s for s in args.files.split(",") if s]:
        n, kib = (int(v) for v in shape.split("x"))
        with tempfile.TemporaryDirectory() as root:
            names, pool = [], []
            for f in range(n):
                if len(pool) < 64:
                    body = bytearray()
                    while len(body) < kib << 10:
                        body += b" ".join(rng.choice(vocab) for _ in range(rng.randint(1, 8))) + b"\n"
                    pool.append(bytes(body))
                names.append(os.path.join(root, f"{f:06d}.log"))
                with open(names[-1], "wb") as out:
                    out.write(pool[f % len(pool)])
            one = timed(lambda: hypergrep_amd.count_values_files(names, FILE_PATTERNS), args.reps)
            loop = timed(lambda: [hypergrep_amd.count_values(name, FILE_PATTERNS) for name in names], args.reps)
            if one[2] != loop[2]:
                raise SystemExit(f"{shape}: the two routes disagree")
            emit(lines, f"{n} x {kib} | {one[0]:.1f}, {one[1]:.1f} | {loop[0]:.1f}, {loop[1]:.1f} | {loop[0] / max(one[0], 1e-3):.1f}")


def old_call(lines, args) -> None:
    import torch

    from hypergrep_amd import benchspec, device

    which = os.environ.get("HG_LIB", "this build")
    emit(lines, "# 3. the old call | library | config | parts | values | values_us (median, min)")
    nbytes = int(args.gib * (1 << 30)) & ~15
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    for config in ("3", "5"):
        pats, needles, hpm = {"3": benchspec.c3_spec, "5": benchspec.c5_spec}[config]()
        device.synth_device(text.data_ptr(), nbytes, seed=23, needles=needles, hit_per_million=hpm)
        torch.cuda.synchronize()
        sc = device.Scanner(device.Database(pats, ids=list(range(len(pats)))), 0)
        st = sc.scan(text.data_ptr(), nbytes, parts=True)
        runs = [sc.count_values(text.data_ptr(), nbytes) for _ in range(args.reps + 1)][1:]
        us = [v.values_us for v in runs]
        emit(lines, f"{which} | c{config} | {st.n_parts} | {runs[-1].n_values} | {statistics.median(us):.0f}, {min(us)}")
        del sc


def main() -> None:
    import torch

    if os.environ.get("HG_LIB"):  # another commit's library (hypergrep_amd/build.py HG_BUILD_OUT), as bench.py takes it
        import hypergrep_amd

        hypergrep_amd.configure_libraries(libhs=os.path.abspath(os.environ["HG_LIB"]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--distinct-gib", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="3,5,d")
    ap.add_argument("--files", default="1024x1,1024x16,1024x256")
    ap.add_argument("--old-call", action="store_true", help="only section 3: values_us of hg_count_values (HG_LIB chooses the library)")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench needs a GPU: there is nothing to measure without one")
    lines = []
    emit(lines, f"# tools/rank_bench.py --gib {args.gib:g} --distinct-gib {args.distinct_gib:g} --reps {args.reps} --configs {args.configs} --files {args.files}: one MI355X")
    if args.old_call:
        old_call(lines, args)
    else:
        the_cut(lines, args)
        many_files(lines, args)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
