"""Cost of gathering the matched parts on the GPU (hg_gather_parts, csrc/hg_partlines.hip) for text resident in HBM.

usage: python tools/partlines_bench.py [--gib 8] [--reps 5] [--configs 3,5] [--out FILE]
(the record: profiles/partlines_bench.txt)
Text: the benchmark's synthetic log (hg_synth_device), --gib GiB of it in one buffer, with config 3's expression set and
needles (256 expressions, three tiers) and with config 5's (4096 literals).  Per config, after one scan with parts, medians of
--reps gathers each in parts mode (NUMBER | BYTE_OFFSET | TERMINATE: grep -o -n -b) and in line mode (LINE | TERMINATE with
grep's colour escapes as marks: grep --color):
  gather_us   the whole stage (HIP events: entries, scan, the host synchronisation that sizes the output, spans, copy);
  bound       the stage's traffic over the HBM rate: the text runs read and the output written, plus per part the 16-byte part
              record read three times (its own lane and both neighbours'), the 32 bytes of its piece's record, and the entry
              descriptor, size, offset and per-entry arrays written and the descriptor and offset read again by the copy pass,
              over 8.0 TB/s (the part's peak) and 6.29 TB/s (the rate a float4 copy reaches on it; tools/bw_ceiling.hip);
  host route  what a caller had to do before: hg_copy_parts (16-byte records and expression indices), the gathered lines
              (hg_gather_lines with flags 0, its arrays and bytes) to the host, and the parts sliced out with numpy; timed in
              the same run, the download alone and with the slicing.
The passes' kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -- python tools/partlines_bench.py
--configs <one> --reps 3, whose kernel statistics name hg_partlines_entry_kernel, hg_partlines_span_kernel and
hg_partlines_copy_kernel.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_SPEC, PEAK_COPY = 8.0e12, 6.29e12  # bytes per second: the part's HBM peak, and what a float4 copy reaches
PARTS_MODE, LINE_MODE = 1 | 2 | 4, 8 | 4  # HG_PARTS_NUMBER | BYTE_OFFSET | TERMINATE; HG_PARTS_LINE | TERMINATE
COLOR = (b"\x1b[01;31m\x1b[K", b"\x1b[m\x1b[K")


def emit(lines, line) -> None:
    """One line of the report: shown at once (a long run stays visibly alive), kept for --out."""
    lines.append(line)
    print(line, flush=True)


def traffic(n_parts: int, n_bytes: int, text_bytes: int) -> int:
    """Bytes the stage moves: text runs read, output written, and per part 3 x 16 (part records) + 4 (expression) + 32 (the
    piece's record) read, 48 + 8 + 8 + 8 + 4 + 4 (descriptor, size, offset, line number, kind, expression) written and 48 + 8
    (descriptor, offset) read again by the copy pass."""
    return text_bytes + n_bytes + n_parts * (3 * 16 + 4 + 32 + 48 + 8 + 8 + 8 + 4 + 4 + 48 + 8)


def host_route(sc, d_text: int, nbytes: int):
    """The route without the stage: part records and gathered lines to the host, the parts sliced out there.  Returns
    (download ms, download + slicing ms, bytes of parts)."""
    import ctypes

    import numpy as np

    from hypergrep_amd import device

    t0 = time.perf_counter()
    n = sc._last_parts.n_parts  # pylint: disable=protected-access
    recs = np.zeros((max(n, 1), 2), dtype=np.uint64)  # hg_part_t: line_number, then from | to << 32
    pattern = np.zeros(max(n, 1), dtype=np.uint32)
    if n and device.lib().hg_copy_parts(sc._h, recs.ctypes.data_as(ctypes.POINTER(device.HgPart)), pattern.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n) != 0:  # pylint: disable=protected-access
        raise SystemExit("hg_copy_parts failed")
    recs = recs[:n]
    sc.gather(d_text, nbytes)
    a = sc.lines_arrays()
    t1 = time.perf_counter()
    blob = np.frombuffer(a["bytes"], dtype=np.uint8)
    line = recs[:, 0]
    frm = (recs[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    to = (recs[:, 1] >> np.uint64(32)).astype(np.int64)
    entry = np.searchsorted(a["line_number"], line)  # the gathered line of each part
    begin = a["entry_off"][entry].astype(np.int64) + frm
    lens = to - frm
    out_off = np.concatenate(([0], np.cumsum(lens)))
    idx = np.repeat(begin - out_off[:-1], lens) + np.arange(out_off[-1])  # one gather of every part's bytes
    parts_bytes = blob[idx]
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3, int(parts_bytes.size)


def main() -> None:
    import torch

    from hypergrep_amd import benchspec, device

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("partlines_bench needs a GPU: there is nothing to measure without one")
    nbytes = int(args.gib * (1 << 30)) & ~15
    lines = []
    emit(lines, f"# tools/partlines_bench.py --gib {args.gib:g} --reps {args.reps} --configs {args.configs}: one MI355X, {nbytes} bytes of synthetic log resident, buffer_size 262140")
    emit(lines, "# config | lines | records | parts | parts_us | mode | n_bytes | gather_us (median, min) | output GB/s | traffic bound us at 8.0 / 6.29 TB/s | gather / bound(6.29) | "
         "host route ms: download, download + slicing | host / gather")
    text = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    for config in args.configs.split(","):
        pats, needles, hpm = {"3": benchspec.c3_spec, "5": benchspec.c5_spec}[config]()
        device.synth_device(text.data_ptr(), nbytes, seed=23, needles=needles, hit_per_million=hpm)
        torch.cuda.synchronize()
        sc = device.Scanner(device.Database(pats, ids=list(range(len(pats)))), 0)
        try:
            st = sc.scan(text.data_ptr(), nbytes, parts=True)
        except ValueError as e:  # a set the parts stage is not offered for
            emit(lines, f"c{config} | no parts: {e}")
            continue
        down_ms, host_ms, part_bytes = host_route(sc, text.data_ptr(), nbytes)
        line_bytes = sc._last_lines.n_bytes  # pylint: disable=protected-access
        plain = sc._gather_parts(text.data_ptr(), nbytes, 0)  # pylint: disable=protected-access
        if (plain.n_entries, plain.n_bytes) != (st.n_parts, part_bytes):  # the two routes agree on what the parts are
            raise SystemExit(f"c{config}: the stage gathered {plain.n_bytes} bytes of {plain.n_entries} parts, the host route {part_bytes} of {st.n_parts}")
        for mode, flags, mark in (("parts", PARTS_MODE, (b"", b"")), ("line", LINE_MODE, COLOR)):
            us = []
            for rep in range(args.reps + 1):
                g = sc._gather_parts(text.data_ptr(), nbytes, flags, mark)  # pylint: disable=protected-access
                if rep:  # (the first gather allocates the stage's buffers)
                    us.append(g.gather_us)
            bytes_moved = traffic(g.n_entries, g.n_bytes, part_bytes if mode == "parts" else line_bytes)
            med = statistics.median(us)
            emit(lines, f"c{config} | {st.n_lines} | {st.n_hits} | {st.n_parts} | {st.parts_us} | {mode} | {g.n_bytes} | {med:.0f}, {min(us)} | {g.n_bytes / max(med, 1) / 1e3:.1f} | "
                 f"{bytes_moved / PEAK_SPEC * 1e6:.0f} / {bytes_moved / PEAK_COPY * 1e6:.0f} | {med / max(bytes_moved / PEAK_COPY * 1e6, 1e-9):.1f} | {down_ms:.0f}, {host_ms:.0f} | "
                 f"{host_ms * 1e3 / max(med, 1):.0f}")
        del sc
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
