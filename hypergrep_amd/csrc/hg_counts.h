// Counts per report id (hg_count_records): how many records, and how many distinct (segment, line), the last scan left for
// every distinct report id of the database.  The scalar rules here are shared by the kernels (hg_counts.hip) and the host
// replay of the tests (tests/native/countsim.cpp compiles this header for x86); the product only calls them from device code.
//
// The stage works on ONE ordered record list the scan left on the device: the final hits, or the surviving records of a scan
// with segments, ordered by (segment, line, id, to).
//  - BIN.  A bin is a distinct report id of the database, ascending (HgDb::report_ids).  A record's bin is the index of its
//    id in that table: a binary search (hg_counts_bin), so only the 16-byte hit record is read; an id that is not in the
//    table (no scan delivers one) has no bin and is not counted.
//  - HEAD.  A record counts as a new line for its bin iff it is record 0 or differs from the record before it in segment,
//    line or id (hg_counts_head): by the order of the list every (segment, line, id) group is one run of neighbours.  This
//    is the one place a neighbour is read.
//  - RUNS.  The list is cut into runs of HG_COUNTS_RUN records, one per workgroup.  The head rule of a run's first record
//    reads the last record of the run before it; nothing else crosses a run boundary, and integer sums make the result
//    independent of the split.
#pragma once
#include "hg_core.h"

constexpr uint32_t HG_COUNTS_THREADS = 256;  // lanes of a workgroup
#ifndef HG_COUNTS_RUN
#define HG_COUNTS_RUN 16384u  // records per workgroup (the value hypergrep_amd/device.py publishes)
#endif
static_assert(HG_COUNTS_RUN % HG_COUNTS_THREADS == 0, "a run is a whole number of steps");
constexpr uint32_t HG_COUNTS_LDS_MAX = 4096;  // HG_COUNTS_LDS_BINS of the C ABI: up to this many bins a workgroup counts in LDS
constexpr uint32_t HG_COUNTS_F_ACCUMULATE = 1u, HG_COUNTS_F_PER_SEGMENT = 2u;  // HG_COUNTS_* of the C ABI
constexpr uint32_t HG_COUNTS_NO_BIN = 0xFFFFFFFFu;
constexpr uint64_t HG_COUNTS_MAX_CELLS = 1ull << 28;  // n_seg * n_bins of the per-segment matrices

// The record list.  seg_of == nullptr: no segments (every record is of segment 0).
struct HgCountsList {
  const HgHit *hits;
  const uint32_t *seg_of;
  uint64_t n;
};

// What the kernels work on (hg_counts_launch, hg_engine.h).
struct HgCountsArgs {
  HgCountsList list;
  const uint32_t *ids;  // n_bins report ids, ascending
  uint32_t n_bins;
  uint32_t n_seg;       // rows of the matrices (0: none)
  unsigned long long *n_lines, *n_reports;  // n_bins totals, added to
  uint32_t *seg_lines, *seg_reports;        // n_seg x n_bins, zeroed before the launch; nullptr without HG_COUNTS_PER_SEGMENT
};

HG_HD uint32_t hg_counts_seg(const HgCountsList &l, uint64_t i) { return l.seg_of ? l.seg_of[i] : 0u; }

// The bin of report id `id`: its index in ids[0, n_bins) (ascending, distinct), or HG_COUNTS_NO_BIN.
HG_HD uint32_t hg_counts_bin(const uint32_t *ids, uint32_t n_bins, uint32_t id) {
  uint32_t lo = 0, hi = n_bins;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n_bins && ids[lo] == id ? lo : HG_COUNTS_NO_BIN;
}

// The head rule on two neighbours: does the record (seg, line, id) open a new line of its bin, given the record before it?
// has_prev false: it is record 0.
HG_HD bool hg_counts_head(bool has_prev, uint32_t prev_seg, uint64_t prev_line, uint32_t prev_id, uint32_t seg, uint64_t line, uint32_t id) {
  return !has_prev || prev_seg != seg || prev_line != line || prev_id != id;
}
// ... and on record i of the list.
HG_HD bool hg_counts_head_at(const HgCountsList &l, uint64_t i) {
  if (i == 0) return true;
  return hg_counts_head(true, hg_counts_seg(l, i - 1), l.hits[i - 1].line_no, l.hits[i - 1].id, hg_counts_seg(l, i), l.hits[i].line_no, l.hits[i].id);
}

// The records [first, last) of run `run` of `run_len` records each.
HG_HD void hg_counts_run(uint64_t n, uint64_t run_len, uint64_t run, uint64_t *first, uint64_t *last) {
  *first = run * run_len < n ? run * run_len : n;
  *last = n - *first < run_len ? n : *first + run_len;
}
HG_HD uint64_t hg_counts_runs(uint64_t n, uint64_t run_len) { return (n + run_len - 1) / run_len; }
// A cell of the per-segment matrices, or false when the segment is out of range (no scan leaves such a record).
HG_HD bool hg_counts_cell(uint32_t n_seg, uint32_t n_bins, uint32_t seg, uint32_t bin, uint64_t *cell) {
  *cell = static_cast<uint64_t>(seg) * n_bins + bin;
  return seg < n_seg;
}
