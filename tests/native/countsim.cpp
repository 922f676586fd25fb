// TEST-ONLY host replay of the counts stage: compiles hypergrep_amd/csrc/hg_counts.h for x86 and runs its rules — the head
// rule, the bin lookup, the split into runs — over a record list, run after run as the kernel's workgroups take them, each
// run adding its own sums to the totals.  tests/countsim_py.py is its ctypes face.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_counts.h"

extern "C" {

uint32_t countsim_run_length() { return HG_COUNTS_RUN; }
uint32_t countsim_lds_bins() { return HG_COUNTS_LDS_MAX; }
uint32_t countsim_bin(const uint32_t *ids, uint32_t n_bins, uint32_t id) { return hg_counts_bin(ids, n_bins, id); }

// recs: n rows of (segment, line, id).  with_seg == 0: the list has no segment array (every record is of segment 0).
// n_lines / n_reports: n_bins totals, added to.  seg_lines / seg_reports: n_seg x n_bins, or NULL.  Returns the number of
// records that had no bin or whose segment had no row, which no scan produces.
uint64_t countsim_run(const uint64_t *recs, uint64_t n, int with_seg, const uint32_t *ids, uint32_t n_bins, uint32_t n_seg, uint64_t run_len, uint64_t *n_lines,
                      uint64_t *n_reports, uint32_t *seg_lines, uint32_t *seg_reports) {
  std::vector<HgHit> hits(n + 1);
  std::vector<uint32_t> seg_of(n + 1);
  for (uint64_t i = 0; i < n; i++) {
    hits[i] = HgHit{recs[3 * i + 1], static_cast<uint32_t>(recs[3 * i + 2]), 0};
    seg_of[i] = static_cast<uint32_t>(recs[3 * i]);
  }
  const HgCountsList list{hits.data(), with_seg ? seg_of.data() : nullptr, n};
  uint64_t skipped = 0;
  for (uint64_t run = 0; run < hg_counts_runs(n, run_len); run++) {
    uint64_t first, last;
    hg_counts_run(n, run_len, run, &first, &last);
    std::vector<uint32_t> lines(n_bins, 0), reports(n_bins, 0);  // the workgroup's own counters
    for (uint64_t r = first; r < last; r++) {
      const uint32_t bin = hg_counts_bin(ids, n_bins, list.hits[r].id);
      if (bin == HG_COUNTS_NO_BIN) {
        skipped++;
        continue;
      }
      const bool head = hg_counts_head_at(list, r);
      reports[bin]++;
      lines[bin] += head;
      if (seg_lines) {
        uint64_t cell;
        if (hg_counts_cell(n_seg, n_bins, hg_counts_seg(list, r), bin, &cell)) {
          seg_reports[cell]++;
          seg_lines[cell] += head;
        } else {
          skipped++;
        }
      }
    }
    for (uint32_t b = 0; b < n_bins; b++) n_lines[b] += lines[b], n_reports[b] += reports[b];
  }
  return skipped;
}

}  // extern "C"
