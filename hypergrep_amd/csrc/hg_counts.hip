// gfx950 kernel of the counts stage (hg_count_records): records and distinct lines per report id of the list the last scan
// left (hg_counts.h has the rules and every scalar routine; HgCounts::run in hg_engine.hip is the launch sequence).  One
// launch on the caller's stream:
//
//   hg_counts_kernel<LDS, SEG>  a workgroup per run of HG_COUNTS_RUN records, a lane per record and step.  A lane reads its
//                               16-byte hit (and its segment), takes the record before it from the lane below (lane 0 of a
//                               wave reads it from memory: the one neighbour read, also across run boundaries), applies the
//                               head rule and finds its bin by a binary search of the id.
//                               LDS (n_bins <= HG_COUNTS_LDS_MAX): the id table and two uint32 counters per bin live in LDS
//                               (48 KiB); a run is far below 2^32 records, so they cannot overflow.  At the end the non-zero
//                               bins are added to the 64-bit totals.  Else the table is searched in memory and the totals are
//                               added to directly.
//                               A wave whose counted lanes agree on the bin adds once, the population counts, from one lane:
//                               without it one expression that matches every line serialises 64 lanes on one address.
//                               SEG: the same for the cell (segment, bin) of the two n_seg x n_bins matrices, 32-bit atomics
//                               in memory.
//
// Integer atomics only: the result is exact whatever the order.  No text is read.  Every index is checked where it is made: a
// record is read below list.n, a bin comes out of the search (below n_bins) or the record is skipped, a segment at or above
// n_seg touches no cell.
#include <hip/hip_runtime.h>

#include "hg_counts.h"
#include "hg_engine.h"

template <bool LDS, bool SEG>
__global__ __launch_bounds__(HG_COUNTS_THREADS) void hg_counts_kernel(HgCountsArgs a) {
  constexpr uint32_t kLds = LDS ? HG_COUNTS_LDS_MAX : 1;
  __shared__ uint32_t s_ids[kLds], s_lines[kLds], s_reports[kLds];
  if (LDS) {
    for (uint32_t b = threadIdx.x; b < a.n_bins; b += HG_COUNTS_THREADS) s_ids[b] = a.ids[b], s_lines[b] = 0, s_reports[b] = 0;
    __syncthreads();
  }
  const uint32_t *ids = LDS ? s_ids : a.ids;
  uint64_t first, last;
  hg_counts_run(a.list.n, HG_COUNTS_RUN, blockIdx.x, &first, &last);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t r0 = first; r0 < last; r0 += HG_COUNTS_THREADS) {  // (block-uniform: every lane of a wave takes part in the exchanges)
    const uint64_t r = r0 + threadIdx.x;
    const bool valid = r < last;
    HgHit h{0, 0, 0};
    uint32_t seg = 0;
    if (valid) h = a.list.hits[r], seg = hg_counts_seg(a.list, r);
    // the record before it: the lane below has it, but for lane 0 of the wave
    uint32_t p_id = __shfl_up(h.id, 1), p_seg = __shfl_up(seg, 1);
    uint32_t p_lo = __shfl_up(static_cast<uint32_t>(h.line_no), 1), p_hi = __shfl_up(static_cast<uint32_t>(h.line_no >> 32), 1);
    if (lane == 0 && valid && r > 0) {
      const HgHit p = a.list.hits[r - 1];
      p_id = p.id, p_seg = hg_counts_seg(a.list, r - 1), p_lo = static_cast<uint32_t>(p.line_no), p_hi = static_cast<uint32_t>(p.line_no >> 32);
    }
    const bool head = valid && hg_counts_head(r > 0, p_seg, (static_cast<uint64_t>(p_hi) << 32) | p_lo, p_id, seg, h.line_no, h.id);
    const uint32_t bin = valid ? hg_counts_bin(ids, a.n_bins, h.id) : HG_COUNTS_NO_BIN;
    const bool counted = bin != HG_COUNTS_NO_BIN;
    const unsigned long long act = __ballot(counted);
    if (!act) continue;  // (wave-uniform)
    const int leader = __ffsll(act) - 1;
    const uint32_t b0 = __shfl(bin, leader), s0 = __shfl(seg, leader);
    const bool one_bin = __ballot(counted && bin != b0) == 0;
    const unsigned long long heads = __ballot(counted && head);
    if (one_bin) {
      if (lane == static_cast<uint32_t>(leader)) {
        if (LDS) {
          atomicAdd(&s_reports[b0], static_cast<uint32_t>(__popcll(act)));
          if (heads) atomicAdd(&s_lines[b0], static_cast<uint32_t>(__popcll(heads)));
        } else {
          atomicAdd(&a.n_reports[b0], static_cast<unsigned long long>(__popcll(act)));
          if (heads) atomicAdd(&a.n_lines[b0], static_cast<unsigned long long>(__popcll(heads)));
        }
      }
    } else if (counted) {
      if (LDS) {
        atomicAdd(&s_reports[bin], 1u);
        if (head) atomicAdd(&s_lines[bin], 1u);
      } else {
        atomicAdd(&a.n_reports[bin], 1ull);
        if (head) atomicAdd(&a.n_lines[bin], 1ull);
      }
    }
    if (SEG) {
      const bool one_cell = one_bin && __ballot(counted && seg != s0) == 0;
      uint64_t cell;
      if (one_cell) {
        if (lane == static_cast<uint32_t>(leader) && hg_counts_cell(a.n_seg, a.n_bins, s0, b0, &cell)) {
          atomicAdd(&a.seg_reports[cell], static_cast<uint32_t>(__popcll(act)));
          if (heads) atomicAdd(&a.seg_lines[cell], static_cast<uint32_t>(__popcll(heads)));
        }
      } else if (counted && hg_counts_cell(a.n_seg, a.n_bins, seg, bin, &cell)) {
        atomicAdd(&a.seg_reports[cell], 1u);
        if (head) atomicAdd(&a.seg_lines[cell], 1u);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < a.n_bins; b += HG_COUNTS_THREADS) {
      const uint32_t nr = s_reports[b], nl = s_lines[b];
      if (nr) atomicAdd(&a.n_reports[b], static_cast<unsigned long long>(nr));
      if (nl) atomicAdd(&a.n_lines[b], static_cast<unsigned long long>(nl));
    }
  }
}

hipError_t hg_counts_launch(const HgCountsArgs &a, hipStream_t stream) {
  if (!a.list.n || !a.n_bins) return hipSuccess;
  const dim3 grid(static_cast<uint32_t>(hg_counts_runs(a.list.n, HG_COUNTS_RUN))), block(HG_COUNTS_THREADS);
  const bool lds = a.n_bins <= HG_COUNTS_LDS_MAX, seg = a.seg_lines != nullptr;
  if (lds && seg) hipLaunchKernelGGL((hg_counts_kernel<true, true>), grid, block, 0, stream, a);
  else if (lds) hipLaunchKernelGGL((hg_counts_kernel<true, false>), grid, block, 0, stream, a);
  else if (seg) hipLaunchKernelGGL((hg_counts_kernel<false, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((hg_counts_kernel<false, false>), grid, block, 0, stream, a);
  return hipGetLastError();
}
