// gfx950 kernels of the rank stage (hg_rank_values): the distinct matched values of the last scan with parts ordered by count, per
// file if asked, and cut to the `top` most frequent (hg_rank.h has the rules and every scalar routine; HgRank::run in
// hg_engine.hip is the launch sequence).  The groups come from the values stage (HgValues::group): without HG_RANK_PER_SEGMENT
// from its own kernels, with it from the three below, then in both cases from its mark and compact kernels and its sort by first.
//
//   hg_rank_hash_kernel    hg_values_hash_kernel, hg_values_long_kernel and hg_values_insert_kernel (hg_values.hip has their
//   hg_rank_long_kernel    description, atomics and bounds; hg_values_dev.h their bodies) with the segment as a third key
//   hg_rank_insert_kernel  component: a key word per part, one more Horner step, the key word compared in place of the expression.
//
// Then, on the caller's stream:
//
//   (sort of the pairs by descending count: rocPRIM, stable)
//   hg_rank_keys_kernel    a lane per group: its segment (that of part `first`) and its place.  HG_RANK_PER_SEGMENT only.
//   (sort of those by segment: rocPRIM, stable)
//   hg_rank_counts_kernel  a lane per group: its count in the final order, and a zero behind.   (exclusive scan: rocPRIM)
//   hg_rank_bounds_kernel  a lane per segment: two lower bounds among the groups' segments give its first group, its distinct
//                          values, its parts (a difference of the scan) and how many rows it keeps.  (exclusive scan: rocPRIM)
//   hg_rank_place_kernel   a lane per group: a group inside the cut writes its row (count, first, pattern, line number,
//                          segment, length, copy entry); one beyond it writes nothing.           (exclusive scan: rocPRIM)
//   (hg_gather_span_kernel, hg_gather_copy_kernel of hg_gather.hip, as they are, over the kept rows' entries)
//
// The last four: no atomics, no LDS, no text reads; no lane waits for another or reads what a lane of the same launch wrote.
// Every index is checked where it is made (hg_rank.h).
#include <hip/hip_runtime.h>

#include "hg_engine.h"
#include "hg_rank.h"
#include "hg_values_dev.h"

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_rank_hash_kernel(HgValuesArgs a) { hg_values_dev::hash_body<true>(a); }

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_rank_long_kernel(HgValuesArgs a) { hg_values_dev::long_body<true>(a); }

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_rank_insert_kernel(HgValuesArgs a) { hg_values_dev::insert_body<true>(a); }

__global__ __launch_bounds__(HG_RANK_THREADS) void hg_rank_keys_kernel(HgRankArgs a) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * HG_RANK_THREADS + threadIdx.x;
  if (j < a.n_groups) hg_rank_keys(a, j);
}

__global__ __launch_bounds__(HG_RANK_THREADS) void hg_rank_counts_kernel(HgRankArgs a) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * HG_RANK_THREADS + threadIdx.x;
  if (j <= a.n_groups) hg_rank_counts(a, j);
}

__global__ __launch_bounds__(HG_RANK_THREADS) void hg_rank_bounds_kernel(HgRankArgs a) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * HG_RANK_THREADS + threadIdx.x;
  if (s <= a.n_seg) hg_rank_bounds(a, s);
}

__global__ __launch_bounds__(HG_RANK_THREADS) void hg_rank_place_kernel(HgRankArgs a) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * HG_RANK_THREADS + threadIdx.x;
  if (j < a.n_groups) hg_rank_place(a, j);
}

hipError_t hg_rank_launch(const HgRankArgs &a, HgRankStep step, hipStream_t stream) {
  const dim3 block(HG_RANK_THREADS);
  const auto blocks = [](uint64_t n) { return dim3(static_cast<uint32_t>((n + HG_RANK_THREADS - 1) / HG_RANK_THREADS)); };
  switch (step) {
    case HgRankStep::Keys:
      if (a.n_groups) hipLaunchKernelGGL(hg_rank_keys_kernel, blocks(a.n_groups), block, 0, stream, a);
      break;
    case HgRankStep::Counts:
      hipLaunchKernelGGL(hg_rank_counts_kernel, blocks(a.n_groups + 1), block, 0, stream, a);
      break;
    case HgRankStep::Bounds:
      hipLaunchKernelGGL(hg_rank_bounds_kernel, blocks(static_cast<uint64_t>(a.n_seg) + 1), block, 0, stream, a);
      break;
    case HgRankStep::Place:
      if (a.n_groups) hipLaunchKernelGGL(hg_rank_place_kernel, blocks(a.n_groups), block, 0, stream, a);
      break;
  }
  return hipGetLastError();
}

hipError_t hg_rank_group_launch(const HgValuesArgs &a, HgValuesStep step, hipStream_t stream) {
  const dim3 block(HG_VALUES_THREADS);
  const auto blocks = [](uint64_t n) { return dim3(static_cast<uint32_t>((n + HG_VALUES_THREADS - 1) / HG_VALUES_THREADS)); };
  if (!a.key || !a.n_parts) return a.n_parts ? hipErrorInvalidValue : hipSuccess;
  switch (step) {
    case HgValuesStep::Hash:
      hipLaunchKernelGGL(hg_rank_hash_kernel, blocks(a.n_parts), block, 0, stream, a);
      break;
    case HgValuesStep::Long:
      hipLaunchKernelGGL(hg_rank_long_kernel, dim3(static_cast<uint32_t>(std::min<uint64_t>((a.n_parts + 3) / 4, HG_VALUES_LONG_BLOCKS))), block, 0, stream, a);
      break;
    case HgValuesStep::Insert:
      hipLaunchKernelGGL(hg_rank_insert_kernel, blocks(a.n_parts), block, 0, stream, a);
      break;
    default:
      return hipErrorInvalidValue;  // (the other steps have no segment-keyed form)
  }
  return hipGetLastError();
}
