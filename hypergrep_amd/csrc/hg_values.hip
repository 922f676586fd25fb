// gfx950 kernels of the values stage (hg_count_values): the distinct matched parts of the last scan with parts and how often
// each occurs (hg_values.h has the rules and every scalar routine; HgValues::run in hg_engine.hip is the launch sequence).  On
// the caller's stream:
//
//   hg_values_hash_kernel     a lane per part: where its value lies (a lower bound in the final records) and how long it is; the
//                             hash of a part of at most HG_VALUES_LANE_MAX bytes, by aligned dwords; a longer part goes on a list.
//   hg_values_long_kernel     a wavefront per listed part (a fixed grid strides over the list): the hash, a dword a lane and
//                             round, summed over the wave; then the probe, lane 0 reading and claiming the slot, all 64 lanes
//                             comparing the bytes.
//   hg_values_insert_kernel   a lane per short part: the probe (hg_values_insert).  A wave whose lanes all found the same slot
//                             adds its population count once, from its first lane, which also has the smallest part index;
//                             any other wave adds lane by lane.  Logs have few distinct values and many parts.
//   hg_values_mark_kernel     a lane per slot: 1 if occupied.   (exclusive scan: rocPRIM)
//   hg_values_compact_kernel  a lane per slot: the (first, count) pair of an occupied slot to its rank; the last lane leaves the
//                             number of values.                 (sort of the pairs by first: rocPRIM)
//   hg_values_derive_kernel   a lane per value: pattern, line number, segment, length and the copy pass's entry from part `first`.
//   (hg_gather_span_kernel, hg_gather_copy_kernel of hg_gather.hip, as they are: the line gather's span and copy pass over those
//                             entries, a workgroup per HG_GATHER_TILE output bytes, a lane 16 bytes at a time, one aligned
//                             16-byte store each)
//
// Atomics: a 64-bit atomicCAS claims a slot, atomicAdd and atomicMin on 64-bit words count; all plain vector atomics on
// integers, so the result is exact whatever the order.  No lane waits for another: a probe reads the slot word, the arrays the
// hash kernel finished before this launch, and the text.  A probe is bounded by the capacity; one that runs out sets
// counters[HG_VALUES_OVERFLOW] and the call fails.  Every index is checked where it is made: a part below n_parts, a slot masked
// to the capacity, a representative below n_parts (hg_values_candidate), a list entry below the list's length.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_values.h"
#include "hg_values_dev.h"

// (the bodies of the first three are hg_values_dev.h's, which the rank stage instantiates once more with the segment in the key)
__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_hash_kernel(HgValuesArgs a) { hg_values_dev::hash_body<false>(a); }

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_long_kernel(HgValuesArgs a) { hg_values_dev::long_body<false>(a); }

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_insert_kernel(HgValuesArgs a) { hg_values_dev::insert_body<false>(a); }

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_mark_kernel(HgValuesArgs a) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * HG_VALUES_THREADS + threadIdx.x;
  if (i < (uint64_t{1} << a.table_log2)) a.pos[i] = a.slot[i] != HG_VALUES_EMPTY;
}

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_compact_kernel(HgValuesArgs a) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * HG_VALUES_THREADS + threadIdx.x, cap = uint64_t{1} << a.table_log2;
  if (i >= cap) return;
  const bool occupied = a.slot[i] != HG_VALUES_EMPTY;
  const uint64_t j = a.pos[i];
  if (occupied && j < a.n_parts) a.pair_first[j] = a.first[i], a.pair_count[j] = a.count[i];
  if (i == cap - 1) a.counters[HG_VALUES_N_VALUES] = j + (occupied ? 1 : 0);
}

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_derive_kernel(HgValuesArgs a) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * HG_VALUES_THREADS + threadIdx.x;
  if (j <= a.n_values && (j == a.n_values || a.v_first[j] < a.n_parts)) hg_values_derive(a, j);
}

hipError_t hg_values_launch(const HgValuesArgs &a, HgValuesStep step, hipStream_t stream) {
  const dim3 block(HG_VALUES_THREADS);
  const uint64_t cap = uint64_t{1} << a.table_log2;
  const auto blocks = [](uint64_t n) { return dim3(static_cast<uint32_t>((n + HG_VALUES_THREADS - 1) / HG_VALUES_THREADS)); };
  switch (step) {
    case HgValuesStep::Hash:
      if (a.n_parts) hipLaunchKernelGGL(hg_values_hash_kernel, blocks(a.n_parts), block, 0, stream, a);
      break;
    case HgValuesStep::Long:
      if (a.n_parts) hipLaunchKernelGGL(hg_values_long_kernel, dim3(static_cast<uint32_t>(std::min<uint64_t>((a.n_parts + 3) / 4, HG_VALUES_LONG_BLOCKS))), block, 0, stream, a);
      break;
    case HgValuesStep::Insert:
      if (a.n_parts) hipLaunchKernelGGL(hg_values_insert_kernel, blocks(a.n_parts), block, 0, stream, a);
      break;
    case HgValuesStep::Mark:
      hipLaunchKernelGGL(hg_values_mark_kernel, blocks(cap), block, 0, stream, a);
      break;
    case HgValuesStep::Compact:
      hipLaunchKernelGGL(hg_values_compact_kernel, blocks(cap), block, 0, stream, a);
      break;
    case HgValuesStep::Derive:
      hipLaunchKernelGGL(hg_values_derive_kernel, blocks(a.n_values + 1), block, 0, stream, a);
      break;
  }
  return hipGetLastError();
}
