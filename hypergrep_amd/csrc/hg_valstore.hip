// gfx950 kernels of the value store (hg_accumulate_values, hg_rank_accumulated): distinct matched values that survive scans
// (hg_valstore.h has the rules and every scalar routine; HgValueStore in hg_engine.hip is the launch sequence).  The call's groups
// come from the values stage (HgValues::group, an instance of the store's own).  Then, on the caller's stream:
//
//   hg_valstore_lookup_kernel  a lane per group: a group of at most HG_VALUES_LANE_MAX bytes probes the store's table read-only
//                              (hg_valstore_lookup) and leaves match[j]; a longer one goes on a list.
//   hg_valstore_long_kernel    a wavefront per listed group (a fixed grid strides over the list, as hg_values_long_kernel does):
//                              lane 0 reads the slot, all 64 lanes compare the bytes.
//   hg_valstore_size_kernel    a lane per group: 1 and its length if it is new.          (two exclusive scans: rocPRIM)
//   hg_valstore_rehash_kernel  a lane per stored value, when the table changes size: its claim in the new table.
//   hg_valstore_apply_kernel   a lane per group: a found one adds its count, a new one writes its row and its copy entry and
//                              claims its slot.
//   (hg_gather_span_kernel, hg_gather_copy_kernel of hg_gather.hip, as they are: the new values' bytes from the text to the
//                              arena's tail)
//   hg_valstore_place_kernel   a lane per kept place of a ranking: the row's arrays and a copy entry into the arena.
//   (sort of the indices by descending count, scan of the lengths: rocPRIM; then the span and copy pass with the arena as text)
//
// Atomics: a 64-bit atomicCAS claims an empty slot (rehash, apply); an integer atomicAdd numbers the long list, whose order
// does not matter.  No lane waits for another, and none reads what a lane of the same launch wrote: the lookup reads the table,
// the store's rows and the arena as the calls before left them; a found group's add is a plain add, since groups of one call
// have distinct keys; a claim compares nothing.  Every probe is bounded by the capacity; one that runs out writes
// counters[HG_VALSTORE_OVERFLOW] and the call fails.  Every index is checked where it is made (hg_valstore.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_valstore.h"
#include "hg_values_dev.h"

namespace {

struct ReadTable {
  const unsigned long long *slot;
  __device__ uint64_t load(uint64_t i) const { return slot[i]; }
};

}  // namespace

__global__ __launch_bounds__(HG_VALSTORE_THREADS) void hg_valstore_lookup_kernel(HgValStoreArgs a) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * HG_VALSTORE_THREADS + threadIdx.x;
  if (j >= a.n_groups) return;
  const uint64_t f = a.g_first[j];
  if (f < a.n_parts && hg_values_is_long(a.len[f])) {
    const unsigned long long k = atomicAdd(&a.counters[HG_VALSTORE_N_LONG], 1ull);
    if (k < a.n_groups) a.long_list[k] = j;
    return;  // (the long kernel writes match[j])
  }
  bool overflow = false;
  a.match[j] = hg_valstore_lookup(a, a.text, a.arena, ReadTable{a.slot}, j, &overflow);
  if (overflow) a.counters[HG_VALSTORE_OVERFLOW] = 1;
}

__global__ __launch_bounds__(HG_VALSTORE_THREADS) void hg_valstore_long_kernel(HgValStoreArgs a) {
  const uint32_t lane = threadIdx.x & (HG_VALUES_WAVE - 1);
  const uint64_t wave = (static_cast<uint64_t>(blockIdx.x) * HG_VALSTORE_THREADS + threadIdx.x) / HG_VALUES_WAVE;
  const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * (HG_VALSTORE_THREADS / HG_VALUES_WAVE);
  const uint64_t n_long = std::min<uint64_t>(a.counters[HG_VALSTORE_N_LONG], a.n_groups), cap = uint64_t{1} << a.store_log2;
  for (uint64_t i = wave; i < n_long; i += n_waves) {  // (wave-uniform)
    const uint64_t j = a.long_list[i];
    if (j >= a.n_groups) continue;
    const uint64_t f = a.g_first[j];
    if (f >= a.n_parts) continue;
    const uint64_t h = a.hash[f], src = a.src[f];
    const uint32_t len = a.len[f], pat = a.part_pattern[f];
    uint64_t s = hg_values_home(h, a.store_log2), found = HG_VALSTORE_NONE;
    bool ended = a.n_values == 0;
    for (uint64_t probe = 0; !ended && probe < cap; probe++, s = (s + 1) & (cap - 1)) {
      uint64_t w = 0;
      if (lane == 0) w = a.slot[s];
      w = hg_values_dev::shfl64(w, 0);
      if (w == HG_VALUES_EMPTY) {
        ended = true;
        break;
      }
      uint64_t idx;
      if (hg_valstore_candidate(a, w, h, len, pat, &idx) && __all(hg_valstore_equal_wave_lane(a.text, src, a.arena, a.v_off[idx], len, lane))) {
        found = idx;
        ended = true;
        break;
      }
    }
    if (lane == 0) {
      a.match[j] = found;
      if (!ended) a.counters[HG_VALSTORE_OVERFLOW] = 1;
    }
  }
}

__global__ __launch_bounds__(HG_VALSTORE_THREADS) void hg_valstore_size_kernel(HgValStoreArgs a) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * HG_VALSTORE_THREADS + threadIdx.x;
  if (j <= a.n_groups) hg_valstore_size(a, j);
}

__global__ __launch_bounds__(HG_VALSTORE_THREADS) void hg_valstore_rehash_kernel(HgValStoreArgs a) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * HG_VALSTORE_THREADS + threadIdx.x;
  if (i < a.n_values && !hg_valstore_rehash(a, hg_values_dev::DevTable{a.slot_new}, i)) a.counters[HG_VALSTORE_OVERFLOW] = 1;
}

__global__ __launch_bounds__(HG_VALSTORE_THREADS) void hg_valstore_apply_kernel(HgValStoreArgs a) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * HG_VALSTORE_THREADS + threadIdx.x;
  if (j <= a.n_groups && !hg_valstore_apply(a, hg_values_dev::DevTable{a.slot}, j)) a.counters[HG_VALSTORE_OVERFLOW] = 1;
}

__global__ __launch_bounds__(HG_VALSTORE_THREADS) void hg_valstore_place_kernel(HgValRankArgs a) {
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * HG_VALSTORE_THREADS + threadIdx.x;
  if (r <= a.n_rows) hg_valstore_place(a, r);
}

hipError_t hg_valstore_launch(const HgValStoreArgs &a, HgValStoreStep step, hipStream_t stream) {
  const dim3 block(HG_VALSTORE_THREADS);
  const auto blocks = [](uint64_t n) { return dim3(static_cast<uint32_t>((n + HG_VALSTORE_THREADS - 1) / HG_VALSTORE_THREADS)); };
  switch (step) {
    case HgValStoreStep::Lookup:
      if (a.n_groups) hipLaunchKernelGGL(hg_valstore_lookup_kernel, blocks(a.n_groups), block, 0, stream, a);
      break;
    case HgValStoreStep::Long:
      if (a.n_groups) hipLaunchKernelGGL(hg_valstore_long_kernel, dim3(static_cast<uint32_t>(std::min<uint64_t>((a.n_groups + 3) / 4, HG_VALUES_LONG_BLOCKS))), block, 0, stream, a);
      break;
    case HgValStoreStep::Size:
      hipLaunchKernelGGL(hg_valstore_size_kernel, blocks(a.n_groups + 1), block, 0, stream, a);
      break;
    case HgValStoreStep::Rehash:
      if (a.n_values) hipLaunchKernelGGL(hg_valstore_rehash_kernel, blocks(a.n_values), block, 0, stream, a);
      break;
    case HgValStoreStep::Apply:
      hipLaunchKernelGGL(hg_valstore_apply_kernel, blocks(a.n_groups + 1), block, 0, stream, a);
      break;
  }
  return hipGetLastError();
}

hipError_t hg_valstore_place_launch(const HgValRankArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(hg_valstore_place_kernel, dim3(static_cast<uint32_t>((a.n_rows + 1 + HG_VALSTORE_THREADS - 1) / HG_VALSTORE_THREADS)), dim3(HG_VALSTORE_THREADS), 0, stream, a);
  return hipGetLastError();
}
