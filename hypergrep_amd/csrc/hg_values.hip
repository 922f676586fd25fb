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

namespace {

struct DevTable {
  unsigned long long *slot;
  __device__ uint64_t load(uint64_t i) const { return __atomic_load_n(&slot[i], __ATOMIC_RELAXED); }
  __device__ uint64_t claim(uint64_t i, uint64_t word) const { return atomicCAS(&slot[i], static_cast<unsigned long long>(HG_VALUES_EMPTY), static_cast<unsigned long long>(word)); }
};

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), lane), hi = __shfl(static_cast<uint32_t>(v >> 32), lane);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

}  // namespace

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_hash_kernel(HgValuesArgs a) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * HG_VALUES_THREADS + threadIdx.x;
  if (q >= a.n_parts) return;
  uint64_t src;
  const uint32_t len = hg_values_locate(a, q, &src);
  a.src[q] = src;
  a.len[q] = len;
  if (!len) {
    a.hash[q] = 0;
  } else if (hg_values_is_long(len)) {
    a.hash[q] = 0;  // (the long kernel writes it)
    const unsigned long long k = atomicAdd(&a.counters[HG_VALUES_N_LONG], 1ull);
    if (k < a.n_parts) a.long_list[k] = q;
  } else {
    a.hash[q] = hg_values_hash_dwords(a.text, src, len, a.flags, a.part_pattern[q], a.hash_bits);
  }
}

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_long_kernel(HgValuesArgs a) {
  const uint32_t lane = threadIdx.x & (HG_VALUES_WAVE - 1);
  const uint64_t wave = (static_cast<uint64_t>(blockIdx.x) * HG_VALUES_THREADS + threadIdx.x) / HG_VALUES_WAVE;
  const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * (HG_VALUES_THREADS / HG_VALUES_WAVE);
  const uint64_t n_long = std::min<uint64_t>(a.counters[HG_VALUES_N_LONG], a.n_parts), cap = uint64_t{1} << a.table_log2;
  const DevTable t{a.slot};
  for (uint64_t i = wave; i < n_long; i += n_waves) {  // (wave-uniform)
    const uint64_t q = a.long_list[i];
    if (q >= a.n_parts) continue;
    const uint64_t src = a.src[q];
    const uint32_t len = a.len[q];
    uint64_t sum = hg_values_hash_wave_lane(a.text, src, len, a.flags, a.part_pattern[q], lane);
    for (int d = 1; d < static_cast<int>(HG_VALUES_WAVE); d <<= 1) sum += shfl64(sum, static_cast<int>(lane) ^ d);  // (every lane ends with the wave's sum)
    const uint64_t h = hg_values_hash_wave_end(a.text, sum, src, len, a.hash_bits);
    if (lane == 0) a.hash[q] = h;
    const uint64_t mine = hg_values_slot_word(h, q);
    uint64_t s = hg_values_home(h, a.table_log2), found = HG_VALUES_NO_SLOT;
    for (uint64_t probe = 0; probe < cap; probe++, s = (s + 1) & (cap - 1)) {
      uint64_t w = 0;
      if (lane == 0) {
        w = t.load(s);
        if (w == HG_VALUES_EMPTY) {
          const uint64_t old = t.claim(s, mine);
          w = old == HG_VALUES_EMPTY ? mine : old;
        }
      }
      w = shfl64(w, 0);
      if (w == mine) {  // claimed now, or a slot this part claimed (no other part has its index)
        found = s;
        break;
      }
      uint64_t rep;
      // (a long representative was hashed by this kernel: its src and len are the hash kernel's, which is all that is read)
      if (hg_values_candidate(a, w, q, h, &rep) && __all(hg_values_equal_wave_lane(a.text, a.src[rep], src, len, lane))) {
        found = s;
        break;
      }
    }
    if (lane == 0) {
      if (found == HG_VALUES_NO_SLOT) {
        atomicOr(&a.counters[HG_VALUES_OVERFLOW], 1ull);
      } else {
        atomicAdd(&a.count[found], 1ull);
        atomicMin(&a.first[found], static_cast<unsigned long long>(q));
      }
    }
  }
}

__global__ __launch_bounds__(HG_VALUES_THREADS) void hg_values_insert_kernel(HgValuesArgs a) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * HG_VALUES_THREADS + threadIdx.x;
  const uint32_t lane = threadIdx.x & (HG_VALUES_WAVE - 1);
  const DevTable t{a.slot};
  uint64_t s = HG_VALUES_NO_SLOT;
  bool mine = false;
  if (q < a.n_parts) {
    const uint32_t len = a.len[q];
    mine = len != 0 && !hg_values_is_long(len);
    if (mine) s = hg_values_insert(a, a.text, t, q);
  }
  const bool counted = mine && s != HG_VALUES_NO_SLOT;
  if (mine && !counted) atomicOr(&a.counters[HG_VALUES_OVERFLOW], 1ull);
  const unsigned long long act = __ballot(counted);
  if (!act) return;  // (wave-uniform)
  const int leader = __ffsll(act) - 1;
  const uint64_t s0 = shfl64(s, leader);
  if (__ballot(counted && s != s0) == 0) {
    if (lane == static_cast<uint32_t>(leader)) {  // (part indices ascend with the lane: the leader's is the smallest)
      atomicAdd(&a.count[s0], static_cast<unsigned long long>(__popcll(act)));
      atomicMin(&a.first[s0], static_cast<unsigned long long>(q));
    }
  } else if (counted) {
    atomicAdd(&a.count[s], 1ull);
    atomicMin(&a.first[s], static_cast<unsigned long long>(q));
  }
}

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
