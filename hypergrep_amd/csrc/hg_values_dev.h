// Device bodies of the values stage's hash, long and insert pass, shared by hg_values.hip (SEG = false: hg_count_values) and
// hg_rank.hip (SEG = true: the segment in the key; hg_values.h, KEY).  What each pass does, its atomics and its bounds are
// described at the head of hg_values.hip; the SEG bodies differ in the key word the hash pass leaves per part, in the value a
// hash starts from and in the comparison of hg_values_candidate, and in nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_values.h"

namespace hg_values_dev {

struct DevTable {
  unsigned long long *slot;
  __device__ uint64_t load(uint64_t i) const { return __atomic_load_n(&slot[i], __ATOMIC_RELAXED); }
  __device__ uint64_t claim(uint64_t i, uint64_t word) const { return atomicCAS(&slot[i], static_cast<unsigned long long>(HG_VALUES_EMPTY), static_cast<unsigned long long>(word)); }
};

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), lane), hi = __shfl(static_cast<uint32_t>(v >> 32), lane);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

template <bool SEG>
__device__ __forceinline__ void hash_body(const HgValuesArgs &a) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * HG_VALUES_THREADS + threadIdx.x;
  if (q >= a.n_parts) return;
  uint64_t src;
  const uint32_t len = hg_values_locate(a, q, &src);
  a.src[q] = src;
  a.len[q] = len;
  uint64_t key = 0;
  if (SEG) a.key[q] = key = hg_values_key_word(a.flags, a.part_pattern[q], a.part_seg ? a.part_seg[q] : 0u);
  if (!len) {
    a.hash[q] = 0;
  } else if (hg_values_is_long(len)) {
    a.hash[q] = 0;  // (the long kernel writes it)
    const unsigned long long k = atomicAdd(&a.counters[HG_VALUES_N_LONG], 1ull);
    if (k < a.n_parts) a.long_list[k] = q;
  } else if (SEG) {
    a.hash[q] = hg_values_hash_dwords_from(a.text, hg_values_init_key(len, key), src, len, a.hash_bits);
  } else {
    a.hash[q] = hg_values_hash_dwords(a.text, src, len, a.flags, a.part_pattern[q], a.hash_bits);
  }
}

template <bool SEG>
__device__ __forceinline__ void long_body(const HgValuesArgs &a) {
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
    uint64_t sum = SEG ? hg_values_hash_wave_lane_from(a.text, hg_values_init_key(len, a.key[q]), src, len, lane)
                       : hg_values_hash_wave_lane(a.text, src, len, a.flags, a.part_pattern[q], lane);
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
      if (hg_values_candidate<SEG>(a, w, q, h, &rep) && __all(hg_values_equal_wave_lane(a.text, a.src[rep], src, len, lane))) {
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

template <bool SEG>
__device__ __forceinline__ void insert_body(const HgValuesArgs &a) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * HG_VALUES_THREADS + threadIdx.x;
  const uint32_t lane = threadIdx.x & (HG_VALUES_WAVE - 1);
  const DevTable t{a.slot};
  uint64_t s = HG_VALUES_NO_SLOT;
  bool mine = false;
  if (q < a.n_parts) {
    const uint32_t len = a.len[q];
    mine = len != 0 && !hg_values_is_long(len);
    if (mine) s = hg_values_insert<SEG>(a, a.text, t, q);
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

}  // namespace hg_values_dev
