// Device-only half of the parts walks: the per-lane walk state and the lane-level routine that the kernels of the parts stage
// (hg_parts.hip) and of the per-file parts stage (hg_segparts.hip) share.  hg_parts.h has the scalar routines they call.
#pragma once
#include <hip/hip_runtime.h>

#include "hg_parts.h"

namespace {

constexpr uint32_t kPartsThreads = 64;  // one wave per workgroup: the multi-word state lives in LDS, 2 * nw words per lane

template <int NW>
struct RegState {
  uint32_t r[NW], t[NW];
  __device__ __forceinline__ uint32_t nw() const { return NW; }
  __device__ __forceinline__ uint32_t &R(uint32_t w) { return r[w]; }
  __device__ __forceinline__ uint32_t &T(uint32_t w) { return t[w]; }
};
struct LdsState {
  uint32_t *base;  // this lane's first word
  uint32_t n;
  __device__ __forceinline__ uint32_t nw() const { return n; }
  __device__ __forceinline__ uint32_t &R(uint32_t w) { return base[w * kPartsThreads]; }
  __device__ __forceinline__ uint32_t &T(uint32_t w) { return base[(n + w) * kPartsThreads]; }
};

// hg_parts_at on the device for the lane's start s (active lanes only), over the expressions that can start with the lane's byte.
// Args: the stage's argument struct (its `first`, `first_words`, `patterns` and `pool`: HgPartsArgs, HgSegPartsArgs).
template <typename Args>
__device__ __forceinline__ void lane_parts_at(const Args &a, const uint8_t *data, uint32_t len, uint32_t s, bool active, uint32_t *lds, uint32_t *to,
                                              uint32_t *pattern) {
  uint32_t best = 0, who = 0, c0 = 0, pc0 = HG_PC_START;
  if (active) {
    c0 = data[s];
    if (s) pc0 = hg_prev_ctx(data[s - 1]);
  }
  const uint32_t *row = a.first + c0 * a.first_words;
  for (uint32_t fw = 0; fw < a.first_words; fw++)
    for (uint32_t bits = active ? row[fw] : 0u; bits; bits &= bits - 1) {
      const uint32_t j = fw * 32 + hg_ctz(bits);
      const HgPattern &p = a.patterns[j];
      uint32_t e;
      if (p.nw == 1) {
        RegState<1> st;
        e = hg_parts_walk(a.pool, p, data, len, s, c0, pc0, st);
      } else if (p.nw == 2) {
        RegState<2> st;
        e = hg_parts_walk(a.pool, p, data, len, s, c0, pc0, st);
      } else {
        LdsState st{lds + threadIdx.x, p.nw};
        e = hg_parts_walk(a.pool, p, data, len, s, c0, pc0, st);
      }
      if (e > best) {
        best = e;
        who = j;
      }
    }
  *to = best;
  *pattern = who;
}

}  // namespace
