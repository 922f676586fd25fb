// Start-of-match pass (HS_FLAG_SOM_LEFTMOST): one launch after the finalize, over the final ordered hits of a scan.
// Lane i takes hit i (hits are ordered by line, so a wave's walks touch neighbouring lines) and computes what the scalar
// reference hg_hit_som (hg_som.h) computes: the leftmost start over the SOM expressions of the hit's id, by walking the
// reverse automaton backwards from `to`.  The text is read backwards in aligned 16-byte chunks, up to four loads in
// flight (walk_back4, hg_confirm_dev.h); the walk of an expression is bounded by its longest match (max_len) when it has
// one, and literal-only expressions alone on their id need no walk at all.  Hits of expressions without the flag get 0.
// The engine launches this kernel only for databases with SOM expressions (HgDb::nsom), so every other scan is unchanged.
// The match-length pass (hg_minlen_kernel, below) is the same walk with an early exit, over a pass's raw reports.
#include <hip/hip_runtime.h>

#include "hg_confirm_dev.h"
#include "hg_engine.h"
#include "hg_som.h"

namespace {

constexpr uint32_t kSomThreads = 64;  // one wave per workgroup: the multi-word state lives in LDS, 2 * nw words per lane

// Walk state: one or two words in registers, or nw words per lane in LDS (lane-interleaved: word w of a lane at
// [w * kSomThreads], so the 64 lanes of a wave hit 64 different banks).
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
  __device__ __forceinline__ uint32_t &R(uint32_t w) { return base[w * kSomThreads]; }
  __device__ __forceinline__ uint32_t &T(uint32_t w) { return base[(n + w) * kSomThreads]; }
};

// hg_nfa_som on the device.  The byte before a position decides that position's entry condition, so the walk keeps ONE
// position pending: visiting byte j finalises position j + 1 (entry condition, start test) and steps the state onto j.
// EARLY (the match-length pass, hg_nfa_minlen): the walk ends at the first start at or below `limit` and returns it;
// starts above `limit` do not count, HG_NONE32 when there is none at or below it.
template <bool EARLY, typename St>
__device__ __forceinline__ uint32_t som_walk(const uint8_t *text, uint64_t a, uint32_t len, uint32_t to, const HgPattern &p, const uint32_t *pool, St &st,
                                             uint32_t limit = 0) {
  const uint32_t nw = st.nw();
  const uint32_t *reach = pool + p.reach_off, *rfollow = pool + p.som_follow_off, *init = pool + p.init_off;
  const uint32_t *amask = pool + p.amask_off, *acc = pool + p.acc_off;
  const uint32_t lo = (p.max_len && to > p.max_len) ? to - p.max_len : 0u;
  const uint32_t floor = lo ? lo - 1 : 0u;  // the lowest byte read: the one before lo decides lo's entry condition
  const uint32_t nc = to == len ? static_cast<uint32_t>(HG_NC_END) : hg_own_ctx(text[a + to], to + 1 == len);
  const uint32_t *ac = acc + (hg_prev_ctx(text[a + to - 1]) * 5 + nc) * nw;
  for (uint32_t w = 0; w < nw; w++) st.R(w) = ac[w];
  uint32_t best = HG_NONE32, q = to - 1, cq = 0;  // pending position and its byte
  bool stopped = false;
  // finalise the pending position q given the context of the byte before it: false = the walk is over
  auto finish = [&](uint32_t pc) {
    const uint32_t *r = reach + cq * nw, *m = amask + (pc * 4 + hg_own_ctx(cq, q + 1 == len)) * nw;
    uint32_t any = 0, start = 0;
    for (uint32_t w = 0; w < nw; w++) {
      const uint32_t x = st.R(w) & r[w] & m[w];
      st.R(w) = x;
      any |= x;
      start |= x & init[w];
    }
    if (EARLY) {
      if (start && q <= limit) {
        best = q;
        return false;
      }
    } else if (start) {
      best = q;
    }
    return any != 0 && q != lo;
  };
  // The text backwards in aligned 16-byte chunks, the (up to) four chunks of a 64-byte line in flight at once, as walk_back4
  // (hg_confirm_dev.h) reads them; the per-byte step is written out once (a visitor inlined per chunk would be four copies of it).
  const uint64_t top = a + to - 1, bottom = a + floor, lowest = bottom & ~15ull;
  uint64_t chunk = top & ~15ull;
  bool more = true;
  while (more) {
    const uint64_t base = chunk & ~63ull;
    auto load = [&](uint32_t j) {
      uint64_t c = base + 16u * j;
      if (c > chunk || c < lowest) c = chunk;  // (not visited: any address that is)
      return *reinterpret_cast<const uint4 *>(text + c);
    };
    // (four values, not an array, and no indexing by a loop counter: a dynamically indexed chunk lands in scratch)
    uint4 v0 = load(0), v1 = load(1), v2 = load(2), v3 = load(3);
#pragma unroll 1
    for (int j = 3; j >= 0 && more; j--) {
      const uint64_t c = base + 16u * static_cast<uint32_t>(j);
      uint4 cv = v3;  // chunk j, its bytes shifted out at the top one by one
      v3 = v2;
      v2 = v1;
      v1 = v0;
      if (c > chunk) continue;
      if (c < lowest) {
        more = false;
        break;
      }
#pragma unroll 1
      for (int i = 15; i >= 0; i--) {
        const uint64_t at = c + static_cast<uint32_t>(i);
        const uint32_t b = cv.w >> 24;  // byte i of the chunk
        cv.w = (cv.w << 8) | (cv.z >> 24);
        cv.z = (cv.z << 8) | (cv.y >> 24);
        cv.y = (cv.y << 8) | (cv.x >> 24);
        cv.x <<= 8;
        if (at > top) continue;
        if (at < bottom) {
          more = false;
          break;
        }
        if (at == top) {
          cq = b;
          continue;
        }
        if (!finish(hg_prev_ctx(b))) {
          stopped = true;
          more = false;
          break;
        }
        // step onto position q - 1: its nodes are the predecessors of the live ones
        for (uint32_t w = 0; w < nw; w++) st.T(w) = 0;
        for (uint32_t w = 0; w < nw; w++)
          for (uint32_t x = st.R(w); x; x &= x - 1) {
            const uint32_t *f = rfollow + (w * 32 + (__ffs(x) - 1)) * nw;
            for (uint32_t k = 0; k < nw; k++) st.T(k) |= f[k];
          }
        for (uint32_t w = 0; w < nw; w++) st.R(w) = st.T(w);
        q--;
        cq = b;
      }
    }
    if (base <= lowest) break;
    chunk = base - 16u;
  }
  if (!stopped && q == 0) finish(HG_PC_START);  // the walk reached the piece start
  return best;
}

}  // namespace

__global__ __launch_bounds__(kSomThreads) void hg_som_kernel(const uint8_t *text, const HgHit *hits, const HgHitAux *aux, uint64_t n,
                                                           const HgPattern *patterns, const uint32_t *pool, const uint32_t *min_lengths, uint32_t *from) {
  extern __shared__ uint32_t som_lds[];
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSomThreads + threadIdx.x;
  if (i >= n) return;
  const HgHitAux x = aux[i];
  const uint32_t to = hits[i].to;
  const HgPattern &p0 = patterns[x.pattern];
  if (!(p0.flags & HG_FLAG_SOM_LEFTMOST)) {
    from[i] = 0;
    return;
  }
  if (p0.som_next == x.pattern && p0.literal_only && p0.max_len && p0.max_len <= to) {
    from[i] = to - p0.max_len;
    return;
  }
  uint32_t best = HG_NONE32, j = x.pattern;
  do {
    const HgPattern &p = patterns[j];
    uint32_t s;
    if (p.nw == 1) {
      RegState<1> st;
      s = som_walk<false>(text, x.start, x.len, to, p, pool, st);
    } else if (p.nw == 2) {
      RegState<2> st;
      s = som_walk<false>(text, x.start, x.len, to, p, pool, st);
    } else {
      LdsState st{som_lds + threadIdx.x, p.nw};
      s = som_walk<false>(text, x.start, x.len, to, p, pool, st);
    }
    // (an expression of a shared id counts only if its own report at `to` survives its min_length: hg_hit_som)
    if (s != HG_NONE32 && to - s >= (min_lengths ? min_lengths[j] : 0u)) best = s < best ? s : best;
    j = p.som_next;
  } while (j != x.pattern);
  from[i] = best;
}

// The match-length pass (hs_expr_ext_t min_length): one launch over the RAW compact reports of a pass, before the finalize
// (the filter applies before the report rules).  Lane i takes raw record i.  Records of expressions without a filtering
// min_length are kept without touching the text; the others are kept iff hg_nfa_minlen holds: the walk above with its
// early exit.  The kept records are compacted into out_*: a wave ballot, ONE global atomic per wave (= workgroup) and the
// lane's rank among the kept lanes below it.  Their order does not matter: the finalize sorts.
__global__ __launch_bounds__(kSomThreads) void hg_minlen_kernel(const uint8_t *text, const HgHit *hits, const HgHitAux *aux, uint32_t n, const HgPattern *patterns,
                                                              const uint32_t *pool, const uint32_t *min_lengths, HgHit *out_hits, HgHitAux *out_aux,
                                                              uint32_t *count) {
  extern __shared__ uint32_t som_lds[];
  const uint32_t i = blockIdx.x * kSomThreads + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const HgHitAux x = aux[i];
    const uint32_t to = hits[i].to, need = min_lengths[x.pattern];
    if (!need) {
      keep = true;
    } else if (to >= need && to <= x.len) {
      const HgPattern &p = patterns[x.pattern];
      const uint32_t limit = to - need;
      uint32_t s;
      if (p.nw == 1) {
        RegState<1> st;
        s = som_walk<true>(text, x.start, x.len, to, p, pool, st, limit);
      } else if (p.nw == 2) {
        RegState<2> st;
        s = som_walk<true>(text, x.start, x.len, to, p, pool, st, limit);
      } else {
        LdsState st{som_lds + threadIdx.x, p.nw};
        s = som_walk<true>(text, x.start, x.len, to, p, pool, st, limit);
      }
      keep = s != HG_NONE32;
    }
  }
  const uint64_t km = __builtin_amdgcn_ballot_w64(keep);
  if (!km) return;
  uint32_t base = 0;
  if (threadIdx.x == 0) base = atomicAdd(count, static_cast<uint32_t>(__popcll(km)));
  base = __builtin_amdgcn_readfirstlane(base);
  if (keep) {
    const uint32_t at = base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(km >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(km), 0u));
    out_hits[at] = hits[i];  // (read again: a record held across the walk went through scratch)
    out_aux[at] = aux[i];
  }
}

hipError_t hg_som_launch(const uint8_t *text, const HgHit *hits, const HgHitAux *aux, uint64_t n, const HgPattern *patterns, const uint32_t *pool, uint32_t max_nw,
                         const uint32_t *min_lengths, uint32_t *from, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + kSomThreads - 1) / kSomThreads;
  const size_t lds = max_nw > 2 ? 2u * max_nw * kSomThreads * sizeof(uint32_t) : 0u;  // (single- and two-word walks keep their state in registers)
  hipLaunchKernelGGL(hg_som_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kSomThreads), lds, stream, text, hits, aux, n, patterns, pool, min_lengths, from);
  return hipGetLastError();
}

hipError_t hg_minlen_launch(const uint8_t *text, const HgHit *hits, const HgHitAux *aux, uint32_t n, const HgPattern *patterns, const uint32_t *pool, uint32_t max_nw,
                            const uint32_t *min_lengths, HgHit *out_hits, HgHitAux *out_aux, uint32_t *count, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t blocks = (n + kSomThreads - 1) / kSomThreads;
  const size_t lds = max_nw > 2 ? 2u * max_nw * kSomThreads * sizeof(uint32_t) : 0u;  // (as hg_som_launch)
  hipLaunchKernelGGL(hg_minlen_kernel, dim3(blocks), dim3(kSomThreads), lds, stream, text, hits, aux, n, patterns, pool, min_lengths, out_hits, out_aux, count);
  return hipGetLastError();
}
