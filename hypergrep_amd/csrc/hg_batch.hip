// Batched block scan (hg_scan_blocks): one launch scans many independent short blocks, each exactly as hs_scan's one-launch
// path scans one (hg_nfa_scan_slice over the block's real bytes and real end; include/hypergrep_amd.h, batched block scan,
// and DESIGN.md §8f).
//
// Grid: (group of expressions) x (shard of items), flattened.  A workgroup stages its group's automaton tables in LDS ONCE
// when they fit (HG_BLOCK_SMALL_POOL, as hg_block_small_kernel does per call and hg_flow_scan_kernel per item), then walks
// the items of its shard in rounds (hg_batch.h has the geometry, which the tests' replay runs too): the lanes are cut
// into teams, each team stages one item's text in its share of the LDS text tile with 16-byte loads and runs (expression,
// slice by start position) lanes over it, an end found from two slices emitted once through a bitmap of ends.  Reports
// {item, id, to | single} are gathered in LDS and appended to one array with ONE global atomic per workgroup and round
// (a round with more than HG_BATCH_REPS reports adds the rest one by one).  Past the array's capacity the kernel only
// counts; the host grows the array and repeats the launch.  The last workgroup to finish publishes the count and the call's
// sequence number in pinned memory.
#include <hip/hip_runtime.h>

#include "hg_batch.h"
#include "hg_batch_launch.h"
#include "hg_engine.h"

static_assert(HG_BATCH_ITEM_MAX == HG_BLOCK_SMALL_MAX, "the batch kernel takes what hs_scan's one-launch path takes");
static_assert(HG_BATCH_SINGLE_BIT == HG_HIT_SINGLE_BIT, "raw records carry the SINGLEMATCH bit as the short-block path does");

__global__ __launch_bounds__(256) void hg_block_batch_kernel(HgBatchArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_text[HG_BATCH_ITEM_MAX];
  __shared__ __attribute__((aligned(16))) uint32_t s_pool[HG_BLOCK_SMALL_POOL];
  __shared__ uint32_t s_seen[HG_BATCH_SEEN_WORDS];
  __shared__ HgHit s_rep[HG_BATCH_REPS];
  __shared__ uint32_t s_len[HG_BATCH_MAX_TEAMS];
  __shared__ uint32_t s_off[HG_BATCH_MAX_TEAMS];  // (16-byte units: a launch holds less than 2^32 of them)
  __shared__ uint32_t s_pass[HG_BATCH_MAX_TEAMS];  // passes of each team's item in this round
  __shared__ uint32_t s_n, s_base;
  const uint32_t group = blockIdx.x % a.ngroups, shard = blockIdx.x / a.ngroups;
  const uint32_t first = group * a.ppw, last = min(first + a.ppw, a.npatterns);  // (first < npatterns: the grid is sized so)
  const uint32_t npat = last - first;
  const HgPattern &pl = a.patterns[last - 1];
  const uint32_t lo = a.patterns[first].reach_off, hi = pl.acc_off + 20u * pl.nw;
  const bool staged = hi - lo <= HG_BLOCK_SMALL_POOL;  // (uniform)
  if (staged)
    for (uint32_t i = threadIdx.x; i < hi - lo; i += blockDim.x) s_pool[i] = a.pool[lo + i];
  const uint32_t *pool = staged ? s_pool : a.pool;
  const uint32_t shift = staged ? lo : 0u;
  // items of this shard: shard, shard + nshards, ...
  const uint32_t mine = shard < a.nitems ? (a.nitems - shard + a.nshards - 1) / a.nshards : 0u;
  for (uint32_t cur = 0; cur < mine;) {
    const uint32_t avail = min(mine - cur, HG_BATCH_MAX_TEAMS);
    if (threadIdx.x < avail) {
      const HgBatchItem it = a.items[shard + static_cast<uint64_t>(cur + threadIdx.x) * a.nshards];
      s_len[threadIdx.x] = it.len;
      s_off[threadIdx.x] = static_cast<uint32_t>(it.text_off >> 4);
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();  // (also: the tables are in place; the previous round's reports have left s_rep)
    uint32_t ts;
    const uint32_t taken = hg_batch_round(s_len, avail, npat, blockDim.x, &ts);  // (uniform)
    const uint32_t teams = blockDim.x / ts;
    const uint32_t team = threadIdx.x / ts, tl = threadIdx.x % ts;
    const bool busy = team < taken;
    const uint32_t len = busy ? s_len[team] : 0u;
    uint8_t *text = s_text + team * hg_batch_text_share(teams);
    uint32_t *seen = s_seen + team * hg_batch_seen_share(teams);
    HgBatchGeom g{};
    if (busy) {
      g = hg_batch_geom(npat, len, ts, teams);
      const uint4 *src = reinterpret_cast<const uint4 *>(a.text) + s_off[team];
      for (uint32_t i = tl; i < (len + 15u) >> 4; i += ts) reinterpret_cast<uint4 *>(text)[i] = src[i];
    }
    if (busy && tl == 0) s_pass[team] = g.passes;
    uint32_t passes = 1;  // (uniform: the most passes of any team of the round, known behind the first pass's barrier)
    const uint64_t item = shard + static_cast<uint64_t>(cur + team) * a.nshards;
    for (uint32_t pass = 0; pass < passes; pass++) {
      if (busy && pass < g.passes)
        for (uint32_t i = tl; i < g.epp * g.words; i += ts) seen[i] = 0;
      __syncthreads();  // text and cleared bitmaps are in place
      if (pass == 0)
        for (uint32_t t = 0; t < taken; t++) passes = max(passes, s_pass[t]);
      uint32_t e, slot, from, upto;
      if (busy && pass < g.passes && hg_batch_lane(g, npat, len, pass, tl, &e, &slot, &from, &upto)) {
        HgPattern pat = a.patterns[first + e];
        pat.reach_off -= shift, pat.follow_off -= shift, pat.init_off -= shift, pat.amask_off -= shift, pat.acc_off -= shift;
        const uint32_t single = pat.single ? HG_HIT_SINGLE_BIT : 0u;
        uint32_t *bits = seen + slot * g.words;
        hg_nfa_scan_slice(pool, pat, text, len, from, upto, [&](uint32_t to) {
          if (g.nslices > 1 && (atomicOr(&bits[to >> 5], 1u << (to & 31)) >> (to & 31) & 1u)) return;
          const HgHit rec{item, pat.id, to | single};
          const uint32_t at = atomicAdd(&s_n, 1u);
          if (at < HG_BATCH_REPS) {
            s_rep[at] = rec;
          } else {  // a crowded round: the rest go one by one
            const uint32_t slot_g = atomicAdd(a.d_total, 1u);
            if (slot_g < a.cap) a.out[slot_g] = rec;
          }
        });
      }
      __syncthreads();  // every lane is done with the bitmaps (the next pass clears them) and with s_n
    }
    const uint32_t n = min(s_n, HG_BATCH_REPS);  // (passes >= 1: behind a barrier)
    if (threadIdx.x == 0 && n) s_base = atomicAdd(a.d_total, n);
    __syncthreads();
    if (n) {
      const uint32_t base = s_base;
      for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
        if (base + i < a.cap && base + i >= base) a.out[base + i] = s_rep[i];
    }
    cur += taken;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();  // this workgroup's reports are visible to the host ...
    if (atomicAdd(a.d_done, 1u) == gridDim.x - 1) {  // ... and it was the last one
      a.h_flag[0] = atomicAdd(a.d_total, 0u);
      *a.d_done = 0;
      *a.d_total = 0;
      __threadfence_system();
      __hip_atomic_store(a.h_flag + 1, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

int hg_batch_launch(const HgBatchArgs &args, hipStream_t stream) {
  if (args.nitems == 0 || args.ngroups == 0 || args.nshards == 0) return -1;
  const uint64_t grid = static_cast<uint64_t>(args.ngroups) * args.nshards;
  if (grid > 0x7FFFFFFFull) return -1;
  hipLaunchKernelGGL(hg_block_batch_kernel, dim3(static_cast<uint32_t>(grid)), dim3(256), 0, stream, args);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
