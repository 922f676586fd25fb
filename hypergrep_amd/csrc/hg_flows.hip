// Stream mode (hs_scan_stream, hg_scan_stream_batch): one launch scans the pending writes of a batch of streams, each
// expression's automaton carried across writes (the flow routines of hg_core.h; rules in include/hypergrep_amd.h, stream
// mode, and DESIGN.md §8d).
//
// Grid: (batch item) x (group of HG_FLOW_PPW expressions), flattened.  A workgroup stages its group's automaton tables in LDS
// when they fit (as hg_block_small_kernel does) and walks its item's write in pieces of HG_FLOW_PIECE bytes staged in LDS.
// Per piece the lanes are (expression, slice by start position): slice 0 is seeded with the carried state (of the previous
// piece, or of the stream at the first), the others start empty and inject start states only in their slice, each runs on
// past its slice until its states die.  The state at the piece's end is the OR over slices (LDS atomicOr), the ends found
// twice are emitted once (a bitmap of ends per expression).  After the last piece one lane per expression applies the
// write-end rules (hg_flow_finish) and writes the state back.  Reports go to one pinned array through a device counter;
// the last workgroup to finish publishes the count and the call's sequence number in pinned memory.
// Expressions with start of match (HS_MODE_SOM_HORIZON_*) run in hg_flow_som_kernel instead, launched first.
#include <hip/hip_runtime.h>

#include "hg_engine.h"
#include "hg_flows.h"

namespace {
constexpr uint32_t SEEN_WORDS = HG_FLOW_PIECE / 32 + 1;  // ends 0 .. HG_FLOW_PIECE of a piece
}  // namespace

__global__ __launch_bounds__(256) void hg_flow_scan_kernel(HgFlowArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_text[HG_FLOW_PIECE + 16];
  __shared__ __attribute__((aligned(16))) uint32_t s_pool[HG_BLOCK_SMALL_POOL];
  __shared__ uint32_t s_seen[HG_FLOW_PPW * SEEN_WORDS];
  __shared__ uint32_t s_state[2][HG_FLOW_PPW * HG_MAX_W];  // piece q reads [q & 1] (q > 0), ORs its end state into [(q + 1) & 1]
  __shared__ uint32_t s_emitted;                            // bit j: expression j of the group has reported in this call
  const uint32_t group = blockIdx.x % a.ngroups, item = blockIdx.x / a.ngroups;
  const HgFlowItem it = a.items[item];
  const uint32_t first = group * HG_FLOW_PPW, last = min(first + HG_FLOW_PPW, a.npatterns);
  const uint32_t npat = last - first;
  const HgPattern &pl = a.patterns[last - 1];
  const uint32_t lo = a.patterns[first].reach_off, hi = pl.acc_off + 20u * pl.nw;
  const bool staged = hi - lo <= HG_BLOCK_SMALL_POOL;  // (uniform)
  if (staged)
    for (uint32_t i = threadIdx.x; i < hi - lo; i += blockDim.x) s_pool[i] = a.pool[lo + i];
  if (threadIdx.x == 0) s_emitted = 0;
  __syncthreads();  // the tables and s_emitted are in place before any lane reads them (a zero-length item runs no piece loop)
  const uint32_t *pool = staged ? s_pool : a.pool;
  const uint32_t j = threadIdx.x % npat, k = threadIdx.x / npat;  // expression of the group, slice
  HgPattern pat = a.patterns[first + j];
  if (staged) pat.reach_off -= lo, pat.follow_off -= lo, pat.init_off -= lo, pat.amask_off -= lo, pat.acc_off -= lo;
  const bool som = (pat.flags & HG_FLAG_SOM_LEFTMOST) != 0;  // (run and written back by hg_flow_som_kernel)
  const uint32_t nw = pat.nw;
  const uint32_t off = a.soff[first + j];
  const uint32_t *sin = a.state_in + static_cast<uint64_t>(item) * a.swords + off;
  uint32_t *sout = a.state_out + static_cast<uint64_t>(item) * a.swords + off;
  const uint32_t hdr = sin[0];
  const bool dead = (hdr & HG_FLOW_DEAD) != 0;
  const uint8_t *txt = a.text + it.text_off;
  const uint32_t len = it.len;
  const bool close = (it.flags & HG_FLOW_ITEM_CLOSE) != 0;
  const bool held_now = !close && len > 0 && txt[len - 1] == '\n' && (hdr & HG_FLOW_HOLD);
  const uint32_t stop_w = held_now ? len - 1 : len;  // (len > 0) lanes test and step positions [0, stop_w)
  const uint32_t most = blockDim.x / npat;
  const uint32_t npieces = (len + HG_FLOW_PIECE - 1) / HG_FLOW_PIECE;
  HgHit *out = a.out;
  uint32_t S[HG_MAX_W];  // a lane's state (one array for the piece loop and the write's end: fewer registers)
  for (uint32_t q = 0; q < npieces; q++) {
    const uint32_t pbase = q * HG_FLOW_PIECE, plen = min(HG_FLOW_PIECE, len - pbase);
    const uint32_t chunks = (plen + 15u) >> 4;  // (the staging area is readable up to each write's length rounded up to 16)
    for (uint32_t i = threadIdx.x; i < chunks; i += blockDim.x) reinterpret_cast<uint4 *>(s_text)[i] = reinterpret_cast<const uint4 *>(txt + pbase)[i];
    for (uint32_t i = threadIdx.x; i < npat * SEEN_WORDS; i += blockDim.x) s_seen[i] = 0;
    for (uint32_t i = threadIdx.x; i < npat * HG_MAX_W; i += blockDim.x) s_state[(q + 1) & 1][i] = 0;
    // reported in an EARLIER piece: read before the barrier, behind which lanes of this piece may set their bits
    const bool gone = pat.single && ((s_emitted >> j) & 1u);  // (uniform per expression)
    __syncthreads();
    const uint32_t slice_len = max(8u, (plen + most - 1) / most);
    const uint32_t nslices = (plen + slice_len - 1) / slice_len;
    if (!dead && !som && !gone && k < nslices) {
      const uint32_t from = k * slice_len, upto = min(from + slice_len, plen);
      const uint32_t pstop = min(stop_w - pbase, plen);
      for (uint32_t w = 0; w < HG_MAX_W; w++) S[w] = 0;
      uint32_t pc = 0, em = 0;
      bool skip = false;
      auto emit_at = [&](int32_t i) {  // write-relative position i, piece-relative pi = i - pbase (-1: the held '\n')
        const int32_t pi = i - static_cast<int32_t>(pbase);
        if (pi >= 0 && (atomicOr(&s_seen[j * SEEN_WORDS + (pi >> 5)], 1u << (pi & 31)) >> (pi & 31) & 1u)) return;
        const uint32_t slot = atomicAdd(a.d_total, 1u);
        if (slot < a.cap) out[slot] = HgHit{(static_cast<uint64_t>(first + j) << 32) | item, pat.id, static_cast<uint32_t>(i + 1)};
      };
      if (k == 0 && q == 0) {
        for (uint32_t w = 0; w < nw; w++) S[w] = sin[1 + w];
        pc = hdr & HG_FLOW_PC;
        skip = (hdr & HG_FLOW_ACC_DONE) != 0;
        if (hdr & HG_FLOW_HELD) {
          em |= hg_flow_unhold(pool, pat, S, &pc, false, skip, emit_at);
          skip = false;
        }
      } else if (k == 0) {
        for (uint32_t w = 0; w < nw; w++) S[w] = s_state[q & 1][j * HG_MAX_W + w];
        pc = hg_prev_ctx(txt[pbase - 1]);
      } else {
        pc = hg_prev_ctx(s_text[from - 1]);
      }
      const uint32_t final_nl = close && q + 1 == npieces ? plen - 1 : HG_NONE32;
      if (!(pat.single && em))
        em |= hg_flow_scan_slice(pool, pat, s_text, from, upto, pstop, final_nl, S, pc, skip, [&](uint32_t i) { emit_at(static_cast<int32_t>(pbase + i)); });
      if (em) atomicOr(&s_emitted, 1u << j);
      if (!(pat.single && em))  // (an expression that stops at its first end is not run again: its state is not needed)
        for (uint32_t w = 0; w < nw; w++)
          if (S[w]) atomicOr(&s_state[(q + 1) & 1][j * HG_MAX_W + w], S[w]);
    }
    __syncthreads();
  }
  if (k == 0 && !som) {  // the write's end: one lane per expression
    for (uint32_t w = 0; w < HG_MAX_W; w++) S[w] = 0;
    uint32_t h = hdr;
    if (!dead) {
      uint32_t pc, em = (s_emitted >> j) & 1u;
      int32_t stop;
      bool held, acc_done;
      if (len == 0) {
        for (uint32_t w = 0; w < nw; w++) S[w] = sin[1 + w];
        held = (hdr & HG_FLOW_HELD) != 0;
        acc_done = (hdr & HG_FLOW_ACC_DONE) != 0;
        pc = hdr & HG_FLOW_PC;
        stop = held ? -1 : 0;
      } else {
        for (uint32_t w = 0; w < nw; w++) S[w] = s_state[npieces & 1][j * HG_MAX_W + w];
        held = held_now;
        stop = static_cast<int32_t>(stop_w);
        pc = stop_w > 0 ? hg_prev_ctx(txt[stop_w - 1]) : ((hdr & HG_FLOW_HELD) ? HG_PC_NL : (hdr & HG_FLOW_PC));
        acc_done = stop_w == 0 && !(hdr & HG_FLOW_HELD) && (hdr & HG_FLOW_ACC_DONE);
      }
      const bool gone = pat.single && em;
      if (!gone) {
        h = hg_flow_finish(pool, pat, S, pc, hdr, stop, held, acc_done, close, &em, [&](int32_t i) {
          const uint32_t slot = atomicAdd(a.d_total, 1u);
          if (slot < a.cap) out[slot] = HgHit{(static_cast<uint64_t>(first + j) << 32) | item, pat.id, static_cast<uint32_t>(i + 1)};
        });
      }
      if (pat.single && em) {
        h = (hdr & HG_FLOW_HOLD) | HG_FLOW_DEAD;
        for (uint32_t w = 0; w < nw; w++) S[w] = 0;
      }
    }
    sout[0] = h;
    for (uint32_t w = 0; w < nw; w++) sout[1 + w] = S[w];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();  // this workgroup's reports and states are visible to the host ...
    if (atomicAdd(a.d_done, 1u) == gridDim.x - 1) {  // ... and it was the last one
      a.h_flag[0] = atomicAdd(a.d_total, 0u);
      *a.d_done = 0;
      *a.d_total = 0;
      __threadfence_system();
      __hip_atomic_store(a.h_flag + 1, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// Start of match (HS_MODE_SOM_HORIZON_*): one lane per (item, SOM expression) walks the item's write serially
// (hg_flow_som_write: a start is the minimum over predecessors, not linear in the state, so the write is not sliced).  The
// starts of the automaton's nodes live in two buffers of device memory per lane (no per-node array in registers, where the
// compiler would put it in scratch).  Lanes are expression-major (neighbouring lanes: one expression, consecutive items) and
// the buffers node-major: SOM expression k owns 2 x nitems x nnodes starts from nitems x 2 x (nodes of the SOM expressions
// before k), node t of item i at t x nitems + i, so lanes that touch the same node touch neighbouring words.  Reports go to the same array and counter as hg_flow_scan_kernel's, with the start in
// from_out; that kernel runs next on the stream and publishes the count.
__global__ __launch_bounds__(64) void hg_flow_som_kernel(HgFlowArgs a, uint32_t nitems) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nitems * a.nsom) return;
  const uint32_t k = g / nitems, item = g % nitems, e = a.som_list[k];
  const HgFlowItem it = a.items[item];
  const HgPattern pat = a.patterns[e];
  const uint32_t nw = pat.nw;
  const uint32_t *sin = a.state_in + static_cast<uint64_t>(item) * a.swords + a.soff[e];
  uint32_t *sout = a.state_out + static_cast<uint64_t>(item) * a.swords + a.soff[e];
  int64_t *base = a.som_work + static_cast<uint64_t>(nitems) * 2u * a.som_list[a.nsom + k] + item;
  HgSomStarts st{base, nitems}, tmp{base + static_cast<uint64_t>(nitems) * pat.nnodes, nitems};
  const uint32_t hdr = sin[0];
  uint32_t S[HG_FLOW_SOM_W];
  for (uint32_t w = 0; w < HG_FLOW_SOM_W; w++) S[w] = w < nw ? sin[1 + w] : 0u;
  hg_flow_som_load(sin + 1 + nw, a.som_width, S, nw, (hdr & HG_FLOW_HELD) ? -1 : 0, st);
  int32_t carried = 0;
  const uint32_t h = hg_flow_som_write(a.pool, pat, a.text + it.text_off, it.len, (it.flags & HG_FLOW_ITEM_CLOSE) != 0, hdr, S, &st, &tmp, &carried,
                                       [&](int32_t i, int64_t s) {
                                         const uint32_t slot = atomicAdd(a.d_total, 1u);
                                         if (slot < a.cap) {
                                           a.out[slot] = HgHit{(static_cast<uint64_t>(e) << 32) | item, pat.id, static_cast<uint32_t>(i + 1)};
                                           a.from_out[slot] = s;
                                         }
                                       });
  sout[0] = h;
  for (uint32_t w = 0; w < nw; w++) sout[1 + w] = S[w];
  hg_flow_som_store(sout + 1 + nw, a.som_width, S, pat.nnodes, carried, st);
}

int hg_flow_launch(const HgFlowArgs &args, uint32_t nitems, hipStream_t stream) {
  if (nitems == 0 || args.ngroups == 0) return -1;
  const uint64_t grid = static_cast<uint64_t>(nitems) * args.ngroups;
  if (grid > 0x7FFFFFFFull) return -1;
  if (args.nsom) {
    const uint64_t lanes = static_cast<uint64_t>(nitems) * args.nsom;
    if (lanes > 0xFFFFFFFFull) return -1;
    hipLaunchKernelGGL(hg_flow_som_kernel, dim3(static_cast<uint32_t>((lanes + 63) / 64)), dim3(64), 0, stream, args, nitems);
  }
  hipLaunchKernelGGL(hg_flow_scan_kernel, dim3(static_cast<uint32_t>(grid)), dim3(256), 0, stream, args);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
