// gfx950 kernels of the per-file context stage (hg_scan_device_segments_context, grep -r -A / -B / -C): behind the segment
// stage, enumerate in order the line pieces around the records each file keeps, inside that file only (hg_segctx.h has the
// windows and the classes).  Wave64, the shape of the context stage (hg_context.hip), five steps on the caller's stream:
//
//   hg_segctx_prep_kernel   a lane per surviving record: its packed piece number back (K) and its segment's window (W).
//   hg_segctx_count_kernel  a wave per 16 KiB tile: its piece range from the scan's tile states, then the context pieces of that
//                           range from K and W alone (hg_segctx_contrib, a lane per record).  No text is read.
//   (exclusive scan of the counts: rocPRIM, hg_engine.hip)
//   hg_segctx_write_kernel  a wave per tile with a non-zero count: wave_write_tile's walk (hg_wave_dev.h) with the class of a
//                           piece where it asks whether a piece is selected.  No piece looks up its segment.
//   hg_segctx_map_kernel    a lane per context record: made file-relative in place, its segment noted.
//   hg_segctx_first_kernel  a lane per segment: first_context[s] by binary search in the records' segments.
//
// No sort and no per-record atomic.  Byte/integer work, HBM-bound; a tile without context pieces is skipped without touching
// its text.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_segctx.h"
#include "hg_wave_dev.h"

namespace {
constexpr uint32_t kSegCtxThreads = 256;  // four waves, a tile each
constexpr uint32_t kSegCtxWaves = kSegCtxThreads / 64;

__device__ __forceinline__ uint64_t first_piece(const HgSegCtxArgs &a, uint64_t tile) {
  if (tile >= a.ntiles) return a.end_piece;
  const uint64_t t0 = tile << HG_TILE_SHIFT, t1 = t0 + HG_TILE_BYTES < a.nbytes ? t0 + HG_TILE_BYTES : a.nbytes;
  return hg_invert_first_piece(a.bases[tile], a.sums[tile], t0, t1, a.bs1);
}
// (a wave-uniform value kept in a vector register: the write pass's walk is short of scalar ones)
__device__ __forceinline__ uint32_t in_vgpr(uint32_t x) {
  asm("" : "+v"(x));
  return x;
}
}  // namespace

__global__ __launch_bounds__(kSegCtxThreads) void hg_segctx_prep_kernel(HgSegCtxArgs a) {
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kSegCtxThreads + threadIdx.x; j < a.n_kept; j += static_cast<uint64_t>(gridDim.x) * kSegCtxThreads) {
    const HgHit h = a.seg_hits[j];
    const uint32_t s = a.seg_of[j];
    a.K[j] = HgHit{h.line_no + a.B[s], h.id, h.to};
    // (with a limit a segment has a handful of records: each finds its segment's stop itself)
    a.W[j] = HgSegCtxWin{a.B[s], hg_segctx_stop(a.hits, a.aux, a.n_hits, a.B[s], a.E[s], a.seg_end[s], a.invert != 0, a.limit, a.r0[s], a.kept[s])};
  }
}

__global__ __launch_bounds__(kSegCtxThreads) void hg_segctx_count_kernel(HgSegCtxArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const HgContextWin w = hg_context_win(0, a.end_piece, 0, 0, 0, false);  // no carry, no tail: hg_context_tile's window is the tile
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kSegCtxWaves + wave; t < a.ntiles; t += static_cast<uint64_t>(gridDim.x) * kSegCtxWaves) {
    const HgContextTile ct = hg_context_tile(a.K, a.n_kept, first_piece(a, t), first_piece(a, t + 1), w);
    uint32_t c = 0;  // (two's complement sum of hg_segctx_contrib; the tile's pieces at most)
    for (uint64_t i = ct.r0 + lane; i < ct.r1; i += 64) c += static_cast<uint32_t>(hg_segctx_contrib(a.K, a.W, i, ct, a.before, a.after));
    c = wave_inclusive_scan(c, lane);
    if (lane == 63) a.count[t] = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int32_t>(c)));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.count[a.ntiles] = 0;
}

// (the write pass gets only the fields it reads: the walk is short of scalar registers)
struct HgSegCtxWrite {
  const uint8_t *text;
  uint64_t nbytes, bs1, ntiles;
  uint32_t before, after;
  const HgTileSum *sums;
  const HgTileBase *bases;
  const HgHit *K;
  const HgSegCtxWin *W;
  uint64_t n_kept;
  const uint64_t *pos;
  HgHit *out_hits;
  HgHitAux *out_aux;
};

__global__ __launch_bounds__(kSegCtxThreads) void hg_segctx_write_kernel(HgSegCtxWrite a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t before = in_vgpr(a.before), after = in_vgpr(a.after);
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kSegCtxWaves + wave; t < a.ntiles; t += static_cast<uint64_t>(gridDim.x) * kSegCtxWaves) {
    wave_write_tile(a.text, a.nbytes, a.bs1, t, a.bases, a.sums, a.K, a.n_kept, a.pos, a.out_hits, a.out_aux, lane, [&](uint64_t h, uint64_t number) {
      return hg_segctx_class(a.K, a.W, h, a.n_kept, number, before, after) == HG_CTX_CONTEXT ? HG_CTX_ID_CONTEXT : HG_WALK_SKIP;
    });
  }
}

__global__ __launch_bounds__(kSegCtxThreads) void hg_segctx_map_kernel(HgSegCtxArgs a) {
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kSegCtxThreads + threadIdx.x; j < a.n_ctx; j += static_cast<uint64_t>(gridDim.x) * kSegCtxThreads) {
    HgHit h = a.out_hits[j];
    HgHitAux x = a.out_aux[j];
    a.out_seg[j] = hg_segctx_map_record(a.B, a.seg_start, a.seg_end, a.n_seg, &h, &x);
    a.out_hits[j] = h;
    a.out_aux[j] = x;
  }
}

__global__ __launch_bounds__(kSegCtxThreads) void hg_segctx_first_kernel(HgSegCtxArgs a) {
  for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kSegCtxThreads + threadIdx.x; s <= a.n_seg; s += static_cast<uint64_t>(gridDim.x) * kSegCtxThreads)
    a.first_ctx[s] = hg_segctx_first(a.out_seg, a.n_ctx, s);
}

hipError_t hg_segctx_launch(const HgSegCtxArgs &a, HgSegCtxStep step, uint32_t num_cus, hipStream_t stream) {
  const auto grid = [&](uint64_t items, uint32_t per_block) { return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, static_cast<uint64_t>(num_cus) * 8))); };
  switch (step) {
    case HgSegCtxStep::Prep:
      hipLaunchKernelGGL(hg_segctx_prep_kernel, dim3(grid(a.n_kept, kSegCtxThreads)), dim3(kSegCtxThreads), 0, stream, a);
      break;
    case HgSegCtxStep::Count:
      hipLaunchKernelGGL(hg_segctx_count_kernel, dim3(grid(a.ntiles, kSegCtxWaves)), dim3(kSegCtxThreads), 0, stream, a);
      break;
    case HgSegCtxStep::Write:
      hipLaunchKernelGGL(hg_segctx_write_kernel, dim3(grid(a.ntiles, kSegCtxWaves)), dim3(kSegCtxThreads), 0, stream,
                         HgSegCtxWrite{a.text, a.nbytes, a.bs1, a.ntiles, static_cast<uint32_t>(a.before), static_cast<uint32_t>(a.after), a.sums, a.bases, a.K, a.W, a.n_kept, a.pos, a.out_hits, a.out_aux});
      break;
    case HgSegCtxStep::Map:
      if (a.n_ctx) hipLaunchKernelGGL(hg_segctx_map_kernel, dim3(grid(a.n_ctx, kSegCtxThreads)), dim3(kSegCtxThreads), 0, stream, a);
      break;
    case HgSegCtxStep::First:
      hipLaunchKernelGGL(hg_segctx_first_kernel, dim3(grid(a.n_seg + 1, kSegCtxThreads)), dim3(kSegCtxThreads), 0, stream, a);
      break;
  }
  return hipGetLastError();
}
