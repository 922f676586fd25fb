// gfx950 kernels of the context stage (hg_scan_device_context, grep -A / -B / -C): after a call's records are final,
// enumerate in order the line pieces around them (hg_context.h has the classes).  Wave64, one wave per 16 KiB tile, three steps
// on the caller's stream, the shape of the invert stage (hg_invert.hip):
//
//   hg_context_count_kernel  per tile: its piece range from the scan's tile states (hg_invert_first_piece of this tile and the
//                            next), then the covered pieces of that range from the hit lines alone (hg_context_tile /
//                            hg_context_contrib, a lane per record) minus the hit lines inside it.  No text is read.
//   (exclusive scan of the counts: rocPRIM, hg_engine.hip)
//   hg_context_write_kernel  per tile with a non-zero count: the invert write pass's walk (wave_write_tile, hg_wave_dev.h: 16 B
//                            per lane, 1 KiB per row, newline and NUL ballots, wave prefix sums, the open line at the tile's
//                            end) with the class of a piece where that pass asks whether a piece is selected, and the
//                            class's id in the record.
//
// Byte/integer work, HBM-bound; a tile without context pieces is skipped without touching its text.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_context.h"
#include "hg_engine.h"
#include "hg_wave_dev.h"

namespace {
constexpr uint32_t kContextThreads = 256;  // four waves, a tile each
constexpr uint32_t kContextWaves = kContextThreads / 64;
}  // namespace

__global__ __launch_bounds__(kContextThreads) void hg_context_count_kernel(HgContextArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kContextWaves + wave; t < a.ntiles; t += static_cast<uint64_t>(gridDim.x) * kContextWaves) {
    auto first_piece = [&](uint64_t tile) {
      const uint64_t t0 = tile << HG_TILE_SHIFT, t1 = t0 + HG_TILE_BYTES < a.nbytes ? t0 + HG_TILE_BYTES : a.nbytes;
      return hg_invert_first_piece(a.bases[tile], a.sums[tile], t0, t1, a.bs1);
    };
    const uint64_t f0 = first_piece(t), f1 = t + 1 < a.ntiles ? first_piece(t + 1) : a.win.end_piece;
    const HgContextTile ct = hg_context_tile(a.hits, a.n_hits, f0, f1, a.win);
    const bool tails = ct.whi < f1;  // the tile holds tail candidates: a second sum tells how many of its records are tails
    uint32_t c = 0, c_plain = 0;     // (two's complement sums of hg_context_contrib; each is the tile's pieces at most)
    for (uint64_t i = ct.r0 + lane; i < ct.r1; i += 64) {
      c += static_cast<uint32_t>(hg_context_contrib(a.hits, i, ct, ct.whi, a.win));
      if (tails) c_plain += static_cast<uint32_t>(hg_context_contrib(a.hits, i, ct, f1, a.win));
    }
    c = wave_inclusive_scan(c, lane);
    if (tails) c_plain = wave_inclusive_scan(c_plain, lane);
    if (lane == 63) {
      const uint64_t count = hg_context_count(ct, ct.whi, static_cast<int32_t>(c));
      a.count[t] = count;
      if (tails) {
        const uint64_t plain = hg_context_count(ct, f1, static_cast<int32_t>(c_plain));
        if (count > plain) atomicAdd(reinterpret_cast<unsigned long long *>(a.n_tail), static_cast<unsigned long long>(count - plain));
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.count[a.ntiles] = 0;
}

__global__ __launch_bounds__(kContextThreads) void hg_context_write_kernel(HgContextArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kContextWaves + wave; t < a.ntiles; t += static_cast<uint64_t>(gridDim.x) * kContextWaves) {
    wave_write_tile(a.text, a.nbytes, a.bs1, t, a.bases, a.sums, a.hits, a.n_hits, a.pos, a.out_hits, a.out_aux, lane, [&](uint64_t h, uint64_t number) {
      const uint32_t cls = hg_context_class(a.hits, h, a.n_hits, number, a.win);
      return cls == HG_CTX_TAIL ? HG_CTX_ID_TAIL : cls == HG_CTX_CONTEXT ? HG_CTX_ID_CONTEXT : HG_WALK_SKIP;
    });
  }
}

hipError_t hg_context_launch(const HgContextArgs &a, bool write, uint32_t num_cus, hipStream_t stream) {
  if (a.ntiles == 0) return hipSuccess;
  const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((a.ntiles + kContextWaves - 1) / kContextWaves, static_cast<uint64_t>(num_cus) * 8));
  if (write) hipLaunchKernelGGL(hg_context_write_kernel, dim3(blocks), dim3(kContextThreads), 0, stream, a);
  else hipLaunchKernelGGL(hg_context_count_kernel, dim3(blocks), dim3(kContextThreads), 0, stream, a);
  return hipGetLastError();
}
