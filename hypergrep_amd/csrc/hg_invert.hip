// gfx950 kernels of the inverted match (hg_scan_device_invert): after a scan's hits are final, enumerate in order the line
// pieces none of them lies in.  Wave64, one wave per 16 KiB tile, three steps on the caller's stream:
//
//   hg_invert_count_kernel   per tile: pieces that start in it (from the scan's tile states alone: hg_invert_first_piece of
//                            this tile and the next) minus the distinct hit lines among them.  No text is read.
//   (exclusive scan of the counts: rocPRIM, hg_engine.hip)
//   hg_invert_write_kernel   per tile with a non-zero count: stream the tile once (16 B per lane, 1 KiB per row), find the
//                            newlines with ballots, number the pieces, drop the ones in the hit list and write the two
//                            16-byte records of the others at the tile's offset.  The output is ordered with no sort.
//                            The walk is wave_write_tile (hg_wave_dev.h), shared with the context stage.
//
// Byte/integer work, HBM-bound; a tile whose pieces all matched is skipped without touching its text.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_invert.h"
#include "hg_wave_dev.h"

static_assert(HG_ID_INVERT == HG_NONE32, "hg_invert_record writes HG_NONE32 as the id");

namespace {
constexpr uint32_t kInvertThreads = 256;  // four waves, a tile each
constexpr uint32_t kInvertWaves = kInvertThreads / 64;

}  // namespace

__global__ __launch_bounds__(kInvertThreads) void hg_invert_count_kernel(HgInvertArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kInvertWaves + wave; t < a.ntiles; t += static_cast<uint64_t>(gridDim.x) * kInvertWaves) {
    auto first_piece = [&](uint64_t tile) {
      const uint64_t t0 = tile << HG_TILE_SHIFT, t1 = t0 + HG_TILE_BYTES < a.nbytes ? t0 + HG_TILE_BYTES : a.nbytes;
      return hg_invert_first_piece(a.bases[tile], a.sums[tile], t0, t1, a.bs1);
    };
    const uint64_t f0 = first_piece(t), f1 = t + 1 < a.ntiles ? first_piece(t + 1) : a.end_piece;
    const uint64_t h0 = hg_invert_lower_bound(a.hits, 0, a.n_hits, f0), h1 = hg_invert_lower_bound(a.hits, h0, a.n_hits, f1);
    uint32_t c = 0;  // distinct hit lines among the tile's pieces (hg_invert_hit_lines, a lane per record)
    for (uint64_t i = h0 + lane; i < h1; i += 64) c += (i == h0 || a.hits[i].line_no != a.hits[i - 1].line_no) ? 1u : 0u;
    c = wave_inclusive_scan(c, lane);
    if (lane == 63) a.count[t] = f1 - f0 - c;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.count[a.ntiles] = 0;
}

__global__ __launch_bounds__(kInvertThreads) void hg_invert_write_kernel(HgInvertArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kInvertWaves + wave; t < a.ntiles; t += static_cast<uint64_t>(gridDim.x) * kInvertWaves) {
    wave_write_tile(a.text, a.nbytes, a.bs1, t, a.bases, a.sums, a.hits, a.n_hits, a.pos, a.out_hits, a.out_aux, lane,
                    [&](uint64_t h, uint64_t number) { return hg_invert_selected(a.hits, h, a.n_hits, number) ? HG_ID_INVERT : HG_WALK_SKIP; });
  }
}

hipError_t hg_invert_launch(const HgInvertArgs &a, bool write, uint32_t num_cus, hipStream_t stream) {
  if (a.ntiles == 0) return hipSuccess;
  const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((a.ntiles + kInvertWaves - 1) / kInvertWaves, static_cast<uint64_t>(num_cus) * 8));
  if (write) hipLaunchKernelGGL(hg_invert_write_kernel, dim3(blocks), dim3(kInvertThreads), 0, stream, a);
  else hipLaunchKernelGGL(hg_invert_count_kernel, dim3(blocks), dim3(kInvertThreads), 0, stream, a);
  return hipGetLastError();
}
