// gfx950 kernels of the segment stage (hg_scan_device_segments): one scan of a buffer of many files turned into per-file
// results.  Wave64, four steps on the caller's stream (hg_segments.h has the rules):
//
//   hg_seg_check_kernel    a lane per segment, BEFORE the scan: the argument check into one flag word.
//   (inverted calls: hg_seg_pad_flag_kernel / hg_seg_pad_write_kernel remove the hits that lie in a pad, in order, BEFORE the
//   invert stage: a piece whose only reports lie in the pad is selected, as the file scanned alone selects it)
//   hg_seg_bases_kernel    a wave per 16 KiB tile: the boundaries inside the tile come from two binary searches; a tile with
//                          none reads no text.  Otherwise the wave streams the tile ONCE (16 B per lane, 1 KiB per row) and
//                          leaves, per 16-byte chunk, the pieces that start in the tile on lines ending before the chunk and
//                          the start of the line open at it (8 KiB of LDS); then a lane per boundary finishes inside its
//                          chunk (hg_seg_pieces_upto).  300 one-line files in a tile cost one walk, not 300.
//   hg_seg_runs_kernel     a lane per segment: its run of surviving records (hg_seg_run: phantom rule and limit), n_lines.
//   (exclusive scan of the run lengths: rocPRIM, hg_engine.hip -> first_record)
//   hg_seg_write_kernel    a lane per record: its segment by binary search, the record made file-relative and written at
//                          first_record[s] + its rank in the run: an ordered compaction with no sort; n_selected counted.
//
// Byte/integer work, HBM-bound.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_segments.h"
#include "hg_wave_dev.h"

namespace {
constexpr uint32_t kSegThreads = 256;
constexpr uint32_t kTileChunks = HG_TILE_BYTES / HG_SEG_CHUNK;
constexpr uint32_t kOpenCarry = 0xFFFFFFFFu;  // the line open at a chunk is the tile's carry-in line
}  // namespace

__global__ __launch_bounds__(kSegThreads) void hg_seg_check_kernel(HgSegArgs a) {
  for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kSegThreads + threadIdx.x; s < a.n_seg; s += static_cast<uint64_t>(gridDim.x) * kSegThreads) {
    const uint32_t bad = hg_seg_check(a.text, a.nbytes, a.seg_start, a.seg_end, a.n_seg, s);
    if (bad) atomicOr(a.flag, bad);
  }
}

// One wave per block: the block's barrier is the wave's, and every lane of it takes the same trips through the tile loop.
__global__ __launch_bounds__(64) void hg_seg_bases_kernel(HgSegArgs a) {
  __shared__ uint32_t s_before[kTileChunks];  // pieces that start in the tile on lines ending before the chunk
  __shared__ uint32_t s_open[kTileChunks];    // tile-relative start of the line open at the chunk, or kOpenCarry
  const uint32_t lane = threadIdx.x;
  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const uint64_t t0 = t << HG_TILE_SHIFT, t1 = t0 + HG_TILE_BYTES < a.nbytes ? t0 + HG_TILE_BYTES : a.nbytes;
    // the boundaries inside [t0, t1)
    uint64_t js0 = hg_seg_lower_bound(a.seg_start, 0, a.n_seg, t0), js1 = js0;
    if (js0 < a.n_seg && a.seg_start[js0] < t1) js1 = hg_seg_lower_bound(a.seg_start, js0, a.n_seg, t1);
    uint64_t je0 = hg_seg_lower_bound(a.seg_end, 0, a.n_seg, t0), je1 = je0;
    if (je0 < a.n_seg && a.seg_end[je0] < t1) je1 = hg_seg_lower_bound(a.seg_end, je0, a.n_seg, t1);
    if (js0 == js1 && je0 == je1) continue;  // no boundary: the tile's text is not read
    const HgTileBase tb = a.bases[t];
    const uint64_t first = hg_invert_first_piece(tb, a.sums[t], t0, t1, a.bs1);
    uint64_t s = tb.cs;  // start of the line open at the current row; wave-uniform, like q
    uint32_t q = 0;      // pieces that start in the tile on the lines that ended in the rows so far
    for (uint32_t row = 0; row < HG_TILE_BYTES && t0 + row < t1; row += 1024) {
      const uint64_t p = t0 + row + lane * 16u;  // this lane's 16 bytes
      uint32_t nlm = 0;
      if (p < t1) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a.text + p);
        nlm = newline_bits16(v) & (t1 - p < 16 ? (1u << (t1 - p)) - 1u : 0xFFFFu);
      }
      const uint32_t rel = row + lane * 16u;
      const uint32_t my_nl_end = nlm ? rel + 32u - hg_clz32(nlm) : 0u;
      const uint64_t nl_lanes = __builtin_amdgcn_ballot_w64(nlm != 0);
      const uint64_t nl_below = nl_lanes & (lane ? ~0ull >> (64u - lane) : 0ull);
      const uint32_t nl_from = __shfl(my_nl_end, nl_below ? 63 - __builtin_clzll(nl_below) : 0, 64);
      const uint64_t s_in = nl_below ? t0 + nl_from : s;  // the line open at this lane's chunk
      uint32_t npieces = 0;  // pieces (that start in the tile) of the lines that END in this lane's bytes
      {
        uint64_t ls = s_in, k0, k1;
        for (uint32_t m = nlm; m; m &= m - 1) {
          const uint64_t e = p + hg_ctz(m) + 1;
          hg_invert_cuts(ls, e, t0, a.bs1, &k0, &k1);
          npieces += static_cast<uint32_t>(k1 - k0);
          ls = e;
        }
      }
      const uint32_t incl = wave_inclusive_scan(npieces, lane);
      s_before[rel >> 4] = q + (incl - npieces);
      s_open[rel >> 4] = s_in >= t0 ? static_cast<uint32_t>(s_in - t0) : kOpenCarry;
      if (nl_lanes) s = t0 + __shfl(my_nl_end, 63 - __builtin_clzll(nl_lanes), 64);
      q += __shfl(incl, 63, 64);
    }
    __syncthreads();
    auto serve = [&](const uint64_t *bounds, uint64_t j0, uint64_t j1, uint64_t *out) {
      for (uint64_t j = j0 + lane; j < j1; j += 64) {
        const uint64_t b = bounds[j];
        const uint32_t c = static_cast<uint32_t>(b - t0) >> 4;  // (b < t1: a chunk the walk has written)
        const uint32_t open = s_open[c];
        out[j] = first + s_before[c] + hg_seg_pieces_upto(a.text, t0 + c * 16u, b, open == kOpenCarry ? tb.cs : t0 + open, t0, a.bs1);
      }
    };
    serve(a.seg_start, js0, js1, a.B);
    serve(a.seg_end, je0, je1, a.E);
    __syncthreads();  // the next tile's walk overwrites the chunk states
  }
}

__global__ __launch_bounds__(kSegThreads) void hg_seg_runs_kernel(HgSegArgs a) {
  for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kSegThreads + threadIdx.x; s < a.n_seg; s += static_cast<uint64_t>(gridDim.x) * kSegThreads) {
    // (a boundary at the text's end lies in no tile: the first piece at or after it is the one past the buffer's last)
    const uint64_t Bs = a.seg_start[s] == a.nbytes ? a.end_piece : a.B[s], Es = a.seg_end[s] == a.nbytes ? a.end_piece : a.E[s];
    uint64_t r0, r2;
    hg_seg_run(a.hits, a.aux, a.n_hits, Bs, Es, a.seg_end[s], a.invert != 0, a.limit, &r0, &r2);
    a.B[s] = Bs;
    a.E[s] = Es;
    a.r0[s] = r0;
    a.kept[s] = r2 - r0;
    a.n_lines[s] = Es - Bs;
    a.n_selected[s] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.kept[a.n_seg] = 0;
}

__global__ __launch_bounds__(kSegThreads) void hg_seg_write_kernel(HgSegArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kSegThreads;
  for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kSegThreads + (threadIdx.x & ~63u); i0 < a.n_hits; i0 += stride) {  // (wave-uniform trips: the ballot below)
    const uint64_t i = i0 + lane;
    uint32_t s = HG_SEG_NONE;
    bool keep = false, new_line = false;
    if (i < a.n_hits) {
      const HgHit h = a.hits[i];
      s = hg_seg_of_line(a.B, a.n_seg, h.line_no);
      if (s != HG_SEG_NONE) {
        const uint64_t r0 = a.r0[s];
        keep = i >= r0 && i - r0 < a.first[s + 1] - a.first[s];
        if (keep) {
          const uint64_t at = a.first[s] + (i - r0);
          hg_seg_map_record(h, a.aux[i], a.B[s], a.seg_start[s], a.seg_end[s], &a.out_hits[at], &a.out_aux[at]);
          a.out_seg[at] = s;
          if (a.from) a.out_from[at] = a.from[i];
          new_line = i == r0 || a.hits[i - 1].line_no != h.line_no;
        }
      }
    }
    // n_selected: the lines of a wave that lies inside one segment are added by one lane
    const uint32_t s_first = __shfl(s, 0, 64);
    const uint64_t lines = __builtin_amdgcn_ballot_w64(new_line);
    if (__builtin_amdgcn_ballot_w64(s != s_first) == 0) {
      if (lane == 0 && lines) atomicAdd(reinterpret_cast<unsigned long long *>(&a.n_selected[s_first]), static_cast<unsigned long long>(__popcll(lines)));
    } else if (new_line) {
      atomicAdd(reinterpret_cast<unsigned long long *>(&a.n_selected[s]), 1ull);
    }
  }
}

// The pad filter of an inverted call, in front of the invert stage: flag the hits that lie in no pad, and (behind the exclusive
// scan of the flags) write those in order.
__global__ __launch_bounds__(kSegThreads) void hg_seg_pad_flag_kernel(HgSegArgs a) {
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSegThreads + threadIdx.x; i < a.n_hits; i += static_cast<uint64_t>(gridDim.x) * kSegThreads)
    a.pad_keep[i] = hg_seg_pad_hit(a.seg_start, a.seg_end, a.n_seg, a.aux[i].start) ? 0u : 1u;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.pad_keep[a.n_hits] = 0;
}
__global__ __launch_bounds__(kSegThreads) void hg_seg_pad_write_kernel(HgSegArgs a) {
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSegThreads + threadIdx.x; i < a.n_hits; i += static_cast<uint64_t>(gridDim.x) * kSegThreads)
    if (a.pad_pos[i + 1] != a.pad_pos[i]) {
      a.out_hits[a.pad_pos[i]] = a.hits[i];
      a.out_aux[a.pad_pos[i]] = a.aux[i];
    }
}

hipError_t hg_segments_launch(const HgSegArgs &a, HgSegStep step, uint32_t num_cus, hipStream_t stream) {
  const auto grid = [&](uint64_t items, uint32_t per_block) { return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, static_cast<uint64_t>(num_cus) * 8))); };
  switch (step) {
    case HgSegStep::Check:
      if (a.n_seg) hipLaunchKernelGGL(hg_seg_check_kernel, dim3(grid(a.n_seg, kSegThreads)), dim3(kSegThreads), 0, stream, a);
      break;
    case HgSegStep::Bases:
      if (a.n_seg && a.ntiles) hipLaunchKernelGGL(hg_seg_bases_kernel, dim3(grid(a.ntiles, 1)), dim3(64), 0, stream, a);
      break;
    case HgSegStep::Runs:
      hipLaunchKernelGGL(hg_seg_runs_kernel, dim3(grid(a.n_seg, kSegThreads)), dim3(kSegThreads), 0, stream, a);
      break;
    case HgSegStep::PadFlag:
      if (a.n_hits) hipLaunchKernelGGL(hg_seg_pad_flag_kernel, dim3(grid(a.n_hits, kSegThreads)), dim3(kSegThreads), 0, stream, a);
      break;
    case HgSegStep::PadWrite:
      if (a.n_hits) hipLaunchKernelGGL(hg_seg_pad_write_kernel, dim3(grid(a.n_hits, kSegThreads)), dim3(kSegThreads), 0, stream, a);
      break;
    case HgSegStep::Write:
      if (a.n_hits && a.n_seg) hipLaunchKernelGGL(hg_seg_write_kernel, dim3(grid(a.n_hits, kSegThreads)), dim3(kSegThreads), 0, stream, a);
      break;
  }
  return hipGetLastError();
}
