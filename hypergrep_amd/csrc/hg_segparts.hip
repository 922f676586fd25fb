// gfx950 kernels of the per-file parts stage (hg_scan_device_segments_parts, grep -r -o): behind the segment stage, the
// matched parts of every line piece a file keeps a record of (hg_segparts.h has the rules, hg_parts.h the walk).  Wave64, one
// wave per workgroup, the shape of the parts stage (hg_parts.hip) on the caller's stream:
//
//   hg_segparts_kernel<false>  count: a wave per surviving record; the record that heads a piece (hg_segparts_head: first of
//                              its segment's line) walks that piece where it lies in the packed text, every other wave moves
//                              on after four loads.  count[i] = parts of the piece headed by record i, 0 for the others.
//   (exclusive scan of the counts: rocPRIM, hg_engine.hip)
//   hg_segparts_kernel<true>   write: the same walk; the parts of the piece headed by record i go to out[pos[i] ..] with the
//                              record's file-relative line, their expressions and the segment beside them: ordered by
//                              (segment, line, from) without a sort, and nothing is renumbered afterwards.
//   hg_segparts_first_kernel   a lane per segment: first_part[s] = pos[first_record[s]].
//
// The walk of a piece, the ballot loop over 64 candidate starts, the first-byte bitmap and the register / LDS state are the
// parts stage's (lane_parts_at, hg_parts_dev.h).  The text is read byte-wise inside [start, start + len) of pieces that have a
// kept record only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_parts_dev.h"
#include "hg_segparts.h"

template <bool WRITE>
__global__ __launch_bounds__(kPartsThreads) void hg_segparts_kernel(HgSegPartsArgs a) {
  extern __shared__ uint32_t segparts_lds[];
  const uint32_t lane = threadIdx.x;
  for (uint64_t h = blockIdx.x; h < a.n_hits; h += gridDim.x) {  // (wave-uniform: record h heads a piece or the wave moves on)
    if (!hg_segparts_head(a.hits, a.seg_of, h)) {
      if (!WRITE && lane == 0) a.count[h] = 0;
      continue;
    }
    const uint64_t line_no = a.hits[h].line_no;
    const uint32_t seg = a.seg_of[h];
    const HgHitAux x = a.aux[h];
    const uint8_t *data = a.text + hg_segparts_offset(a.seg_start, seg, x);
    const uint32_t len = x.len;
    const uint64_t at = WRITE ? a.pos[h] : 0;
    uint32_t n = 0, cursor = 0;
    for (uint32_t base = 0; base < len;) {
      const uint32_t s = base + lane;
      uint32_t to, pattern;
      lane_parts_at(a, data, len, s, s < len, segparts_lds, &to, &pattern);
      for (;;) {
        const uint64_t m = __builtin_amdgcn_ballot_w64(to != 0 && s >= cursor);
        if (!m) break;
        const int w = __builtin_ctzll(m);
        const uint32_t part_to = static_cast<uint32_t>(__shfl(static_cast<int>(to), w)), part_pattern = static_cast<uint32_t>(__shfl(static_cast<int>(pattern), w));
        if (WRITE && lane == 0) {
          a.out[at + n] = HgPart{line_no, base + static_cast<uint32_t>(w), part_to};
          a.out_pattern[at + n] = part_pattern;
          a.out_seg[at + n] = seg;
        }
        n++;
        cursor = part_to;
      }
      base = cursor > base + 64 ? cursor : base + 64;
    }
    if (!WRITE && lane == 0) a.count[h] = n;
  }
  if (!WRITE && blockIdx.x == 0 && threadIdx.x == 0) a.count[a.n_hits] = 0;
}

__global__ __launch_bounds__(256) void hg_segparts_first_kernel(HgSegPartsArgs a) {
  for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; s <= a.n_seg; s += static_cast<uint64_t>(gridDim.x) * 256)
    a.first_part[s] = hg_segparts_first(a.pos, a.first_record, s);
}

hipError_t hg_segparts_launch(const HgSegPartsArgs &a, HgSegPartsStep step, uint32_t max_nw, uint32_t num_cus, hipStream_t stream) {
  if (step == HgSegPartsStep::First) {
    const uint32_t blocks = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((a.n_seg + 1 + 255) / 256, static_cast<uint64_t>(num_cus) * 8)));
    hipLaunchKernelGGL(hg_segparts_first_kernel, dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
  }
  if (a.n_hits == 0) return hipSuccess;
  const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(a.n_hits, static_cast<uint64_t>(num_cus) * 64));
  const size_t lds = max_nw > 2 ? 2u * max_nw * kPartsThreads * sizeof(uint32_t) : 0u;  // (single- and two-word walks keep their state in registers)
  if (step == HgSegPartsStep::Write) hipLaunchKernelGGL(hg_segparts_kernel<true>, dim3(blocks), dim3(kPartsThreads), lds, stream, a);
  else hipLaunchKernelGGL(hg_segparts_kernel<false>, dim3(blocks), dim3(kPartsThreads), lds, stream, a);
  return hipGetLastError();
}
