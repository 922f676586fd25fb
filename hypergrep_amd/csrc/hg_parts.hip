// gfx950 kernels of the parts stage (hg_scan_device_parts, grep -o): after a scan's hits are final, the matched parts of
// every line piece that has a hit, over all expressions at once (hg_parts.h has the definition and the scalar routines).
// Wave64, one wave per workgroup, the shape of the invert and context stages on the caller's stream:
//
//   hg_parts_kernel<false>   count: a wave per hit; the hit that is the first of its line (the hits are ordered by line)
//                            heads a piece and its wave walks that piece, every other wave moves on after two loads.
//                            count[i] = parts of the piece headed by hit i, 0 for every other hit.
//   (exclusive scan of the counts: rocPRIM, hg_engine.hip)
//   hg_parts_kernel<true>    write: the same walk, the parts of the piece headed by hit i go to out[pos[i] ..], so the
//                            records are ordered by (line, from) without a sort.
//
// The walk of a piece.  Lanes are 64 consecutive candidate starts.  Each lane runs, for every expression in turn, the
// anchored forward walk of hg_parts.h from its start (hg_parts_walk: the kernel and the host replay share it) and keeps the
// longest end and the lowest expression that reaches it.  A ballot then picks the lowest lane at or behind the cursor that
// has a match: its start, end and expression are the next part, the cursor jumps to the end, and the ballot is asked again
// (the lanes behind the new cursor keep what they found: a match is judged in the piece's real context, not from the
// cursor).  When no lane is left the next 64 starts follow, from the cursor if that lies further on.  A lane tries only the
// expressions that can start with its byte: HgPartsArgs::first is a bitmap per byte value over the expressions (bit j of row
// c: init & reach[c] of expression j is not empty; the engine builds it from the database's tables), walked in ascending
// expression order, so the lowest expression wins a tie as in hg_parts_at.
// State: one or two words in registers; more (up to HG_MAX_W) per lane in LDS, lane-interleaved as in hg_som.hip.
// The text is read byte-wise, inside [start, start + len) of pieces that have a hit only: neighbouring lanes read
// neighbouring bytes, and a walk's next byte is its neighbour lane's current one, so the bytes come from L1 / L2.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_parts.h"
#include "hg_parts_dev.h"  // kPartsThreads, RegState / LdsState, lane_parts_at: shared with hg_segparts.hip

template <bool WRITE>
__global__ __launch_bounds__(kPartsThreads) void hg_parts_kernel(HgPartsArgs a) {
  extern __shared__ uint32_t parts_lds[];
  const uint32_t lane = threadIdx.x;
  for (uint64_t h = blockIdx.x; h < a.n_hits; h += gridDim.x) {  // (wave-uniform: hit h heads a piece or the wave moves on)
    const uint64_t line_no = a.hits[h].line_no;
    if (h != 0 && a.hits[h - 1].line_no == line_no) {
      if (!WRITE && lane == 0) a.count[h] = 0;
      continue;
    }
    {
      const HgHitAux x = a.aux[h];
      const uint8_t *data = a.text + x.start;
      const uint32_t len = x.len;
      const uint64_t at = WRITE ? a.pos[h] : 0;
      uint32_t n = 0, cursor = 0;
      for (uint32_t base = 0; base < len;) {
        const uint32_t s = base + lane;
        uint32_t to, pattern;
        lane_parts_at(a, data, len, s, s < len, parts_lds, &to, &pattern);
        for (;;) {
          const uint64_t m = __builtin_amdgcn_ballot_w64(to != 0 && s >= cursor);
          if (!m) break;
          const int w = __builtin_ctzll(m);
          const uint32_t part_to = static_cast<uint32_t>(__shfl(static_cast<int>(to), w)), part_pattern = static_cast<uint32_t>(__shfl(static_cast<int>(pattern), w));
          if (WRITE && lane == 0) {
            a.out[at + n] = HgPart{line_no, base + static_cast<uint32_t>(w), part_to};
            a.out_pattern[at + n] = part_pattern;
          }
          n++;
          cursor = part_to;
        }
        base = cursor > base + 64 ? cursor : base + 64;
      }
      if (!WRITE && lane == 0) a.count[h] = n;
    }
  }
  if (!WRITE && blockIdx.x == 0 && threadIdx.x == 0) a.count[a.n_hits] = 0;
}

hipError_t hg_parts_launch(const HgPartsArgs &a, bool write, uint32_t max_nw, uint32_t num_cus, hipStream_t stream) {
  if (a.n_hits == 0) return hipSuccess;
  const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(a.n_hits, static_cast<uint64_t>(num_cus) * 64));
  const size_t lds = max_nw > 2 ? 2u * max_nw * kPartsThreads * sizeof(uint32_t) : 0u;  // (single- and two-word walks keep their state in registers)
  if (write) hipLaunchKernelGGL(hg_parts_kernel<true>, dim3(blocks), dim3(kPartsThreads), lds, stream, a);
  else hipLaunchKernelGGL(hg_parts_kernel<false>, dim3(blocks), dim3(kPartsThreads), lds, stream, a);
  return hipGetLastError();
}
