// gfx950 kernels of the parts gather (hg_gather_parts): the bytes of every matched part the last scan left a record for, or
// every matching line with its parts wrapped in markers, in one compact ordered buffer (hg_partlines.h has the rules and every
// scalar routine; HgPartLines::run in hg_engine.hip is the launch sequence).  On the caller's stream:
//
//   hg_partlines_entry_kernel  a lane per part: the piece's record (a lower bound in the final records), first / last of its
//                              piece from the neighbouring parts, the entry's fields (one text byte is read for the
//                              terminator), its size and the per-entry arrays.
//   (exclusive scan of the sizes, 64-bit: rocPRIM; the host reads the total to size the output)
//   hg_partlines_span_kernel   a lane per span of HG_GATHER_TILE output bytes: the entry the span begins in (binary search in `off`).
//   hg_partlines_copy_kernel   a workgroup per span, whatever the entries are: it stages the offsets of its entries in LDS, then
//                              every lane builds 16 output bytes at a time (a search in LDS, the entry, its text) and stores them
//                              as one aligned 16-byte word, 4 KiB per step coalesced over the workgroup.
//
// No atomics.  The output buffer is a multiple of 16 bytes with 16 of slack; the bytes past n_bytes in the last word are
// written as 0.  Text reads: hg_partlines.h (never past nbytes rounded up to 4).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_partlines.h"

__global__ __launch_bounds__(256) void hg_partlines_entry_kernel(HgPartLinesArgs a) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (q < a.n_parts) hg_partlines_entry(a, a.text, q);
  else if (q == a.n_parts) a.size[q] = 0;
}

__global__ __launch_bounds__(256) void hg_partlines_span_kernel(HgPartLinesArgs a) {
  const uint64_t n_spans = (a.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE, t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t <= n_spans) a.span[t] = hg_partlines_span(a, HG_GATHER_TILE, t);
}

__global__ __launch_bounds__(HG_GATHER_THREADS) void hg_partlines_copy_kernel(HgPartLinesArgs a) {
  __shared__ uint64_t span_off[HG_GATHER_SPAN_OFFSETS];
  const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * HG_GATHER_TILE;  // (< n_bytes: the grid is sized from it)
  const uint64_t tile_last = std::min<uint64_t>(tile + HG_GATHER_TILE, a.n_bytes) - 1;
  // the entries the span's bytes lie in (the span pass found them), and their offsets off[j_lo .. j_hi + 1] in LDS if they fit:
  // a lane's search then costs no trip to memory
  const uint64_t j_lo = a.span[blockIdx.x], j_hi = a.span[blockIdx.x + 1];
  const bool staged = j_hi - j_lo + 2 <= HG_GATHER_SPAN_OFFSETS;
  if (staged) {
    for (uint32_t i = threadIdx.x; i < j_hi - j_lo + 2; i += HG_GATHER_THREADS) span_off[i] = a.off[j_lo + i];
    __syncthreads();
  }
  for (uint32_t step = 0; step < HG_GATHER_TILE / (16 * HG_GATHER_THREADS); step++) {
    const uint64_t pos = tile + (static_cast<uint64_t>(step) * HG_GATHER_THREADS + threadIdx.x) * 16;
    if (pos > tile_last) break;
    uint64_t j, begin, end;
    if (staged) {
      const uint64_t k = hg_gather_find(span_off, 0, j_hi - j_lo, pos);
      j = j_lo + k, begin = span_off[k], end = span_off[k + 1];
    } else {
      j = hg_gather_find(a.off, j_lo, j_hi, pos), begin = a.off[j], end = a.off[j + 1];
    }
    const HgGatherChunk c = hg_partlines_chunk(a, a.text, pos, j, begin, end);
    *reinterpret_cast<uint4 *>(a.out + pos) = make_uint4(c.w0, c.w1, c.w2, c.w3);
  }
}

hipError_t hg_partlines_launch(const HgPartLinesArgs &a, HgPartLinesStep step, hipStream_t stream) {
  switch (step) {
    case HgPartLinesStep::Entry:
      hipLaunchKernelGGL(hg_partlines_entry_kernel, dim3(static_cast<uint32_t>((a.n_parts + 1 + 255) / 256)), dim3(256), 0, stream, a);
      break;
    case HgPartLinesStep::Span:
      if (a.n_bytes)
        hipLaunchKernelGGL(hg_partlines_span_kernel, dim3(static_cast<uint32_t>(((a.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE + 1 + 255) / 256)), dim3(256), 0, stream, a);
      break;
    case HgPartLinesStep::Copy:
      if (a.n_bytes)
        hipLaunchKernelGGL(hg_partlines_copy_kernel, dim3(static_cast<uint32_t>((a.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE)), dim3(HG_GATHER_THREADS), 0, stream, a);
      break;
  }
  return hipGetLastError();
}
