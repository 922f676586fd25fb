// gfx950 kernels of the gather stage (hg_gather_lines): the bytes of every line piece the last scan left a
// record for, in one compact ordered buffer (hg_gather.h has the rules and every scalar routine; HgGather::run in hg_engine.hip
// is the launch sequence).  On the caller's stream:
//
//   hg_gather_flag_kernel   a lane per record of the two lists: does it head a (segment, line)?
//   (exclusive scan of the flags: rocPRIM)
//   hg_gather_entry_kernel  a lane per record: a head finds its entry index (its own heads before it plus a lower bound in the
//                           other list), the optional parts (one text byte is read for the terminator) and writes the entry,
//                           its size and the per-entry arrays.
//   hg_gather_first_kernel  a lane per segment: first_entry[s].
//   (exclusive scan of the sizes, 64-bit: rocPRIM; the host reads the two totals to size the output)
//   hg_gather_span_kernel   a lane per span of HG_GATHER_TILE output bytes: the entry the span begins in (binary search in `off`).
//   hg_gather_copy_kernel   a workgroup per span, whatever the entries are: it stages the offsets of its entries in LDS, then every
//                           lane builds 16 output bytes at a time (a search in LDS, the entry, its text) and stores them as one
//                           aligned 16-byte word, 4 KiB per step coalesced over the workgroup.  A 1 GiB piece and ten million
//                           20-byte lines spread over the chip alike.
//
// No atomics.  The output buffer is a multiple of 16 bytes with 16 of slack; the bytes past n_bytes in the last word
// are written as 0.  Text reads: hg_gather.h (never past nbytes rounded up to 4).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_engine.h"
#include "hg_gather.h"

__global__ __launch_bounds__(256) void hg_gather_flag_kernel(HgGatherArgs a) {
  const uint64_t n = a.main.n + a.ctx.n, r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r < n) a.head[r] = hg_gather_flag(a, r);
  else if (r == n) a.head[r] = 0;
}

__global__ __launch_bounds__(256) void hg_gather_entry_kernel(HgGatherArgs a) {
  const uint64_t n = a.main.n + a.ctx.n, r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r < n) hg_gather_entry(a, a.text, r);
}

__global__ __launch_bounds__(256) void hg_gather_first_kernel(HgGatherArgs a) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (s <= a.n_seg) a.first_entry[s] = hg_gather_first(a, s);
}

__global__ __launch_bounds__(256) void hg_gather_span_kernel(HgGatherArgs a) {
  const uint64_t n_spans = (a.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE, t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t <= n_spans) a.span[t] = hg_gather_span(a, HG_GATHER_TILE, t);
}

__global__ __launch_bounds__(HG_GATHER_THREADS) void hg_gather_copy_kernel(HgGatherArgs a) {
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
    const HgGatherChunk c = hg_gather_chunk(a, a.text, pos, j, begin, end);
    *reinterpret_cast<uint4 *>(a.out + pos) = make_uint4(c.w0, c.w1, c.w2, c.w3);
  }
}

hipError_t hg_gather_launch(const HgGatherArgs &a, HgGatherStep step, hipStream_t stream) {
  const uint64_t n = a.main.n + a.ctx.n;
  switch (step) {
    case HgGatherStep::Flag:
      hipLaunchKernelGGL(hg_gather_flag_kernel, dim3(static_cast<uint32_t>((n + 1 + 255) / 256)), dim3(256), 0, stream, a);
      break;
    case HgGatherStep::Entry:
      if (n) hipLaunchKernelGGL(hg_gather_entry_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, stream, a);
      break;
    case HgGatherStep::First:
      hipLaunchKernelGGL(hg_gather_first_kernel, dim3(static_cast<uint32_t>((a.n_seg + 1 + 255) / 256)), dim3(256), 0, stream, a);
      break;
    case HgGatherStep::Span:
      if (a.n_bytes)
        hipLaunchKernelGGL(hg_gather_span_kernel, dim3(static_cast<uint32_t>(((a.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE + 1 + 255) / 256)), dim3(256), 0, stream, a);
      break;
    case HgGatherStep::Copy:
      if (a.n_bytes)
        hipLaunchKernelGGL(hg_gather_copy_kernel, dim3(static_cast<uint32_t>((a.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE)), dim3(HG_GATHER_THREADS), 0, stream, a);
      break;
  }
  return hipGetLastError();
}
