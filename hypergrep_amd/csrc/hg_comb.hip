// Combination pass (HS_FLAG_COMBINATION, HS_FLAG_QUIET): runs over the final ordered hits of a scan pass, before the
// start-of-match pass.  Lane i takes hit i: it finds its piece's run of hits (binary searches on line_no), then hands on what
// the scalar routine hg_comb_hit (hg_comb.h) yields: the hit itself unless its expression is QUIET, and a report (C.id, to)
// for every combination C its id feeds that is true at its `to` (one binary search per operand in the run, sorted by
// (id, to)).  The engine launches the kernel twice: once to count each lane's records, then, after an exclusive scan of the
// counts has sized the output, to write them at their positions.  The union is then ordered and filtered by the compact
// finalize (HgScanner::finalize_compact: the report rules of hg_post.h), like any raw hits.
// Launched only for databases with combinations or QUIET expressions (HgDb::comb_pass), so every other scan is unchanged.
#include <hip/hip_runtime.h>

#include "hg_comb.h"
#include "hg_engine.h"

namespace {

constexpr uint32_t kCombThreads = 256;

// [lo, hi) of the hits of hit i's piece (hits ordered by line_no)
__device__ __forceinline__ void piece_run(const HgHit *hits, uint64_t n, uint64_t i, uint64_t line, uint64_t *lo, uint64_t *hi) {
  uint64_t a = 0, b = i;
  while (a < b) {
    const uint64_t m = a + ((b - a) >> 1);
    if (hits[m].line_no < line) a = m + 1;
    else b = m;
  }
  *lo = a;
  a = i + 1;
  b = n;
  while (a < b) {
    const uint64_t m = a + ((b - a) >> 1);
    if (hits[m].line_no <= line) a = m + 1;
    else b = m;
  }
  *hi = a;
}

// EMIT == false: count[i] = records of hit i, count[n] = 0 (the exclusive scan of count then ends with the total).
// EMIT == true: the records of hit i go to out[pos[i] ..]; pos[i] + (their number) <= pos[n], the size of the output.
template <bool EMIT>
__global__ __launch_bounds__(kCombThreads) void hg_comb_kernel(HgCombArgs a) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCombThreads + threadIdx.x;
  if (i > a.n) return;
  if (i == a.n) {
    if (!EMIT) a.count[i] = 0;
    return;
  }
  const HgHit h = a.hits[i];
  const HgHitAux x = a.aux[i];
  uint64_t lo, hi;
  piece_run(a.hits, a.n, i, h.line_no, &lo, &hi);
  const bool quiet = (a.patterns[x.pattern].flags & HG_FLAG_QUIET) != 0;
  uint64_t pos = EMIT ? a.pos[i] : 0;
  const uint32_t k = hg_comb_hit(a.combs, a.words, a.feed, a.nfeed, a.hits, lo, hi, i, quiet, [&](uint32_t id, uint32_t pattern) {
    if (!EMIT) return;
    a.out_hits[pos] = HgHit{h.line_no, id, h.to};
    a.out_aux[pos] = HgHitAux{x.start, x.len, pattern != HG_NONE32 ? pattern : x.pattern};
    pos++;
  });
  if (!EMIT) a.count[i] = k;
}

}  // namespace

hipError_t hg_comb_launch(const HgCombArgs &a, bool emit, hipStream_t stream) {
  const uint64_t blocks = (a.n + 1 + kCombThreads - 1) / kCombThreads;
  if (emit) hipLaunchKernelGGL(hg_comb_kernel<true>, dim3(static_cast<uint32_t>(blocks)), dim3(kCombThreads), 0, stream, a);
  else hipLaunchKernelGGL(hg_comb_kernel<false>, dim3(static_cast<uint32_t>(blocks)), dim3(kCombThreads), 0, stream, a);
  return hipGetLastError();
}
