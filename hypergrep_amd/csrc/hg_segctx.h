// Context lines of a buffer of many files (hg_scan_device_segments_context, grep -r -A / -B / -C): the line pieces around the
// records each file KEEPS, enumerated in order on the GPU behind the segment stage, per file: no context crosses a file
// boundary, lands in a pad or on a phantom piece.  The scalar routines here are shared by the kernels (hg_segctx.hip) and the
// host replay of the tests (tests/native/segctxsim.cpp compiles this header for x86); the product only calls them from device
// code.
//
// The stage works in PACKED piece numbers (hg_segments.h: segment s has the pieces [B[s], E[s])).  K is the kept records of
// all segments in packed numbers, ordered by line: segment s's run [r0[s], r0[s] + kept[s]) of the packed scan's records, one
// run after the other.  Each segment has one WINDOW [B[s], stop[s]): stop[s] is E[s], or, when the per-segment limit cut the
// run, the line of the first record the limit removed (the next matching piece of that file: the after-context of the last
// kept line ends before it, and nothing behind it is context).  Every record of K carries its segment's window (W, beside
// K).  With b = before and a = after, a piece q is
//   a MATCH   if q is a line of K,
//   CONTEXT   else if some m in K has q - a <= m <= q + b AND q lies in m's window,
//   nothing   otherwise (phantoms, pads and the tail a limit cut lie in no window of a kept line's).
// The kept lines of segment s all lie in its window and those of every other segment lie outside it, and the windows ascend
// without overlap.  So of all m only hg_context_class' two neighbours of q decide: the next line of K (q is below it, hence
// below its window's end: q >= lo is the test) and the previous one (q is above it: q < hi is the test).  No piece looks up
// its segment: the walk is the context stage's with two more comparisons.  (One array stop[s] and a search of B per piece,
// or per tile where its pieces share a segment, would do with less memory; the search inside the walk's piece loops cost
// the write kernel scalar-register spills, the 16 bytes per kept record cost nothing that shows.)
//
// Count.  The line m with the window [lo_w, hi_w) covers I(m) = [max(m - b, lo_w), min(m + a, hi_w - 1)].  Both ends of I(m)
// are non-decreasing in m over the whole of K: inside a segment the clamps are constants, and from one segment to a later one
// hi_w - 1 < lo_w' <= lo(m').  So
//  - the pieces of I(m_i) that no earlier line covers are those above hi(m_(i-1)): a piece x of I(m_i) with x <= hi(m_(i-1))
//    has x >= lo(m_i) >= lo(m_(i-1)) and lies in I(m_(i-1)).  free_from is hi(m_(i-1)) + 1 WITH the previous line's clamp,
//    min(m_(i-1) + a, its hi_w - 1) + 1: the unclamped m_(i-1) + a + 1 would take before-context from the first lines of the
//    next file;
//  - of the lines below a tile [f0, f1) only the last one matters (its hi is the largest, and lo <= m < f0 for all of them),
//    of the lines from f1 on only the first (its lo is the smallest, and hi >= m >= f1 for all of them): the records
//    [r0, r1) of hg_context_tile decide, however large a and b are.
// All arithmetic on piece numbers saturates as in hg_context.h.
#pragma once
#include "hg_context.h"
#include "hg_segments.h"

struct HgSegCtxWin {
  uint64_t lo, hi;  // [B[s], stop[s]) of the record's segment; lo <= the record's line < hi
};

// stop[s] (above).  hits / aux: the packed scan's n ordered records; [r0, r0 + kept): the run hg_seg_run kept with the limit.
HG_HD uint64_t hg_segctx_stop(const HgHit *hits, const HgHitAux *aux, uint64_t n, uint64_t Bs, uint64_t Es, uint64_t seg_end, bool invert, uint64_t limit,
                              uint64_t r0, uint64_t kept) {
  if (limit == 0) return Es;
  uint64_t a, z;
  hg_seg_run(hits, aux, n, Bs, Es, seg_end, invert, 0, &a, &z);  // the run without the limit
  return r0 + kept < z ? hits[r0 + kept].line_no : Es;
}

// The class of piece q.  `h` as for hg_context_class: every record of K below index h has a smaller line number than q.
HG_HD uint32_t hg_segctx_class(const HgHit *K, const HgSegCtxWin *W, uint64_t h, uint64_t n, uint64_t q, uint64_t before, uint64_t after) {
  const uint64_t i = hg_invert_lower_bound(K, h, n, q);
  if (i < n && K[i].line_no == q) return HG_CTX_MATCH;
  if (i < n && K[i].line_no - q <= before && q >= W[i].lo) return HG_CTX_CONTEXT;
  if (i > 0 && q - K[i - 1].line_no <= after && q < W[i - 1].hi) return HG_CTX_CONTEXT;
  return HG_CTX_NONE;
}

// What record i of [t.r0, t.r1) (hg_context_tile over K) adds to the count of context pieces of the tile [t.f0, t.f1): the
// pieces of the tile its line is the first to cover, minus one if the line is a piece of the tile.  0 for a line's later records.
HG_HD int32_t hg_segctx_contrib(const HgHit *K, const HgSegCtxWin *W, uint64_t i, const HgContextTile &t, uint64_t before, uint64_t after) {
  const uint64_t m = K[i].line_no;
  if (i > t.r0 && K[i - 1].line_no == m) return 0;
  if (t.f1 <= t.f0) return 0;
  int32_t c = m >= t.f0 && m < t.f1 ? -1 : 0;
  uint64_t lo = hg_sat_sub(m, before), hi = hg_sat_add(m, after);
  if (lo < W[i].lo) lo = W[i].lo;
  if (hi > W[i].hi - 1) hi = W[i].hi - 1;  // (hi_w > m >= 0)
  if (i > t.r0) {
    uint64_t reach = hg_sat_add(K[i - 1].line_no, after);
    if (reach > W[i - 1].hi - 1) reach = W[i - 1].hi - 1;
    if (lo < reach + 1) lo = reach + 1;  // (reach < its hi_w <= 2^64 - 1)
  }
  if (lo < t.f0) lo = t.f0;
  if (hi > t.f1 - 1) hi = t.f1 - 1;
  if (lo <= hi) c += static_cast<int32_t>(hi - lo + 1);
  return c;
}

// The piece walk of one tile, one byte at a time: emit(piece number, piece start) for every context piece that starts in
// [tile_start, tile_end), ascending.  What hg_segctx_write_kernel does with a wave; the host replay runs this.
template <typename Emit>
HG_HD void hg_segctx_walk_tile(const uint8_t *text, const HgTileBase &tb, const HgTileSum &ts, uint64_t tile_start, uint64_t tile_end, uint64_t bs1, const HgHit *K,
                               const HgSegCtxWin *W, uint64_t n, uint64_t before, uint64_t after, Emit &&emit) {
  const uint64_t h = hg_invert_lower_bound(K, 0, n, hg_invert_first_piece(tb, ts, tile_start, tile_end, bs1));
  hg_invert_walk_tile(text, tb, ts, tile_start, tile_end, bs1, [&](uint64_t q, uint64_t ps) {
    if (hg_segctx_class(K, W, h, n, q, before, after) == HG_CTX_CONTEXT) emit(q, ps);
  });
}

// A context record in packed form made file-relative, in place (hg_seg_map_record: a last piece of NULs only, whose scanned
// bytes begin in the pad, gets start = the file's size and len = 0).  Returns its segment.
HG_HD uint32_t hg_segctx_map_record(const uint64_t *B, const uint64_t *seg_start, const uint64_t *seg_end, uint64_t n_seg, HgHit *h, HgHitAux *x) {
  const uint32_t s = hg_seg_of_line(B, n_seg, h->line_no);
  if (s == HG_SEG_NONE) return s;  // (never: a context piece lies in a window)
  HgHit oh;
  HgHitAux ox;
  hg_seg_map_record(*h, *x, B[s], seg_start[s], seg_end[s], &oh, &ox);
  *h = oh;
  *x = ox;
  return s;
}

// First index j in [0, n) with seg[j] >= s (the records' segments ascend): first_context[s].
HG_HD uint64_t hg_segctx_first(const uint32_t *seg, uint64_t n, uint64_t s) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (seg[mid] < s) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// What the stage works on (hg_segctx_launch, hg_engine.h).
struct HgSegCtxArgs {
  const uint8_t *text;
  uint64_t nbytes, bs1, ntiles;
  uint64_t end_piece;  // the buffer's pieces
  uint64_t before, after;
  const HgTileSum *sums;  // the scan's tile summaries and prefix states
  const HgTileBase *bases;
  const HgHit *hits;  // the packed scan's ordered records (what the segment stage read) ...
  const HgHitAux *aux;
  uint64_t n_hits;
  const uint64_t *seg_start, *seg_end;
  uint64_t n_seg, limit;
  uint32_t invert;
  const uint64_t *B, *E, *r0, *kept;  // ... and what the segment stage left per segment
  const HgHit *seg_hits;              // the surviving records, file-relative, with their segments
  const uint32_t *seg_of;
  uint64_t n_kept;
  HgHit *K;        // prepare: the surviving records in packed piece numbers ...
  HgSegCtxWin *W;  // ... and the window of each
  uint64_t *count;      // count pass: context records per tile, count[ntiles] = 0
  const uint64_t *pos;  // write pass: the exclusive scan of count
  HgHit *out_hits;      // write: packed records; map: the same made file-relative
  HgHitAux *out_aux;
  uint64_t n_ctx;
  uint32_t *out_seg;     // map: the segment of each context record
  uint64_t *first_ctx;   // first: n_seg + 1 offsets into the context records
};
