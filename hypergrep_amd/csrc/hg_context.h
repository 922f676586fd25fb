// Context lines (hg_scan_device_context, grep -A / -B / -C): the line pieces around the pieces a scan delivers a record for,
// enumerated in order on the GPU after the scan.  The scalar routines here are shared by the kernels (hg_context.hip) and the
// host replay of the tests (tests/native/contextsim.cpp compiles this header for x86); the product only calls them from
// device code.
//
// Pieces, tiles and the ordered hit list are those of hg_invert.h.  With M the piece numbers among the hits, B = before and
// A = after, a piece q of the buffer [line_base, end_piece) is
//   a MATCH    if q is in M,
//   CONTEXT    else if some m in M has q - A <= m <= q + B, or q < line_base + carry_after (after-context the previous buffer owes),
//   a TAIL     else if the caller asked for them and q is among the buffer's last B pieces (the next buffer's before-context, maybe),
//   nothing    otherwise.
// The covered pieces (match or context) of a tile are a union of intervals of piece numbers, so their number follows from the
// hit lines alone (hg_context_tile / hg_context_contrib): the count pass reads no text.  All arithmetic on piece numbers
// saturates: q - A stops at 0, m + A and line_base + carry_after at 2^64 - 1.
#pragma once
#include "hg_invert.h"

constexpr uint32_t HG_CTX_ID_CONTEXT = 0xFFFFFFFEu;  // the ids of the records (HG_ID_CONTEXT, HG_ID_CONTEXT_TAIL of the C ABI)
constexpr uint32_t HG_CTX_ID_TAIL = 0xFFFFFFFDu;
enum : uint32_t { HG_CTX_NONE = 0, HG_CTX_MATCH = 1, HG_CTX_CONTEXT = 2, HG_CTX_TAIL = 3 };

HG_HD uint64_t hg_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
HG_HD uint64_t hg_sat_sub(uint64_t a, uint64_t b) { return a > b ? a - b : 0; }

// One call's windows, in piece numbers.
struct HgContextWin {
  uint64_t before, after;
  uint64_t carry_end;  // pieces below it are owed after-context by the previous buffer (<= end_piece; line_base: none)
  uint64_t tail_lo;    // pieces from it on are tail candidates (>= line_base; end_piece: none)
  uint64_t end_piece;  // line_base + the buffer's pieces
};
HG_HD HgContextWin hg_context_win(uint64_t line_base, uint64_t n_pieces, uint32_t before, uint32_t after, uint64_t carry_after, bool tail) {
  HgContextWin w;
  w.before = before;
  w.after = after;
  w.end_piece = line_base + n_pieces;
  w.carry_end = carry_after < n_pieces ? line_base + carry_after : w.end_piece;
  w.tail_lo = !tail ? w.end_piece : before < n_pieces ? w.end_piece - before : line_base;
  return w;
}

// What a call asks of the stage (hg_context_t of the C ABI).
struct HgContextParams {
  uint32_t before, after;
  uint64_t carry_after;  // after-context the previous buffer still owes, in pieces
  bool tail;             // also deliver the last `before` pieces that are neither match nor context, as tail records
  bool any() const { return before || after || carry_after || tail; }
};

// After-context still owed past the buffer's end.  last_line: the line of the last hit (n_hits != 0).
HG_HD uint64_t hg_context_owed(uint64_t n_hits, uint64_t last_line, uint64_t line_base, uint64_t n_pieces, uint32_t after, uint64_t carry_after) {
  if (!n_hits) return hg_sat_sub(carry_after, n_pieces);
  return hg_sat_sub(hg_sat_add(last_line, after), line_base + n_pieces - 1);  // (a hit's line lies in the buffer: n_pieces >= 1)
}

// The class of piece q.  Every hit below index lo has a smaller line number than q (hg_invert_lower_bound's contract): one
// lookup finds the first hit at or after q, whose line and whose predecessor's decide.
HG_HD uint32_t hg_context_class(const HgHit *hits, uint64_t lo, uint64_t n, uint64_t q, const HgContextWin &w) {
  const uint64_t i = hg_invert_lower_bound(hits, lo, n, q);
  if (i < n && hits[i].line_no == q) return HG_CTX_MATCH;
  if (i < n && hits[i].line_no - q <= w.before) return HG_CTX_CONTEXT;
  if (i > 0 && q - hits[i - 1].line_no <= w.after) return HG_CTX_CONTEXT;
  if (q < w.carry_end) return HG_CTX_CONTEXT;
  return q >= w.tail_lo ? HG_CTX_TAIL : HG_CTX_NONE;
}

// What the count of the tile with the pieces [f0, f1) reads.  Outside [wlo, whi) every piece of the tile is covered or a tail
// candidate whatever the hits say (carry below, tail above); inside, the hit line m_i covers [m_i - B, m_i + A], of which
// [max(m_i - B, m_(i-1) + A + 1), m_i + A] is not covered by an earlier line already.  Of the lines below f0 only the last one
// matters (it reaches furthest into the tile, and m - B lies below the tile for all of them), of the lines from f1 on only
// the first: the records [r0, r1) decide, however large A and B are.
struct HgContextTile {
  uint64_t f0, f1, wlo, whi, r0, r1;
};
HG_HD HgContextTile hg_context_tile(const HgHit *hits, uint64_t n, uint64_t f0, uint64_t f1, const HgContextWin &w) {
  HgContextTile t;
  t.f0 = f0;
  t.f1 = f1;
  t.wlo = w.carry_end < f0 ? f0 : w.carry_end < f1 ? w.carry_end : f1;
  t.whi = w.tail_lo < t.wlo ? t.wlo : w.tail_lo < f1 ? w.tail_lo : f1;
  const uint64_t g0 = hg_invert_lower_bound(hits, 0, n, f0), g1 = hg_invert_lower_bound(hits, g0, n, f1);
  t.r0 = g0 ? hg_invert_lower_bound(hits, 0, g0, hits[g0 - 1].line_no) : 0;  // the first record of the last line below the tile
  t.r1 = g1 < n ? g1 + 1 : n;
  return t;
}
// What record i of [t.r0, t.r1) adds to the tile's count of context pieces: the pieces of [wlo, whi) its line is the first to
// cover (`whi` is t.whi, or t.f1 for the count without tail candidates), minus one if the line is a piece of the tile (a match
// is no context).  0 for a line's later records.  At most the tile's pieces in magnitude.
HG_HD int32_t hg_context_contrib(const HgHit *hits, uint64_t i, const HgContextTile &t, uint64_t whi, const HgContextWin &w) {
  const uint64_t m = hits[i].line_no;
  if (i > t.r0 && hits[i - 1].line_no == m) return 0;
  int32_t c = m >= t.f0 && m < t.f1 ? -1 : 0;
  if (whi > t.wlo) {
    uint64_t lo = hg_sat_sub(m, w.before), hi = hg_sat_add(m, w.after);
    if (i > t.r0) {
      const uint64_t free_from = hg_sat_add(hg_sat_add(hits[i - 1].line_no, w.after), 1);
      if (lo < free_from) lo = free_from;
    }
    if (lo < t.wlo) lo = t.wlo;
    if (hi > whi - 1) hi = whi - 1;
    if (lo <= hi) c += static_cast<int32_t>(hi - lo + 1);
  }
  return c;
}
// The tile's count from the sum of its records' contributions: context and tail records (whi == t.whi).
HG_HD uint64_t hg_context_count(const HgContextTile &t, uint64_t whi, int64_t contrib_sum) {
  return static_cast<uint64_t>(static_cast<int64_t>((t.f1 - t.f0) - (whi - t.wlo)) + contrib_sum);
}

// The record of the context (or tail) piece `q` with the scanned bytes [a, z).
HG_HD void hg_context_record(uint64_t q, uint64_t a, uint64_t z, uint32_t cls, HgHit *h, HgHitAux *x) {
  h->line_no = q;
  h->id = cls == HG_CTX_TAIL ? HG_CTX_ID_TAIL : HG_CTX_ID_CONTEXT;
  h->to = 0;
  x->start = a;
  x->len = static_cast<uint32_t>(z - a);
  x->pattern = HG_NONE32;
}

// The piece walk of one tile, one byte at a time: emit(piece number, piece start, class) for every context or tail piece
// that starts in [tile_start, tile_end), ascending.  What hg_context_write_kernel does with a wave; the host replay runs this.
template <typename Emit>
HG_HD void hg_context_walk_tile(const uint8_t *text, const HgTileBase &tb, const HgTileSum &ts, uint64_t tile_start, uint64_t tile_end, uint64_t bs1,
                                const HgHit *hits, uint64_t n_hits, const HgContextWin &w, Emit &&emit) {
  const uint64_t h = hg_invert_lower_bound(hits, 0, n_hits, hg_invert_first_piece(tb, ts, tile_start, tile_end, bs1));
  hg_invert_walk_tile(text, tb, ts, tile_start, tile_end, bs1, [&](uint64_t q, uint64_t ps) {
    const uint32_t cls = hg_context_class(hits, h, n_hits, q, w);
    if (cls == HG_CTX_CONTEXT || cls == HG_CTX_TAIL) emit(q, ps, cls);
  });
}

// What the stage works on (hg_context_launch, hg_engine.h).
struct HgContextArgs {
  const uint8_t *text;
  uint64_t nbytes, bs1, ntiles;
  HgContextWin win;
  const HgTileSum *sums;  // the scan's tile summaries and prefix states, all ntiles of them
  const HgTileBase *bases;
  const HgHit *hits;  // the call's final records (the hits, or the selected pieces of an inverted call), ordered by line
  uint64_t n_hits;
  uint64_t *count;      // count pass: context + tail records per tile, count[ntiles] = 0
  uint64_t *n_tail;     // ... and the tail records among them, added up (zero before the launch)
  const uint64_t *pos;  // write pass: the exclusive scan of count, pos[ntiles] = their total
  HgHit *out_hits;
  HgHitAux *out_aux;
};
