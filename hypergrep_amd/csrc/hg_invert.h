// Inverted match (hg_scan_device_invert, grep -v): the line pieces NO delivered report lies in, enumerated in order on the
// GPU after a scan.  The scalar routines here are shared by the kernels (hg_invert.hip) and the host replay of the tests
// (tests/native/invertsim.cpp compiles this header for x86); the product only calls them from device code.
//
// A piece is what the line pipeline numbers (hg_core.h): lines end at '\n', a line longer than bs1 = buffer_size - 1 bytes
// is cut at multiples of bs1 from its start, and a piece BELONGS TO THE TILE ITS FIRST BYTE LIES IN.  The scan leaves, per
// 16 KiB tile, the start `cs` and piece number `L` of the line open at the tile start (HgTileBase) and the tile's first
// newline (HgTileSum): the number of the first piece of a tile follows from those alone (hg_invert_first_piece), so the
// count pass needs no text.  The final hits are ordered by line number: a piece is selected iff its number is not among
// them (hg_invert_selected).
#pragma once
#include "hg_core.h"

// The cuts of the line segment [s, e) (e: just past its '\n', or where the tile / the text ends): its pieces start at
// s + k * bs1 for k < *k1; those that start at or after `from` have k >= *k0 (*k0 == *k1: none).
HG_HD void hg_invert_cuts(uint64_t s, uint64_t e, uint64_t from, uint64_t bs1, uint64_t *k0, uint64_t *k1) {
  if (s >= from && e - s <= bs1) {  // a line of one piece that starts at or after `from`: the common case, without a 64-bit division
    *k0 = 0;
    *k1 = e > s ? 1 : 0;
    return;
  }
  *k1 = e > s ? hg_pieces(e - s, bs1) : 0;
  *k0 = s >= from ? 0 : hg_pieces(from - s, bs1);
  if (*k0 > *k1) *k0 = *k1;
}

// Number of the first piece that starts at or after tile_start, for the tile [tile_start, tile_end) (tile_end: its end or
// the text's).  Whether or not such a piece starts inside the tile: the difference between two tiles' values is the
// number of pieces that start between them.
HG_HD uint64_t hg_invert_first_piece(const HgTileBase &tb, const HgTileSum &ts, uint64_t tile_start, uint64_t tile_end, uint64_t bs1) {
  const uint64_t e = ts.nl_count ? tile_start + ts.first_nl + 1 : tile_end;  // where the carry-in line ends, as far as this tile knows
  uint64_t k0, k1;
  hg_invert_cuts(tb.cs, e, tile_start, bs1, &k0, &k1);
  return tb.L + k0;
}

// First index i in [lo, n) with hits[i].line_no >= q, given that every hit below lo has a smaller line number.  Gallops
// from lo: a tile's pieces are looked up in ascending order from the tile's first hit, a few records away each (the
// forward merge, one lane per piece).
HG_HD uint64_t hg_invert_lower_bound(const HgHit *hits, uint64_t lo, uint64_t n, uint64_t q) {
  uint64_t hi = lo, step = 1;
  while (hi < n && hits[hi].line_no < q) {
    lo = hi + 1;
    hi += step;
    step <<= 1;
  }
  if (hi > n) hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (hits[mid].line_no < q) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
HG_HD bool hg_invert_selected(const HgHit *hits, uint64_t lo, uint64_t n, uint64_t q) {
  const uint64_t i = hg_invert_lower_bound(hits, lo, n, q);
  return !(i < n && hits[i].line_no == q);
}

// Distinct line numbers among hits[h0, h1) (a line may have several reports).
HG_HD uint64_t hg_invert_hit_lines(const HgHit *hits, uint64_t h0, uint64_t h1) {
  uint64_t c = 0;
  for (uint64_t i = h0; i < h1; i++) c += (i == h0 || hits[i].line_no != hits[i - 1].line_no) ? 1 : 0;
  return c;
}

// The records of the selected piece `q` that starts at ps: hg_hit_t{q, HG_ID_INVERT, 0}, hg_hit_aux_t{start, len, 0xFFFFFFFF}
// with the scanned bytes of hg_trim_piece.
HG_HD void hg_invert_record(uint64_t q, uint64_t a, uint64_t z, HgHit *h, HgHitAux *x) {
  h->line_no = q;
  h->id = HG_NONE32;
  h->to = 0;
  x->start = a;
  x->len = static_cast<uint32_t>(z - a);
  x->pattern = HG_NONE32;
}

// The piece walk of one tile, one byte at a time: emit(piece number, piece start) for every piece that starts in
// [tile_start, tile_end), ascending.  What hg_invert_write_kernel does with a wave; the host replay runs this.
template <typename Emit>
HG_HD void hg_invert_walk_tile(const uint8_t *text, const HgTileBase &tb, const HgTileSum &ts, uint64_t tile_start, uint64_t tile_end, uint64_t bs1, Emit &&emit) {
  uint64_t s = tb.cs, q = hg_invert_first_piece(tb, ts, tile_start, tile_end, bs1), k0, k1;
  for (uint64_t i = tile_start; i < tile_end; i++)
    if (text[i] == '\n') {
      hg_invert_cuts(s, i + 1, tile_start, bs1, &k0, &k1);
      for (uint64_t k = k0; k < k1; k++) emit(q++, s + k * bs1);
      s = i + 1;
    }
  hg_invert_cuts(s, tile_end, tile_start, bs1, &k0, &k1);  // the line still open at the tile's end
  for (uint64_t k = k0; k < k1; k++) emit(q++, s + k * bs1);
}

// What the stage works on (hg_invert_launch, hg_engine.h).
struct HgInvertArgs {
  const uint8_t *text;
  uint64_t nbytes, bs1, ntiles;
  uint64_t end_piece;  // line_base + the buffer's pieces: the first piece number past the last tile
  const HgTileSum *sums;    // the scan's tile summaries and prefix states, all ntiles of them
  const HgTileBase *bases;
  const HgHit *hits;  // the scan's final hits, ordered by line
  uint64_t n_hits;
  uint64_t *count;      // count pass: selected pieces per tile, count[ntiles] = 0
  const uint64_t *pos;  // write pass: the exclusive scan of count, pos[ntiles] = their total
  HgHit *out_hits;
  HgHitAux *out_aux;
};
