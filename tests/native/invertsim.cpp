// TEST-ONLY host harness for the inverted match (never shipped): compiles the scalar routines of hg_invert.h for x86 and
// replays the invert stage over tiles of ANY size: the tile summaries and prefix states the scan would leave (hg_post.h's
// monoid, one tile after the other), the count pass from those states and the hit lines alone, then the piece walk of each
// tile with the membership test and the trim rule.  The two must agree tile by tile; the records are what the GPU must write.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_invert.h"
#include "../../hypergrep_amd/csrc/hg_post.h"

extern "C" {

// text[0, nbytes) in tiles of `tile` bytes, pieces of at most bs1 bytes numbered from line_base; hit_lines: the line numbers
// of the scan's hits, ascending, repeats allowed.  out receives {line_number, start, len, id, to, pattern} per selected piece.
// Returns their number; -1: cap too small; -2: a tile's count (from the states) and its walk disagree; -3: the tiles' first
// piece numbers and the piece total disagree.  *n_pieces: the buffer's pieces.
long invertsim_run(const uint8_t *text, uint64_t nbytes, uint64_t tile, uint64_t bs1, uint64_t line_base, const uint64_t *hit_lines, uint64_t n_hits,
                   uint64_t *out, uint64_t cap, uint64_t *n_pieces) {
  const uint64_t ntiles = (nbytes + tile - 1) / tile;
  std::vector<HgHit> hits(n_hits);
  for (uint64_t i = 0; i < n_hits; i++) hits[i] = HgHit{hit_lines[i], 7, 1};
  std::vector<HgTileSum> sums(ntiles);
  std::vector<HgTileBase> bases(ntiles + 1);
  HgTileBase st{0, line_base};
  for (uint64_t t = 0; t < ntiles; t++) {
    const uint64_t t0 = t * tile, t1 = t0 + tile < nbytes ? t0 + tile : nbytes;
    HgTileSum s{0, HG_NONE32, HG_NONE32, 0};
    for (uint64_t i = t0; i < t1; i++)
      if (text[i] == '\n') {
        if (!s.nl_count++) s.first_nl = static_cast<uint32_t>(i - t0);
        s.last_nl = static_cast<uint32_t>(i - t0);
      }
    if (s.nl_count) s.inner = static_cast<uint32_t>(hg_inner_pieces(text, t0 + s.first_nl + 1, t0 + s.last_nl + 1, bs1));
    sums[t] = s;
    bases[t] = st;
    st = hg_tile_apply(st, hg_tile_elem(s, t0), bs1);
  }
  *n_pieces = st.L - line_base + (nbytes > st.cs ? hg_pieces(nbytes - st.cs, bs1) : 0);  // (as HgScanner::run_once)
  const uint64_t end_piece = line_base + *n_pieces;
  auto bounds = [&](uint64_t t, uint64_t *t0, uint64_t *t1) {
    *t0 = t * tile;
    *t1 = *t0 + tile < nbytes ? *t0 + tile : nbytes;
  };
  auto first_piece = [&](uint64_t t) {
    uint64_t t0, t1;
    bounds(t, &t0, &t1);
    return hg_invert_first_piece(bases[t], sums[t], t0, t1, bs1);
  };
  uint64_t n = 0, expect_first = line_base;
  for (uint64_t t = 0; t < ntiles; t++) {
    uint64_t t0, t1;
    bounds(t, &t0, &t1);
    const uint64_t f0 = first_piece(t), f1 = t + 1 < ntiles ? first_piece(t + 1) : end_piece;
    if (f0 != expect_first || f1 < f0) return -3;
    expect_first = f1;
    const uint64_t h0 = hg_invert_lower_bound(hits.data(), 0, n_hits, f0), h1 = hg_invert_lower_bound(hits.data(), h0, n_hits, f1);
    const uint64_t count = f1 - f0 - hg_invert_hit_lines(hits.data(), h0, h1);
    uint64_t walked = 0;
    bool full = false;
    hg_invert_walk_tile(text, bases[t], sums[t], t0, t1, bs1, [&](uint64_t q, uint64_t ps) {
      if (!hg_invert_selected(hits.data(), h0, n_hits, q)) return;
      walked++;
      if (n >= cap) {
        full = true;
        return;
      }
      uint64_t a, z;
      hg_trim_piece(text, ps, ps + bs1 < nbytes ? ps + bs1 : nbytes, a, z);
      HgHit h;
      HgHitAux x;
      hg_invert_record(q, a, z, &h, &x);
      uint64_t *o = out + 6 * n++;
      o[0] = h.line_no, o[1] = x.start, o[2] = x.len, o[3] = h.id, o[4] = h.to, o[5] = x.pattern;
    });
    if (full) return -1;
    if (walked != count) return -2;
  }
  if (ntiles == 0 && end_piece != line_base) return -3;
  return static_cast<long>(n);
}

}  // extern "C"
