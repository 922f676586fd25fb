// TEST-ONLY host harness for the segment stage (never shipped): compiles the scalar routines of hg_segments.h for x86 and
// replays the stage over tiles of ANY size: the argument check, the tile states the scan would leave (hg_post.h's monoid),
// the segments' line bases both ways the device computes them (one piece walk per tile that serves all its boundaries, and
// the per-chunk finish of hg_seg_bases_kernel; the two must agree), the runs of surviving records, their exclusive scan and
// the ordered write.  The results are what the GPU must leave.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_invert.h"
#include "../../hypergrep_amd/csrc/hg_post.h"
#include "../../hypergrep_amd/csrc/hg_segments.h"

// (replay only: the kernel has no such walk, it finishes per chunk)  The boundaries bounds[j0, j1) (ascending, all inside [tile_start, tile_end)) served by ONE piece walk of the tile:
// put(j, number of the first piece that starts at or after bounds[j]).
template <typename Put>
static void hg_seg_walk_bounds(const uint8_t *text, const HgTileBase &tb, const HgTileSum &ts, uint64_t tile_start, uint64_t tile_end, uint64_t bs1,
                              const uint64_t *bounds, uint64_t j0, uint64_t j1, Put &&put) {
  uint64_t j = j0, next = hg_invert_first_piece(tb, ts, tile_start, tile_end, bs1);
  hg_invert_walk_tile(text, tb, ts, tile_start, tile_end, bs1, [&](uint64_t q, uint64_t ps) {
    while (j < j1 && bounds[j] <= ps) put(j++, q);
    next = q + 1;
  });
  while (j < j1) put(j++, next);  // behind the tile's last piece start: the next tile's first piece
}

extern "C" {

// 1 if a hit whose scanned bytes begin at `start` lies in a pad (hg_seg_pad_hit), the filter of an inverted call.
int segsim_pad_hit(const uint64_t *seg_start, const uint64_t *seg_end, uint64_t n_seg, uint64_t start) { return hg_seg_pad_hit(seg_start, seg_end, n_seg, start) ? 1 : 0; }

// text[0, nbytes) in tiles of `tile` bytes, pieces of at most bs1 bytes.  recs: the packed scan's ordered records, six words
// each {line_number, id, to, start, len, pattern}; from: their starts of match.  Outputs: out_recs (six words per surviving
// record, file-relative), out_from, out_seg, first_record[n_seg + 1], n_lines[n_seg], n_selected[n_seg], base[n_seg].
// Returns the surviving records; -1: the segments are malformed (*bad: HG_SEG_BAD_* bits); -2: the two ways to a line base
// disagree; -3: a tile with boundaries was not needed / the tiles do not chain.
long segsim_run(const uint8_t *text, uint64_t nbytes, uint64_t tile, uint64_t bs1, const uint64_t *recs, const uint32_t *from, uint64_t n,
                const uint64_t *seg_start, const uint64_t *seg_end, uint64_t n_seg, uint64_t limit, int invert, uint64_t *out_recs, uint32_t *out_from,
                uint32_t *out_seg, uint64_t *first_record, uint64_t *n_lines, uint64_t *n_selected, uint64_t *base, uint32_t *bad, uint64_t *tiles_walked) {
  *bad = 0;
  *tiles_walked = 0;
  for (uint64_t s = 0; s < n_seg; s++) *bad |= hg_seg_check(text, nbytes, seg_start, seg_end, n_seg, s);
  if (*bad) return -1;
  const uint64_t ntiles = (nbytes + tile - 1) / tile;
  std::vector<HgHit> hits(n);
  std::vector<HgHitAux> aux(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t *r = recs + 6 * i;
    hits[i] = HgHit{r[0], static_cast<uint32_t>(r[1]), static_cast<uint32_t>(r[2])};
    aux[i] = HgHitAux{r[3], static_cast<uint32_t>(r[4]), static_cast<uint32_t>(r[5])};
  }
  std::vector<HgTileSum> sums(ntiles);
  std::vector<HgTileBase> bases(ntiles + 1);
  HgTileBase st{0, 0};
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
  const uint64_t end_piece = st.L + (nbytes > st.cs ? hg_pieces(nbytes - st.cs, bs1) : 0);  // (as HgScanner::run_once)
  std::vector<uint64_t> B(n_seg + 1, ~0ull), E(n_seg + 1, ~0ull), r0(n_seg + 1), kept(n_seg + 1, 0);
  // the line bases, tile by tile (hg_seg_bases_kernel)
  for (uint64_t t = 0; t < ntiles; t++) {
    const uint64_t t0 = t * tile, t1 = t0 + tile < nbytes ? t0 + tile : nbytes;
    const uint64_t js0 = hg_seg_lower_bound(seg_start, 0, n_seg, t0), js1 = hg_seg_lower_bound(seg_start, js0, n_seg, t1);
    const uint64_t je0 = hg_seg_lower_bound(seg_end, 0, n_seg, t0), je1 = hg_seg_lower_bound(seg_end, je0, n_seg, t1);
    if (js0 == js1 && je0 == je1) continue;
    ++*tiles_walked;
    hg_seg_walk_bounds(text, bases[t], sums[t], t0, t1, bs1, seg_start, js0, js1, [&](uint64_t j, uint64_t q) { B[j] = q; });
    hg_seg_walk_bounds(text, bases[t], sums[t], t0, t1, bs1, seg_end, je0, je1, [&](uint64_t j, uint64_t q) { E[j] = q; });
    // the kernel's way: the walk's state at the boundary's 16-byte chunk, then the finish inside the chunk
    const uint64_t first = hg_invert_first_piece(bases[t], sums[t], t0, t1, bs1);
    auto by_chunk = [&](uint64_t b) {
      const uint64_t p = t0 + ((b - t0) & ~static_cast<uint64_t>(HG_SEG_CHUNK - 1));
      uint64_t ls = bases[t].cs, before = 0, k0, k1;
      for (uint64_t i = t0; i < p; i++)
        if (text[i] == '\n') {
          hg_invert_cuts(ls, i + 1, t0, bs1, &k0, &k1);
          before += k1 - k0;
          ls = i + 1;
        }
      return first + before + hg_seg_pieces_upto(text, p, b, ls, t0, bs1);
    };
    for (uint64_t j = js0; j < js1; j++)
      if (by_chunk(seg_start[j]) != B[j]) return -2;
    for (uint64_t j = je0; j < je1; j++)
      if (by_chunk(seg_end[j]) != E[j]) return -2;
  }
  // the runs (hg_seg_runs_kernel)
  for (uint64_t s = 0; s < n_seg; s++) {
    if (seg_start[s] == nbytes) B[s] = end_piece;
    if (seg_end[s] == nbytes) E[s] = end_piece;
    if (B[s] == ~0ull || E[s] == ~0ull || E[s] < B[s]) return -3;
    uint64_t a, z;
    hg_seg_run(hits.data(), aux.data(), n, B[s], E[s], seg_end[s], invert != 0, limit, &a, &z);
    r0[s] = a;
    kept[s] = z - a;
    n_lines[s] = E[s] - B[s];
    n_selected[s] = 0;
    base[s] = B[s];
  }
  first_record[0] = 0;
  for (uint64_t s = 0; s < n_seg; s++) first_record[s + 1] = first_record[s] + kept[s];
  // the write (hg_seg_write_kernel): a record at a time, each on its own
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t s = hg_seg_of_line(B.data(), n_seg, hits[i].line_no);
    if (s == HG_SEG_NONE || i < r0[s] || i - r0[s] >= kept[s]) continue;
    const uint64_t at = first_record[s] + (i - r0[s]);
    HgHit h;
    HgHitAux x;
    hg_seg_map_record(hits[i], aux[i], B[s], seg_start[s], seg_end[s], &h, &x);
    uint64_t *o = out_recs + 6 * at;
    o[0] = h.line_no, o[1] = h.id, o[2] = h.to, o[3] = x.start, o[4] = x.len, o[5] = x.pattern;
    out_seg[at] = s;
    out_from[at] = from[i];
    if (i == r0[s] || hits[i - 1].line_no != hits[i].line_no) n_selected[s]++;
  }
  return static_cast<long>(first_record[n_seg]);
}

}  // extern "C"
