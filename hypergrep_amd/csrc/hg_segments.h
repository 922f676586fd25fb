// Segments (hg_scan_device_segments, grep -r): one scan of a buffer that holds many files one after the other, turned into
// per-file results on the GPU.  The scalar routines here are shared by the kernels (hg_segments.hip) and the host replay of
// the tests (tests/native/segsim.cpp compiles this header for x86); the product only calls them from device code.  What is
// NOT shared is the wave-level walk of hg_seg_bases_kernel (ballots, the per-chunk state in LDS): the replay re-derives the
// state at a chunk with scalar code and checks it against a plain piece walk of its own, so the kernel's lane logic is covered
// by the GPU tests only.
//
// Segment s is the bytes [seg_start[s], seg_end[s]) of the text (include/hypergrep_amd.h has the packing rule).  A segment
// start is a line start, so no piece spans two segments and the pieces of a segment are numbered in one run: its LINE BASE
// B[s] is the number of the first piece that starts at or after seg_start[s], E[s] that of the first piece that starts at or
// after seg_end[s].  The segment has E[s] - B[s] pieces; the pieces [E[s], B[s + 1]) start in the pad behind it and belong to
// no file (phantoms).  The records of a scan are ordered by piece number, so segment s owns one run of them, and what the
// per-segment limit and the phantom rule remove is the END of that run: the surviving records are [r0[s], r2[s]), and the
// compacted list is those runs one after the other (first_record = the exclusive scan of their lengths).
#pragma once
#include "hg_core.h"
#include "hg_invert.h"

constexpr uint32_t HG_SEG_NONE = 0xFFFFFFFFu;
constexpr uint32_t HG_SEG_CHUNK = 16;  // bytes a lane of the tile walk loads at once: the walk leaves its state per chunk
// bits of the flag word of the argument check
enum : uint32_t { HG_SEG_BAD_ORDER = 1, HG_SEG_BAD_END = 2, HG_SEG_BAD_START = 4 };

// First index i in [lo, n) with a[i] >= q, a ascending.
HG_HD uint64_t hg_seg_lower_bound(const uint64_t *a, uint64_t lo, uint64_t n, uint64_t q) {
  uint64_t hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid] < q) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// First index i in [lo, n) with aux[i].start >= q (the records are ordered by line, hence by start).
HG_HD uint64_t hg_seg_start_bound(const HgHitAux *aux, uint64_t lo, uint64_t n, uint64_t q) {
  uint64_t hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (aux[mid].start < q) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The argument check of segment s: HG_SEG_BAD_* bits, 0 if it is well formed.
HG_HD uint32_t hg_seg_check(const uint8_t *text, uint64_t nbytes, const uint64_t *seg_start, const uint64_t *seg_end, uint64_t n_seg, uint64_t s) {
  const uint64_t a = seg_start[s], z = seg_end[s];
  uint32_t bad = 0;
  if (a > z || (s + 1 < n_seg && z > seg_start[s + 1])) bad |= HG_SEG_BAD_ORDER;
  if (z > nbytes) bad |= HG_SEG_BAD_END;
  if (a > 0 && (a > nbytes || text[a - 1] != '\n')) bad |= HG_SEG_BAD_START;
  return bad;
}

// Does a hit whose scanned bytes begin at `start` lie in the pad behind a segment (or in any other gap between two
// segments)?  Such a hit belongs to no file.  An inverted call removes these hits BEFORE the invert stage (hg_seg_pad_flag_kernel),
// so that a file's last piece of NULs only, whose scanned bytes are the pad's "\n", is selected as the file alone selects it
// even under an expression that matches a bare newline.
HG_HD bool hg_seg_pad_hit(const uint64_t *seg_start, const uint64_t *seg_end, uint64_t n_seg, uint64_t start) {
  uint64_t lo = 0, hi = n_seg;  // first s with seg_start[s] > start
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (seg_start[mid] <= start) lo = mid + 1;
    else hi = mid;
  }
  return lo > 0 && start >= seg_end[lo - 1];
}

// Pieces that start in [from, b) among the lines that end behind p, for a boundary b with p <= b: `ls` is the start of the
// line open at p, and no piece of an EARLIER line is counted.  Added to the pieces that start in [from, ..) on lines ending at
// or before p this is the number of pieces that start in [from, b).  The kernel calls it with p = the start of b's 16-byte
// chunk (the tile walk leaves `ls` and the earlier lines' pieces per chunk), the replay also with p = the tile start.
HG_HD uint64_t hg_seg_pieces_upto(const uint8_t *text, uint64_t p, uint64_t b, uint64_t ls, uint64_t from, uint64_t bs1) {
  uint64_t n = 0, k0, k1;
  for (uint64_t i = p; i < b; i++)
    if (text[i] == '\n') {
      hg_invert_cuts(ls, i + 1, from, bs1, &k0, &k1);
      n += k1 - k0;
      ls = i + 1;
    }
  hg_invert_cuts(ls, b, from, bs1, &k0, &k1);  // the line b lies in: its pieces that start before b
  return n + (k1 - k0);
}

// The segment of the piece `line`: the last s with B[s] <= line (empty segments share their base with the segment behind
// them, which owns the pieces), HG_SEG_NONE for a piece in front of the first segment.  A phantom piece gets the segment
// it lies behind; hg_seg_run leaves it out of that segment's run.
HG_HD uint32_t hg_seg_of_line(const uint64_t *B, uint64_t n_seg, uint64_t line) {
  uint64_t lo = 0, hi = n_seg;  // first s with B[s] > line
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (B[mid] <= line) lo = mid + 1;
    else hi = mid;
  }
  return lo ? static_cast<uint32_t>(lo - 1) : HG_SEG_NONE;
}

// The run of records segment s keeps: [*r0, *r2) of the ordered list hits / aux (n records).
//  - its own pieces are [Bs, Es): the records of the phantom pieces behind them are left out;
//  - a HIT whose scanned bytes begin at or after seg_end lies in the pad (the segment's last piece is NULs up to its end, so
//    the file scanned alone has no report there): left out as well.  The record of an inverted list for such a piece stays:
//    hg_seg_map_record gives it the empty scanned bytes the file scanned alone has;
//  - with a limit m > 0 the run ends with the line on which the segment's record count reaches m.
HG_HD void hg_seg_run(const HgHit *hits, const HgHitAux *aux, uint64_t n, uint64_t Bs, uint64_t Es, uint64_t seg_end, bool invert, uint64_t m, uint64_t *r0,
                      uint64_t *r2) {
  const uint64_t a = hg_invert_lower_bound(hits, 0, n, Bs);
  uint64_t z = hg_invert_lower_bound(hits, a, n, Es);
  if (!invert) z = hg_seg_start_bound(aux, a, z, seg_end);
  if (m > 0 && z - a >= m) z = hg_invert_lower_bound(hits, a + (m - 1), z, hits[a + (m - 1)].line_no + 1);
  *r0 = a;
  *r2 = z;
}

// Record i of segment s as the file scanned alone has it: the line number counts from the segment's base, the start from
// the segment's first byte.  (An inverted record that begins in the pad: see hg_seg_run.)
HG_HD void hg_seg_map_record(const HgHit &h, const HgHitAux &x, uint64_t Bs, uint64_t seg_start, uint64_t seg_end, HgHit *oh, HgHitAux *ox) {
  *oh = h;
  *ox = x;
  oh->line_no = h.line_no - Bs;
  if (x.start >= seg_end) {
    ox->start = seg_end - seg_start;
    ox->len = 0;
  } else {
    ox->start = x.start - seg_start;
  }
}

// What the stage works on (hg_segments_launch, hg_engine.h).
struct HgSegArgs {
  const uint8_t *text;
  uint64_t nbytes, bs1, ntiles;
  uint64_t end_piece;  // the buffer's pieces: the number of the first piece past the last tile (segments count from line 0)
  const HgTileSum *sums;  // the scan's tile summaries and prefix states
  const HgTileBase *bases;
  const HgHit *hits;  // the final ordered records of the call (hits, or the invert stage's records) ...
  const HgHitAux *aux;
  const uint32_t *from;  // ... and their starts of match, or nullptr
  uint64_t n_hits;
  const uint64_t *seg_start, *seg_end;  // the caller's device arrays
  uint64_t n_seg, limit;
  uint32_t invert;
  uint32_t *flag;   // HG_SEG_BAD_* bits of the argument check
  uint64_t *B, *E;  // per segment: line base and end (above)
  uint64_t *r0;     // per segment: the first record of its run
  uint64_t *kept;   // per segment: the length of its run; kept[n_seg] = 0
  const uint64_t *first;  // the exclusive scan of kept: first_record, n_seg + 1 entries
  uint64_t *n_lines, *n_selected;
  HgHit *out_hits;
  HgHitAux *out_aux;
  uint32_t *out_from;
  uint32_t *out_seg;
  uint64_t *pad_keep;       // pad filter of an inverted call: 1 per hit that lies in no pad, pad_keep[n_hits] = 0 ...
  const uint64_t *pad_pos;  // ... and the exclusive scan of those
};
