// Matched parts of a buffer of many files (hg_scan_device_segments_parts, grep -r -o): the parts of every line piece a file
// KEEPS a record of, computed on the GPU behind the segment stage, per file.  The scalar rules here are shared by the kernels
// (hg_segparts.hip) and the host replay of the tests (tests/native/segpartssim.cpp compiles this header and hg_parts.h for
// x86); the product only calls them from device code.
//
// The stage works DIRECTLY on what the segment stage left: the surviving records, file-relative (line_no counts from the
// file's first piece, aux.start from its first byte), with the segment of each (seg_of), segment after segment and ordered by
// line inside a segment.  No packed copy of the records is made and no part is renumbered afterwards:
//  - HEAD.  A piece is named by (segment, file-relative line), not by the line alone: the first matching lines of two files
//    may both be line 0.  Record h heads a piece if it is the first record, or its segment or its line differs from the
//    previous record's.  A hit the phantom rule, the pad rule or the per-segment limit removed is not among the records, so
//    it heads nothing and its line has no part.
//  - ADDRESS.  The piece's scanned bytes are text + seg_start[seg_of[h]] + aux[h].start, aux[h].len of them: the bytes the
//    file scanned alone has (the pad "\0\n" behind an unterminated last line is outside them, so $, \z and \Z see the file's
//    end).  The sum is a 64-bit offset: a resident buffer may exceed 4 GiB.  The walk itself is the parts stage's
//    (hg_parts.h), which reads nothing outside [0, len).
//  - FIRST.  count[h] = the parts of the piece record h heads (0 for every other record), pos = its exclusive scan over the
//    n + 1 entries (pos[n] = all parts).  The records are in segment order, so segment s owns the parts
//    [pos[first_record[s]], pos[first_record[s + 1]]): first_part[s] = pos[first_record[s]], s = 0 .. n_seg
//    (first_record[n_seg] = n).
// The parts come out ordered by (segment, line, from) and carry the file-relative line, as the file scanned alone has them.
#pragma once
#include "hg_parts.h"
#include "hg_segments.h"

// Does surviving record h head a piece?
HG_HD bool hg_segparts_head(const HgHit *hits, const uint32_t *seg_of, uint64_t h) {
  return h == 0 || seg_of[h - 1] != seg_of[h] || hits[h - 1].line_no != hits[h].line_no;
}

// Offset in the packed text of the scanned bytes of a file-relative record of segment s.
HG_HD uint64_t hg_segparts_offset(const uint64_t *seg_start, uint32_t s, const HgHitAux &x) { return seg_start[s] + x.start; }

// first_part[s], s in [0, n_seg].
HG_HD uint64_t hg_segparts_first(const uint64_t *pos, const uint64_t *first_record, uint64_t s) { return pos[first_record[s]]; }

// What the stage works on (hg_segparts_launch, hg_engine.h).
struct HgSegPartsArgs {
  const uint8_t *text;
  const HgHit *hits;  // the surviving records, file-relative ...
  const HgHitAux *aux;
  const uint32_t *seg_of;  // ... and the segment of each
  uint64_t n_hits;
  const uint64_t *seg_start;     // the caller's device array
  const uint64_t *first_record;  // the segment stage's, n_seg + 1
  uint64_t n_seg;
  const HgPattern *patterns;
  const uint32_t *pool;
  uint32_t npatterns;
  const uint32_t *first;  // the parts stage's first-byte bitmap (HgPartsArgs::first)
  uint32_t first_words;
  uint64_t *count;      // count pass: parts per record, count[n_hits] = 0
  const uint64_t *pos;  // write pass: the exclusive scan of count
  HgPart *out;
  uint32_t *out_pattern;
  uint32_t *out_seg;     // the segment of each part
  uint64_t *first_part;  // first: n_seg + 1 offsets into the parts
};
