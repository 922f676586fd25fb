// The matched parts themselves (hg_gather_parts; grep -o -n -b, grep --color): the bytes of every part the last scan with parts
// left a record for, gathered on the GPU into one compact, ordered, optionally print-ready buffer.  The scalar rules here are
// shared by the kernels (hg_partlines.hip) and the host replay of the tests (tests/native/partlinesim.cpp compiles this header
// for x86); the product only calls them from device code.  hg_gather.h lends its searches, its decimal digits and its funnel
// shift unchanged.
//
// The stage works on the part records (ordered by (segment, line, from)) and on the scan's final records (ordered by (segment,
// line)).  One ENTRY per part, in the parts' order.
//  - PIECE.  Part q belongs to the piece (segment, line_no); its record is found by a lower bound in the final records.
//    S = (seg_start[segment] after a scan with segments, else 0) + aux.start, in 64 bits; len = aux.len.  Part q is the FIRST of
//    its piece if it is part 0 or part q - 1 differs in segment or line, the LAST likewise with part q + 1; prev_to is the `to`
//    of part q - 1 if q is not a first, else 0.
//  - LAYOUT.  Parts mode:  [number][offset] [mark_on] text[S+from, S+to) [mark_off] [terminator]
//             Line mode:   [number][offset] text[S+prev_to, S+from) [mark_on] text[S+from, S+to) [mark_off] [text[S+to, S+len) [terminator]]
//    (line mode: number and offset on a first part only, the trailing text and the terminator on a last part only, so that the
//    entries of a piece joined are the line with its parts marked).  Both are one form, three text runs of which the first and
//    the last may be empty: gap = text[S+gap, S+from), part = text[S+from, S+to), trail = text[S+to, S+trail).
//    hg_partlines_entry decides the fields (the terminator test reads one text byte), hg_partlines_size adds them up,
//    hg_partlines_plan gives byte k of an entry: the one definition of the layout.  off = exclusive scan of the sizes (64-bit).
//  - COPY.  As the line gather's: the output is cut into spans of HG_GATHER_TILE bytes, one per workgroup; a pass of its own
//    finds the entry every span begins in; the workgroup stages the offsets of its entries in LDS when they are at most
//    HG_GATHER_SPAN_OFFSETS; a lane owns 16 output bytes at a time, finds the entry that covers the first by an upper bound in
//    those offsets (entries of size 0 share an offset: the last of them has the bytes) and builds its four dwords
//    (hg_partlines_chunk).  A chunk that lies inside one text run is four or five aligned dword loads funnel-shifted into four;
//    any other is built byte by byte from hg_partlines_plan, the entry's fields reloaded only where the entry changes.  Source
//    reads never leave [0, nbytes rounded up to 4): the aligned dwords of a run that ends at or before nbytes.
#pragma once
#include "hg_gather.h"
#include "hg_parts.h"

constexpr uint32_t HG_PARTLINES_NUMBER = 1u, HG_PARTLINES_BYTE_OFFSET = 2u, HG_PARTLINES_TERMINATE = 4u, HG_PARTLINES_LINE = 8u;  // HG_PARTS_* of the C ABI
constexpr uint32_t HG_PARTLINES_ALL = 15u;
constexpr uint32_t HG_PARTLINES_FIRST = 1u, HG_PARTLINES_LAST = 2u;  // HG_PART_FIRST, HG_PART_LAST: the per-entry kind bits
constexpr uint32_t HG_PARTLINES_MARK_MAX = 16;                       // HG_PARTS_MARK_MAX
// HgPartLinesEntry::form: the terminator, and the decimal digits of the two numbers (0: no such prefix)
constexpr uint32_t HG_PARTLINES_FORM_TERM = 1u, HG_PARTLINES_FORM_NUMBER_SHIFT = 8, HG_PARTLINES_FORM_OFFSET_SHIFT = 16, HG_PARTLINES_FORM_DIGITS_MASK = 31u;

// The two markers, by value in the launch arguments: 16 bytes each as two little-endian words, so that byte k is a shift and
// never an indexed read of an argument array.
struct HgPartLinesMarks {
  uint64_t on_lo, on_hi, off_lo, off_hi;
  uint32_t on_len, off_len;
};
HG_HD uint8_t hg_partlines_mark_byte(uint64_t lo, uint64_t hi, uint32_t k) { return static_cast<uint8_t>((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFFu); }
inline HgPartLinesMarks hg_partlines_marks(const uint8_t *on, uint32_t on_len, const uint8_t *off, uint32_t off_len) {  // (host: the engine, the replay)
  HgPartLinesMarks m{0, 0, 0, 0, on_len, off_len};
  for (uint32_t k = 0; k < on_len && k < HG_PARTLINES_MARK_MAX; k++) (k < 8 ? m.on_lo : m.on_hi) |= static_cast<uint64_t>(on[k]) << (8 * (k & 7));
  for (uint32_t k = 0; k < off_len && k < HG_PARTLINES_MARK_MAX; k++) (k < 8 ? m.off_lo : m.off_hi) |= static_cast<uint64_t>(off[k]) << (8 * (k & 7));
  return m;
}

// One entry as the copy pass reads it.
struct HgPartLinesEntry {
  uint64_t src;     // S: offset in the text of the piece's first scanned byte
  uint64_t line;    // the part's line_number (the number prefix is line + 1)
  uint64_t offset;  // the value of the offset prefix
  uint32_t gap;     // gap run = text[src + gap, src + from): prev_to in line mode, from in parts mode (empty)
  uint32_t from, to;
  uint32_t trail;   // trail run = text[src + to, src + trail): len on a last part in line mode, else to (empty)
  uint32_t form;    // HG_PARTLINES_FORM_*
  uint32_t reserved;
};
static_assert(sizeof(HgPartLinesEntry) == 48, "HgPartLinesEntry layout");

// What the kernels work on (hg_partlines_launch, hg_engine.h).
struct HgPartLinesArgs {
  HgGatherText text;
  HgGatherList recs;             // the last scan's final records (seg_of == nullptr: no segments)
  const HgPart *parts;           // the last scan's parts, their expressions and (after segments) their segments
  const uint32_t *part_pattern, *part_seg;
  uint64_t n_parts;
  const uint64_t *seg_start;     // the last scan's device array, nullptr without segments
  uint32_t flags;                // HG_PARTLINES_*
  uint64_t byte_base;
  HgPartLinesMarks marks;
  uint64_t *size;                // entry pass: size[q] (and size[n_parts] = 0)
  HgPartLinesEntry *entries;     // entry pass writes, copy pass reads
  uint64_t *line_number;         // per entry, the ABI's arrays
  uint32_t *kind, *pattern, *segment;  // (segment nullptr without segments)
  const uint64_t *off;           // exclusive scan of size: n_parts + 1
  uint64_t n_entries, n_bytes;   // span and copy pass
  uint64_t *span;                // span pass: per output span of HG_GATHER_TILE bytes the entry its first byte lies in, and n_entries - 1 behind the last
  uint8_t *out;                  // n_bytes rounded up to 16
};

HG_HD uint32_t hg_partlines_number_digits(uint32_t form) { return (form >> HG_PARTLINES_FORM_NUMBER_SHIFT) & HG_PARTLINES_FORM_DIGITS_MASK; }
HG_HD uint32_t hg_partlines_offset_digits(uint32_t form) { return (form >> HG_PARTLINES_FORM_OFFSET_SHIFT) & HG_PARTLINES_FORM_DIGITS_MASK; }
// Bytes in front of the gap run, and the whole entry.
HG_HD uint32_t hg_partlines_prefix(uint32_t form) {
  const uint32_t nd = hg_partlines_number_digits(form), od = hg_partlines_offset_digits(form);
  return (nd ? nd + 1 : 0u) + (od ? od + 1 : 0u);
}
HG_HD uint64_t hg_partlines_size(const HgPartLinesEntry &e, const HgPartLinesMarks &m) {
  return static_cast<uint64_t>(hg_partlines_prefix(e.form)) + (e.from - e.gap) + m.on_len + (e.to - e.from) + m.off_len + (e.trail - e.to) + ((e.form & HG_PARTLINES_FORM_TERM) ? 1u : 0u);
}

// Byte k of an entry, k < hg_partlines_size(e, m): its value, or -1 and *at = the text offset it is read from.  The one
// definition of the entry layout.
HG_HD int hg_partlines_plan(const HgPartLinesEntry &e, const HgPartLinesMarks &m, uint64_t k, uint64_t *at) {
  const uint32_t nd = hg_partlines_number_digits(e.form), od = hg_partlines_offset_digits(e.form);
  if (nd) {
    if (k < nd) return hg_gather_digit(e.line + 1, nd, static_cast<uint32_t>(k));
    if (k == nd) return ':';
    k -= nd + 1;
  }
  if (od) {
    if (k < od) return hg_gather_digit(e.offset, od, static_cast<uint32_t>(k));
    if (k == od) return ':';
    k -= od + 1;
  }
  if (k < e.from - e.gap) {
    *at = e.src + e.gap + k;
    return -1;
  }
  k -= e.from - e.gap;
  if (k < m.on_len) return hg_partlines_mark_byte(m.on_lo, m.on_hi, static_cast<uint32_t>(k));
  k -= m.on_len;
  if (k < e.to - e.from) {
    *at = e.src + e.from + k;
    return -1;
  }
  k -= e.to - e.from;
  if (k < m.off_len) return hg_partlines_mark_byte(m.off_lo, m.off_hi, static_cast<uint32_t>(k));
  k -= m.off_len;
  if (k < e.trail - e.to) {
    *at = e.src + e.to + k;
    return -1;
  }
  return '\n';
}
template <typename Text>
HG_HD uint8_t hg_partlines_byte(const Text &text, const HgPartLinesEntry &e, const HgPartLinesMarks &m, uint64_t k) {
  uint64_t at = 0;
  const int v = hg_partlines_plan(e, m, k, &at);
  return v < 0 ? text.byte(at) : static_cast<uint8_t>(v);
}

HG_HD uint32_t hg_partlines_seg(const HgPartLinesArgs &a, uint64_t q) { return a.part_seg ? a.part_seg[q] : 0u; }

// The entry pass for part q < n_parts: the entry's fields, its size and the ABI's per-entry arrays.  A part whose piece has no
// record (the parts stage never leaves one) gives an entry of no bytes.
template <typename Text>
HG_HD void hg_partlines_entry(const HgPartLinesArgs &a, const Text &text, uint64_t q) {
  const HgPart p = a.parts[q];
  const uint32_t seg = hg_partlines_seg(a, q);
  const bool first = q == 0 || a.parts[q - 1].line_no != p.line_no || hg_partlines_seg(a, q - 1) != seg;
  const bool last = q + 1 == a.n_parts || a.parts[q + 1].line_no != p.line_no || hg_partlines_seg(a, q + 1) != seg;
  const bool line_mode = (a.flags & HG_PARTLINES_LINE) != 0;
  const uint64_t r = hg_gather_lower_bound(a.recs, seg, p.line_no);
  HgPartLinesEntry e{0, p.line_no, 0, p.from, p.from, p.from, p.from, 0, 0};
  uint64_t size = 0;
  if (r < a.recs.n && a.recs.hits[r].line_no == p.line_no && hg_gather_seg(a.recs, r) == seg) {
    const HgHitAux x = a.recs.aux[r];
    e.src = (a.seg_start ? a.seg_start[seg] : 0) + x.start;
    e.to = p.to;
    e.gap = line_mode ? (first ? 0u : a.parts[q - 1].to) : p.from;
    e.trail = line_mode && last ? x.len : p.to;
    e.offset = a.byte_base + x.start + (line_mode ? 0u : p.from);
    if (!line_mode || first) {
      if (a.flags & HG_PARTLINES_NUMBER) e.form |= hg_gather_digits(p.line_no + 1) << HG_PARTLINES_FORM_NUMBER_SHIFT;
      if (a.flags & HG_PARTLINES_BYTE_OFFSET) e.form |= hg_gather_digits(e.offset) << HG_PARTLINES_FORM_OFFSET_SHIFT;
    }
    // (e.trail >= e.to >= 1: a part is never empty)
    if ((a.flags & HG_PARTLINES_TERMINATE) && (!line_mode || last) && text.byte(e.src + e.trail - 1) != '\n') e.form |= HG_PARTLINES_FORM_TERM;
    size = hg_partlines_size(e, a.marks);
  }
  a.entries[q] = e;
  a.size[q] = size;
  a.line_number[q] = p.line_no;
  a.kind[q] = (first ? HG_PARTLINES_FIRST : 0u) | (last ? HG_PARTLINES_LAST : 0u);
  a.pattern[q] = a.part_pattern[q];
  if (a.segment) a.segment[q] = seg;
}

// span[t] for the output spans of `tile` bytes, t in [0, n_spans]: the entry that holds byte t * tile, and n_entries - 1 for
// t == n_spans.  The bytes of span t lie in the entries [span[t], span[t + 1]].  (n_bytes > 0.)
HG_HD uint64_t hg_partlines_span(const HgPartLinesArgs &a, uint64_t tile, uint64_t t) {
  return t * tile < a.n_bytes ? hg_gather_find(a.off, 0, a.n_entries - 1, t * tile) : a.n_entries - 1;
}

// (the walk of a chunk that is not inside one text run: the entry under the cursor and its span of the output)
struct HgPartLinesCursor {
  uint64_t j, begin, end;
  HgPartLinesEntry e;
};
// Four output bytes from pos on, in two steps so that the text reads of a word are in flight together: where every byte comes
// from (the cursor moves on over the entries; no text is read), then the reads.
template <typename Text>
HG_HD uint32_t hg_partlines_word(const HgPartLinesArgs &a, const Text &text, uint64_t pos, HgPartLinesCursor &c) {
  uint64_t at0 = 0, at1 = 0, at2 = 0, at3 = 0;
  int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
#define HG_PARTLINES_PLAN(b, v, at)                                         \
  if (pos + (b) < a.n_bytes) {                                              \
    while (pos + (b) >= c.end) { /* (entries of size 0 are stepped over) */ \
      c.j++;                                                                \
      c.e = a.entries[c.j];                                                 \
      c.begin = c.end;                                                      \
      c.end = a.off[c.j + 1];                                               \
    }                                                                       \
    v = hg_partlines_plan(c.e, a.marks, pos + (b)-c.begin, &at);            \
  }
  HG_PARTLINES_PLAN(0, v0, at0)
  HG_PARTLINES_PLAN(1, v1, at1)
  HG_PARTLINES_PLAN(2, v2, at2)
  HG_PARTLINES_PLAN(3, v3, at3)
#undef HG_PARTLINES_PLAN
  const uint32_t b0 = v0 < 0 ? text.byte(at0) : static_cast<uint32_t>(v0), b1 = v1 < 0 ? text.byte(at1) : static_cast<uint32_t>(v1);
  const uint32_t b2 = v2 < 0 ? text.byte(at2) : static_cast<uint32_t>(v2), b3 = v3 < 0 ? text.byte(at3) : static_cast<uint32_t>(v3);
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}
// The 16 output bytes [pos, pos + 16), pos a multiple of 16 below n_bytes, as four little-endian dwords; j: the entry that holds
// byte pos (hg_gather_find) and [begin, end) = [off[j], off[j + 1]) its span of the output.  Bytes at or past n_bytes are 0.
template <typename Text>
HG_HD HgGatherChunk hg_partlines_chunk(const HgPartLinesArgs &a, const Text &text, uint64_t pos, uint64_t j, uint64_t begin, uint64_t end) {
  HgPartLinesCursor c{j, begin, end, a.entries[j]};
  const uint64_t k = pos - c.begin;
  // the three text runs of the entry: where each begins in it, and the run (if any) that holds all of [k, k + 16)
  const uint64_t r0 = hg_partlines_prefix(c.e.form), r1 = r0 + (c.e.from - c.e.gap) + a.marks.on_len, r2 = r1 + (c.e.to - c.e.from) + a.marks.off_len;
  uint64_t s = 0;
  bool inside = false;
  if (k >= r2) inside = k + 16 <= r2 + (c.e.trail - c.e.to), s = c.e.src + c.e.to + (k - r2);
  else if (k >= r1) inside = k + 16 <= r1 + (c.e.to - c.e.from), s = c.e.src + c.e.from + (k - r1);
  else if (k >= r0) inside = k + 16 <= r0 + (c.e.from - c.e.gap), s = c.e.src + c.e.gap + (k - r0);
  if (inside) {
    const uint64_t base = s & ~static_cast<uint64_t>(3);
    const uint32_t shift = static_cast<uint32_t>(s & 3);
    const uint32_t d0 = text.dword(base), d1 = text.dword(base + 4), d2 = text.dword(base + 8), d3 = text.dword(base + 12);
    if (!shift) return HgGatherChunk{d0, d1, d2, d3};  // (unshifted, a fifth dword may lie past the readable range)
    const uint32_t d4 = text.dword(base + 16);
    return HgGatherChunk{hg_gather_funnel(d0, d1, shift), hg_gather_funnel(d1, d2, shift), hg_gather_funnel(d2, d3, shift), hg_gather_funnel(d3, d4, shift)};
  }
  HgGatherChunk out;
  out.w0 = hg_partlines_word(a, text, pos, c);
  out.w1 = hg_partlines_word(a, text, pos + 4, c);
  out.w2 = hg_partlines_word(a, text, pos + 8, c);
  out.w3 = hg_partlines_word(a, text, pos + 12, c);
  return out;
}
