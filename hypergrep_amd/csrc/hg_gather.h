// The lines themselves (hg_gather_lines): the bytes of every line piece the last scan left a record for, gathered on the GPU
// into one compact, ordered, optionally print-ready buffer.  The scalar rules here are shared by the kernels (hg_gather.hip)
// and the host replay of the tests (tests/native/gathersim.cpp compiles this header for x86); the product only calls them
// from device code.
//
// The stage works on two ordered record lists the scan left on the device: the MAIN list (the final hits, the selected pieces
// of an inverted scan, or the surviving records of a scan with segments) and, with HG_LINES_CONTEXT, the CONTEXT list (context
// and tail pieces).  Either is ordered by (segment, line) and the two share no line; the main list may hold several records
// per line.  Records are numbered in one space: r in [0, n_main) is main record r, r in [n_main, n_main + n_ctx) context
// record r - n_main.
//  - HEAD.  An entry is a distinct (segment, line): record r heads one if it is the first of its list or differs from the
//    record before it in segment or line (hg_gather_head).  F = exclusive scan of the head flags over the n + 1 numbers.
//  - RANK.  The entry index of a head is the heads before it in its own list plus the heads of the other list with a smaller
//    (segment, line): a lower bound in the other list and F there (hg_gather_rank).  No sort.
//  - LAYOUT.  Entry j is [separator "--\n"][decimal line + 1, then ':' (match) or '-' (context, tail)] body [terminator '\n'],
//    the body being text[src, src + len) as it is.  hg_gather_form decides the optional parts (the terminator test reads the
//    body's last byte), hg_gather_size adds them up, hg_gather_byte gives byte k of an entry: the one definition of the layout.
//    off = exclusive scan of the sizes (64-bit).
//  - COPY.  The output is cut into spans of HG_GATHER_TILE bytes, one per workgroup.  A pass of its own finds the entry every
//    span begins in (hg_gather_span: a lane per span, so the binary searches run side by side instead of one in front of every
//    workgroup); the workgroup stages the offsets of its entries in LDS when they are at most HG_GATHER_SPAN_OFFSETS; a lane owns 16 output bytes at a time, finds the entry that covers the first by an upper bound in
//    those offsets (entries of size 0 share an offset: the last of them is the one that has bytes), and builds its four dwords
//    (hg_gather_chunk).  A chunk that lies inside one body is five aligned
//    dword loads funnel-shifted into four; any other is built byte by byte from hg_gather_byte, the entry's fields reloaded
//    only where the entry changes.  Source reads never leave [0, nbytes rounded up to 4): the aligned dwords of a body that
//    ends at or before nbytes.
#pragma once
#include "hg_context.h"
#include "hg_core.h"

#ifndef HG_GATHER_TILE
#define HG_GATHER_TILE 16384u  // output bytes per workgroup of the copy pass (the value include/hypergrep_amd.h publishes)
#endif
constexpr uint32_t HG_GATHER_THREADS = 256;  // its lanes: 16 bytes each per step, HG_GATHER_TILE / 4096 steps
static_assert(HG_GATHER_TILE % (16 * HG_GATHER_THREADS) == 0, "a span is a whole number of steps");
constexpr uint32_t HG_GATHER_SPAN_OFFSETS = 2048;  // entry offsets of a span the copy pass stages in LDS (16 KiB); spans of more entries search `off` in memory
constexpr uint32_t HG_GATHER_CONTEXT = 1u, HG_GATHER_TERMINATE = 2u, HG_GATHER_NUMBER = 4u, HG_GATHER_SEPARATOR = 8u;  // HG_LINES_* of the C ABI
constexpr uint32_t HG_GATHER_MATCH = 0, HG_GATHER_KIND_CONTEXT = 1, HG_GATHER_KIND_TAIL = 2;                          // HG_LINE_*
// HgGatherEntry::form: what the entry has besides its body
constexpr uint32_t HG_GATHER_FORM_SEP = 1u, HG_GATHER_FORM_TERM = 2u, HG_GATHER_FORM_KIND_SHIFT = 2, HG_GATHER_FORM_DIGITS_SHIFT = 8;

// Where the stage reads the scanned text.  The replay has a type of its own with the same two members (it checks the range).
struct HgGatherText {
  const uint8_t *p;
  HG_HD uint8_t byte(uint64_t o) const { return p[o]; }
  HG_HD uint32_t dword(uint64_t o) const { return *reinterpret_cast<const uint32_t *>(p + o); }  // o is a multiple of 4
};

// One of the two record lists.  seg_of == nullptr: no segments (every record is of segment 0).
struct HgGatherList {
  const HgHit *hits;
  const HgHitAux *aux;
  const uint32_t *seg_of;
  uint64_t n;
};

// One entry as the copy pass reads it.
struct HgGatherEntry {
  uint64_t src;   // offset in the text of the body's first byte
  uint64_t line;  // the record's line_number
  uint32_t len;   // the body
  uint32_t form;  // HG_GATHER_FORM_*: separator, terminator, kind << 2, digits of line + 1 << 8 (0: no number prefix)
};

// What the kernels work on (hg_gather_launch, hg_engine.h).
struct HgGatherArgs {
  HgGatherText text;
  HgGatherList main, ctx;      // ctx.n == 0 without HG_LINES_CONTEXT
  const uint64_t *seg_start;   // the last scan's device array, nullptr without segments
  const uint64_t *first_record, *first_context;  // n_seg + 1 each (first_context nullptr: no context list), nullptr without segments
  uint64_t n_seg;
  uint32_t flags;              // HG_GATHER_*
  uint64_t *head;              // flag pass: n_main + n_ctx + 1 head flags (the last 0)
  const uint64_t *F;           // their exclusive scan
  uint64_t *size;              // entry pass: size[j] of entry j (zeroed up to n_main + n_ctx + 1 before)
  HgGatherEntry *entries;      // entry pass writes, copy pass reads
  uint64_t *line_number;       // per entry, the ABI's arrays
  uint32_t *kind, *segment;    // (segment nullptr without segments)
  uint64_t *first_entry;       // n_seg + 1
  const uint64_t *off;         // exclusive scan of size: n_entries + 1 (and on, constant)
  uint64_t n_entries, n_bytes; // span and copy pass
  uint64_t *span;              // span pass: per output span of HG_GATHER_TILE bytes the entry its first byte lies in, and n_entries - 1 behind the last
  uint8_t *out;                // n_bytes rounded up to 16
};

HG_HD uint32_t hg_gather_seg(const HgGatherList &l, uint64_t i) { return l.seg_of ? l.seg_of[i] : 0u; }

// Does record i of the list head an entry?
HG_HD bool hg_gather_head(const HgGatherList &l, uint64_t i) {
  return i == 0 || l.hits[i - 1].line_no != l.hits[i].line_no || hg_gather_seg(l, i - 1) != hg_gather_seg(l, i);
}

// First index i of the list with (segment, line) >= (seg, line).
HG_HD uint64_t hg_gather_lower_bound(const HgGatherList &l, uint32_t seg, uint64_t line) {
  uint64_t lo = 0, hi = l.n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint32_t s = hg_gather_seg(l, mid);
    if (s < seg || (s == seg && l.hits[mid].line_no < line)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Merge rank: the entry index of head record i of `own` (own_base: the number of own's record 0 in F), given lb = the lower
// bound of its (segment, line) in `other` (other_base likewise).  F[base + k] - F[base] = heads among a list's first k records.
HG_HD uint64_t hg_gather_rank(const uint64_t *F, uint64_t own_base, uint64_t i, uint64_t other_base, uint64_t lb) {
  return (F[own_base + i] - F[own_base]) + (F[other_base + lb] - F[other_base]);
}

// Decimal digits of v (1 .. 20).
HG_HD uint32_t hg_gather_digits(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) {
    v /= 10;
    d++;
  }
  return d;
}

// Digit k (0: the most significant) of v, which has d digits.
HG_HD uint8_t hg_gather_digit(uint64_t v, uint32_t d, uint32_t k) {
  if (v <= 0xFFFFFFFFull) {  // (no 64-bit division for the line numbers of ordinary texts)
    uint32_t w = static_cast<uint32_t>(v);
    for (uint32_t j = k + 1; j < d; j++) w /= 10;
    return static_cast<uint8_t>('0' + w % 10);
  }
  for (uint32_t j = k + 1; j < d; j++) v /= 10;
  return static_cast<uint8_t>('0' + v % 10);
}

// The optional parts of an entry.  has_prev: it is not entry 0; (prev_seg, prev_line): the entry before it in the output.
template <typename Text>
HG_HD uint32_t hg_gather_form(const Text &text, uint32_t flags, uint32_t kind, uint64_t src, uint32_t len, uint32_t seg, uint64_t line, bool has_prev, uint32_t prev_seg,
                              uint64_t prev_line) {
  uint32_t form = kind << HG_GATHER_FORM_KIND_SHIFT;
  if ((flags & HG_GATHER_SEPARATOR) && has_prev && (seg != prev_seg || line != prev_line + 1)) form |= HG_GATHER_FORM_SEP;
  if ((flags & HG_GATHER_TERMINATE) && (len == 0 || text.byte(src + len - 1) != '\n')) form |= HG_GATHER_FORM_TERM;
  if (flags & HG_GATHER_NUMBER) form |= hg_gather_digits(line + 1) << HG_GATHER_FORM_DIGITS_SHIFT;
  return form;
}

// Bytes in front of the body, and the whole entry.
HG_HD uint32_t hg_gather_prefix(uint32_t form) {
  const uint32_t digits = form >> HG_GATHER_FORM_DIGITS_SHIFT;
  return ((form & HG_GATHER_FORM_SEP) ? 3u : 0u) + (digits ? digits + 1 : 0u);
}
HG_HD uint64_t hg_gather_size(uint32_t form, uint32_t len) { return static_cast<uint64_t>(hg_gather_prefix(form)) + len + ((form & HG_GATHER_FORM_TERM) ? 1u : 0u); }

// Byte k of an entry, k < hg_gather_size(e.form, e.len): its value, or -1 and *at = the text offset it is read from.  The one
// definition of the entry layout.
HG_HD int hg_gather_plan(const HgGatherEntry &e, uint64_t k, uint64_t *at) {
  if (e.form & HG_GATHER_FORM_SEP) {
    if (k < 3) return k == 2 ? '\n' : '-';
    k -= 3;
  }
  const uint32_t digits = e.form >> HG_GATHER_FORM_DIGITS_SHIFT;
  if (digits) {
    if (k < digits) return hg_gather_digit(e.line + 1, digits, static_cast<uint32_t>(k));
    if (k == digits) return ((e.form >> HG_GATHER_FORM_KIND_SHIFT) & 3u) == HG_GATHER_MATCH ? ':' : '-';
    k -= digits + 1;
  }
  if (k >= e.len) return '\n';
  *at = e.src + k;
  return -1;
}
template <typename Text>
HG_HD uint8_t hg_gather_byte(const Text &text, const HgGatherEntry &e, uint64_t k) {
  uint64_t at = 0;
  const int v = hg_gather_plan(e, k, &at);
  return v < 0 ? text.byte(at) : static_cast<uint8_t>(v);
}

// The flag pass: head flag of record r of the one numbering (r < n_main + n_ctx).
HG_HD uint64_t hg_gather_flag(const HgGatherArgs &a, uint64_t r) { return r < a.main.n ? hg_gather_head(a.main, r) : hg_gather_head(a.ctx, r - a.main.n); }

// The entry pass for record r: nothing unless it heads an entry; else the entry's index, with its fields, size and the ABI's
// per-entry arrays written.
template <typename Text>
HG_HD void hg_gather_entry(const HgGatherArgs &a, const Text &text, uint64_t r) {
  const bool is_main = r < a.main.n;
  const HgGatherList &own = is_main ? a.main : a.ctx, &other = is_main ? a.ctx : a.main;
  const uint64_t own_base = is_main ? 0 : a.main.n, other_base = is_main ? a.main.n : 0, i = r - own_base;
  if (!hg_gather_head(own, i)) return;
  const uint32_t seg = hg_gather_seg(own, i);
  const HgHit h = own.hits[i];
  const HgHitAux x = own.aux[i];
  const uint64_t lb = other.n ? hg_gather_lower_bound(other, seg, h.line_no) : 0;
  const uint64_t j = hg_gather_rank(a.F, own_base, i, other_base, lb);
  // the entry before it: the later of the piece before it in its own list and the last smaller piece of the other
  bool has_prev = false;
  uint32_t prev_seg = 0;
  uint64_t prev_line = 0;
  if (i > 0) has_prev = true, prev_seg = hg_gather_seg(own, i - 1), prev_line = own.hits[i - 1].line_no;
  if (lb > 0) {
    const uint32_t s = hg_gather_seg(other, lb - 1);
    const uint64_t l = other.hits[lb - 1].line_no;
    if (!has_prev || s > prev_seg || (s == prev_seg && l > prev_line)) has_prev = true, prev_seg = s, prev_line = l;
  }
  const uint32_t kind = is_main ? HG_GATHER_MATCH : (h.id == HG_CTX_ID_TAIL ? HG_GATHER_KIND_TAIL : HG_GATHER_KIND_CONTEXT);
  const uint64_t src = (a.seg_start ? a.seg_start[seg] : 0) + x.start;
  const uint32_t form = hg_gather_form(text, a.flags, kind, src, x.len, seg, h.line_no, has_prev, prev_seg, prev_line);
  a.entries[j] = HgGatherEntry{src, h.line_no, x.len, form};
  a.size[j] = hg_gather_size(form, x.len);
  a.line_number[j] = h.line_no;
  a.kind[j] = kind;
  if (a.segment) a.segment[j] = seg;
}

// first_entry[s], s in [0, n_seg]: the entries of the segments before s.
HG_HD uint64_t hg_gather_first(const HgGatherArgs &a, uint64_t s) {
  uint64_t n = a.F[a.first_record[s]];
  if (a.ctx.n && a.first_context) n += a.F[a.main.n + a.first_context[s]] - a.F[a.main.n];
  return n;
}

// The entry that holds output byte pos < n_bytes: the last j in [lo, hi] with off[j] <= pos, given off[lo] <= pos < off[hi + 1].
HG_HD uint64_t hg_gather_find(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t pos) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// span[t] for the output spans of `tile` bytes, t in [0, n_spans]: the entry that holds byte t * tile, and n_entries - 1 for
// t == n_spans.  The bytes of span t lie in the entries [span[t], span[t + 1]].  (n_bytes > 0.)
HG_HD uint64_t hg_gather_span(const HgGatherArgs &a, uint64_t tile, uint64_t t) {
  return t * tile < a.n_bytes ? hg_gather_find(a.off, 0, a.n_entries - 1, t * tile) : a.n_entries - 1;
}

HG_HD uint32_t hg_gather_funnel(uint32_t lo, uint32_t hi, uint32_t byte_shift) {
  return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (8 * byte_shift));
}

// The 16 output bytes [pos, pos + 16), pos a multiple of 16 below n_bytes, as four little-endian dwords; j: the entry that holds
// byte pos (hg_gather_find) and [begin, end) = [off[j], off[j + 1]) its span of the output.  Bytes at or past n_bytes are 0.
struct HgGatherChunk {
  uint32_t w0, w1, w2, w3;
};
// (the walk of a chunk that is not inside one body: the entry under the cursor and its span of the output)
struct HgGatherCursor {
  uint64_t j, begin, end;
  HgGatherEntry e;
};
// Four output bytes from pos on, in two steps so that the text reads of a word are in flight together: where every byte comes
// from (the cursor moves on over the entries; no text is read), then the reads.
template <typename Text>
HG_HD uint32_t hg_gather_word(const HgGatherArgs &a, const Text &text, uint64_t pos, HgGatherCursor &c) {
  uint64_t at0 = 0, at1 = 0, at2 = 0, at3 = 0;
  int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
#define HG_GATHER_PLAN(b, v, at)                                            \
  if (pos + (b) < a.n_bytes) {                                              \
    while (pos + (b) >= c.end) { /* (entries of size 0 are stepped over) */ \
      c.j++;                                                                \
      c.e = a.entries[c.j];                                                 \
      c.begin = c.end;                                                      \
      c.end = a.off[c.j + 1];                                               \
    }                                                                       \
    v = hg_gather_plan(c.e, pos + (b)-c.begin, &at);                        \
  }
  HG_GATHER_PLAN(0, v0, at0)
  HG_GATHER_PLAN(1, v1, at1)
  HG_GATHER_PLAN(2, v2, at2)
  HG_GATHER_PLAN(3, v3, at3)
#undef HG_GATHER_PLAN
  const uint32_t b0 = v0 < 0 ? text.byte(at0) : static_cast<uint32_t>(v0), b1 = v1 < 0 ? text.byte(at1) : static_cast<uint32_t>(v1);
  const uint32_t b2 = v2 < 0 ? text.byte(at2) : static_cast<uint32_t>(v2), b3 = v3 < 0 ? text.byte(at3) : static_cast<uint32_t>(v3);
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}
template <typename Text>
HG_HD HgGatherChunk hg_gather_chunk(const HgGatherArgs &a, const Text &text, uint64_t pos, uint64_t j, uint64_t begin, uint64_t end) {
  HgGatherCursor c{j, begin, end, a.entries[j]};
  const uint64_t k = pos - c.begin;
  const uint32_t prefix = hg_gather_prefix(c.e.form);
  if (k >= prefix && k + 16 <= static_cast<uint64_t>(prefix) + c.e.len) {  // inside one body
    const uint64_t s = c.e.src + (k - prefix), base = s & ~static_cast<uint64_t>(3);
    const uint32_t shift = static_cast<uint32_t>(s & 3);
    const uint32_t d0 = text.dword(base), d1 = text.dword(base + 4), d2 = text.dword(base + 8), d3 = text.dword(base + 12);
    if (!shift) return HgGatherChunk{d0, d1, d2, d3};  // (unshifted, a fifth dword may lie past the readable range)
    const uint32_t d4 = text.dword(base + 16);
    return HgGatherChunk{hg_gather_funnel(d0, d1, shift), hg_gather_funnel(d1, d2, shift), hg_gather_funnel(d2, d3, shift), hg_gather_funnel(d3, d4, shift)};
  }
  HgGatherChunk out;
  out.w0 = hg_gather_word(a, text, pos, c);
  out.w1 = hg_gather_word(a, text, pos + 4, c);
  out.w2 = hg_gather_word(a, text, pos + 8, c);
  out.w3 = hg_gather_word(a, text, pos + 12, c);
  return out;
}
