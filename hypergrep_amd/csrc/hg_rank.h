// The matched values ranked by count, per file if asked, and cut to the `top` most frequent on the GPU (hg_rank_values; grep -o |
// sort | uniq -c | sort -rn | head): only the kept rows' bytes are gathered and leave the device.  The scalar rules here are
// shared by the kernels (hg_rank.hip) and the host replay of the tests (tests/native/ranksim.cpp compiles this header for x86).
// hg_values.h lends the VALUE rule, the hash, the table and the compaction; hg_gather.h its copy pass.
//
//  - GROUPS.  hg_values.h's groups with the key (segment, [expression,] bytes): the segment is in the key with
//    HG_RANK_F_PER_SEGMENT (HG_VALUES_F_BY_SEGMENT), the expression with HG_RANK_F_BY_PATTERN.  They arrive as (first, count)
//    pairs sorted by ascending first (n_groups of them: n_distinct of the result).
//  - ORDER.  A stable sort by descending count leaves ties in ascending first.  With HG_RANK_F_PER_SEGMENT every group then
//    takes its segment, part_seg[first], as a key and its place as the value (hg_rank_keys), and a second stable sort by that
//    key gives (segment ascending, count descending, first ascending).  first is unique, so the order is total.
//  - BOUNDS.  A lane per segment s <= n_seg: lo, hi = the lower bounds of s and s + 1 among the sorted groups' segments (without
//    HG_RANK_F_PER_SEGMENT there is one segment that owns every group).  first_group[s] = lo, seg_distinct[s] = hi - lo,
//    seg_parts[s] = cum[hi] - cum[lo] (cum: the exclusive scan of the counts in the final order) and kept[s] = min(seg_distinct[s],
//    top), seg_distinct[s] for top == 0.  A segment without parts has lo == hi: an empty range.  No lane reads what another wrote.
//  - PLACE.  first_value = exclusive scan of kept.  Group j of segment s has rank r = j - first_group[s]; with r < kept[s] it is
//    row first_value[s] + r and takes count and first from its pair and pattern, line number, segment, length and copy entry
//    from part `first`; a group beyond the cut writes nothing.  The lengths of the rows (zero behind the last) are scanned to
//    off, and the line gather's span and copy pass move the bytes.
// Every index is checked where it is made: a group below n_groups, a part below n_parts, a segment below n_seg, a row below
// n_groups.  Nothing here reads the text.
#pragma once
#include "hg_values.h"

constexpr uint32_t HG_RANK_F_BY_PATTERN = HG_VALUES_F_BY_PATTERN, HG_RANK_F_PER_SEGMENT = HG_VALUES_F_BY_SEGMENT;  // HG_RANK_* of the C ABI
constexpr uint32_t HG_RANK_THREADS = 256;

struct HgRankArgs {
  const HgPart *parts;  // the last scan's parts, their expressions and (after segments) their segments
  const uint32_t *part_pattern, *part_seg;
  uint64_t n_parts;
  const uint64_t *src;  // the values stage's hash pass, per part: where the value lies and how long it is
  const uint32_t *len;
  uint32_t flags;       // HG_RANK_F_*
  uint32_t n_seg;       // with HG_RANK_F_PER_SEGMENT the scan's segments, else 1
  uint64_t top;         // 0: no cut
  uint64_t n_groups;
  const uint64_t *g_first, *g_count;  // the groups by (count descending, first ascending)
  // keys pass (HG_RANK_F_PER_SEGMENT only), and the same arrays after the sort by segment
  uint32_t *key_seg;
  uint64_t *key_idx;
  const uint32_t *s_seg;  // nullptr without HG_RANK_F_PER_SEGMENT: every group in segment 0, s_idx the identity
  const uint64_t *s_idx;
  // counts pass: the counts in the final order, n_groups + 1 (the last 0); cum is their exclusive scan
  uint64_t *s_count;
  const uint64_t *cum;
  // bounds pass: n_seg + 1 each (kept's last 0; seg_distinct and seg_parts n_seg); first_value is kept's exclusive scan
  uint64_t *first_group, *seg_distinct, *seg_parts, *kept;
  const uint64_t *first_value;
  // place pass, per row
  uint64_t *out_first, *out_count;
  uint64_t *size;          // n_groups + 1, zeroed before the pass
  HgGatherEntry *entries;  // what the copy pass reads: {src, line, len, form 0}
  uint32_t *pattern, *segment;  // (segment nullptr without segments)
  uint64_t *line_number;
};

// The first group at or behind segment s in the final order.
HG_HD uint64_t hg_rank_lower_bound(const HgRankArgs &a, uint64_t s) {
  if (!a.s_seg) return s == 0 ? 0 : a.n_groups;
  uint64_t lo = 0, hi = a.n_groups;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a.s_seg[mid] < s) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Keys pass, group j < n_groups of the count order: its segment and its place.
HG_HD void hg_rank_keys(const HgRankArgs &a, uint64_t j) {
  const uint64_t f = a.g_first[j];
  const uint32_t s = (f < a.n_parts && a.part_seg) ? a.part_seg[f] : 0u;
  a.key_seg[j] = s < a.n_seg ? s : a.n_seg - 1;  // (a part's segment is below n_seg: nothing is clamped)
  a.key_idx[j] = j;
}

// Counts pass, j <= n_groups of the final order.
HG_HD void hg_rank_counts(const HgRankArgs &a, uint64_t j) {
  if (j >= a.n_groups) {
    a.s_count[j] = 0;
    return;
  }
  const uint64_t g = a.s_idx ? a.s_idx[j] : j;
  a.s_count[j] = g < a.n_groups ? a.g_count[g] : 0;
}

// Bounds pass, segment s <= n_seg.
HG_HD void hg_rank_bounds(const HgRankArgs &a, uint64_t s) {
  if (s >= a.n_seg) {
    a.first_group[s] = a.n_groups;
    a.kept[s] = 0;
    return;
  }
  const uint64_t lo = hg_rank_lower_bound(a, s), hi = hg_rank_lower_bound(a, s + 1), n = hi - lo;
  a.first_group[s] = lo;
  a.seg_distinct[s] = n;
  a.seg_parts[s] = a.cum[hi] - a.cum[lo];
  a.kept[s] = (a.top && a.top < n) ? a.top : n;
}

// Place pass, group j < n_groups of the final order.
HG_HD void hg_rank_place(const HgRankArgs &a, uint64_t j) {
  const uint64_t s = a.s_seg ? a.s_seg[j] : 0u, g = a.s_idx ? a.s_idx[j] : j;
  if (s >= a.n_seg || g >= a.n_groups || j < a.first_group[s]) return;
  const uint64_t r = j - a.first_group[s];
  if (r >= a.kept[s]) return;  // beyond the cut
  const uint64_t row = a.first_value[s] + r, f = a.g_first[g];
  if (row >= a.n_groups || f >= a.n_parts) return;
  const HgPart p = a.parts[f];
  a.out_first[row] = f;
  a.out_count[row] = a.g_count[g];
  a.size[row] = a.len[f];
  a.entries[row] = HgGatherEntry{a.src[f], p.line_no, a.len[f], 0u};
  a.pattern[row] = a.part_pattern[f];
  a.line_number[row] = p.line_no;
  if (a.segment) a.segment[row] = a.part_seg ? a.part_seg[f] : 0u;
}
