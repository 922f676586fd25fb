// The value store (hg_accumulate_values, hg_rank_accumulated): a device-resident table of distinct matched values that survives
// scans, so that a text that arrives in many buffers is answered as one (grep -o | sort | uniq -c | sort -rn | head over a stream
// of chunks) and only the kept rows leave the GPU.  The scalar rules here are shared by the kernels (hg_valstore.hip) and the
// host replay of the tests (tests/native/valstoresim.cpp compiles this header for x86); the product only calls them from device
// code.  hg_values.h lends the VALUE and KEY rules, the hash and the slot word; hg_gather.h its copy pass.
//
//  - STORE.  Value i < n_values has an offset into the byte arena, a length, the expression, hash, count, first (an ordinal: the
//    parts of the earlier calls plus the part's index in its own call) and line number of its first part.  Index order is the
//    order of first occurrence over all calls.  A table of 2^store_log2 slots holds (tag, store index in 40 bits) words,
//    hg_values.h's fields, at or behind hg_values_home of the stored hash.
//  - CALL.  The values stage's grouping (HgValues::group) turns the call's parts into groups (first, count) sorted by first; src,
//    len and hash per part are its hash pass's, and the store reuses that hash (so hash_bits and the key's flag are fixed when a
//    store begins).
//  - LOOKUP.  Group j probes the table read-only, linearly from its home, for at most the capacity: an empty slot ends the probe
//    (the group is new); an occupied one is the group's iff tag, length, (expression) and bytes are equal.  The bytes are the
//    chunk text at src against the arena at the stored offset: two buffers at two independent alignments, compared by whole
//    aligned dwords of both, funnel-shifted (hg_valstore_equal; hg_valstore_equal_wave_lane is lane l's share for a wave).
//    match[j] is a store index or HG_VALSTORE_NONE.  Nothing of the store changes.
//  - SIZE.  new_flag and new_len per group (zero behind the last) are scanned: a new group's index is n_values + new_idx[j], in
//    the order of first, and its bytes lie at arena_tail + new_off[j].
//  - REHASH.  When the table changes size every stored value claims the first empty slot from its home in the new one.  Stored
//    values are pairwise distinct: nothing is compared.
//  - APPLY.  A group that was found adds its count (groups of one call have distinct keys: one lane per value).  A new one writes
//    its row, its copy entry and claims the first empty slot from its home.  New values differ from each other and from the
//    store: nothing is compared.
//  - RANK.  A stable sort of the indices by descending count leaves ties in index order, which is the order of first.  Place r of
//    the first min(top, n) takes its row from the store and a copy entry into the arena.
// Text reads never leave [0, nbytes rounded up to 4), arena reads never leave [0, its bytes rounded up to 4).  Every index is
// checked where it is made: a group below n_groups, a part below n_parts, a store index below the values, a slot masked to the
// capacity.
#pragma once
#include "hg_values.h"

constexpr uint32_t HG_VALSTORE_F_BY_PATTERN = HG_VALUES_F_BY_PATTERN;  // HG_ACC_BY_PATTERN of the C ABI
constexpr uint32_t HG_VALSTORE_THREADS = 256;
constexpr uint64_t HG_VALSTORE_NONE = ~uint64_t{0};
constexpr uint32_t HG_VALSTORE_N_LONG = 0, HG_VALSTORE_OVERFLOW = 1, HG_VALSTORE_COUNTERS = 2;  // HgValStoreArgs::counters

struct HgValStoreArgs {
  HgGatherText text;   // the call's text
  HgGatherText arena;  // the store's bytes
  // the call's parts and groups (HgValues::group)
  const HgPart *parts;
  const uint32_t *part_pattern;
  uint64_t n_parts;
  const uint64_t *src;  // per part, the hash pass's
  const uint32_t *len;
  const uint64_t *hash;
  const uint64_t *g_first, *g_count;  // per group, sorted by first
  uint64_t n_groups;
  uint32_t flags;  // HG_VALSTORE_F_*
  // the store before the call
  uint32_t store_log2;
  unsigned long long *slot;
  uint64_t n_values;
  uint64_t *v_off, *v_count, *v_first, *v_line, *v_hash;
  uint32_t *v_len, *v_pattern;
  uint64_t parts_before, arena_tail;  // (arena_tail: a multiple of 16, where this call's new bytes begin)
  // lookup
  uint64_t *match;                 // n_groups
  uint64_t *long_list;             // the groups longer than HG_VALUES_LANE_MAX, in any order
  unsigned long long *counters;    // HG_VALSTORE_N_LONG, HG_VALSTORE_OVERFLOW
  // size
  uint64_t *new_flag, *new_len;    // n_groups + 1 (the last 0)
  const uint64_t *new_idx, *new_off;  // their exclusive scans
  // apply
  uint64_t max_values;             // n_values + the new ones: what the per-value arrays and the table were sized for
  HgGatherEntry *entries;          // per new value, what the copy pass reads: {src, line, len, form 0}
  uint64_t *ent_off;               // per new value its offset behind arena_tail, and the total behind the last
  // rehash: the table that is built
  unsigned long long *slot_new;
  uint32_t new_log2;
};

// What a ranking works on.
struct HgValRankArgs {
  uint64_t n_values, n_rows;  // n_rows = min(top, n_values)
  const uint64_t *order;      // store indices by (count descending, index ascending); nullptr: the identity (HG_ACC_ORDER_FIRST)
  const uint64_t *v_off, *v_count, *v_first, *v_line;
  const uint32_t *v_len, *v_pattern;
  uint64_t *out_count, *out_first, *out_line;
  uint32_t *out_pattern;
  uint64_t *size;          // n_rows + 1 (the last 0)
  HgGatherEntry *entries;  // {arena offset, line, len, form 0}
};

// Are ta[sa, sa + n) and tb[sb, sb + n) the same bytes?  By one lane, and lane l's share for a wave (all shares true).
template <typename TextA, typename TextB>
HG_HD bool hg_valstore_equal(const TextA &ta, uint64_t sa, const TextB &tb, uint64_t sb, uint32_t n) {
  const uint32_t full = n / 4;
  for (uint32_t i = 0; i < full; i++)
    if (hg_values_word(ta, sa + 4 * static_cast<uint64_t>(i)) != hg_values_word(tb, sb + 4 * static_cast<uint64_t>(i))) return false;
  for (uint32_t k = 4 * full; k < n; k++)
    if (ta.byte(sa + k) != tb.byte(sb + k)) return false;
  return true;
}
template <typename TextA, typename TextB>
HG_HD bool hg_valstore_equal_wave_lane(const TextA &ta, uint64_t sa, const TextB &tb, uint64_t sb, uint32_t n, uint32_t lane) {
  const uint32_t full = n / 4;
  for (uint32_t i = lane; i < full; i += HG_VALUES_WAVE)
    if (hg_values_word(ta, sa + 4 * static_cast<uint64_t>(i)) != hg_values_word(tb, sb + 4 * static_cast<uint64_t>(i))) return false;
  const uint32_t k = 4 * full + lane;  // (the at most three bytes behind the dwords: lanes 0 .. 2)
  return k >= n || ta.byte(sa + k) == tb.byte(sb + k);
}

// Can the occupied slot word w be the stored value of a group with hash h, length len and expression pat, by everything but
// the bytes?  *idx: the store index.
HG_HD bool hg_valstore_candidate(const HgValStoreArgs &a, uint64_t w, uint64_t h, uint32_t len, uint32_t pat, uint64_t *idx) {
  *idx = w & HG_VALUES_REP_MASK;
  if ((w >> HG_VALUES_REP_BITS) != hg_values_tag(h) || *idx >= a.n_values) return false;
  if (a.v_len[*idx] != len) return false;
  return !(a.flags & HG_VALSTORE_F_BY_PATTERN) || a.v_pattern[*idx] == pat;
}

// The lookup of group j < n_groups by a lane: the store index of its value or HG_VALSTORE_NONE; *overflow is set by a probe that
// went round the whole table.  Table: load(slot).
template <typename TextA, typename TextB, typename Table>
HG_HD uint64_t hg_valstore_lookup(const HgValStoreArgs &a, const TextA &text, const TextB &arena, const Table &t, uint64_t j, bool *overflow) {
  const uint64_t f = a.g_first[j];
  if (f >= a.n_parts || !a.n_values) return HG_VALSTORE_NONE;
  const uint64_t h = a.hash[f], cap = uint64_t{1} << a.store_log2, src = a.src[f];
  const uint32_t len = a.len[f], pat = a.part_pattern[f];
  uint64_t s = hg_values_home(h, a.store_log2);
  for (uint64_t probe = 0; probe < cap; probe++, s = (s + 1) & (cap - 1)) {
    const uint64_t w = t.load(s);
    if (w == HG_VALUES_EMPTY) return HG_VALSTORE_NONE;
    uint64_t idx;
    if (hg_valstore_candidate(a, w, h, len, pat, &idx) && hg_valstore_equal(text, src, arena, a.v_off[idx], len)) return idx;
  }
  *overflow = true;
  return HG_VALSTORE_NONE;
}

// The size pass for group j <= n_groups.
HG_HD void hg_valstore_size(const HgValStoreArgs &a, uint64_t j) {
  const uint64_t f = j < a.n_groups ? a.g_first[j] : a.n_parts;
  const bool is_new = f < a.n_parts && a.match[j] == HG_VALSTORE_NONE;
  a.new_flag[j] = is_new;
  a.new_len[j] = is_new ? a.len[f] : 0;
}

// The claim of the first empty slot from hash h's home for store index idx, in a table of 2^log2 slots; false after a whole
// round.  Table: load(slot) and claim(slot, word), which returns what the slot held.
template <typename Table>
HG_HD bool hg_valstore_claim(const Table &t, uint32_t log2, uint64_t h, uint64_t idx) {
  const uint64_t cap = uint64_t{1} << log2, mine = hg_values_slot_word(h, idx);
  uint64_t s = hg_values_home(h, log2);
  for (uint64_t probe = 0; probe < cap; probe++, s = (s + 1) & (cap - 1))
    if (t.load(s) == HG_VALUES_EMPTY && t.claim(s, mine) == HG_VALUES_EMPTY) return true;
  return false;
}

// The rehash pass for stored value i < n_values (t: the table that is built, 2^new_log2 slots).
template <typename Table>
HG_HD bool hg_valstore_rehash(const HgValStoreArgs &a, const Table &t, uint64_t i) { return hg_valstore_claim(t, a.new_log2, a.v_hash[i], i); }

// The apply pass for group j <= n_groups (t: the store's table, 2^store_log2 slots, sized for max_values); false if a claim
// went round the table.
template <typename Table>
HG_HD bool hg_valstore_apply(const HgValStoreArgs &a, const Table &t, uint64_t j) {
  if (j >= a.n_groups) {
    if (a.new_idx[j] <= a.max_values - a.n_values) a.ent_off[a.new_idx[j]] = a.new_off[j];  // (the totals: the copy pass reads the offset behind the last entry)
    return true;
  }
  const uint64_t f = a.g_first[j], m = a.match[j];
  if (f >= a.n_parts) return true;
  if (m != HG_VALSTORE_NONE) {
    if (m < a.n_values) a.v_count[m] += a.g_count[j];
    return true;
  }
  const uint64_t k = a.new_idx[j], idx = a.n_values + k;
  if (idx >= a.max_values) return true;
  const HgPart p = a.parts[f];
  const uint64_t h = a.hash[f];
  a.v_off[idx] = a.arena_tail + a.new_off[j];
  a.v_len[idx] = a.len[f];
  a.v_pattern[idx] = a.part_pattern[f];
  a.v_hash[idx] = h;
  a.v_count[idx] = a.g_count[j];
  a.v_first[idx] = a.parts_before + f;
  a.v_line[idx] = p.line_no;
  a.entries[k] = HgGatherEntry{a.src[f], p.line_no, a.len[f], 0u};
  a.ent_off[k] = a.new_off[j];
  return hg_valstore_claim(t, a.store_log2, h, idx);
}

// The place pass for place r <= n_rows.
HG_HD void hg_valstore_place(const HgValRankArgs &a, uint64_t r) {
  if (r >= a.n_rows) {
    a.size[r] = 0;
    return;
  }
  const uint64_t i = a.order ? a.order[r] : r;
  if (i >= a.n_values) {  // (an order entry is a store index: nothing comes here)
    a.size[r] = 0;
    a.entries[r] = HgGatherEntry{0, 0, 0u, 0u};
    a.out_count[r] = a.out_first[r] = a.out_line[r] = 0;
    a.out_pattern[r] = 0;
    return;
  }
  a.out_count[r] = a.v_count[i];
  a.out_first[r] = a.v_first[i];
  a.out_line[r] = a.v_line[i];
  a.out_pattern[r] = a.v_pattern[i];
  a.size[r] = a.v_len[i];
  a.entries[r] = HgGatherEntry{a.v_off[i], a.v_line[i], a.v_len[i], 0u};
}

// store_log2 when the caller leaves it open: the smallest power of two at least twice the distinct values and at least 2^10.
inline uint32_t hg_valstore_default_log2(uint64_t n_values) { return hg_values_default_log2(n_values); }
