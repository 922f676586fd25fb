// Distinct matched parts and how often each occurs (hg_count_values; grep -o | sort | uniq -c): the parts of the last scan with
// parts, grouped by their bytes on the GPU, so that only the distinct values leave it.  The scalar rules here are shared by the
// kernels (hg_values.hip) and the host replay of the tests (tests/native/valuesim.cpp compiles this header for x86); the product
// only calls them from device code.  hg_gather.h lends its searches, its funnel shift and its copy pass unchanged.
//
//  - VALUE.  Part q belongs to the piece (segment, line_no); its record is found as the parts gather finds it
//    (hg_gather_lower_bound over the final records, hg_gather_seg; hg_partlines.h, PIECE), S = seg_start[segment] + aux.start, and the
//    value is text[S + from, S + to).  A part whose piece has no record has no value (len 0: a part is never empty) and is not
//    counted.  hg_values_locate is the one place that decides this.
//  - KEY.  The value's bytes; with HG_VALUES_F_BY_PATTERN the pair (part_pattern[q], bytes).  hg_count_values never has the
//    segment in the key.  The rank stage (hg_rank.h) has it with HG_VALUES_F_BY_SEGMENT, a flag no public call of this stage
//    passes on: its own instantiations of the hash, long and insert pass (the SEG template argument, false by default) keep a
//    key word per part, hg_values_key_word = (segment + 1) << 32 | expression step, hash it with one more Horner step
//    (segment + 1) behind the expression's and compare it in hg_values_candidate in place of the expression.  The
//    instantiations without it use the registers they used before the bodies became templates (the same SGPRs, VGPRs and
//    occupancy; the instruction streams differ a little) and were measured against the earlier library.
//  - HASH.  64 bits, a Horner form in 64-bit arithmetic: h = SEED, then h = h * P + v for v = len, then the expression index + 1
//    (0 when not keyed by it), then byte + 1 for every byte, a final mix (hg_values_finish) and the cut to the low hash_bits
//    bits.  hg_values_hash_bytes is that definition, a byte at a time; hg_values_hash_dwords reads whole aligned dwords and
//    funnel-shifts them (the lanes' path); hg_values_hash_wave_lane is lane l's share of a wave's rounds of 256 bytes, 64
//    dwords a round, which sum to the same Horner value (P^256 per round, P^(4 * (63 - l)) per lane).  All three agree.
//  - TABLE.  2^table_log2 slots of one 64-bit word: EMPTY (all ones) or (tag = hash bits 40..63, representative part index in
//    40 bits).  A part starts at slot hash mod 2^table_log2 and probes linearly, at most the capacity: an empty slot is claimed
//    with one compare-and-swap; an occupied one is its group iff tag, length, (expression) and bytes equal the
//    representative's.  Whoever wins the swap is the representative; count[slot] and first[slot] (the smallest part index) are
//    what is reported, so the result does not depend on who won.  Nothing waits: the slot word, the per-part arrays of the hash
//    pass and the text are all a comparison reads.
//  - ORDER.  The occupied slots are marked, scanned and compacted to (first, count) pairs, the pairs sorted by first; group j
//    takes pattern, line_number, segment and length from part first[j]; off = exclusive scan of the lengths; the bytes are
//    copied by the line gather's copy pass (an entry with nothing but a body).
// Text reads never leave [0, nbytes rounded up to 4): bytes of a value, or the aligned dwords that hold some.
#pragma once
#include "hg_gather.h"
#include "hg_partlines.h"
#include "hg_parts.h"

constexpr uint32_t HG_VALUES_F_BY_PATTERN = 1u;  // HG_VALUES_BY_PATTERN of the C ABI
constexpr uint32_t HG_VALUES_F_BY_SEGMENT = 2u;  // internal (hg_rank_values with HG_RANK_PER_SEGMENT): hg_count_values refuses the bit
#ifndef HG_VALUES_LANE_MAX
#define HG_VALUES_LANE_MAX 256u  // a part of at most this many bytes is hashed and compared by one lane, a longer one by a wavefront
#endif
constexpr uint32_t HG_VALUES_THREADS = 256, HG_VALUES_WAVE = 64, HG_VALUES_ROUND = 4 * HG_VALUES_WAVE;  // a wave's round: a dword a lane
constexpr uint32_t HG_VALUES_LONG_BLOCKS = 1024;  // the long kernel's grid at most: its waves stride over the list
constexpr uint32_t HG_VALUES_REP_BITS = 40, HG_VALUES_MAX_TABLE_LOG2 = 40, HG_VALUES_MIN_TABLE_LOG2 = 10;
constexpr uint64_t HG_VALUES_EMPTY = ~uint64_t{0}, HG_VALUES_REP_MASK = (uint64_t{1} << HG_VALUES_REP_BITS) - 1, HG_VALUES_NO_SLOT = ~uint64_t{0};
constexpr uint64_t HG_VALUES_SEED = 0xCBF29CE484222325ull, HG_VALUES_P = 0x9E3779B97F4A7C15ull;  // (P odd)
constexpr uint32_t HG_VALUES_N_LONG = 0, HG_VALUES_OVERFLOW = 1, HG_VALUES_N_VALUES = 2, HG_VALUES_COUNTERS = 4;  // HgValuesArgs::counters

constexpr uint64_t hg_values_cpow(uint64_t b, uint32_t e) { return e == 0 ? 1 : (e & 1 ? b : 1) * hg_values_cpow(b * b, e >> 1); }
constexpr uint64_t HG_VALUES_P_ROUND = hg_values_cpow(HG_VALUES_P, HG_VALUES_ROUND);

// What the kernels work on (hg_values_launch, hg_engine.h).
struct HgValuesArgs {
  HgGatherText text;
  HgGatherList recs;             // the last scan's final records (seg_of == nullptr: no segments)
  const HgPart *parts;           // the last scan's parts, their expressions and (after segments) their segments
  const uint32_t *part_pattern, *part_seg;
  uint64_t n_parts;
  const uint64_t *seg_start;     // the last scan's device array, nullptr without segments
  uint32_t flags;                // HG_VALUES_F_*
  uint32_t hash_bits;            // 1 .. 64
  uint32_t table_log2;           // 2^table_log2 > n_parts
  // hash pass: per part the value's first byte in the text, its length (0: not counted) and its hash
  uint64_t *src;
  uint32_t *len;
  uint64_t *hash;
  uint64_t *long_list;                // the parts longer than HG_VALUES_LANE_MAX, in any order
  unsigned long long *counters;       // HG_VALUES_N_LONG, HG_VALUES_OVERFLOW, HG_VALUES_N_VALUES
  // insert pass: the table
  unsigned long long *slot, *count, *first;
  uint64_t *pos;                      // mark pass: 1 per occupied slot; then its exclusive scan
  uint64_t *pair_first, *pair_count;  // compact pass
  // derive pass, over the pairs sorted by first
  const uint64_t *v_first;
  uint64_t n_values;
  uint64_t *size;                     // n_values + 1 (the last 0)
  HgGatherEntry *entries;             // what the copy pass reads: {src, line, len, form 0}
  uint32_t *pattern, *segment;        // (segment nullptr without segments)
  uint64_t *line_number;
  // the SEG instantiations only (nullptr otherwise): per part its key word, written by their hash pass
  uint64_t *key;
};

HG_HD uint64_t hg_values_step(uint64_t h, uint64_t v) { return h * HG_VALUES_P + v; }
HG_HD uint64_t hg_values_init(uint32_t len, uint32_t flags, uint32_t pattern) {
  return hg_values_step(hg_values_step(HG_VALUES_SEED, len), (flags & HG_VALUES_F_BY_PATTERN) ? static_cast<uint64_t>(pattern) + 1 : 0);
}
// The key word of a part in the SEG instantiations and the Horner value its hash starts from.
HG_HD uint64_t hg_values_key_word(uint32_t flags, uint32_t pattern, uint32_t segment) {
  return ((static_cast<uint64_t>(segment) + 1) << 32) | ((flags & HG_VALUES_F_BY_PATTERN) ? pattern + 1u : 0u);
}
HG_HD uint64_t hg_values_init_key(uint32_t len, uint64_t key) {
  return hg_values_step(hg_values_step(hg_values_step(HG_VALUES_SEED, len), key & 0xFFFFFFFFull), key >> 32);
}
HG_HD uint64_t hg_values_step_dword(uint64_t h, uint32_t w) {  // four byte steps
  h = hg_values_step(h, (w & 0xFFu) + 1);
  h = hg_values_step(h, ((w >> 8) & 0xFFu) + 1);
  h = hg_values_step(h, ((w >> 16) & 0xFFu) + 1);
  return hg_values_step(h, (w >> 24) + 1);
}
HG_HD uint64_t hg_values_finish(uint64_t h, uint32_t hash_bits) {
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return hash_bits >= 64 ? h : h & ((uint64_t{1} << hash_bits) - 1);
}
HG_HD uint64_t hg_values_pow(uint64_t b, uint32_t e) {
  uint64_t r = 1;
  for (; e; e >>= 1, b *= b)
    if (e & 1) r *= b;
  return r;
}

// The four bytes text[at, at + 4), all of them inside a value that ends at or before nbytes: one aligned dword, or two.
template <typename Text>
HG_HD uint32_t hg_values_word(const Text &text, uint64_t at) {
  const uint64_t base = at & ~static_cast<uint64_t>(3);
  const uint32_t shift = static_cast<uint32_t>(at & 3), lo = text.dword(base);
  return shift ? hg_gather_funnel(lo, text.dword(base + 4), shift) : lo;  // (base + 4 < at + 4: it holds a byte of the value)
}

// The Horner steps over text[s, s + n) from h on: the definition, and the same by dwords.
template <typename Text>
HG_HD uint64_t hg_values_run_bytes(const Text &text, uint64_t h, uint64_t s, uint64_t n) {
  for (uint64_t k = 0; k < n; k++) h = hg_values_step(h, static_cast<uint64_t>(text.byte(s + k)) + 1);
  return h;
}
template <typename Text>
HG_HD uint64_t hg_values_run_dwords(const Text &text, uint64_t h, uint64_t s, uint64_t n) {
  const uint64_t base = s & ~static_cast<uint64_t>(3), full = n / 4;
  const uint32_t shift = static_cast<uint32_t>(s & 3);
  uint32_t lo = full ? text.dword(base) : 0u;
  for (uint64_t i = 0; i < full; i++) {
    uint32_t w = lo;
    if (shift) {  // the next dword holds the word's last bytes
      const uint32_t hi = text.dword(base + 4 * (i + 1));
      w = hg_gather_funnel(lo, hi, shift);
      lo = hi;
    } else if (i + 1 < full) {
      lo = text.dword(base + 4 * (i + 1));
    }
    h = hg_values_step_dword(h, w);
  }
  return hg_values_run_bytes(text, h, s + 4 * full, n - 4 * full);
}
template <typename Text>
HG_HD uint64_t hg_values_hash_bytes_from(const Text &text, uint64_t h0, uint64_t s, uint32_t len, uint32_t hash_bits) {  // (h0: hg_values_init or hg_values_init_key)
  return hg_values_finish(hg_values_run_bytes(text, h0, s, len), hash_bits);
}
template <typename Text>
HG_HD uint64_t hg_values_hash_dwords_from(const Text &text, uint64_t h0, uint64_t s, uint32_t len, uint32_t hash_bits) {
  return hg_values_finish(hg_values_run_dwords(text, h0, s, len), hash_bits);
}
template <typename Text>
HG_HD uint64_t hg_values_hash_bytes(const Text &text, uint64_t s, uint32_t len, uint32_t flags, uint32_t pattern, uint32_t hash_bits) {
  return hg_values_hash_bytes_from(text, hg_values_init(len, flags, pattern), s, len, hash_bits);
}
template <typename Text>
HG_HD uint64_t hg_values_hash_dwords(const Text &text, uint64_t s, uint32_t len, uint32_t flags, uint32_t pattern, uint32_t hash_bits) {
  return hg_values_hash_dwords_from(text, hg_values_init(len, flags, pattern), s, len, hash_bits);
}
// Lane l's share of the whole rounds of a long value: the sum over the 64 lanes is the Horner value after len / 256 * 256 bytes.
// hg_values_hash_wave_end turns that sum into the hash (the bytes behind the whole rounds, the mix and the cut).
template <typename Text>
HG_HD uint64_t hg_values_hash_wave_lane_from(const Text &text, uint64_t h0, uint64_t s, uint32_t len, uint32_t lane) {
  uint64_t acc = lane == HG_VALUES_WAVE - 1 ? h0 : 0;
  const uint32_t rounds = len / HG_VALUES_ROUND;
  for (uint32_t r = 0; r < rounds; r++)
    acc = acc * HG_VALUES_P_ROUND + hg_values_step_dword(0, hg_values_word(text, s + static_cast<uint64_t>(r) * HG_VALUES_ROUND + 4 * lane));
  return acc * hg_values_pow(HG_VALUES_P, 4 * (HG_VALUES_WAVE - 1 - lane));
}
template <typename Text>
HG_HD uint64_t hg_values_hash_wave_lane(const Text &text, uint64_t s, uint32_t len, uint32_t flags, uint32_t pattern, uint32_t lane) {
  return hg_values_hash_wave_lane_from(text, hg_values_init(len, flags, pattern), s, len, lane);
}
template <typename Text>
HG_HD uint64_t hg_values_hash_wave_end(const Text &text, uint64_t sum, uint64_t s, uint32_t len, uint32_t hash_bits) {
  const uint32_t done = len / HG_VALUES_ROUND * HG_VALUES_ROUND;
  return hg_values_finish(hg_values_run_dwords(text, sum, s + done, len - done), hash_bits);
}

// Are text[sa, sa + n) and text[sb, sb + n) the same bytes?  By one lane, and lane l's share for a wave (all shares true).
template <typename Text>
HG_HD bool hg_values_equal(const Text &text, uint64_t sa, uint64_t sb, uint32_t n) {
  if (sa == sb) return true;
  const uint32_t full = n / 4;
  for (uint32_t i = 0; i < full; i++)
    if (hg_values_word(text, sa + 4 * static_cast<uint64_t>(i)) != hg_values_word(text, sb + 4 * static_cast<uint64_t>(i))) return false;
  for (uint32_t k = 4 * full; k < n; k++)
    if (text.byte(sa + k) != text.byte(sb + k)) return false;
  return true;
}
template <typename Text>
HG_HD bool hg_values_equal_wave_lane(const Text &text, uint64_t sa, uint64_t sb, uint32_t n, uint32_t lane) {
  if (sa == sb) return true;
  const uint32_t full = n / 4;
  for (uint32_t i = lane; i < full; i += HG_VALUES_WAVE)
    if (hg_values_word(text, sa + 4 * static_cast<uint64_t>(i)) != hg_values_word(text, sb + 4 * static_cast<uint64_t>(i))) return false;
  const uint32_t k = 4 * full + lane;  // (the at most three bytes behind the dwords: lanes 0 .. 2)
  return k >= n || text.byte(sa + k) == text.byte(sb + k);
}

// Where part q's value lies: *src and its length, 0 if its piece has no record.
HG_HD uint32_t hg_values_locate(const HgValuesArgs &a, uint64_t q, uint64_t *src) {
  const HgPart p = a.parts[q];
  const uint32_t seg = a.part_seg ? a.part_seg[q] : 0u;
  const uint64_t r = hg_gather_lower_bound(a.recs, seg, p.line_no);
  *src = 0;
  if (r >= a.recs.n || a.recs.hits[r].line_no != p.line_no || hg_gather_seg(a.recs, r) != seg || p.to <= p.from) return 0;
  *src = (a.seg_start ? a.seg_start[seg] : 0) + a.recs.aux[r].start + p.from;
  return p.to - p.from;
}
HG_HD bool hg_values_is_long(uint32_t len) { return len > HG_VALUES_LANE_MAX; }

// The slot word and its fields.
HG_HD uint64_t hg_values_tag(uint64_t h) { return h >> HG_VALUES_REP_BITS; }
HG_HD uint64_t hg_values_slot_word(uint64_t h, uint64_t q) { return (hg_values_tag(h) << HG_VALUES_REP_BITS) | q; }
HG_HD uint64_t hg_values_home(uint64_t h, uint32_t table_log2) { return h & ((uint64_t{1} << table_log2) - 1); }
// Can the occupied slot word w be the group of part q (hash h), by everything but the bytes?  *rep: its representative.
template <bool SEG = false>
HG_HD bool hg_values_candidate(const HgValuesArgs &a, uint64_t w, uint64_t q, uint64_t h, uint64_t *rep) {
  *rep = w & HG_VALUES_REP_MASK;
  if ((w >> HG_VALUES_REP_BITS) != hg_values_tag(h) || *rep >= a.n_parts) return false;
  if (a.len[*rep] != a.len[q]) return false;
  if (SEG) return a.key[*rep] == a.key[q];
  return !(a.flags & HG_VALUES_F_BY_PATTERN) || a.part_pattern[*rep] == a.part_pattern[q];
}

// The probe of part q (a lane's): the slot of its group, claimed if it is new, or HG_VALUES_NO_SLOT after a whole round of the
// table.  Table: load(slot) and claim(slot, word), which returns what the slot held (HG_VALUES_EMPTY: the claim holds).
template <bool SEG = false, typename Text, typename Table>
HG_HD uint64_t hg_values_insert(const HgValuesArgs &a, const Text &text, const Table &t, uint64_t q) {
  const uint64_t h = a.hash[q], cap = uint64_t{1} << a.table_log2, mine = hg_values_slot_word(h, q);
  uint64_t s = hg_values_home(h, a.table_log2);
  for (uint64_t probe = 0; probe < cap; probe++, s = (s + 1) & (cap - 1)) {
    uint64_t w = t.load(s);
    if (w == HG_VALUES_EMPTY) {
      w = t.claim(s, mine);
      if (w == HG_VALUES_EMPTY) return s;
    }
    uint64_t rep;
    if (hg_values_candidate<SEG>(a, w, q, h, &rep) && hg_values_equal(text, a.src[rep], a.src[q], a.len[q])) return s;
  }
  return HG_VALUES_NO_SLOT;
}

// The derive pass for group j <= n_values of the sorted pairs.
HG_HD void hg_values_derive(const HgValuesArgs &a, uint64_t j) {
  if (j >= a.n_values) {
    a.size[j] = 0;
    return;
  }
  const uint64_t f = a.v_first[j];
  const HgPart p = a.parts[f];
  a.size[j] = a.len[f];
  a.entries[j] = HgGatherEntry{a.src[f], p.line_no, a.len[f], 0u};
  a.pattern[j] = a.part_pattern[f];
  a.line_number[j] = p.line_no;
  if (a.segment) a.segment[j] = a.part_seg ? a.part_seg[f] : 0u;
}

// table_log2 when the caller leaves it open: the smallest power of two at least 2 * n_parts and at least 2^10.
inline uint32_t hg_values_default_log2(uint64_t n_parts) {
  uint32_t k = HG_VALUES_MIN_TABLE_LOG2;
  while (k < 63 && (uint64_t{1} << k) < 2 * n_parts) k++;
  return k;
}
