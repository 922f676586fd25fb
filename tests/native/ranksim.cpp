// TEST-ONLY host harness for the rank stage (never shipped): compiles the scalar rules of hypergrep_amd/csrc/hg_values.h and
// hg_rank.h for x86 and replays the stage's passes one after the other: the values stage's hash pass (with the segment in the
// key: the key word per part and the hash that starts from it, the lane's dword path for short parts, the 64 lane shares of a
// wave for long ones, both checked against the byte-wise definition), its insert pass over a plain table (the parts in their
// own order or, with a seed, in a shuffled one), mark, scan, compact and the sort by first; then the stable sort by descending
// count, the keys pass, the stable sort by segment, the counts pass and its scan, the bounds pass, the scan of the kept rows, the
// place pass, the scan of the lengths and the gathers' copy pass over spans of `tile` bytes.  What the GPU stage (hg_rank.hip,
// HgRank::run) must reproduce; only its launch geometry and its atomics are left to the GPU tests.
// The text is read through a checked view: every byte and dword read must lie inside [0, nbytes rounded up to 4), and `base`
// (a multiple of 4) is added to every start by the caller and subtracted on access.
// With -DRANKSIM_MAIN the file is a program of its own (a sanitized run).
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_rank.h"
#include "../../include/hypergrep_amd.h"

namespace {

struct CheckedText {
  const uint8_t *p;  // a heap block of exactly `readable` bytes
  uint64_t base, readable;
  bool *bad;
  uint8_t byte(uint64_t o) const {
    if (o < base || o - base >= readable) {
      *bad = true;
      return 0;
    }
    return p[o - base];
  }
  uint32_t dword(uint64_t o) const {
    if ((o & 3) || o < base || o - base + 4 > readable) {
      *bad = true;
      return 0;
    }
    uint32_t v;
    memcpy(&v, p + (o - base), 4);
    return v;
  }
};

struct HostTable {
  unsigned long long *slot;
  uint64_t *probes;  // read-out: slots loaded so far
  uint64_t load(uint64_t i) const {
    ++*probes;
    return slot[i];
  }
  uint64_t claim(uint64_t i, uint64_t word) const {
    const uint64_t old = slot[i];
    if (old == HG_VALUES_EMPTY) slot[i] = word;
    return old;
  }
};

// the three hashes of part q, from h0 on; false if they differ
bool hashes(const CheckedText &view, uint64_t h0, uint64_t s, uint32_t len, uint32_t hash_bits, uint64_t *h) {
  const uint64_t want = hg_values_hash_bytes_from(view, h0, s, len, hash_bits);
  if (hg_values_is_long(len)) {
    uint64_t sum = 0;
    for (uint32_t lane = 0; lane < HG_VALUES_WAVE; lane++) sum += hg_values_hash_wave_lane_from(view, h0, s, len, lane);
    *h = hg_values_hash_wave_end(view, sum, s, len, hash_bits);
  } else {
    *h = hg_values_hash_dwords_from(view, h0, s, len, hash_bits);
  }
  return *h == want;
}

// the wave's probe of a long part (long_body of hg_values_dev.h): lane 0's table accesses, all lanes' shares of the comparison
template <bool SEG>
uint64_t wave_insert(const HgValuesArgs &a, const CheckedText &view, const HostTable &t, uint64_t q) {
  const uint64_t h = a.hash[q], cap = uint64_t{1} << a.table_log2, mine = hg_values_slot_word(h, q);
  uint64_t s = hg_values_home(h, a.table_log2);
  for (uint64_t probe = 0; probe < cap; probe++, s = (s + 1) & (cap - 1)) {
    uint64_t w = t.load(s);
    if (w == HG_VALUES_EMPTY) {
      const uint64_t old = t.claim(s, mine);
      w = old == HG_VALUES_EMPTY ? mine : old;
    }
    if (w == mine) return s;
    uint64_t rep;
    if (!hg_values_candidate<SEG>(a, w, q, h, &rep)) continue;
    bool all = true;
    for (uint32_t lane = 0; lane < HG_VALUES_WAVE; lane++) all = hg_values_equal_wave_lane(view, a.src[rep], a.src[q], a.len[q], lane) && all;
    if (all) return s;
  }
  return HG_VALUES_NO_SLOT;
}

template <bool SEG>
uint64_t insert_one(const HgValuesArgs &a, const CheckedText &view, const HostTable &t, uint64_t q) {
  return hg_values_is_long(a.len[q]) ? wave_insert<SEG>(a, view, t, q) : hg_values_insert<SEG>(a, view, t, q);
}

// Read-outs of one run (ranksim_trace): what a cell of tests/value_cells.py claims to reach is proved from these.
struct Trace {
  uint64_t *part;   // RANKSIM_PART_COLS per part: tier (0 none, 1 lane, 2 wave), home, final slot, slots probed, wrapped past the last
                    // slot, claimed (1) or joined (0), the key word (0 without HG_RANK_PER_SEGMENT)
  uint64_t *seg;    // RANKSIM_SEG_COLS per segment (one without HG_RANK_PER_SEGMENT): first_group, seg_distinct, seg_parts, kept
  uint64_t *group;  // per group of the final order: placed (1) or cut (0)
  uint64_t *call;   // RANKSIM_CALL_COLS: groups, the count sort's key width, the segment sort's, slots of the table
};
constexpr uint32_t RANKSIM_PART_COLS = 7, RANKSIM_SEG_COLS = 4, RANKSIM_CALL_COLS = 4;

long run_all(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
             const uint64_t *seg_start, uint32_t n_seg_in, uint32_t flags, uint64_t top, uint32_t hash_bits, uint32_t table_log2, uint64_t order_seed, uint64_t tile,
             uint8_t *out_bytes, uint64_t cap_bytes, uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint32_t *segment,
             uint64_t *first_value, uint64_t *seg_distinct, uint64_t *seg_parts, uint64_t *totals, const Trace *tr);

}  // namespace

extern "C" {

// recs: {line, start, len, segment} per final record, in order; parts: {line, from, to, pattern, segment} per part, in order
// (uint64 each).  Every start (seg_start with segments) already has `base` added.  seg_start: n_seg values or NULL.  flags:
// HG_RANK_*.  order_seed: 0 inserts the parts in their own order, anything else in a shuffled one.  out_bytes: room for
// cap_bytes; off: n_parts + 1; count, first, pattern, line_number, segment: n_parts each; first_value: n_seg + 1, seg_distinct
// and seg_parts: n_seg (written with HG_RANK_PER_SEGMENT only).  totals: {n_values, n_bytes, n_distinct, long parts}.
// Returns 0, -1 if an output is too small or an argument is refused, -2 if a read left the readable range, -3 if two paths that
// must agree do not (the three hashes; the lanes' chunks and the values' bytes), -4 if a probe went round the table, -5 if a
// pass left a row unwritten or wrote one twice.
long ranksim_run(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
                 const uint64_t *seg_start, uint32_t n_seg_in, uint32_t flags, uint64_t top, uint32_t hash_bits, uint32_t table_log2, uint64_t order_seed, uint64_t tile,
                 uint8_t *out_bytes, uint64_t cap_bytes, uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint32_t *segment,
                 uint64_t *first_value, uint64_t *seg_distinct, uint64_t *seg_parts, uint64_t *totals) {
  return run_all(text, nbytes, base, recs, n_recs, parts, n_parts, segments, seg_start, n_seg_in, flags, top, hash_bits, table_log2, order_seed, tile, out_bytes, cap_bytes, off, count,
                 first, pattern, line_number, segment, first_value, seg_distinct, seg_parts, totals, nullptr);
}

// The same run with its read-outs (Trace above): part RANKSIM_PART_COLS * n_parts, seg RANKSIM_SEG_COLS * max(n_seg, 1), group
// n_parts, call RANKSIM_CALL_COLS values.  Home, tier, key and everything per segment and per group do not depend on the
// insertion order; final slot, probes, wrapped and claimed are those of the order the seed gives.
long ranksim_trace(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
                   const uint64_t *seg_start, uint32_t n_seg_in, uint32_t flags, uint64_t top, uint32_t hash_bits, uint32_t table_log2, uint64_t order_seed, uint64_t tile,
                   uint8_t *out_bytes, uint64_t cap_bytes, uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint32_t *segment,
                   uint64_t *first_value, uint64_t *seg_distinct, uint64_t *seg_parts, uint64_t *totals, uint64_t *tr_part, uint64_t *tr_seg, uint64_t *tr_group, uint64_t *tr_call) {
  const Trace tr{tr_part, tr_seg, tr_group, tr_call};
  return run_all(text, nbytes, base, recs, n_recs, parts, n_parts, segments, seg_start, n_seg_in, flags, top, hash_bits, table_log2, order_seed, tile, out_bytes, cap_bytes, off, count,
                 first, pattern, line_number, segment, first_value, seg_distinct, seg_parts, totals, &tr);
}

}  // extern "C"

namespace {

long run_all(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
             const uint64_t *seg_start, uint32_t n_seg_in, uint32_t flags, uint64_t top, uint32_t hash_bits, uint32_t table_log2, uint64_t order_seed, uint64_t tile,
             uint8_t *out_bytes, uint64_t cap_bytes, uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint32_t *segment,
             uint64_t *first_value, uint64_t *seg_distinct, uint64_t *seg_parts, uint64_t *totals, const Trace *tr) {
  if (!hash_bits) hash_bits = 64;
  if (!table_log2) table_log2 = hg_values_default_log2(n_parts);
  const bool per_seg = (flags & HG_RANK_F_PER_SEGMENT) != 0;
  if (table_log2 > 30 || (uint64_t{1} << table_log2) <= n_parts || (flags & ~(HG_RANK_F_BY_PATTERN | HG_RANK_F_PER_SEGMENT)) || (per_seg && !segments)) return -1;
  const uint64_t readable = (nbytes + 3) & ~uint64_t{3}, cap = uint64_t{1} << table_log2;
  uint8_t *block = static_cast<uint8_t *>(calloc(readable ? readable : 1, 1));  // (exactly the readable bytes: a read past them is the sanitizer's to catch, too)
  if (nbytes) memcpy(block, text, nbytes);
  bool bad = false;
  const CheckedText view{block, base, readable, &bad};
  std::vector<HgHit> hits(n_recs + 1);
  std::vector<HgHitAux> aux(n_recs + 1);
  std::vector<uint32_t> seg_of(n_recs + 1), part_seg(n_parts + 1), part_pattern(n_parts + 1);
  std::vector<HgPart> rows(n_parts + 1);
  for (uint64_t i = 0; i < n_recs; i++) {
    hits[i] = HgHit{recs[4 * i], 1, 0};
    aux[i] = HgHitAux{recs[4 * i + 1], static_cast<uint32_t>(recs[4 * i + 2]), 0};
    seg_of[i] = static_cast<uint32_t>(recs[4 * i + 3]);
  }
  for (uint64_t q = 0; q < n_parts; q++) {
    rows[q] = HgPart{parts[5 * q], static_cast<uint32_t>(parts[5 * q + 1]), static_cast<uint32_t>(parts[5 * q + 2])};
    part_pattern[q] = static_cast<uint32_t>(parts[5 * q + 3]);
    part_seg[q] = static_cast<uint32_t>(parts[5 * q + 4]);
  }
  std::vector<uint64_t> src(n_parts + 1), hash(n_parts + 1), key(n_parts + 1), pair_first(n_parts + 1), pair_count(n_parts + 1);
  std::vector<uint32_t> len(n_parts + 1);
  std::vector<unsigned long long> slot(cap, HG_VALUES_EMPTY), slot_count(cap, 0), slot_first(cap, ~0ull);
  HgValuesArgs a{};
  a.recs = HgGatherList{hits.data(), aux.data(), segments ? seg_of.data() : nullptr, n_recs};
  a.parts = rows.data();
  a.part_pattern = part_pattern.data();
  a.part_seg = segments ? part_seg.data() : nullptr;
  a.n_parts = n_parts;
  a.seg_start = segments ? seg_start : nullptr;
  a.flags = flags;
  a.hash_bits = hash_bits;
  a.table_log2 = table_log2;
  a.src = src.data();
  a.len = len.data();
  a.hash = hash.data();
  a.slot = slot.data();
  a.count = slot_count.data();
  a.first = slot_first.data();
  a.pair_first = pair_first.data();
  a.pair_count = pair_count.data();
  a.key = per_seg ? key.data() : nullptr;
  long rc = 0;
  uint64_t n_long = 0;
  // hash pass (hash_body of hg_values_dev.h)
  for (uint64_t q = 0; q < n_parts; q++) {
    len[q] = hg_values_locate(a, q, &src[q]);
    hash[q] = 0;
    if (per_seg) key[q] = hg_values_key_word(flags, part_pattern[q], a.part_seg ? a.part_seg[q] : 0u);
    if (!len[q]) continue;
    n_long += hg_values_is_long(len[q]);
    const uint64_t h0 = per_seg ? hg_values_init_key(len[q], key[q]) : hg_values_init(len[q], flags, part_pattern[q]);
    if (!hashes(view, h0, src[q], len[q], hash_bits, &hash[q])) rc = -3;
  }
  // insert pass
  std::vector<uint64_t> order(n_parts);
  for (uint64_t q = 0; q < n_parts; q++) order[q] = q;
  uint64_t state = order_seed;
  for (uint64_t q = n_parts; order_seed && q > 1; q--) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(order[q - 1], order[(state >> 33) % q]);
  }
  uint64_t probes = 0;
  const HostTable t{slot.data(), &probes};
  if (tr) std::fill(tr->part, tr->part + RANKSIM_PART_COLS * n_parts, 0);
  for (uint64_t i = 0; i < n_parts && !rc; i++) {
    const uint64_t q = order[i];
    if (tr) tr->part[RANKSIM_PART_COLS * q + 6] = per_seg ? key[q] : 0;
    if (!len[q]) continue;
    const uint64_t before = probes;
    const uint64_t s = per_seg ? insert_one<true>(a, view, t, q) : insert_one<false>(a, view, t, q);
    if (s == HG_VALUES_NO_SLOT) {
      rc = -4;
      break;
    }
    slot_count[s]++;
    slot_first[s] = std::min<unsigned long long>(slot_first[s], q);
    if (tr) {
      uint64_t *row = tr->part + RANKSIM_PART_COLS * q;
      row[0] = hg_values_is_long(len[q]) ? 2 : 1;
      row[1] = hg_values_home(hash[q], table_log2);
      row[2] = s;
      row[3] = probes - before;
      row[4] = s < row[1];
      row[5] = (slot[s] & HG_VALUES_REP_MASK) == q;
    }
  }
  // mark, scan, compact, the sort by first
  uint64_t ng = 0;
  for (uint64_t i = 0; i < cap; i++)
    if (slot[i] != HG_VALUES_EMPTY) pair_first[ng] = slot_first[i], pair_count[ng] = slot_count[i], ng++;
  std::vector<std::pair<uint64_t, uint64_t>> pairs(ng);
  for (uint64_t j = 0; j < ng; j++) pairs[j] = {pair_first[j], pair_count[j]};
  std::sort(pairs.begin(), pairs.end());
  // the stable sort by descending count
  std::stable_sort(pairs.begin(), pairs.end(), [](const std::pair<uint64_t, uint64_t> &x, const std::pair<uint64_t, uint64_t> &y) { return x.second > y.second; });
  const uint32_t n_seg = per_seg ? n_seg_in : 1u;
  std::vector<uint64_t> g_first(ng + 1), g_count(ng + 1), key_idx(ng + 1), s_idx(ng + 1), s_count(ng + 1), cum(ng + 2, 0), first_group(n_seg + 1), distinct(n_seg + 1), sparts(n_seg + 1),
      kept(n_seg + 1), fvalue(n_seg + 2, 0), size(ng + 1, 0), offs(ng + 2, 0);
  std::vector<uint32_t> key_seg(ng + 1), s_seg(ng + 1);
  std::vector<HgGatherEntry> entries(ng + 1);
  for (uint64_t j = 0; j < ng; j++) g_first[j] = pairs[j].first, g_count[j] = pairs[j].second;
  std::vector<uint64_t> out_first(ng + 1, ~uint64_t{0}), out_count(ng + 1, 0), out_line(ng + 1, 0);
  std::vector<uint32_t> out_pattern(ng + 1, 0), out_segment(ng + 1, 0);
  HgRankArgs r{};
  r.parts = rows.data();
  r.part_pattern = part_pattern.data();
  r.part_seg = a.part_seg;
  r.n_parts = n_parts;
  r.src = src.data();
  r.len = len.data();
  r.flags = flags;
  r.n_seg = n_seg;
  r.top = top;
  r.n_groups = ng;
  r.g_first = g_first.data();
  r.g_count = g_count.data();
  r.key_seg = key_seg.data();
  r.key_idx = key_idx.data();
  r.s_count = s_count.data();
  r.cum = cum.data();
  r.first_group = first_group.data();
  r.seg_distinct = distinct.data();
  r.seg_parts = sparts.data();
  r.kept = kept.data();
  r.first_value = fvalue.data();
  r.out_first = out_first.data();
  r.out_count = out_count.data();
  r.size = size.data();
  r.entries = entries.data();
  r.pattern = out_pattern.data();
  r.segment = segments ? out_segment.data() : nullptr;
  r.line_number = out_line.data();
  if (per_seg && !rc) {  // keys pass and the stable sort by segment
    for (uint64_t j = 0; j < ng; j++) hg_rank_keys(r, j);
    std::vector<uint64_t> perm(ng);
    for (uint64_t j = 0; j < ng; j++) perm[j] = j;
    std::stable_sort(perm.begin(), perm.end(), [&](uint64_t x, uint64_t y) { return key_seg[x] < key_seg[y]; });
    for (uint64_t j = 0; j < ng; j++) s_seg[j] = key_seg[perm[j]], s_idx[j] = key_idx[perm[j]];
    r.s_seg = s_seg.data();
    r.s_idx = s_idx.data();
  }
  if (!rc) {
    for (uint64_t j = 0; j <= ng; j++) hg_rank_counts(r, j);
    for (uint64_t j = 0; j <= ng; j++) cum[j + 1] = cum[j] + s_count[j];  // (cum[j]: exclusive)
    for (uint64_t s = 0; s <= n_seg; s++) hg_rank_bounds(r, s);
    for (uint64_t s = 0; s <= n_seg; s++) fvalue[s + 1] = fvalue[s] + kept[s];
    for (uint64_t j = 0; j < ng; j++) hg_rank_place(r, j);
  }
  const uint64_t n_values = fvalue[n_seg];
  if (!rc && n_values > ng) rc = -5;
  if (tr && !rc) {
    for (uint64_t s = 0; s < n_seg; s++) {
      const uint64_t row[RANKSIM_SEG_COLS] = {first_group[s], distinct[s], sparts[s], kept[s]};
      memcpy(tr->seg + RANKSIM_SEG_COLS * s, row, sizeof row);
    }
    for (uint64_t j = 0; j < ng; j++) {  // (hg_rank_place's rule, read from what the bounds pass left)
      const uint64_t s = r.s_seg ? r.s_seg[j] : 0;
      tr->group[j] = s < n_seg && j >= first_group[s] && j - first_group[s] < kept[s];
    }
    uint32_t bits = 1, seg_bits = 1;
    while (bits < 64 && (n_parts >> bits)) bits++;            // (HgRank::run: count <= n_parts)
    while (seg_bits < 32 && (n_seg >> seg_bits)) seg_bits++;  // (segment < n_seg)
    const uint64_t call[RANKSIM_CALL_COLS] = {ng, bits, seg_bits, cap};
    memcpy(tr->call, call, sizeof call);
  }
  for (uint64_t j = 0; j <= ng; j++) offs[j + 1] = offs[j] + size[j];
  for (uint64_t j = 0; j < n_values && !rc; j++)
    if (out_first[j] == ~uint64_t{0} || !size[j]) rc = -5;  // every kept row was written
  for (uint64_t j = n_values; j <= ng && !rc; j++)
    if (out_first[j] != ~uint64_t{0} || size[j]) rc = -5;   // and nothing behind them
  totals[0] = n_values;
  totals[1] = offs[n_values];
  totals[2] = ng;
  totals[3] = n_long;
  if (!rc) {
    for (uint64_t j = 0; j < n_values; j++) {
      first[j] = out_first[j], count[j] = out_count[j], pattern[j] = out_pattern[j], line_number[j] = out_line[j];
      if (segments) segment[j] = out_segment[j];
    }
    for (uint64_t j = 0; j <= n_values; j++) off[j] = offs[j];
    if (per_seg) {
      for (uint64_t s = 0; s <= n_seg; s++) first_value[s] = fvalue[s];
      for (uint64_t s = 0; s < n_seg; s++) seg_distinct[s] = distinct[s], seg_parts[s] = sparts[s];
    }
  }
  // copy pass: the line gather's, over the kept rows' entries
  HgGatherArgs g{};
  g.entries = entries.data();
  g.off = offs.data();
  g.n_entries = n_values;
  g.n_bytes = offs[n_values];
  const uint64_t padded = (g.n_bytes + 15) & ~uint64_t{15};
  if (bad) rc = -2;
  else if (!rc && padded > cap_bytes) rc = -1;
  if (!rc && g.n_bytes) {
    std::vector<uint8_t> out(padded + 1, 0xEE);
    const uint64_t n_spans = (g.n_bytes + tile - 1) / tile;
    std::vector<uint64_t> span(n_spans + 1, 0);
    g.span = span.data();
    for (uint64_t s = 0; s <= n_spans; s++) span[s] = hg_gather_span(g, tile, s);
    for (uint64_t t0 = 0; t0 < g.n_bytes; t0 += tile) {  // a workgroup
      const uint64_t tile_last = (t0 + tile < g.n_bytes ? t0 + tile : g.n_bytes) - 1;
      const uint64_t j_lo = span[t0 / tile], j_hi = span[t0 / tile + 1];
      for (uint64_t p = t0; p <= tile_last; p += 16) {  // a lane's chunk
        const uint64_t j = hg_gather_find(g.off, j_lo, j_hi, p);
        const HgGatherChunk c = hg_gather_chunk(g, view, p, j, offs[j], offs[j + 1]);
        const uint32_t w[4] = {c.w0, c.w1, c.w2, c.w3};
        memcpy(out.data() + p, w, 16);
      }
    }
    if (out[padded] != 0xEE) rc = -3;
    for (uint64_t j = 0; j < n_values && !rc; j++)  // the definition, byte by byte
      for (uint64_t k = 0; k < size[j]; k++)
        if (out[offs[j] + k] != view.byte(entries[j].src + k)) rc = -3;
    for (uint64_t p = g.n_bytes; p < padded; p++)
      if (out[p] != 0) rc = -3;
    if (bad) rc = -2;
    if (!rc) memcpy(out_bytes, out.data(), g.n_bytes);
  }
  free(block);
  return rc;
}

}  // namespace

extern "C" {

// {sizeof params, sizeof result, offsets of the params' fields, offsets of the result's fields, the two flags, sizeof
// hg_values_params_t and hg_values_result_t}
void ranksim_sizes(uint32_t *out) {
  const uint32_t v[] = {sizeof(hg_rank_params_t),
                        sizeof(hg_rank_result_t),
                        offsetof(hg_rank_params_t, flags),
                        offsetof(hg_rank_params_t, hash_bits),
                        offsetof(hg_rank_params_t, table_log2),
                        offsetof(hg_rank_params_t, reserved),
                        offsetof(hg_rank_params_t, top),
                        offsetof(hg_rank_result_t, n_values),
                        offsetof(hg_rank_result_t, n_distinct),
                        offsetof(hg_rank_result_t, n_parts),
                        offsetof(hg_rank_result_t, n_bytes),
                        offsetof(hg_rank_result_t, d_bytes),
                        offsetof(hg_rank_result_t, d_off),
                        offsetof(hg_rank_result_t, d_count),
                        offsetof(hg_rank_result_t, d_first),
                        offsetof(hg_rank_result_t, d_pattern),
                        offsetof(hg_rank_result_t, d_line_number),
                        offsetof(hg_rank_result_t, d_segment),
                        offsetof(hg_rank_result_t, d_first_value),
                        offsetof(hg_rank_result_t, d_seg_distinct),
                        offsetof(hg_rank_result_t, d_seg_parts),
                        offsetof(hg_rank_result_t, n_seg),
                        offsetof(hg_rank_result_t, table_log2),
                        offsetof(hg_rank_result_t, rank_us),
                        offsetof(hg_rank_result_t, reserved),
                        HG_RANK_BY_PATTERN,
                        HG_RANK_PER_SEGMENT,
                        sizeof(hg_values_params_t),
                        sizeof(hg_values_result_t)};
  memcpy(out, v, sizeof v);
}

}  // extern "C"

#ifdef RANKSIM_MAIN
// Two files with `user=ab user=abc` / `user=ab` and `user=ab user=abc`: the values ab, abc, ab | ab, abc at every hash width and
// table size, in both insertion orders, with a base above 2^32, whole and per file, uncut and cut to one; then a long value in
// both of two files.
int main() {
  int bad = 0, cases = 0;
  const uint64_t base = (uint64_t{1} << 32) + 64;
  {
    const std::string text = "user=ab user=abc\nuser=ab\nuser=ab user=abc\n";
    const uint64_t recs[] = {0, 0, 17, 0, 1, 17, 8, 0, 0, 0, 17, 1};
    const uint64_t parts[] = {0, 5, 7, 0, 0, 0, 13, 16, 0, 0, 1, 5, 7, 0, 0, 0, 5, 7, 0, 1, 0, 13, 16, 0, 1};
    const uint64_t seg_start[] = {base + 0, base + 25};
    for (uint32_t flags : {0u, 2u, 3u})
      for (uint64_t top : {0, 1})
        for (uint32_t hash_bits : {64, 8, 1})
          for (uint32_t table_log2 : {0, 3})
            for (uint64_t seed : {0, 7}) {
              uint8_t out[64];
              uint64_t off[8], count[8], first[8], line[8], totals[4], fv[3] = {9, 9, 9}, sd[2] = {9, 9}, sp[2] = {9, 9};
              uint32_t pattern[8], segment[8];
              const long rc = ranksim_run(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs, 3, parts, 5, 1, seg_start, 2, flags, top, hash_bits, table_log2, seed,
                                          16, out, sizeof out, off, count, first, pattern, line, segment, fv, sd, sp, totals);
              const std::string got(reinterpret_cast<const char *>(out), rc == 0 ? totals[1] : 0);
              // whole: ab x3 (first 0), abc x2 (first 1).  Per file: ab x2, abc x1 | ab x1 (first 3), abc x1 (first 4)
              bool ok = rc == 0;
              if (ok && flags == 0) ok = totals[2] == 2 && got == (top ? "ab" : "ababc") && count[0] == 3 && first[0] == 0 && (top || (count[1] == 2 && first[1] == 1));
              if (ok && flags != 0)
                ok = totals[2] == 4 && got == (top ? "abab" : "ababcababc") && count[0] == 2 && segment[0] == 0 && first[top ? 1 : 2] == 3 && segment[top ? 1 : 2] == 1 &&
                     fv[0] == 0 && fv[1] == (top ? 1u : 2u) && fv[2] == (top ? 2u : 4u) && sd[0] == 2 && sd[1] == 2 && sp[0] == 3 && sp[1] == 2;
              if (!ok) printf("flags %u top %llu bits %u log2 %u seed %llu: rc %ld \"%s\"\n", flags, (unsigned long long)top, hash_bits, table_log2, (unsigned long long)seed, rc, got.c_str());
              bad |= !ok;
              cases++;
            }
  }
  {
    std::string one(1000, 'x');
    for (size_t i = 0; i < one.size(); i++) one[i] = static_cast<char>('a' + i % 23);
    const std::string text = "." + one + "\n" + one + "\n.." + one;  // starts at 1, 1002 and 2005: three alignments; the last value ends the text
    const uint64_t recs[] = {0, 0, 1002, 0, 0, 0, 1001, 1, 1, 1001, 1002, 1};
    const uint64_t parts[] = {0, 1, 1001, 0, 0, 0, 0, 1000, 0, 1, 1, 2, 1002, 0, 1};
    const uint64_t seg_start[] = {base + 0, base + 1002};
    for (uint32_t flags : {0u, 2u}) {
      std::vector<uint8_t> out(4096);
      uint64_t off[4], count[4], first[4], line[4], totals[4], fv[3], sd[2], sp[2];
      uint32_t pattern[4], segment[4];
      const long rc = ranksim_run(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs, 3, parts, 3, 1, seg_start, 2, flags, 0, 2, 2, 0, 64, out.data(), out.size(), off,
                                  count, first, pattern, line, segment, fv, sd, sp, totals);
      const bool ok = rc == 0 && totals[3] == 3 && memcmp(out.data(), one.data(), 1000) == 0 &&
                      (flags ? totals[0] == 2 && count[0] == 1 && count[1] == 2 && first[1] == 1 && sp[1] == 2 && memcmp(out.data() + 1000, one.data(), 1000) == 0
                             : totals[0] == 1 && count[0] == 3 && first[0] == 0);
      if (!ok) printf("long, flags %u: rc %ld\n", flags, rc);
      bad |= !ok;
      cases++;
      // the same with a cut of one row a file, through the read-outs: three wave parts; with the segment in the key the key
      // words are (1 << 32) and (2 << 32), file 0 has one group, file 1 one; without it one segment owns the one group
      uint64_t tr_part[3 * 7], tr_seg[2 * 4], tr_group[3], tr_call[4];
      const long rc2 = ranksim_trace(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs, 3, parts, 3, 1, seg_start, 2, flags, 1, 2, 2, 0, 64, out.data(), out.size(),
                                     off, count, first, pattern, line, segment, fv, sd, sp, totals, tr_part, tr_seg, tr_group, tr_call);
      const bool ok2 = rc2 == 0 && tr_part[0] == 2 && tr_part[7] == 2 && tr_part[14] == 2 && tr_part[1] < 4 && tr_part[5] == 1 && tr_call[1] == 2 && tr_call[2] == (flags ? 2u : 1u) &&
                       tr_call[3] == 4 &&
                       (flags ? tr_part[6] == (uint64_t{1} << 32) && tr_part[13] == (uint64_t{2} << 32) && tr_call[0] == 2 && tr_seg[0] == 0 && tr_seg[1] == 1 && tr_seg[2] == 1 &&
                                    tr_seg[3] == 1 && tr_seg[4] == 1 && tr_seg[6] == 2 && tr_group[0] == 1 && tr_group[1] == 1
                              : tr_part[6] == 0 && tr_call[0] == 1 && tr_seg[1] == 1 && tr_seg[2] == 3 && tr_seg[3] == 1 && tr_group[0] == 1);
      if (!ok2) printf("long, read-outs, flags %u: rc %ld\n", flags, rc2);
      bad |= !ok2;
      cases++;
    }
  }
  printf(bad ? "FAILED\n" : "%d cases ok\n", cases);
  return bad;
}
#endif
