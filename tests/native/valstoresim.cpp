// TEST-ONLY host harness for the value store (never shipped): compiles the scalar rules of hypergrep_amd/csrc/hg_valstore.h for
// x86 and replays a store over many calls: per call the groups (hg_values.h's locate and hashes; the grouping itself is a plain
// map here, the values stage's table has a replay of its own in valuesim.cpp), the lookup (a lane's path for short values, the
// 64 lane shares of a wave for long ones), the size pass and its scans, the rehash when the table changes size, the apply pass
// and the gathers' copy pass into the arena; and a ranking (sort, place pass, copy pass with the arena as text).  The table
// operations of rehash and apply run in a seeded order: the result may not depend on it.  What the GPU stage (hg_valstore.hip)
// must reproduce; only its launch geometry and its atomics are left to the GPU tests.
// The text and the arena are read through checked views: every byte and dword read must lie inside [0, bytes rounded up to 4)
// of a heap block of exactly that size; `base` (a multiple of 4) is added to every text start by the caller.
// With -DVALSTORESIM_MAIN the file is a program of its own (a sanitized run).
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_valstore.h"
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

// a heap block of exactly the readable bytes of `n` bytes at `src` (a read past them is the sanitizer's to catch, too)
struct Block {
  uint8_t *p;
  uint64_t readable;
  Block(const uint8_t *src, uint64_t n) : readable((n + 3) & ~uint64_t{3}) {
    p = static_cast<uint8_t *>(calloc(readable ? readable : 1, 1));
    if (n) memcpy(p, src, n);
  }
  ~Block() { free(p); }
  Block(const Block &) = delete;
};

struct HostTable {
  unsigned long long *slot;
  uint64_t *probes;
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

std::vector<uint64_t> shuffled(uint64_t n, uint64_t seed) {
  std::vector<uint64_t> order(n);
  for (uint64_t i = 0; i < n; i++) order[i] = i;
  uint64_t state = seed;
  for (uint64_t i = n; seed && i > 1; i--) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(order[i - 1], order[(state >> 33) % i]);
  }
  return order;
}

// the wave's lookup of a long group (hg_valstore_long_kernel): lane 0's table reads, all lanes' shares of the comparison
uint64_t wave_lookup(const HgValStoreArgs &a, const CheckedText &text, const CheckedText &arena, const HostTable &t, uint64_t j, bool *overflow) {
  const uint64_t f = a.g_first[j];
  if (f >= a.n_parts || !a.n_values) return HG_VALSTORE_NONE;
  const uint64_t h = a.hash[f], cap = uint64_t{1} << a.store_log2, src = a.src[f];
  const uint32_t len = a.len[f], pat = a.part_pattern[f];
  uint64_t s = hg_values_home(h, a.store_log2);
  for (uint64_t probe = 0; probe < cap; probe++, s = (s + 1) & (cap - 1)) {
    const uint64_t w = t.load(s);
    if (w == HG_VALUES_EMPTY) return HG_VALSTORE_NONE;
    uint64_t idx;
    if (!hg_valstore_candidate(a, w, h, len, pat, &idx)) continue;
    bool all = true;
    for (uint32_t lane = 0; lane < HG_VALUES_WAVE; lane++) all = hg_valstore_equal_wave_lane(text, src, arena, a.v_off[idx], len, lane) && all;
    if (all) return idx;
  }
  *overflow = true;
  return HG_VALSTORE_NONE;
}

// the gathers' copy pass over entries with nothing but a body, spans of `tile` bytes, into out (n_bytes rounded up to 16)
template <typename View>
bool copy_pass(HgGatherArgs g, const View &view, uint64_t tile, uint8_t *out) {
  if (!g.n_bytes) return true;
  const uint64_t n_spans = (g.n_bytes + tile - 1) / tile;
  std::vector<uint64_t> span(n_spans + 1, 0);
  g.span = span.data();
  for (uint64_t s = 0; s <= n_spans; s++) span[s] = hg_gather_span(g, tile, s);
  for (uint64_t t0 = 0; t0 < g.n_bytes; t0 += tile) {  // a workgroup
    const uint64_t tile_last = (t0 + tile < g.n_bytes ? t0 + tile : g.n_bytes) - 1;
    const uint64_t j_lo = span[t0 / tile], j_hi = span[t0 / tile + 1];
    for (uint64_t p = t0; p <= tile_last; p += 16) {  // a lane's chunk
      const uint64_t j = hg_gather_find(g.off, j_lo, j_hi, p);
      const HgGatherChunk c = hg_gather_chunk(g, view, p, j, g.off[j], g.off[j + 1]);
      const uint32_t w[4] = {c.w0, c.w1, c.w2, c.w3};
      memcpy(out + p, w, 16);
    }
  }
  for (uint64_t j = 0; j < g.n_entries; j++)  // the definition, byte by byte
    for (uint64_t k = 0; k < g.entries[j].len; k++)
      if (out[g.off[j] + k] != view.byte(g.entries[j].src + k)) return false;
  return true;
}

struct Store {
  uint32_t flags, hash_bits, fixed_log2;
  uint32_t log2 = 0;
  uint64_t n_parts = 0, tail = 0, probes = 0, rehashes = 0;
  std::vector<unsigned long long> slot;
  std::vector<uint64_t> v_off, v_count, v_first, v_line, v_hash;
  std::vector<uint32_t> v_len, v_pattern;
  std::vector<uint8_t> arena;
  // read-outs of the last call that ended with 0 (valstoresim_trace)
  std::vector<uint64_t> tr_group;  // VALSTORESIM_GROUP_COLS per group: tier (1 lane, 2 wave), found (1) or new (0), slots probed, probed past the last slot
  std::vector<uint64_t> tr_value;  // VALSTORESIM_VALUE_COLS per stored value behind the call: its home in the table before the call (NONE: no table yet) and behind it
  uint64_t tr_call[8] = {};        // log2 before, log2 behind, a rehash ran, the arena's tail before the call, the same rounded up to 16 (where the new
                                   // bytes begin), the new bytes, the count sort's key width behind the call, long groups
};
constexpr uint32_t VALSTORESIM_GROUP_COLS = 4, VALSTORESIM_VALUE_COLS = 2, VALSTORESIM_CALL_COLS = 8;

}  // namespace

extern "C" {

void *valstoresim_new(uint32_t flags, uint32_t hash_bits, uint32_t store_log2) {
  Store *st = new Store;
  st->flags = flags;
  st->hash_bits = hash_bits ? hash_bits : 64;
  st->fixed_log2 = store_log2;
  return st;
}
void valstoresim_free(void *st) { delete static_cast<Store *>(st); }

// One call.  recs: {line, start, len} per final record, in order; parts: {line, from, to, pattern} per part, in order (uint64
// each); every start already has `base` added.  order_seed: 0 runs the rehash and apply lanes in index order, anything else
// in a shuffled one.  totals: {distinct values, added, groups, store_log2, rehashes so far, table probes so far}.
// Returns 0, -2 if a read left a readable range, -3 if two paths that must agree do not (the hashes; the lane's and the wave's
// comparison; the copied bytes), -4 if a probe went round the table, -5 if the values do not fit the table (the store is as it
// was: HG_ERR_NOMEM).
long valstoresim_add(void *handle, const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts,
                     uint64_t order_seed, uint64_t tile, uint64_t *totals) {
  Store &st = *static_cast<Store *>(handle);
  bool bad = false;
  const Block tblock(text, nbytes), ablock(st.arena.data(), st.tail);
  const CheckedText view{tblock.p, base, tblock.readable, &bad}, arena{ablock.p, 0, ablock.readable, &bad};
  std::vector<HgHit> hits(n_recs + 1);
  std::vector<HgHitAux> aux(n_recs + 1);
  std::vector<HgPart> rows(n_parts + 1);
  std::vector<uint32_t> part_pattern(n_parts + 1), len(n_parts + 1);
  std::vector<uint64_t> src(n_parts + 1), hash(n_parts + 1);
  for (uint64_t i = 0; i < n_recs; i++) {
    hits[i] = HgHit{recs[3 * i], 1, 0};
    aux[i] = HgHitAux{recs[3 * i + 1], static_cast<uint32_t>(recs[3 * i + 2]), 0};
  }
  for (uint64_t q = 0; q < n_parts; q++) {
    rows[q] = HgPart{parts[4 * q], static_cast<uint32_t>(parts[4 * q + 1]), static_cast<uint32_t>(parts[4 * q + 2])};
    part_pattern[q] = static_cast<uint32_t>(parts[4 * q + 3]);
  }
  HgValuesArgs va{};
  va.recs = HgGatherList{hits.data(), aux.data(), nullptr, n_recs};
  va.parts = rows.data();
  va.part_pattern = part_pattern.data();
  va.n_parts = n_parts;
  long rc = 0;
  // the call's groups: the values stage's locate and hash per part, then (first, count) by key, sorted by first
  std::map<std::pair<uint32_t, std::string>, std::pair<uint64_t, uint64_t>> by_key;
  for (uint64_t q = 0; q < n_parts; q++) {
    len[q] = hg_values_locate(va, q, &src[q]);
    hash[q] = 0;
    if (!len[q]) continue;
    const uint64_t want = hg_values_hash_bytes(view, src[q], len[q], st.flags, part_pattern[q], st.hash_bits);
    if (hg_values_is_long(len[q])) {
      uint64_t sum = 0;
      for (uint32_t lane = 0; lane < HG_VALUES_WAVE; lane++) sum += hg_values_hash_wave_lane(view, src[q], len[q], st.flags, part_pattern[q], lane);
      hash[q] = hg_values_hash_wave_end(view, sum, src[q], len[q], st.hash_bits);
    } else {
      hash[q] = hg_values_hash_dwords(view, src[q], len[q], st.flags, part_pattern[q], st.hash_bits);
    }
    if (hash[q] != want) rc = -3;
    std::string value;
    for (uint32_t k = 0; k < len[q]; k++) value.push_back(static_cast<char>(view.byte(src[q] + k)));
    auto it = by_key.emplace(std::make_pair((st.flags & HG_VALSTORE_F_BY_PATTERN) ? part_pattern[q] : 0u, value), std::make_pair(q, uint64_t{0})).first;
    it->second.second++;
  }
  std::vector<std::pair<uint64_t, uint64_t>> pairs;
  for (const auto &kv : by_key) pairs.push_back(kv.second);
  std::sort(pairs.begin(), pairs.end());
  const uint64_t ng = pairs.size(), n_old = st.v_off.size();
  std::vector<uint64_t> g_first(ng + 1), g_count(ng + 1), match(ng + 1), new_flag(ng + 1), new_len(ng + 1), new_idx(ng + 1), new_off(ng + 1);
  for (uint64_t j = 0; j < ng; j++) g_first[j] = pairs[j].first, g_count[j] = pairs[j].second;
  HgValStoreArgs a{};
  a.parts = rows.data();
  a.part_pattern = part_pattern.data();
  a.n_parts = n_parts;
  a.src = src.data();
  a.len = len.data();
  a.hash = hash.data();
  a.g_first = g_first.data();
  a.g_count = g_count.data();
  a.n_groups = ng;
  a.flags = st.flags;
  a.store_log2 = st.log2;
  a.slot = st.slot.data();
  a.n_values = n_old;
  a.v_off = st.v_off.data();
  a.v_count = st.v_count.data();
  a.v_first = st.v_first.data();
  a.v_line = st.v_line.data();
  a.v_hash = st.v_hash.data();
  a.v_len = st.v_len.data();
  a.v_pattern = st.v_pattern.data();
  a.parts_before = st.n_parts;
  a.arena_tail = (st.tail + 15) & ~uint64_t{15};
  a.match = match.data();
  a.new_flag = new_flag.data();
  a.new_len = new_len.data();
  a.new_idx = new_idx.data();
  a.new_off = new_off.data();
  // lookup (read-only): both forms where the lane's is allowed, the wave's alone for long values
  const HostTable t{st.slot.data(), &st.probes};
  bool overflow = false;
  std::vector<uint64_t> tr_group(VALSTORESIM_GROUP_COLS * ng, 0);
  uint64_t n_long = 0;
  for (uint64_t j = 0; j < ng; j++) {
    const uint64_t before = st.probes;
    const uint64_t by_wave = wave_lookup(a, view, arena, t, j, &overflow);
    match[j] = by_wave;
    const bool is_long = hg_values_is_long(len[g_first[j]]);
    n_long += is_long;
    tr_group[VALSTORESIM_GROUP_COLS * j] = is_long ? 2 : 1;
    tr_group[VALSTORESIM_GROUP_COLS * j + 1] = by_wave != HG_VALSTORE_NONE;
    tr_group[VALSTORESIM_GROUP_COLS * j + 2] = st.probes - before;
    tr_group[VALSTORESIM_GROUP_COLS * j + 3] = st.log2 && hg_values_home(hash[g_first[j]], st.log2) + (st.probes - before) > (uint64_t{1} << st.log2);
    if (!hg_values_is_long(len[g_first[j]]) && hg_valstore_lookup(a, view, arena, t, j, &overflow) != by_wave) rc = -3;
  }
  if (overflow) rc = rc ? rc : -4;
  // size
  for (uint64_t j = 0; j <= ng; j++) hg_valstore_size(a, j);
  uint64_t n_new = 0, new_bytes = 0;
  for (uint64_t j = 0; j <= ng; j++) {
    new_idx[j] = n_new, new_off[j] = new_bytes;
    n_new += new_flag[j], new_bytes += new_len[j];
  }
  const uint64_t n_after = n_old + n_new;
  const uint32_t log2_new = st.fixed_log2 ? st.fixed_log2 : std::max(st.log2, hg_valstore_default_log2(n_after));
  if (bad) rc = -2;
  if (rc) return rc;
  if (log2_new > 30 || (uint64_t{1} << log2_new) <= n_after) return -5;
  // grow, keeping the contents; rehash into a table of the new size
  const uint64_t cap_new = uint64_t{1} << log2_new, padded = (new_bytes + 15) & ~uint64_t{15};
  const uint32_t log2_old = st.log2;
  const uint64_t tail_old = st.tail;
  if (log2_new != st.log2) {
    std::vector<unsigned long long> fresh(cap_new, HG_VALUES_EMPTY);
    a.slot_new = fresh.data();
    a.new_log2 = log2_new;
    const HostTable tn{fresh.data(), &st.probes};
    for (uint64_t i : shuffled(n_old, order_seed))
      if (!hg_valstore_rehash(a, tn, i)) rc = -4;
    st.slot.swap(fresh);
    st.log2 = log2_new;
    if (n_old) st.rehashes++;
  }
  for (auto *v : {&st.v_off, &st.v_count, &st.v_first, &st.v_line, &st.v_hash}) v->resize(n_after);
  st.v_len.resize(n_after);
  st.v_pattern.resize(n_after);
  st.arena.resize(a.arena_tail + padded, 0xEE);
  std::vector<HgGatherEntry> entries(n_new + 1);
  std::vector<uint64_t> ent_off(n_new + 1, ~uint64_t{0});
  a.slot = st.slot.data();
  a.store_log2 = log2_new;
  a.v_off = st.v_off.data();
  a.v_count = st.v_count.data();
  a.v_first = st.v_first.data();
  a.v_line = st.v_line.data();
  a.v_hash = st.v_hash.data();
  a.v_len = st.v_len.data();
  a.v_pattern = st.v_pattern.data();
  a.max_values = n_after;
  a.entries = entries.data();
  a.ent_off = ent_off.data();
  // apply
  const HostTable ta{st.slot.data(), &st.probes};
  for (uint64_t j : shuffled(ng + 1, order_seed))
    if (!hg_valstore_apply(a, ta, j)) rc = -4;
  // copy: the new values' bytes from the text to the arena's tail
  HgGatherArgs g{};
  g.entries = entries.data();
  g.off = ent_off.data();
  g.n_entries = n_new;
  g.n_bytes = new_bytes;
  if (ent_off[n_new] != new_bytes) rc = rc ? rc : -3;
  else if (!copy_pass(g, view, tile, st.arena.data() + a.arena_tail)) rc = rc ? rc : -3;
  if (bad) rc = -2;
  st.n_parts += n_parts;
  st.tail = a.arena_tail + new_bytes;
  totals[0] = n_after;
  totals[1] = n_new;
  totals[2] = ng;
  totals[3] = log2_new;
  totals[4] = st.rehashes;
  totals[5] = st.probes;
  if (!rc) {
    st.tr_group.swap(tr_group);
    st.tr_value.assign(VALSTORESIM_VALUE_COLS * n_after, 0);
    for (uint64_t i = 0; i < n_after; i++) {
      st.tr_value[VALSTORESIM_VALUE_COLS * i] = log2_old ? hg_values_home(st.v_hash[i], log2_old) : HG_VALSTORE_NONE;
      st.tr_value[VALSTORESIM_VALUE_COLS * i + 1] = hg_values_home(st.v_hash[i], log2_new);
    }
    uint32_t bits = 1;
    while (bits < 64 && (st.n_parts >> bits)) bits++;  // (HgValueStore::rank: count <= the accumulated parts)
    const uint64_t call[VALSTORESIM_CALL_COLS] = {log2_old, log2_new, log2_new != log2_old && n_old, tail_old, a.arena_tail, new_bytes, bits, n_long};
    memcpy(st.tr_call, call, sizeof call);
  }
  return rc;
}

// The read-outs of the last call that returned 0: groups and values are filled up to their caps; counts: {groups, values}.
void valstoresim_trace(void *handle, uint64_t *groups, uint64_t cap_groups, uint64_t *values, uint64_t cap_values, uint64_t *call, uint64_t *counts) {
  const Store &st = *static_cast<const Store *>(handle);
  counts[0] = st.tr_group.size() / VALSTORESIM_GROUP_COLS;
  counts[1] = st.tr_value.size() / VALSTORESIM_VALUE_COLS;
  for (uint64_t k = 0; k < st.tr_group.size() && k < VALSTORESIM_GROUP_COLS * cap_groups; k++) groups[k] = st.tr_group[k];
  for (uint64_t k = 0; k < st.tr_value.size() && k < VALSTORESIM_VALUE_COLS * cap_values; k++) values[k] = st.tr_value[k];
  memcpy(call, st.tr_call, sizeof st.tr_call);
}

// A ranking.  out_bytes: room for cap_bytes; off: rows + 1; count, first, pattern, line_number: rows each, rows = min(top,
// distinct values) (top 0: all).  totals: {rows, bytes, distinct values, accumulated parts}.  Returns 0, -1 if an output is too
// small, -2 if a read left the arena's readable range, -3 if the copied bytes are not the rows'.
long valstoresim_rank(void *handle, uint64_t top, int order_first, uint64_t tile, uint8_t *out_bytes, uint64_t cap_bytes, uint64_t max_rows, uint64_t *off, uint64_t *count,
                      uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint64_t *totals) {
  const Store &st = *static_cast<const Store *>(handle);
  const uint64_t n = st.v_off.size(), rows = (top && top < n) ? top : n;
  if (rows > max_rows) return -1;
  std::vector<uint64_t> order(n);
  for (uint64_t i = 0; i < n; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return st.v_count[x] > st.v_count[y]; });
  std::vector<uint64_t> size(rows + 1), offs(rows + 1);
  std::vector<HgGatherEntry> entries(rows + 1);
  HgValRankArgs a{};
  a.n_values = n;
  a.n_rows = rows;
  a.order = order_first ? nullptr : order.data();
  a.v_off = st.v_off.data();
  a.v_count = st.v_count.data();
  a.v_first = st.v_first.data();
  a.v_line = st.v_line.data();
  a.v_len = st.v_len.data();
  a.v_pattern = st.v_pattern.data();
  a.out_count = count;
  a.out_first = first;
  a.out_line = line_number;
  a.out_pattern = pattern;
  a.size = size.data();
  a.entries = entries.data();
  for (uint64_t r = 0; r <= rows; r++) hg_valstore_place(a, r);
  uint64_t sum = 0;
  for (uint64_t r = 0; r <= rows; r++) {
    offs[r] = off[r] = sum;
    sum += size[r];
  }
  totals[0] = rows;
  totals[1] = sum;
  totals[2] = n;
  totals[3] = st.n_parts;
  const uint64_t padded = (sum + 15) & ~uint64_t{15};
  if (padded > cap_bytes) return -1;
  bool bad = false;
  const Block ablock(st.arena.data(), st.tail);
  const CheckedText arena{ablock.p, 0, ablock.readable, &bad};
  HgGatherArgs g{};
  g.entries = entries.data();
  g.off = offs.data();
  g.n_entries = rows;
  g.n_bytes = sum;
  std::vector<uint8_t> out(padded + 1, 0xEE);
  long rc = copy_pass(g, arena, tile, out.data()) ? 0 : -3;
  if (out[padded] != 0xEE) rc = -3;
  if (bad) rc = -2;
  if (!rc && sum) memcpy(out_bytes, out.data(), sum);
  return rc;
}

// Are a[sa, sa + n) and b[sb, sb + n) the same bytes, by a lane (wave 0) or by the 64 shares of a wave (wave 1)?  Both live in
// heap blocks of exactly their bytes rounded up to 4; *bad_out is set if a read left one.
int valstoresim_equal(const uint8_t *a, uint64_t na, uint64_t sa, const uint8_t *b, uint64_t nb, uint64_t sb, uint32_t n, int wave, int *bad_out) {
  bool bad = false;
  const Block ba(a, na), bb(b, nb);
  const CheckedText ta{ba.p, 0, ba.readable, &bad}, tb{bb.p, 0, bb.readable, &bad};
  bool eq = true;
  if (wave)
    for (uint32_t lane = 0; lane < HG_VALUES_WAVE; lane++) eq = hg_valstore_equal_wave_lane(ta, sa, tb, sb, n, lane) && eq;
  else
    eq = hg_valstore_equal(ta, sa, tb, sb, n);
  *bad_out = bad;
  return eq;
}

// {sizeof params, result, rank result; offsets of the params' fields; offsets of the results' fields; the flags}
void valstoresim_sizes(uint32_t *out) {
  const uint32_t v[] = {sizeof(hg_acc_params_t),
                        sizeof(hg_acc_result_t),
                        sizeof(hg_acc_rank_result_t),
                        offsetof(hg_acc_params_t, flags),
                        offsetof(hg_acc_params_t, hash_bits),
                        offsetof(hg_acc_params_t, table_log2),
                        offsetof(hg_acc_params_t, store_log2),
                        offsetof(hg_acc_result_t, n_distinct),
                        offsetof(hg_acc_result_t, n_added),
                        offsetof(hg_acc_result_t, n_groups),
                        offsetof(hg_acc_result_t, n_parts),
                        offsetof(hg_acc_result_t, n_parts_total),
                        offsetof(hg_acc_result_t, n_bytes),
                        offsetof(hg_acc_result_t, store_log2),
                        offsetof(hg_acc_result_t, acc_us),
                        offsetof(hg_acc_rank_result_t, n_values),
                        offsetof(hg_acc_rank_result_t, n_distinct),
                        offsetof(hg_acc_rank_result_t, n_parts),
                        offsetof(hg_acc_rank_result_t, n_bytes),
                        offsetof(hg_acc_rank_result_t, d_bytes),
                        offsetof(hg_acc_rank_result_t, d_off),
                        offsetof(hg_acc_rank_result_t, d_count),
                        offsetof(hg_acc_rank_result_t, d_first),
                        offsetof(hg_acc_rank_result_t, d_pattern),
                        offsetof(hg_acc_rank_result_t, d_line_number),
                        offsetof(hg_acc_rank_result_t, store_log2),
                        offsetof(hg_acc_rank_result_t, rank_us),
                        HG_ACC_BY_PATTERN,
                        HG_ACC_RESET,
                        HG_ACC_ORDER_FIRST,
                        sizeof(hg_values_result_t),
                        sizeof(hg_rank_result_t)};
  memcpy(out, v, sizeof v);
}

}  // extern "C"

#ifdef VALSTORESIM_MAIN
// Three buffers of one log (`user=ab user=abc` / `user=ab` / `user=abd user=ab`, the middle one without a part in a fourth
// run), at every hash width, both keys' flags and both orders, with a base above 2^32 and a table fixed at 2^2 (the fourth
// value does not fit: -5, and the store still ranks as before); then long values that differ in the last byte, across calls.
int main() {
  int bad = 0, cases = 0;
  const uint64_t base = (uint64_t{1} << 32) + 64;
  const std::string bufs[3] = {"user=ab user=abc\n", "user=ab\n", ".user=abd user=ab\n"};
  const uint64_t recs[3][3] = {{0, base + 0, 17}, {1, base + 0, 8}, {2, base + 0, 18}};
  const uint64_t parts0[] = {0, 5, 7, 0, 0, 13, 16, 1}, parts1[] = {1, 5, 7, 1}, parts2[] = {2, 6, 9, 0, 2, 15, 17, 0};
  const uint64_t *parts[3] = {parts0, parts1, parts2};
  const uint64_t n_parts[3] = {2, 1, 2};
  for (uint32_t flags = 0; flags < 2; flags++)
    for (uint32_t hash_bits : {64, 8, 1})
      for (uint32_t fixed : {0, 2})
        for (uint64_t seed : {0, 7}) {
          void *st = valstoresim_new(flags, hash_bits, fixed);
          uint64_t totals[6] = {0};
          long rc = 0, last = 0;
          for (int b = 0; b < 3 && !rc; b++) {
            last = valstoresim_add(st, reinterpret_cast<const uint8_t *>(bufs[b].data()), bufs[b].size(), base, recs[b], 1, parts[b], n_parts[b], seed, 16, totals);
            if (last != -5) rc = last;
          }
          uint8_t out[64];
          uint64_t off[8], count[8], first[8], line[8], rt[4];
          uint32_t pattern[8];
          if (!rc) rc = valstoresim_rank(st, 0, 0, 16, out, sizeof out, 8, off, count, first, pattern, line, rt);
          const std::string got(reinterpret_cast<const char *>(out), rc == 0 ? rt[1] : 0);
          // by bytes: ab x3 (first 0), abc (1), abd (3).  By pattern: (0, ab) x2, (1, abc), (1, ab) first 2, (0, abd) first 3.
          // With 2^2 slots: by bytes the third value fits (3 < 4); by pattern the third call has two new ones and is refused.
          bool ok;
          if (flags == 0) ok = rc == 0 && last == 0 && rt[0] == 3 && got == "ababcabd" && count[0] == 3 && first[1] == 1 && first[2] == 3 && line[2] == 2 && rt[3] == 5;
          else if (fixed) ok = rc == 0 && last == -5 && rt[0] == 3 && got == "ababcab" && count[0] == 1 && first[2] == 2 && pattern[2] == 1 && rt[3] == 3;
          else ok = rc == 0 && last == 0 && rt[0] == 4 && got == "ababcababd" && count[0] == 2 && first[0] == 0 && first[1] == 1 && first[2] == 2 && first[3] == 3 && rt[3] == 5;
          if (!ok) printf("flags %u bits %u fixed %u seed %llu: rc %ld last %ld \"%s\"\n", flags, hash_bits, fixed, (unsigned long long)seed, rc, last, got.c_str());
          bad |= !ok;
          cases++;
          valstoresim_free(st);
        }
  {
    std::string one(1027, 'x');
    for (size_t i = 0; i < one.size(); i++) one[i] = static_cast<char>('a' + i % 23);
    std::string other = one;
    other[1026] = '!';
    const std::string b0 = "." + one + "\n", b1 = ".." + other + "\n" + one;  // starts at 1, 2 and 1030 + ...; the last value ends its text
    const uint64_t r0[] = {0, base + 0, 1029}, r1[] = {1, base + 0, 1030, 2, base + 1030, 1027};
    const uint64_t p0[] = {0, 1, 1028, 0}, p1[] = {1, 2, 1029, 0, 2, 0, 1027, 0};
    void *st = valstoresim_new(0, 2, 0);
    uint64_t totals[6];
    long rc = valstoresim_add(st, reinterpret_cast<const uint8_t *>(b0.data()), b0.size(), base, r0, 1, p0, 1, 3, 64, totals);
    if (!rc) rc = valstoresim_add(st, reinterpret_cast<const uint8_t *>(b1.data()), b1.size(), base, r1, 2, p1, 2, 3, 64, totals);
    std::vector<uint8_t> out(4096);
    uint64_t off[4], count[4], first[4], line[4], rt[4];
    uint32_t pattern[4];
    if (!rc) rc = valstoresim_rank(st, 0, 0, 64, out.data(), out.size(), 4, off, count, first, pattern, line, rt);
    const bool ok = rc == 0 && rt[0] == 2 && rt[1] == 2054 && count[0] == 2 && count[1] == 1 && first[0] == 0 && first[1] == 1 && memcmp(out.data(), one.data(), 1027) == 0 &&
                    memcmp(out.data() + 1027, other.data(), 1027) == 0;
    if (!ok) printf("long: rc %ld\n", rc);
    bad |= !ok;
    cases++;
    // the read-outs of the second call: two wave groups, `other` new and `one` found; the first call left 1027 bytes, so the
    // new bytes begin at 1040; both values keep their home (no table before the first call, 2^10 slots since)
    uint64_t groups[2 * 4], values[2 * 2], call[8], counts[2];
    valstoresim_trace(st, groups, 2, values, 2, call, counts);
    const bool ok2 = counts[0] == 2 && counts[1] == 2 && groups[0] == 2 && groups[1] == 0 && groups[4] == 2 && groups[5] == 1 && groups[6] >= 1 && values[0] == values[1] &&
                     values[2] == values[3] && values[0] < 4 && call[0] == 10 && call[1] == 10 && call[2] == 0 && call[3] == 1027 && call[4] == 1040 && call[5] == 1027 && call[6] == 2 &&
                     call[7] == 2;
    if (!ok2) printf("long, read-outs: %llu %llu\n", (unsigned long long)counts[0], (unsigned long long)counts[1]);
    bad |= !ok2;
    cases++;
    valstoresim_free(st);
  }
  printf(bad ? "FAILED\n" : "%d cases ok\n", cases);
  return bad;
}
#endif
