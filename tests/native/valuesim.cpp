// TEST-ONLY host harness for the values stage (never shipped): compiles the scalar rules of hypergrep_amd/csrc/hg_values.h for
// x86 and replays the stage's passes one after the other: the hash pass (a lane's dword path for short parts, the 64 lane
// shares of a wave for long ones, both checked against the byte-wise definition), the insert pass (hg_values_insert over a
// plain table; the parts in their own order or, with a seed, in a shuffled one: the result may not depend on it), mark, scan,
// compact, the sort by first, the derive pass, the scan of the lengths and the gathers' copy pass over spans of `tile` bytes.
// What the GPU stage (hg_values.hip) must reproduce; only its launch geometry and its atomics are left to the GPU tests.
// The text is read through a checked view: every byte and dword read must lie inside [0, nbytes rounded up to 4), and `base`
// (a multiple of 4) is added to every start by the caller and subtracted on access.
// With -DVALUESIM_MAIN the file is a program of its own (a sanitized run).
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_values.h"
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
  uint64_t *probes;
  std::vector<uint64_t> *seen;  // read-out: the slot words the current probe loaded, in order (nullptr: not kept)
  uint64_t load(uint64_t i) const {
    ++*probes;
    if (seen) seen->push_back(slot[i]);
    return slot[i];
  }
  uint64_t claim(uint64_t i, uint64_t word) const {
    const uint64_t old = slot[i];
    if (old == HG_VALUES_EMPTY) slot[i] = word;
    return old;
  }
};

uint64_t wave_hash(const CheckedText &view, uint64_t s, uint32_t len, uint32_t flags, uint32_t pattern, uint32_t hash_bits) {
  uint64_t sum = 0;
  for (uint32_t lane = 0; lane < HG_VALUES_WAVE; lane++) sum += hg_values_hash_wave_lane(view, s, len, flags, pattern, lane);
  return hg_values_hash_wave_end(view, sum, s, len, hash_bits);
}

// the wave's probe of a long part (hg_values_long_kernel): lane 0's table accesses, all lanes' shares of the comparison
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
    if (!hg_values_candidate(a, w, q, h, &rep)) continue;
    bool all = true;
    for (uint32_t lane = 0; lane < HG_VALUES_WAVE; lane++) all = hg_values_equal_wave_lane(view, a.src[rep], a.src[q], a.len[q], lane) && all;
    if (all) return s;
  }
  return HG_VALUES_NO_SLOT;
}

// Read-outs of one run (valuesim_trace): what a cell of tests/value_cells.py claims to reach is proved from these.
struct Trace {
  uint64_t *part;  // VALUESIM_PART_COLS per part: tier (0 none, 1 lane, 2 wave), home, final slot, slots probed, wrapped past the
                   // last slot, claimed (1) or joined (0), occupied slots passed with the part's tag, with another tag
  uint64_t *wave;  // VALUESIM_WAVE_COLS per wave of 64 parts of the insert pass: path (0 no counted lane, 1 one add by the leader,
                   // 2 lane by lane), leader lane, active mask
  uint64_t *call;  // VALUESIM_CALL_COLS: n_long, iterations of the busiest long-kernel wave, last slot occupied, n_values, the
                   // sort's key width, slots of the table, waves of the long kernel's grid, parts without a value
};
constexpr uint32_t VALUESIM_PART_COLS = 8, VALUESIM_WAVE_COLS = 3, VALUESIM_CALL_COLS = 8;

long run_all(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
             const uint64_t *seg_start, uint32_t flags, uint32_t hash_bits, uint32_t table_log2, uint64_t order_seed, uint64_t tile, uint8_t *out_bytes, uint64_t cap_bytes,
             uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint32_t *segment, uint64_t *totals, const Trace *tr);

}  // namespace

extern "C" {

// recs: {line, start, len, segment} per final record, in order; parts: {line, from, to, pattern, segment} per part, in order
// (uint64 each).  Every start (seg_start with segments) already has `base` added.  seg_start: n_seg values or NULL.
// order_seed: 0 inserts the parts in their own order, anything else in a shuffled one.  out_bytes: room for cap_bytes; off:
// n_parts + 1; count, first, pattern, line_number, segment: n_parts each.  totals: {n_values, n_bytes, table probes, long parts}.
// Returns 0, -1 if an output is too small, -2 if a read left the readable range, -3 if two paths that must agree do not (the
// three hashes; the lanes' chunks and the values' bytes), -4 if a probe went round the table.
long valuesim_run(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
                  const uint64_t *seg_start, uint32_t flags, uint32_t hash_bits, uint32_t table_log2, uint64_t order_seed, uint64_t tile, uint8_t *out_bytes, uint64_t cap_bytes,
                  uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint32_t *segment, uint64_t *totals) {
  return run_all(text, nbytes, base, recs, n_recs, parts, n_parts, segments, seg_start, flags, hash_bits, table_log2, order_seed, tile, out_bytes, cap_bytes, off, count, first, pattern,
                 line_number, segment, totals, nullptr);
}

// The same run with its read-outs (Trace above): part VALUESIM_PART_COLS * n_parts, wave VALUESIM_WAVE_COLS * ceil(n_parts / 64),
// call VALUESIM_CALL_COLS values.  The parts are inserted in their own order when order_seed is 0: home, tier, the wave's path and
// the set of occupied slots do not depend on the order; final slot, probes, wrapped and claimed are those of that order.
long valuesim_trace(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
                    const uint64_t *seg_start, uint32_t flags, uint32_t hash_bits, uint32_t table_log2, uint64_t order_seed, uint64_t tile, uint8_t *out_bytes, uint64_t cap_bytes,
                    uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint32_t *segment, uint64_t *totals, uint64_t *tr_part, uint64_t *tr_wave,
                    uint64_t *tr_call) {
  const Trace tr{tr_part, tr_wave, tr_call};
  return run_all(text, nbytes, base, recs, n_recs, parts, n_parts, segments, seg_start, flags, hash_bits, table_log2, order_seed, tile, out_bytes, cap_bytes, off, count, first, pattern,
                 line_number, segment, totals, &tr);
}

}  // extern "C"

namespace {

long run_all(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
             const uint64_t *seg_start, uint32_t flags, uint32_t hash_bits, uint32_t table_log2, uint64_t order_seed, uint64_t tile, uint8_t *out_bytes, uint64_t cap_bytes,
             uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number, uint32_t *segment, uint64_t *totals, const Trace *tr) {
  if (!hash_bits) hash_bits = 64;
  if (!table_log2) table_log2 = hg_values_default_log2(n_parts);
  if (table_log2 > 30 || (uint64_t{1} << table_log2) <= n_parts) return -1;
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
  std::vector<uint64_t> src(n_parts + 1), hash(n_parts + 1), pos(cap + 1), pair_first(n_parts + 1), pair_count(n_parts + 1), v_first(n_parts + 1), size(n_parts + 1, 0);
  std::vector<uint32_t> len(n_parts + 1);
  std::vector<unsigned long long> slot(cap, HG_VALUES_EMPTY), slot_count(cap, 0), slot_first(cap, ~0ull);
  std::vector<HgGatherEntry> entries(n_parts + 1);
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
  a.pos = pos.data();
  a.pair_first = pair_first.data();
  a.pair_count = pair_count.data();
  a.size = size.data();
  a.entries = entries.data();
  a.pattern = pattern;
  a.segment = segments ? segment : nullptr;
  a.line_number = line_number;
  long rc = 0;
  uint64_t probes = 0, n_long = 0;
  // hash pass
  for (uint64_t q = 0; q < n_parts; q++) {
    len[q] = hg_values_locate(a, q, &src[q]);
    hash[q] = 0;
    if (!len[q]) continue;
    const uint64_t want = hg_values_hash_bytes(view, src[q], len[q], flags, part_pattern[q], hash_bits);
    if (hg_values_is_long(len[q])) hash[q] = wave_hash(view, src[q], len[q], flags, part_pattern[q], hash_bits), n_long++;
    else hash[q] = hg_values_hash_dwords(view, src[q], len[q], flags, part_pattern[q], hash_bits);
    if (hash[q] != want) rc = -3;
  }
  // insert pass
  std::vector<uint64_t> order(n_parts);
  for (uint64_t q = 0; q < n_parts; q++) order[q] = q;
  uint64_t state = order_seed;
  for (uint64_t q = n_parts; order_seed && q > 1; q--) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(order[q - 1], order[(state >> 33) % q]);
  }
  std::vector<uint64_t> seen, slot_of(n_parts + 1, HG_VALUES_NO_SLOT);
  const HostTable t{slot.data(), &probes, tr ? &seen : nullptr};
  if (tr) std::fill(tr->part, tr->part + VALUESIM_PART_COLS * n_parts, 0);
  for (uint64_t i = 0; i < n_parts && !rc; i++) {
    const uint64_t q = order[i];
    if (!len[q]) continue;
    seen.clear();
    const uint64_t before = probes;
    const uint64_t s = hg_values_is_long(len[q]) ? wave_insert(a, view, t, q) : hg_values_insert(a, view, t, q);
    if (s == HG_VALUES_NO_SLOT) {
      rc = -4;
      break;
    }
    slot_count[s]++;
    slot_first[s] = std::min<unsigned long long>(slot_first[s], q);
    slot_of[q] = s;
    if (tr) {
      uint64_t *row = tr->part + VALUESIM_PART_COLS * q;
      row[0] = hg_values_is_long(len[q]) ? 2 : 1;
      row[1] = hg_values_home(hash[q], table_log2);
      row[2] = s;
      row[3] = probes - before;
      row[4] = s < row[1];
      row[5] = (slot[s] & HG_VALUES_REP_MASK) == q;
      for (size_t k = 0; k + 1 < seen.size(); k++)  // (the last word seen is the empty slot it claimed or its group's)
        row[(seen[k] >> HG_VALUES_REP_BITS) == hg_values_tag(hash[q]) ? 6 : 7]++;
    }
  }
  if (tr) {  // the insert kernel's waves (insert_body): a lane per part, the short parts with a slot counted
    for (uint64_t w = 0; w * HG_VALUES_WAVE < n_parts; w++) {
      uint64_t act = 0, s0 = HG_VALUES_NO_SLOT;
      bool uniform = true;
      int leader = -1;
      for (uint32_t lane = 0; lane < HG_VALUES_WAVE && w * HG_VALUES_WAVE + lane < n_parts; lane++) {
        const uint64_t q = w * HG_VALUES_WAVE + lane;
        if (!len[q] || hg_values_is_long(len[q]) || slot_of[q] == HG_VALUES_NO_SLOT) continue;
        act |= uint64_t{1} << lane;
        if (leader < 0) leader = static_cast<int>(lane), s0 = slot_of[q];
        uniform = uniform && slot_of[q] == s0;
      }
      uint64_t *row = tr->wave + VALUESIM_WAVE_COLS * w;
      row[0] = !act ? 0 : uniform ? 1 : 2;
      row[1] = leader < 0 ? 0 : static_cast<uint64_t>(leader);
      row[2] = act;
    }
  }
  // mark, scan, compact, sort
  uint64_t n_values = 0;
  for (uint64_t i = 0; i < cap; i++) {
    pos[i] = n_values;
    if (slot[i] != HG_VALUES_EMPTY) pair_first[n_values] = slot_first[i], pair_count[n_values] = slot_count[i], n_values++;
  }
  std::vector<std::pair<uint64_t, uint64_t>> pairs(n_values);
  for (uint64_t j = 0; j < n_values; j++) pairs[j] = {pair_first[j], pair_count[j]};
  std::sort(pairs.begin(), pairs.end());
  for (uint64_t j = 0; j < n_values; j++) v_first[j] = first[j] = pairs[j].first, count[j] = pairs[j].second;
  a.v_first = v_first.data();
  a.n_values = n_values;
  for (uint64_t j = 0; j <= n_values && !rc; j++) hg_values_derive(a, j);
  std::vector<uint64_t> offs(n_values + 1, 0);
  uint64_t sum = 0;
  for (uint64_t j = 0; j <= n_values; j++) {
    offs[j] = off[j] = sum;
    sum += size[j];
  }
  totals[0] = n_values;
  totals[1] = offs[n_values];
  totals[2] = probes;
  totals[3] = n_long;
  if (tr) {
    // the long kernel's grid (hg_values_launch): min((n_parts + 3) / 4, HG_VALUES_LONG_BLOCKS) workgroups of 4 waves, wave i takes
    // the list entries i, i + n_waves, ...
    const uint64_t n_waves = std::min<uint64_t>((n_parts + 3) / 4, HG_VALUES_LONG_BLOCKS) * (HG_VALUES_THREADS / HG_VALUES_WAVE);
    uint32_t bits = 1;
    while (bits < 64 && (n_parts >> bits)) bits++;  // (HgValues::group: first < n_parts)
    uint64_t none = 0;
    for (uint64_t q = 0; q < n_parts; q++) none += !len[q];
    tr->call[0] = n_long;
    tr->call[1] = n_waves ? (n_long + n_waves - 1) / n_waves : 0;
    tr->call[2] = slot[cap - 1] != HG_VALUES_EMPTY;
    tr->call[3] = n_values;
    tr->call[4] = bits;
    tr->call[5] = cap;
    tr->call[6] = n_waves;
    tr->call[7] = none;
  }
  // copy pass: the line gather's, over entries with nothing but a body
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

// The hash of text[s, s + len) by the byte-wise definition (which 0), a lane's dword path (1) and a wave's shares (2); *bad is
// set if a read left [0, nbytes rounded up to 4).
uint64_t valuesim_hash(const uint8_t *text, uint64_t nbytes, uint64_t s, uint32_t len, uint32_t flags, uint32_t pattern, uint32_t hash_bits, int which, int *bad_out) {
  const uint64_t readable = (nbytes + 3) & ~uint64_t{3};
  uint8_t *block = static_cast<uint8_t *>(calloc(readable ? readable : 1, 1));
  if (nbytes) memcpy(block, text, nbytes);
  bool bad = false;
  const CheckedText view{block, 0, readable, &bad};
  const uint64_t h = which == 0   ? hg_values_hash_bytes(view, s, len, flags, pattern, hash_bits)
                     : which == 1 ? hg_values_hash_dwords(view, s, len, flags, pattern, hash_bits)
                                  : wave_hash(view, s, len, flags, pattern, hash_bits);
  free(block);
  *bad_out = bad;
  return h;
}

// {sizeof params, sizeof result, offsets of the params' fields, offsets of the result's fields, HG_VALUES_LANE_MAX, the flag}
void valuesim_sizes(uint32_t *out) {
  const uint32_t v[] = {sizeof(hg_values_params_t),
                        sizeof(hg_values_result_t),
                        offsetof(hg_values_params_t, flags),
                        offsetof(hg_values_params_t, hash_bits),
                        offsetof(hg_values_params_t, table_log2),
                        offsetof(hg_values_params_t, reserved),
                        offsetof(hg_values_result_t, n_values),
                        offsetof(hg_values_result_t, n_parts),
                        offsetof(hg_values_result_t, n_bytes),
                        offsetof(hg_values_result_t, d_bytes),
                        offsetof(hg_values_result_t, d_off),
                        offsetof(hg_values_result_t, d_count),
                        offsetof(hg_values_result_t, d_first),
                        offsetof(hg_values_result_t, d_pattern),
                        offsetof(hg_values_result_t, d_line_number),
                        offsetof(hg_values_result_t, d_segment),
                        offsetof(hg_values_result_t, table_log2),
                        offsetof(hg_values_result_t, values_us),
                        HG_VALUES_LANE_MAX,
                        HG_VALUES_BY_PATTERN,
                        sizeof(hg_part_lines_result_t),
                        sizeof(hg_lines_result_t),
                        sizeof(hg_counts_result_t),
                        sizeof(hg_parts_result_t)};
  memcpy(out, v, sizeof v);
}

}  // extern "C"

#ifdef VALUESIM_MAIN
// `user=ab user=abc` / `user=ab`, and a second file with the same first line: the values ab, abc, ab, ab at every hash width and
// table size, in both insertion orders, with a base above 2^32; then a long value twice and once with another last byte.
int main() {
  int bad = 0, cases = 0;
  const uint64_t base = (uint64_t{1} << 32) + 64;
  {
    const std::string text = "user=ab user=abc\nuser=ab\nuser=ab user=abc\n";
    const uint64_t recs[] = {0, 0, 17, 0, 1, 17, 8, 0, 0, 0, 17, 1};
    const uint64_t parts[] = {0, 5, 7, 0, 0, 0, 13, 16, 1, 0, 1, 5, 7, 0, 0, 0, 5, 7, 1, 1, 0, 13, 16, 0, 1};
    const uint64_t seg_start[] = {base + 0, base + 25};
    for (uint32_t flags = 0; flags < 2; flags++)
      for (uint32_t hash_bits : {64, 8, 1})
        for (uint32_t table_log2 : {0, 3})
          for (uint64_t seed : {0, 7}) {
            uint8_t out[64];
            uint64_t off[8], count[8], first[8], line[8], totals[4];
            uint32_t pattern[8], segment[8];
            const long rc = valuesim_run(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs, 3, parts, 5, 1, seg_start, flags, hash_bits, table_log2, seed, 16, out,
                                         sizeof out, off, count, first, pattern, line, segment, totals);
            const std::string got(reinterpret_cast<const char *>(out), rc == 0 ? totals[1] : 0);
            // by bytes: ab x3 (first 0), abc x2 (first 1).  By pattern: (0, ab) x2, (1, abc) x1, (1, ab) x1 first 3, (0, abc) x1 first 4
            const bool ok = flags == 0 ? rc == 0 && totals[0] == 2 && got == "ababc" && count[0] == 3 && count[1] == 2 && first[0] == 0 && first[1] == 1 && segment[0] == 0
                                       : rc == 0 && totals[0] == 4 && got == "ababcababc" && count[0] == 2 && count[1] == 1 && count[2] == 1 && count[3] == 1 && first[2] == 3 &&
                                             first[3] == 4 && segment[2] == 1 && pattern[2] == 1;
            if (!ok) printf("flags %u bits %u log2 %u seed %llu: rc %ld \"%s\"\n", flags, hash_bits, table_log2, (unsigned long long)seed, rc, got.c_str());
            bad |= !ok;
            cases++;
          }
  }
  {
    std::string one(1000, 'x');
    for (size_t i = 0; i < one.size(); i++) one[i] = static_cast<char>('a' + i % 23);
    std::string other = one;
    other[999] = '!';
    const std::string text = "." + one + "\n" + one + "\n.." + other;  // starts at 1, 1002 and 2005: three alignments; the last value ends the text
    const uint64_t recs[] = {0, base + 0, 1002, 0, 1, base + 1002, 1001, 0, 2, base + 2003, 1002, 0};
    const uint64_t parts[] = {0, 1, 1001, 0, 0, 1, 0, 1000, 0, 0, 2, 2, 1002, 0, 0};
    std::vector<uint8_t> out(4096);
    uint64_t off[4], count[4], first[4], line[4], totals[4];
    uint32_t pattern[4];
    const long rc = valuesim_run(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs, 3, parts, 3, 0, nullptr, 0, 2, 2, 0, 64, out.data(), out.size(), off, count, first,
                                 pattern, line, nullptr, totals);
    const bool ok = rc == 0 && totals[0] == 2 && totals[1] == 2000 && totals[3] == 3 && count[0] == 2 && count[1] == 1 && first[1] == 2 && memcmp(out.data(), one.data(), 1000) == 0 &&
                    memcmp(out.data() + 1000, other.data(), 1000) == 0;
    if (!ok) printf("long: rc %ld\n", rc);
    bad |= !ok;
    cases++;
    // the same through the read-outs: three wave parts, no counted lane in the insert pass's only wave, one iteration a wave,
    // two slots of four taken; in a table of 4 with 2 hash bits every home is a slot of its own or a shared one
    uint64_t tr_part[3 * 8], tr_wave[3], tr_call[8];
    const long rc2 = valuesim_trace(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs, 3, parts, 3, 0, nullptr, 0, 2, 2, 0, 64, out.data(), out.size(), off, count,
                                    first, pattern, line, nullptr, totals, tr_part, tr_wave, tr_call);
    const bool ok2 = rc2 == 0 && totals[0] == 2 && tr_part[0] == 2 && tr_part[8] == 2 && tr_part[16] == 2 && tr_part[5] == 1 && tr_part[8 + 5] == 0 && tr_part[16 + 5] == 1 &&
                     tr_part[2] == tr_part[8 + 2] && tr_part[2] != tr_part[16 + 2] && tr_wave[0] == 0 && tr_call[0] == 3 && tr_call[1] == 1 && tr_call[3] == 2 && tr_call[4] == 2 &&
                     tr_call[5] == 4 && tr_call[6] == 4 && tr_call[7] == 0;
    if (!ok2) printf("long, read-outs: rc %ld\n", rc2);
    bad |= !ok2;
    cases++;
  }
  {  // read-outs of the insert pass: 70 parts, `ab` in lanes 1 .. 63 of wave 0 behind an `abc`, then wave 1 with two values
    std::string text;
    std::vector<uint64_t> recs, parts;
    for (uint64_t q = 0; q < 70; q++) {
      const std::string v = q == 0 || q == 66 ? "abc" : "ab";
      recs.insert(recs.end(), {q, base + text.size(), v.size() + 1, 0});
      parts.insert(parts.end(), {q, 0, v.size(), 0, 0});
      text += v + "\n";
    }
    uint8_t out[64];
    uint64_t off[71], count[71], first[71], line[71], totals[4], tr_part[70 * 8], tr_wave[2 * 3], tr_call[8];
    uint32_t pattern[71];
    const long rc = valuesim_trace(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs.data(), 70, parts.data(), 70, 0, nullptr, 0, 1, 7, 0, 16, out, sizeof out, off, count,
                                   first, pattern, line, nullptr, totals, tr_part, tr_wave, tr_call);
    const bool ok = rc == 0 && totals[0] == 2 && count[0] == 2 && count[1] == 68 && first[1] == 1 && tr_wave[0] == 2 && tr_wave[1] == 0 && tr_wave[2] == ~uint64_t{0} &&
                    tr_wave[3] == 2 && tr_wave[5] == 63 && tr_part[0] == 1 && tr_part[1] < 2 && tr_call[0] == 0 && tr_call[1] == 0 && tr_call[4] == 7 && tr_call[5] == 128;
    if (!ok) printf("insert pass, read-outs: rc %ld\n", rc);
    bad |= !ok;
    cases++;
  }
  printf(bad ? "FAILED\n" : "%d cases ok\n", cases);
  return bad;
}
#endif
