// Stream mode's report rules on the host (Face A, hg_hsface.hip; tests/native/flowsim.cpp replays them): what hs_scan's
// small path does to the raw reports of one block, carried across the writes of a stream.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "hg_core.h"

// What the rules remember between a stream's calls.
struct HgFlowRuleState {
  uint64_t offset = 0;                              // bytes written so far
  std::vector<uint32_t> done;                       // SINGLEMATCH ids already reported (sorted)
  std::vector<std::pair<uint64_t, uint32_t>> tail;  // (to, id) delivered with to >= offset - 1: the only ones a later call can repeat
};
struct HgFlowRep {
  uint64_t to;
  uint32_t id;
  bool single;
  uint64_t from = 0;  // start of match (SOM expressions of a database with a horizon; HG_FLOW_PAST_HORIZON past it)
};
constexpr uint64_t HG_FLOW_PAST_HORIZON = ~0ull;  // HS_OFFSET_PAST_HORIZON

// One write of `len` bytes at st.offset: raw[k] = (expression, position in the write + 1; a held '\n' sits at -1) as the
// kernel reports them.  Offset bounds on stream offsets (bounds: {lo, hi} per expression, nullptr when none), one report per
// SINGLEMATCH id per stream (the smallest `to`), an identical (id, to) once.  reps = what to deliver, in (to, id) order;
// st advances past the write.  Start of match: raw_from[k] is raw[k]'s write-relative start (hg_flow_som_write; HG_SOM_FAR
// past the horizon), read for SOM expressions only; an identical (id, to) keeps its smallest `from`, and a span
// to - from >= 2^horizon_bits (0: no horizon) gives HG_FLOW_PAST_HORIZON.
inline void hg_flow_rules(const HgPattern *patterns, const uint32_t *bounds, HgFlowRuleState &st, uint32_t len, const std::pair<uint32_t, uint32_t> *raw,
                          size_t nraw, std::vector<HgFlowRep> &reps, const int64_t *raw_from = nullptr, uint32_t horizon_bits = 0) {
  const uint64_t base = st.offset;
  reps.clear();
  for (size_t k = 0; k < nraw; k++) {
    const uint32_t pi = raw[k].first;
    const uint64_t to = base + raw[k].second - 1;
    if (bounds) {
      const uint32_t lo = bounds[2 * pi], hi = bounds[2 * pi + 1];
      if (to < lo || (hi != HG_BOUND_NONE && to > hi)) continue;
    }
    uint64_t from = 0;
    if (raw_from && (patterns[pi].flags & HG_FLAG_SOM_LEFTMOST)) {
      const int64_t s = raw_from[k];
      from = s == HG_SOM_FAR ? HG_FLOW_PAST_HORIZON : static_cast<uint64_t>(static_cast<int64_t>(base) + s);
      if (from != HG_FLOW_PAST_HORIZON && horizon_bits && to - from >= (1ull << horizon_bits)) from = HG_FLOW_PAST_HORIZON;
    }
    reps.push_back(HgFlowRep{to, patterns[pi].id, hg_report_single(patterns[pi]), from});
  }
  std::sort(reps.begin(), reps.end(), [](const HgFlowRep &a, const HgFlowRep &b) {
    if (a.id != b.id) return a.id < b.id;
    if (a.to != b.to) return a.to < b.to;
    if (a.single != b.single) return a.single < b.single;
    return a.from + 1 < b.from + 1;  // the smallest start first (HG_FLOW_PAST_HORIZON, ~0, is the smallest of all)
  });
  size_t kept = 0;
  bool seen_single = false;
  for (size_t r = 0; r < reps.size(); r++) {
    const HgFlowRep x = reps[r];
    if (r == 0 || x.id != reps[r - 1].id) seen_single = std::binary_search(st.done.begin(), st.done.end(), x.id);
    const bool dup = (r > 0 && x.id == reps[r - 1].id && x.to == reps[r - 1].to) ||
                     std::find(st.tail.begin(), st.tail.end(), std::make_pair(x.to, x.id)) != st.tail.end();
    const bool keep = !dup && !(x.single && seen_single);
    if (x.single && !seen_single) {
      seen_single = true;
      st.done.insert(std::upper_bound(st.done.begin(), st.done.end(), x.id), x.id);
    }
    if (keep) reps[kept++] = x;
  }
  reps.resize(kept);
  std::sort(reps.begin(), reps.end(), [](const HgFlowRep &a, const HgFlowRep &b) { return a.to != b.to ? a.to < b.to : a.id < b.id; });
  st.offset = base + len;
  const uint64_t edge = st.offset ? st.offset - 1 : 0;
  st.tail.erase(std::remove_if(st.tail.begin(), st.tail.end(), [&](const std::pair<uint64_t, uint32_t> &t) { return t.first < edge; }), st.tail.end());
  for (const HgFlowRep &x : reps)
    if (x.to >= edge) st.tail.emplace_back(x.to, x.id);
}

// Which expressions hold a write's trailing '\n' (HG_FLOW_HOLD): those that tell a final '\n' from another
// (hg_flow_needs_hold), and every expression that shares a SINGLEMATCH id with one of them (the reports of such an id then
// never arrive out of order across a write boundary, and the smallest `to` is the one delivered).
inline std::vector<bool> hg_flow_hold_flags(const uint32_t *pool, const HgPattern *patterns, uint32_t np) {
  std::vector<uint32_t> hold_ids;
  for (uint32_t i = 0; i < np; i++)
    if (hg_report_single(patterns[i]) && hg_flow_needs_hold(pool, patterns[i])) hold_ids.push_back(patterns[i].id);
  std::sort(hold_ids.begin(), hold_ids.end());
  std::vector<bool> hold(np);
  for (uint32_t i = 0; i < np; i++)
    hold[i] = hg_flow_needs_hold(pool, patterns[i]) ||
              (hg_report_single(patterns[i]) && std::binary_search(hold_ids.begin(), hold_ids.end(), patterns[i].id));
  return hold;
}

// The static header bits of SOM expressions that share their report id (the som_next cycle, hg_db.h): HG_FLOW_LATE, and
// HG_FLOW_HOLD when any expression of the id holds.  Every report (id, to) of such an id then arrives in one call, where
// the report rules keep the smallest `from`.  0 for every other expression.
inline std::vector<uint32_t> hg_flow_som_bits(const HgPattern *patterns, uint32_t np, const std::vector<bool> &hold) {
  std::vector<uint32_t> bits(np, 0u);
  for (uint32_t i = 0; i < np; i++) {
    const HgPattern &p = patterns[i];
    if (!(p.flags & HG_FLAG_SOM_LEFTMOST) || p.som_next == i) continue;
    bool any = false;
    uint32_t j = i;
    do {
      any = any || hold[j];
      j = patterns[j].som_next;
    } while (j != i);
    bits[i] = HG_FLOW_LATE | (any ? HG_FLOW_HOLD : 0u);
  }
  return bits;
}

// A stream's state layout (Face A; the tests' replays): per expression its header word and nw state words, then for a SOM
// expression (som_width > 0) hg_flow_som_words(nnodes, som_width) words of carried starts.  init: a fresh stream's words.
struct HgFlowLayout {
  std::vector<uint32_t> soff;  // per expression: offset of its header word
  std::vector<uint32_t> init;  // swords
  std::vector<uint32_t> som;   // the SOM expressions, then per SOM expression the nodes of the SOM expressions before it
  uint32_t swords = 0, som_total = 0;  // som_total: the nodes of all SOM expressions
};
inline HgFlowLayout hg_flow_layout(const uint32_t *pool, const HgPattern *patterns, uint32_t np, uint32_t som_width) {
  HgFlowLayout l;
  const std::vector<bool> hold = hg_flow_hold_flags(pool, patterns, np);
  const std::vector<uint32_t> bits = hg_flow_som_bits(patterns, np, hold);
  for (uint32_t i = 0; i < np; i++) {
    const HgPattern &p = patterns[i];
    const bool som = som_width && (p.flags & HG_FLAG_SOM_LEFTMOST);
    const uint32_t words = 1 + p.nw + (som ? hg_flow_som_words(p.nnodes, som_width) : 0u);
    l.soff.push_back(l.swords);
    l.init.push_back(HG_PC_START | (hold[i] ? HG_FLOW_HOLD : 0u) | bits[i]);
    l.init.resize(l.init.size() + words - 1, 0u);
    l.swords += words;
    if (som) {
      l.som.push_back(i);
      l.som_total += p.nnodes;
    }
  }
  const size_t nsom = l.som.size();
  for (size_t k = 0, pre = 0; k < nsom; k++) {
    l.som.push_back(static_cast<uint32_t>(pre));
    pre += patterns[l.som[k]].nnodes;
  }
  return l;
}
