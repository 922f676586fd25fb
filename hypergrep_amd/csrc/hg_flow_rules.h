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
};

// One write of `len` bytes at st.offset: raw[k] = (expression, position in the write + 1; a held '\n' sits at -1) as the
// kernel reports them.  Offset bounds on stream offsets (bounds: {lo, hi} per expression, nullptr when none), one report per
// SINGLEMATCH id per stream (the smallest `to`), an identical (id, to) once.  reps = what to deliver, in (to, id) order;
// st advances past the write.
inline void hg_flow_rules(const HgPattern *patterns, const uint32_t *bounds, HgFlowRuleState &st, uint32_t len, const std::pair<uint32_t, uint32_t> *raw,
                          size_t nraw, std::vector<HgFlowRep> &reps) {
  const uint64_t base = st.offset;
  reps.clear();
  for (size_t k = 0; k < nraw; k++) {
    const uint32_t pi = raw[k].first;
    const uint64_t to = base + raw[k].second - 1;
    if (bounds) {
      const uint32_t lo = bounds[2 * pi], hi = bounds[2 * pi + 1];
      if (to < lo || (hi != HG_BOUND_NONE && to > hi)) continue;
    }
    reps.push_back(HgFlowRep{to, patterns[pi].id, hg_report_single(patterns[pi])});
  }
  std::sort(reps.begin(), reps.end(), [](const HgFlowRep &a, const HgFlowRep &b) {
    if (a.id != b.id) return a.id < b.id;
    if (a.to != b.to) return a.to < b.to;
    return a.single < b.single;
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
