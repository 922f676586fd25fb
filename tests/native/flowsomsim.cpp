// TEST-ONLY host harness for start of match in stream mode (never shipped): compiles the product's pattern compiler and
// the flow routines of hg_core.h for x86 and replays one stream the way Face A and its kernels do: the state laid out by
// hg_flow_layout; per write each SOM expression runs hg_flow_som_write on starts loaded from and stored back to the carried
// words (hg_flow_som_load / hg_flow_som_store, as one lane of hg_flow_som_kernel), each other expression the plain flow
// routines over the write as one piece and one slice; then the report rules of hg_flow_rules.h with the starts.
// fss_block is the block-mode reference: hg_nfa_scan over the concatenation and hg_hit_som (hg_som.h) for `from`.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_flow_rules.h"
#include "../../hypergrep_amd/csrc/hg_som.h"

extern "C" {

void *fss_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, const hs_expr_ext_t *const *ext, unsigned n, char *err, size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  if (hgc_compile_ext(exprs, flags, ids, ext, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
void fss_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// Static header bits of expression i (HG_FLOW_HOLD, HG_FLOW_LATE) in a database with start of match.
uint32_t fss_header(void *h, uint32_t i) {
  const HgDb &db = *static_cast<HgDb *>(h);
  const HgFlowLayout l = hg_flow_layout(db.pool.data(), db.patterns.data(), static_cast<uint32_t>(db.patterns.size()), 8);
  return l.init[l.soff[i]];
}

// The stream data[0, len) written at the cuts (ascending; equal cuts = empty writes), then closed, with `width` bytes per
// carried start and the horizon `hbits` (0: exact).  out[4 k] = call (ncuts + 1: the close), id, from, to: the delivered
// reports in delivery order.
long fss_run(void *h, const uint8_t *data, uint32_t len, const uint32_t *cuts, uint32_t ncuts, uint32_t width, uint32_t hbits, uint64_t *out, size_t cap) {
  const HgDb &db = *static_cast<HgDb *>(h);
  const uint32_t *pool = db.pool.data();
  const uint32_t np = static_cast<uint32_t>(db.patterns.size());
  const HgFlowLayout layout = hg_flow_layout(pool, db.patterns.data(), np, width);
  std::vector<uint32_t> state = layout.init;
  HgFlowRuleState rules;
  std::vector<HgFlowRep> reps;
  size_t n = 0;
  for (uint32_t call = 0; call <= ncuts + 1; call++) {
    const uint32_t a = call == 0 ? 0 : (call <= ncuts ? cuts[call - 1] : len);
    const uint32_t b = call < ncuts ? cuts[call] : len;
    const bool close = call == ncuts + 1;
    const uint8_t *txt = data + a;
    const uint32_t wlen = close ? 0 : b - a;
    std::vector<std::pair<uint32_t, uint32_t>> raw;
    std::vector<int64_t> raw_from;
    for (uint32_t e = 0; e < np; e++) {
      const HgPattern &pat = db.patterns[e];
      uint32_t *words = state.data() + layout.soff[e];
      const uint32_t hdr = words[0];
      if (width && (pat.flags & HG_FLAG_SOM_LEFTMOST)) {
        // (interleaved with stride 3, as the kernel interleaves its lanes' buffers)
        std::vector<int64_t> A(3 * pat.nnodes, HG_SOM_NONE), B(3 * pat.nnodes, HG_SOM_NONE);
        HgSomStarts st{A.data() + 1, 3}, tmp{B.data() + 2, 3};
        uint32_t S[HG_FLOW_SOM_W] = {};
        for (uint32_t w = 0; w < pat.nw; w++) S[w] = words[1 + w];
        hg_flow_som_load(words + 1 + pat.nw, width, S, pat.nw, (hdr & HG_FLOW_HELD) ? -1 : 0, st);
        int32_t carried = 0;
        words[0] = hg_flow_som_write(pool, pat, txt, wlen, close, hdr, S, &st, &tmp, &carried, [&](int32_t i, int64_t s) {
          raw.emplace_back(e, static_cast<uint32_t>(i + 1));
          raw_from.push_back(s);
        });
        for (uint32_t w = 0; w < pat.nw; w++) words[1 + w] = S[w];
        hg_flow_som_store(words + 1 + pat.nw, width, S, pat.nnodes, carried, st);
        continue;
      }
      if (hdr & HG_FLOW_DEAD) continue;
      // the plain flow routines, the write as one piece and one slice (hg_flow_scan_kernel with one lane)
      std::vector<uint32_t> S(words + 1, words + 1 + pat.nw);
      S.resize(HG_MAX_W, 0u);
      uint32_t em = 0;
      auto emit = [&](int32_t i) {
        raw.emplace_back(e, static_cast<uint32_t>(i + 1));
        raw_from.push_back(0);
        em = 1;
      };
      uint32_t pc = hdr & HG_FLOW_PC;
      bool held = (hdr & HG_FLOW_HELD) != 0, acc_done = (hdr & HG_FLOW_ACC_DONE) != 0;
      int32_t stop = held ? -1 : 0;
      if (wlen > 0) {
        if (held) {
          em |= hg_flow_unhold(pool, pat, S.data(), &pc, false, acc_done, emit);
          acc_done = false;
        }
        const bool held_now = !close && txt[wlen - 1] == '\n' && (hdr & HG_FLOW_HOLD);
        const uint32_t stop_w = held_now ? wlen - 1 : wlen;
        if (stop_w > 0 && !(pat.single && em)) {
          hg_flow_scan_slice(pool, pat, txt, 0, stop_w, stop_w, close ? wlen - 1 : HG_NONE32, S.data(), pc, acc_done, [&](uint32_t i) { emit(static_cast<int32_t>(i)); });
          pc = hg_prev_ctx(txt[stop_w - 1]);
          acc_done = false;
        }
        held = held_now;
        stop = static_cast<int32_t>(stop_w);
      }
      uint32_t nh = hdr;
      if (!(pat.single && em)) nh = hg_flow_finish(pool, pat, S.data(), pc, hdr, stop, held, acc_done, close, &em, emit);
      if (pat.single && em) {
        nh = (hdr & HG_FLOW_HOLD) | HG_FLOW_DEAD;
        std::fill(S.begin(), S.end(), 0u);
      }
      words[0] = nh;
      for (uint32_t w = 0; w < pat.nw; w++) words[1 + w] = S[w];
    }
    hg_flow_rules(db.patterns.data(), db.bounds.empty() ? nullptr : db.bounds.data(), rules, wlen, raw.data(), raw.size(), reps, raw_from.data(), hbits);
    for (const HgFlowRep &x : reps) {
      if (n < cap) out[4 * n] = call, out[4 * n + 1] = x.id, out[4 * n + 2] = x.from, out[4 * n + 3] = x.to;
      n++;
    }
  }
  return static_cast<long>(n);
}

// hs_scan(data) on a block-mode twin: out[3 k] = id, from, to in (to, id) order, `from` cut at the horizon hbits.
long fss_block(void *h, const uint8_t *data, uint32_t len, uint32_t hbits, uint64_t *out, size_t cap) {
  const HgDb &db = *static_cast<HgDb *>(h);
  const uint32_t *pool = db.pool.data();
  std::vector<std::tuple<uint32_t, uint32_t, bool, uint32_t>> hits;  // id, to, single, pattern
  for (uint32_t p = 0; p < db.patterns.size(); p++)
    hg_nfa_scan(pool, db.patterns[p], data, len, [&](uint32_t to) {
      if (!db.bounds.empty()) {
        const uint32_t lo = db.bounds[2 * p], hi = db.bounds[2 * p + 1];
        if (to < lo || (hi != HG_BOUND_NONE && to > hi)) return;
      }
      hits.emplace_back(db.patterns[p].id, to, hg_report_single(db.patterns[p]), p);
    });
  std::sort(hits.begin(), hits.end());
  std::vector<std::tuple<uint64_t, uint32_t, uint64_t>> rep;  // to, id, from
  for (size_t k = 0; k < hits.size(); k++) {
    const auto &x = hits[k];
    if (k > 0 && std::get<0>(hits[k - 1]) == std::get<0>(x) && (std::get<1>(hits[k - 1]) == std::get<1>(x) || std::get<2>(x))) continue;
    const uint32_t to = std::get<1>(x);
    uint64_t from = hg_hit_som(pool, db.patterns.data(), std::get<3>(x), data, len, to);
    if ((db.patterns[std::get<3>(x)].flags & HG_FLAG_SOM_LEFTMOST) && hbits && to - from >= (1ull << hbits)) from = HG_FLOW_PAST_HORIZON;
    rep.emplace_back(to, std::get<0>(x), from);
  }
  std::sort(rep.begin(), rep.end());
  for (size_t k = 0; k < rep.size() && k < cap; k++) out[3 * k] = std::get<1>(rep[k]), out[3 * k + 1] = std::get<2>(rep[k]), out[3 * k + 2] = std::get<0>(rep[k]);
  return static_cast<long>(rep.size());
}

}  // extern "C"
