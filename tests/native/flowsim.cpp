// TEST-ONLY host harness for stream mode (never shipped): compiles the product's pattern compiler and the flow routines of
// hg_core.h (hg_flow_scan_slice, hg_flow_unhold, hg_flow_finish) for x86 and replays what hg_flow_scan_kernel does with
// them: a stream's writes cut into pieces, each piece split over lanes by start position, the slices' end states OR-ed, ends
// found twice kept once, the write-end rules applied per expression: raw ends (expression, stream offset, call).  flowsim_deliver
// applies Face A's report rules (hg_flow_rules.h) to them; flowsim_block runs hg_nfa_scan over the concatenation.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_flow_rules.h"

extern "C" {

void *flowsim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, const hs_expr_ext_t *const *ext, unsigned n, char *err,
                      size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  if (hgc_compile_ext(exprs, flags, ids, ext, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
void flowsim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// Does expression i hold a write's trailing '\n' (hg_flow_hold_flags, as the Face A compile decides it)?
uint32_t flowsim_hold(void *h, uint32_t i) {
  const HgDb &db = *static_cast<HgDb *>(h);
  return hg_flow_hold_flags(db.pool.data(), db.patterns.data(), static_cast<uint32_t>(db.patterns.size()))[i] ? 1u : 0u;
}

// Words of automaton tables of group g (expressions [g * HG_FLOW_PPW, ...)) by hg_flow_scan_kernel's formula: the kernel stages
// the group in LDS when this is at most HG_BLOCK_SMALL_POOL (flowsim_pool_words), else reads the tables from HBM.
uint32_t flowsim_group_span(void *h, uint32_t g) {
  const HgDb &db = *static_cast<HgDb *>(h);
  const uint32_t np = static_cast<uint32_t>(db.patterns.size());
  const uint32_t first = g * HG_FLOW_PPW, last = std::min(first + HG_FLOW_PPW, np);
  if (first >= last) return 0;
  const HgPattern &pl = db.patterns[last - 1];
  return pl.acc_off + 20u * pl.nw - db.patterns[first].reach_off;
}
uint32_t flowsim_words(void *h, uint32_t i) { return static_cast<HgDb *>(h)->patterns[i].nw; }

// Raw ends of every expression over data[0, len) as one block: out[2 k] = expression, out[2 k + 1] = end.
long flowsim_block(void *h, const uint8_t *data, uint32_t len, uint32_t *out, size_t cap) {
  const HgDb &db = *static_cast<HgDb *>(h);
  size_t n = 0;
  for (uint32_t p = 0; p < db.patterns.size(); p++)
    hg_nfa_scan(db.pool.data(), db.patterns[p], data, len, [&](uint32_t to) {
      if (n < cap) out[2 * n] = p, out[2 * n + 1] = to;
      n++;
    });
  return static_cast<long>(n);
}

// The stream data[0, len) written at the cuts (ascending offsets; equal cuts = empty writes), then closed.  piece: the
// bytes of a piece (at least 1); lanes: lanes per expression (slices of at least `min_slice` bytes, as the kernel).
// out[3 k] = call (write number; ncuts + 1 = the close), out[3 k + 1] = expression, out[3 k + 2] = stream offset.
long flowsim_run(void *h, const uint8_t *data, uint32_t len, const uint32_t *cuts, uint32_t ncuts, uint32_t piece, uint32_t lanes, uint32_t min_slice,
                 uint32_t *out, size_t cap) {
  const HgDb &db = *static_cast<HgDb *>(h);
  const uint32_t *pool = db.pool.data();
  size_t n = 0;
  const std::vector<bool> hold = hg_flow_hold_flags(pool, db.patterns.data(), static_cast<uint32_t>(db.patterns.size()));
  for (uint32_t e = 0; e < db.patterns.size(); e++) {
    const HgPattern &pat = db.patterns[e];
    std::vector<uint32_t> S(HG_MAX_W, 0u), T(HG_MAX_W);
    uint32_t hdr = HG_PC_START | (hold[e] ? HG_FLOW_HOLD : 0u);
    for (uint32_t call = 0; call <= ncuts + 1; call++) {
      const uint32_t a = call == 0 ? 0 : (call <= ncuts ? cuts[call - 1] : len);
      const uint32_t b = call < ncuts ? cuts[call] : len;
      const bool close = call == ncuts + 1;
      const uint8_t *txt = data + a;
      const uint32_t wlen = close ? 0 : b - a;
      if (hdr & HG_FLOW_DEAD) continue;
      uint32_t em = 0;
      auto emit_abs = [&](int64_t rel) {
        if (n < cap) out[3 * n] = call, out[3 * n + 1] = e, out[3 * n + 2] = static_cast<uint32_t>(a + rel);
        n++;
        em = 1;
      };
      const bool held_now = !close && wlen > 0 && txt[wlen - 1] == '\n' && (hdr & HG_FLOW_HOLD);
      const uint32_t stop_w = held_now ? wlen - 1 : wlen;
      const uint32_t npieces = (wlen + piece - 1) / piece;
      std::vector<uint32_t> acc(HG_MAX_W, 0u);
      for (uint32_t q = 0; q < npieces; q++) {
        const uint32_t pbase = q * piece, plen = std::min(piece, wlen - pbase);
        const uint32_t slice_len = std::max(min_slice, (plen + lanes - 1) / lanes);
        const uint32_t nslices = (plen + slice_len - 1) / slice_len;
        const uint32_t pstop = std::min(stop_w - pbase, plen);
        std::set<uint32_t> seen;
        std::vector<uint32_t> next(HG_MAX_W, 0u);
        bool gone = false;
        for (uint32_t k = 0; k < nslices && !gone; k++) {
          const uint32_t from = k * slice_len, upto = std::min(from + slice_len, plen);
          std::fill(T.begin(), T.end(), 0u);
          uint32_t pc, lem = 0;
          bool skip = false;
          auto emit_at = [&](int32_t i) {
            const int32_t pi = i - static_cast<int32_t>(pbase);
            if (pi >= 0 && !seen.insert(static_cast<uint32_t>(pi)).second) return;
            emit_abs(i);
          };
          if (k == 0 && q == 0) {
            for (uint32_t w = 0; w < pat.nw; w++) T[w] = S[w];
            pc = hdr & HG_FLOW_PC;
            skip = (hdr & HG_FLOW_ACC_DONE) != 0;
            if (hdr & HG_FLOW_HELD) {
              lem |= hg_flow_unhold(pool, pat, T.data(), &pc, false, skip, emit_at);
              skip = false;
            }
          } else if (k == 0) {
            for (uint32_t w = 0; w < pat.nw; w++) T[w] = acc[w];
            pc = hg_prev_ctx(txt[pbase - 1]);
          } else {
            pc = hg_prev_ctx(txt[pbase + from - 1]);
          }
          const uint32_t final_nl = close && q + 1 == npieces ? plen - 1 : HG_NONE32;
          if (!(pat.single && lem))
            lem |= hg_flow_scan_slice(pool, pat, txt + pbase, from, upto, pstop, final_nl, T.data(), pc, skip, [&](uint32_t i) { emit_at(static_cast<int32_t>(pbase + i)); });
          if (pat.single && lem) gone = true;
          else
            for (uint32_t w = 0; w < pat.nw; w++) next[w] |= T[w];
        }
        acc = next;
        if (gone) break;
      }
      if (pat.single && em) {
        hdr = (hdr & HG_FLOW_HOLD) | HG_FLOW_DEAD;
        continue;
      }
      uint32_t pc;
      int32_t stop;
      bool held, acc_done;
      if (wlen == 0) {
        held = (hdr & HG_FLOW_HELD) != 0;
        acc_done = (hdr & HG_FLOW_ACC_DONE) != 0;
        pc = hdr & HG_FLOW_PC;
        stop = held ? -1 : 0;
      } else {
        S = acc;
        held = held_now;
        stop = static_cast<int32_t>(stop_w);
        pc = stop_w > 0 ? hg_prev_ctx(txt[stop_w - 1]) : ((hdr & HG_FLOW_HELD) ? HG_PC_NL : (hdr & HG_FLOW_PC));
        acc_done = stop_w == 0 && !(hdr & HG_FLOW_HELD) && (hdr & HG_FLOW_ACC_DONE);
      }
      hdr = hg_flow_finish(pool, pat, S.data(), pc, hdr, stop, held, acc_done, close, &em, emit_abs);
      if (pat.single && em) hdr = (hdr & HG_FLOW_HOLD) | HG_FLOW_DEAD;
    }
  }
  return static_cast<long>(n);
}

// Face A's report rules (hg_flow_rules.h) over the raw ends of flowsim_run (raw[3 k] = call, expression, stream offset)
// for the same cuts.  out[3 k] = call, id, to (per call in delivery order).
long flowsim_deliver(void *h, const uint32_t *raw, size_t nraw, uint32_t len, const uint32_t *cuts, uint32_t ncuts, uint32_t *out, size_t cap) {
  const HgDb &db = *static_cast<HgDb *>(h);
  HgFlowRuleState st;
  std::vector<HgFlowRep> reps;
  size_t n = 0;
  for (uint32_t call = 0; call <= ncuts + 1; call++) {
    const uint32_t a = call == 0 ? 0 : (call <= ncuts ? cuts[call - 1] : len);
    const uint32_t b = call < ncuts ? cuts[call] : len;
    const uint32_t wlen = call == ncuts + 1 ? 0 : b - a;
    std::vector<std::pair<uint32_t, uint32_t>> mine;
    for (size_t k = 0; k < nraw; k++)
      if (raw[3 * k] == call) mine.emplace_back(raw[3 * k + 1], raw[3 * k + 2] - a + 1);
    hg_flow_rules(db.patterns.data(), db.bounds.empty() ? nullptr : db.bounds.data(), st, wlen, mine.data(), mine.size(), reps);
    for (const HgFlowRep &x : reps) {
      if (n < cap) out[3 * n] = call, out[3 * n + 1] = x.id, out[3 * n + 2] = static_cast<uint32_t>(x.to);
      n++;
    }
  }
  return static_cast<long>(n);
}

}  // extern "C"
