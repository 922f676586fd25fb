// Matched parts (hg_scan_device_parts, grep -o): the scalar reference routines of the parts stage (hg_parts.hip).  The host
// tests replay them (tests/native/partssim.cpp); the gfx950 kernels call the same anchored walk, a candidate start per lane.
//
// Expression p matches exactly [s, e) of a piece's scanned bytes data[0, len) if it has a match spanning those bytes with
// every assertion evaluated in the real context (the byte before s or the piece start, the byte at e or the piece end): the
// notion of hg_som.h.  The parts of a piece are GNU grep's -o rule over all expressions at once: from a cursor, the smallest
// start s >= cursor at which any expression matches exactly some [s, e), the largest such e over all expressions, the lowest
// expression that matches exactly [s, that e); the cursor moves to e.  HS_FLAG_SINGLEMATCH and HS_FLAG_SOM_LEFTMOST do not
// enter: they govern reports.
//
// The walk is the forward step of hg_nfa_scan, S' = (init | follow(S)) & reach[c] & amask[prev ctx][own ctx], ANCHORED: init
// enters at byte s only, so the state holds the matches that start at s and nothing else; it runs until the state is empty
// or the piece ends and keeps the last position at which an accepting node was live.  Only dense automata (nw <= HG_MAX_W):
// the engine refuses the stage for a database with a huge one.
#pragma once
#include "hg_core.h"
#include "hg_som.h"

struct HgPart {
  uint64_t line_no;  // the piece: hg_hit_t.line_number of its hits
  uint32_t from;     // [from, to) inside the scanned bytes, the origin of hg_hit_t.to
  uint32_t to;
};
static_assert(sizeof(HgPart) == 16, "HgPart layout");

// Walk state in an array (the host replay; the kernels keep one or two words in registers and more in LDS: hg_parts.hip).
struct HgPartsArrayState {
  uint32_t r[HG_MAX_W], t[HG_MAX_W];
  uint32_t n;
  HG_HD uint32_t nw() const { return n; }
  HG_HD uint32_t &R(uint32_t w) { return r[w]; }
  HG_HD uint32_t &T(uint32_t w) { return t[w]; }
};

// The largest e such that expression p matches exactly [s, e) of data[0, len), 0 if it matches nothing that starts at s
// (s < len).  c0 = data[s], pc0 = the context of the byte before s (HG_PC_START at the piece start): the caller has them
// for every expression it tries at s.  `simple` expressions (one word, no conditions) take the form without masks.
// (HG_PARTS_UNROLL: the word loops carry independent loads; unrolled by four a multi-word step keeps four of them in flight)
#if defined(__clang__)
#define HG_PARTS_UNROLL _Pragma("unroll 4")
#else
#define HG_PARTS_UNROLL
#endif
template <typename St>
HG_HD uint32_t hg_parts_walk(const uint32_t *pool, const HgPattern &p, const uint8_t *data, uint32_t len, uint32_t s, uint32_t c0, uint32_t pc0, St &st) {
  const uint32_t *reach = pool + p.reach_off, *follow = pool + p.follow_off;
  if (p.simple) {
    uint32_t S = p.init_word & reach[c0], best = 0;
    for (uint32_t i = s + 1; S; i++) {
      if (S & p.acc_all) best = i;
      if (i == len) break;
      uint32_t T = 0;
      for (uint32_t x = S; x; x &= x - 1) T |= follow[hg_ctz(x)];
      S = T & reach[data[i]];
    }
    return best;
  }
  const uint32_t nw = st.nw();
  const uint32_t *init = pool + p.init_off, *amask = pool + p.amask_off, *acc = pool + p.acc_off;
  uint32_t any = 0;
  {
    const uint32_t *r = reach + c0 * nw, *m = amask + (pc0 * 4 + hg_own_ctx(c0, s + 1 == len)) * nw;
    for (uint32_t w = 0; w < nw; w++) {
      const uint32_t x = init[w] & r[w] & m[w];
      st.R(w) = x;
      any |= x;
    }
  }
  uint32_t best = 0, pc = hg_prev_ctx(c0);
  for (uint32_t i = s + 1; any; i++) {
    // the state has consumed data[s, i): accept against the context of the byte at i
    const uint32_t c = i < len ? data[i] : 0u;
    const uint32_t nc = i == len ? static_cast<uint32_t>(HG_NC_END) : hg_own_ctx(c, i + 1 == len);
    const uint32_t *a = acc + (pc * 5 + nc) * nw;
    uint32_t hit = 0;
    HG_PARTS_UNROLL
    for (uint32_t w = 0; w < nw; w++) hit |= st.R(w) & a[w];
    if (hit) best = i;
    if (i == len) break;
    for (uint32_t w = 0; w < nw; w++) st.T(w) = 0;
    for (uint32_t w = 0; w < nw; w++)
      for (uint32_t x = st.R(w); x; x &= x - 1) {
        const uint32_t *f = follow + (w * 32 + hg_ctz(x)) * nw;
        HG_PARTS_UNROLL
        for (uint32_t k = 0; k < nw; k++) st.T(k) |= f[k];
      }
    const uint32_t *r = reach + c * nw, *m = amask + (pc * 4 + nc) * nw;
    any = 0;
    HG_PARTS_UNROLL
    for (uint32_t w = 0; w < nw; w++) {
      const uint32_t x = st.T(w) & r[w] & m[w];
      st.R(w) = x;
      any |= x;
    }
    pc = hg_prev_ctx(c);
  }
  return best;
}

// The part that starts at s, if any: *to = the largest end over the n expressions, *pattern = the lowest expression that
// reaches it.  False when no expression matches anything that starts at s.
HG_HD bool hg_parts_at(const uint32_t *pool, const HgPattern *patterns, uint32_t n, const uint8_t *data, uint32_t len, uint32_t s, uint32_t *to, uint32_t *pattern) {
  const uint32_t c0 = data[s], pc0 = s ? hg_prev_ctx(data[s - 1]) : static_cast<uint32_t>(HG_PC_START);
  uint32_t best = 0, who = 0;
  HgPartsArrayState st;
  for (uint32_t j = 0; j < n; j++) {
    const HgPattern &p = patterns[j];
    if (p.nw == 0 || p.nw > HG_MAX_W) continue;  // (no dense tables: the engine refuses such databases)
    st.n = p.nw;
    const uint32_t e = hg_parts_walk(pool, p, data, len, s, c0, pc0, st);
    if (e > best) {
      best = e;
      who = j;
    }
  }
  *to = best;
  *pattern = who;
  return best != 0;
}

// The next part of the piece data[0, len) at or behind `cursor`: false when there is none.  The parts of a piece are the
// results of calling this with cursor = 0 and then each part's `to`.
HG_HD bool hg_parts_next(const uint32_t *pool, const HgPattern *patterns, uint32_t n, const uint8_t *data, uint32_t len, uint32_t cursor, uint32_t *from, uint32_t *to,
                         uint32_t *pattern) {
  for (uint32_t s = cursor; s < len; s++)
    if (hg_parts_at(pool, patterns, n, data, len, s, to, pattern)) {
      *from = s;
      return true;
    }
  return false;
}

// Why the stage is not offered for a database, nullptr when it is (the contract in include/hypergrep_amd.h).
inline const char *hg_parts_refusal(uint32_t nhuge, uint32_t ncomb, uint32_t nquiet, bool any_ext) {
  if (nhuge) return "matched parts are not offered for a database with an automaton above HG_MAX_NODES nodes (no dense tables to walk)";
  if (ncomb) return "matched parts are not offered for a database with HS_FLAG_COMBINATION expressions (a combination has no match span)";
  if (nquiet) return "matched parts are not offered for a database with HS_FLAG_QUIET expressions";
  if (any_ext) return "matched parts are not offered for a database with extended parameters (hs_expr_ext_t: distances, offset bounds, min_length)";
  return nullptr;
}
