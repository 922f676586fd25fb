// Start of match (HS_FLAG_SOM_LEFTMOST) and match length (hs_expr_ext_t min_length): the scalar reference routines of the
// start-of-match pass and the match-length pass (hg_som.hip).  The host tests replay them (tests/native/somsim.cpp,
// tests/native/minlensim.cpp); the gfx950 kernels compute the same values with the text read in 16-byte chunks.
//
// A report (id, to) of a SOM expression gets from = the smallest s such that the expression has a match spanning [s, to)
// of the piece's scanned bytes, with every assertion evaluated in the real context (the byte before s, or the piece start).
// The forward automaton's step S' = (init | follow(S)) & reach[c] & amask[prev ctx][own ctx] runs backwards over the same
// nodes: start from the nodes that accept at `to`, step with the transposed follow table (HgPattern::som_follow_off), and
// every position p where the state meets `init` (entry condition of p's node checked against the byte before p) is the
// start of a match that ends at `to`.  The last such p before the state dies is the leftmost.
#pragma once
#include "hg_core.h"

// context of byte c at a position of a piece as the byte a node consumes (the next-context classes of hg_db.h)
HG_HD uint32_t hg_own_ctx(uint32_t c, bool last) { return c == '\n' ? (last ? HG_NC_NLFINAL : HG_NC_NL) : (hg_is_word(c) ? HG_NC_WORD : HG_NC_OTHER); }

// The leftmost start of a match of expression p that ends at `to` (0 < to <= len) in the scanned bytes data[0, len), or
// HG_NONE32 when no match of p ends there.  The walk stops when the state is empty, at offset 0, or max_len bytes before `to`.
HG_HD uint32_t hg_nfa_som(const uint32_t *pool, const HgPattern &p, const uint8_t *data, uint32_t len, uint32_t to) {
  const uint32_t nw = p.nw;
  if (nw > HG_MAX_W || to == 0 || to > len) return HG_NONE32;  // (huge automata carry no reverse tables: the compiler rejects SOM on them)
  const uint32_t *reach = pool + p.reach_off, *rfollow = pool + p.som_follow_off, *init = pool + p.init_off;
  const uint32_t *amask = pool + p.amask_off, *acc = pool + p.acc_off;
  const uint32_t lo = (p.max_len && to > p.max_len) ? to - p.max_len : 0u;
  const uint32_t nc = to == len ? static_cast<uint32_t>(HG_NC_END) : hg_own_ctx(data[to], to + 1 == len);
  const uint32_t *a = acc + (hg_prev_ctx(data[to - 1]) * 5 + nc) * nw;
  uint32_t R[HG_MAX_W], T[HG_MAX_W];
  for (uint32_t w = 0; w < nw; w++) R[w] = a[w];
  uint32_t best = HG_NONE32;
  for (uint32_t q = to; q-- > lo;) {
    const uint32_t c = data[q];
    const uint32_t cc = hg_own_ctx(c, q + 1 == len), pc = q ? hg_prev_ctx(data[q - 1]) : static_cast<uint32_t>(HG_PC_START);
    const uint32_t *r = reach + c * nw, *m = amask + (pc * 4 + cc) * nw;
    uint32_t any = 0, start = 0;
    for (uint32_t w = 0; w < nw; w++) {
      R[w] &= r[w] & m[w];
      any |= R[w];
      start |= R[w] & init[w];
    }
    if (!any) break;
    if (start) best = q;
    if (q == lo) break;
    for (uint32_t w = 0; w < nw; w++) T[w] = 0;
    for (uint32_t w = 0; w < nw; w++)
      for (uint32_t x = R[w]; x; x &= x - 1) {
        const uint32_t *f = rfollow + (w * 32 + hg_ctz(x)) * nw;
        for (uint32_t k = 0; k < nw; k++) T[k] |= f[k];
      }
    for (uint32_t w = 0; w < nw; w++) R[w] = T[w];
  }
  return best;
}

// min_length (hs_expr_ext_t): does expression p have a match of at least min_len bytes that ends at `to` in the scanned bytes
// data[0, len)?  The walk of hg_nfa_som with two early exits: false at once when `to` is below min_len (no such match fits),
// true at the first start q <= to - min_len (the walk meets starts from the right, so the leftmost start, which is what
// decides, is at most that one).  It stops when the state is empty or max_len bytes before `to`, as hg_nfa_som does.  The
// match-length pass (hg_som.hip, hg_minlen_kernel) computes the same for every raw report of a filtering expression.
HG_HD bool hg_nfa_minlen(const uint32_t *pool, const HgPattern &p, const uint8_t *data, uint32_t len, uint32_t to, uint32_t min_len) {
  const uint32_t nw = p.nw;
  if (nw > HG_MAX_W || to == 0 || to > len || to < min_len) return false;
  const uint32_t *reach = pool + p.reach_off, *rfollow = pool + p.som_follow_off, *init = pool + p.init_off;
  const uint32_t *amask = pool + p.amask_off, *acc = pool + p.acc_off;
  const uint32_t lo = (p.max_len && to > p.max_len) ? to - p.max_len : 0u;
  const uint32_t nc = to == len ? static_cast<uint32_t>(HG_NC_END) : hg_own_ctx(data[to], to + 1 == len);
  const uint32_t *a = acc + (hg_prev_ctx(data[to - 1]) * 5 + nc) * nw;
  uint32_t R[HG_MAX_W], T[HG_MAX_W];
  for (uint32_t w = 0; w < nw; w++) R[w] = a[w];
  for (uint32_t q = to; q-- > lo;) {
    const uint32_t c = data[q];
    const uint32_t cc = hg_own_ctx(c, q + 1 == len), pc = q ? hg_prev_ctx(data[q - 1]) : static_cast<uint32_t>(HG_PC_START);
    const uint32_t *r = reach + c * nw, *m = amask + (pc * 4 + cc) * nw;
    uint32_t any = 0, start = 0;
    for (uint32_t w = 0; w < nw; w++) {
      R[w] &= r[w] & m[w];
      any |= R[w];
      start |= R[w] & init[w];
    }
    if (!any) break;
    if (start && q <= to - min_len) return true;
    if (q == lo) break;
    for (uint32_t w = 0; w < nw; w++) T[w] = 0;
    for (uint32_t w = 0; w < nw; w++)
      for (uint32_t x = R[w]; x; x &= x - 1) {
        const uint32_t *f = rfollow + (w * 32 + hg_ctz(x)) * nw;
        for (uint32_t k = 0; k < nw; k++) T[k] |= f[k];
      }
    for (uint32_t w = 0; w < nw; w++) R[w] = T[w];
  }
  return false;
}

// `from` of one final report: hit (id, to) of expression `pattern` in the piece data[0, len).  0 for expressions without the
// flag; otherwise the smallest start over the SOM expressions that share the report's id (the som_next cycle: the report
// rules deliver an identical (id, to) once, whichever of them produced it).  A literal-only expression alone on its id needs
// no walk: its only match ending at `to` is its literal.  min_lengths (HgDb::min_lengths, or nullptr): an expression of the
// cycle counts only if its own report at `to` survives its min_length, i.e. its leftmost start s has to - s >= min_length
// (the delivered report's own expression does: the pass has kept it).
HG_HD uint32_t hg_hit_som(const uint32_t *pool, const HgPattern *patterns, uint32_t pattern, const uint8_t *data, uint32_t len, uint32_t to,
                          const uint32_t *min_lengths = nullptr) {
  const HgPattern &p = patterns[pattern];
  if (!(p.flags & HG_FLAG_SOM_LEFTMOST)) return 0;
  if (p.som_next == pattern && p.literal_only && p.max_len && p.max_len <= to) return to - p.max_len;
  uint32_t best = HG_NONE32, j = pattern;
  do {
    const uint32_t s = hg_nfa_som(pool, patterns[j], data, len, to);
    const uint32_t need = min_lengths ? min_lengths[j] : 0u;
    if (s != HG_NONE32 && to - s >= need) best = s < best ? s : best;
    j = patterns[j].som_next;
  } while (j != pattern);
  return best;
}
