// Logical combinations (HS_FLAG_COMBINATION, HS_FLAG_QUIET): the scalar routines of the combination pass (hg_comb.hip).
// The host tests replay them (tests/native/combsim.cpp); the gfx950 kernel calls the same functions.
//
// The rules are per line piece, on the piece's reports after the report rules (hg_post.h): ordered by (id, to), an identical
// (id, to) once, a SINGLEMATCH id with its first end only.
//  * The status of operand id X at offset t is true iff X has a report in the piece with to <= t.
//  * A combination C reports (C.id, t) at every t where one of its operands reports, if its formula is true with the
//    statuses at t (all reports at offsets <= t applied first: `1 & !2` with both ending at 10 does not report).
//  * Reports of QUIET expressions count as operand events but are not delivered.
//  * The combination reports join the delivered ones under the report rules (ordering, duplicates, SINGLEMATCH).
// Because a status only depends on the FIRST `to` of its id in the piece (the head of the id's run in (id, to) order), the
// value of C at t takes one binary search per operand: the per-report cost is O(operands * log reports of the piece).
#pragma once
#include "hg_core.h"

// The formula's value for operand statuses `status` (bit s: slot s is true).  The stack is a 64-bit mask, top in bit 0:
// the compiler orders the program so that it never holds more than 64 values (hg_compile.cpp).
HG_HD bool hg_comb_eval(const uint32_t *prog, uint32_t len, uint64_t status) {
  uint64_t st = 0;
  for (uint32_t k = 0; k < len; k++) {
    const uint32_t op = prog[k];
    if (op < HG_COMB_NOT) {
      st = (st << 1) | ((status >> op) & 1u);
    } else if (op == HG_COMB_NOT) {
      st ^= 1u;
    } else {
      const uint64_t a = st & 1u, b = (st >> 1) & 1u;
      st = ((st >> 2) << 1) | (op == HG_COMB_AND ? (a & b) : (a | b));
    }
  }
  return (st & 1u) != 0;
}

// True with nothing matched: Hyperscan reports such a combination at the end of the data, which this project does not do
// (the compiler rejects it).
HG_HD bool hg_comb_true_when_empty(const HgComb &c, const uint32_t *words) { return hg_comb_eval(words + c.prog_off, c.prog_len, 0); }

// hits[lo, hi): one piece's reports in (id, to) order.  The first `to` of report id `id` among them, HG_NONE32 if it has none.
HG_HD uint32_t hg_comb_first_to(const HgHit *hits, uint64_t lo, uint64_t hi, uint32_t id) {
  uint64_t a = lo, b = hi;
  while (a < b) {
    const uint64_t m = a + ((b - a) >> 1);
    if (hits[m].id < id) a = m + 1;
    else b = m;
  }
  return a < hi && hits[a].id == id ? hits[a].to : HG_NONE32;
}

// [first, last) of the combinations report id `id` feeds (feed: nfeed ids in ascending order, then nfeed combination indices)
HG_HD void hg_comb_feed_range(const uint32_t *feed, uint32_t nfeed, uint32_t id, uint32_t *first, uint32_t *last) {
  uint32_t a = 0, b = nfeed;
  while (a < b) {
    const uint32_t m = (a + b) >> 1;
    if (feed[m] < id) a = m + 1;
    else b = m;
  }
  uint32_t e = a;
  while (e < nfeed && feed[e] == id) e++;
  *first = a;
  *last = e;
}

// Combination c at offset t, for the piece hits[lo, hi)
HG_HD bool hg_comb_at(const HgComb &c, const uint32_t *words, const HgHit *hits, uint64_t lo, uint64_t hi, uint32_t t) {
  uint64_t status = 0;
  for (uint32_t s = 0; s < c.nops; s++) {
    const uint32_t f = hg_comb_first_to(hits, lo, hi, words[c.ops_off + s]);
    if (f <= t) status |= 1ull << s;  // (HG_NONE32 > every `to`: a piece is at most an int)
  }
  return hg_comb_eval(words + c.prog_off, c.prog_len, status);
}

// The records report i of the piece hits[lo, hi) (i in [lo, hi)) hands to the finalize: itself unless its expression is
// QUIET, then one report (C.id, to) of each combination C its id feeds that is true at its `to`.  emit(id, pattern) per
// record; returns their number.  Reports of several operands at the same `to` give C's report more than once: the report
// rules deliver it once.
template <typename Emit>
HG_HD uint32_t hg_comb_hit(const HgComb *combs, const uint32_t *words, const uint32_t *feed, uint32_t nfeed, const HgHit *hits, uint64_t lo, uint64_t hi,
                           uint64_t i, bool quiet, Emit &&emit) {
  const HgHit h = hits[i];
  uint32_t n = 0;
  if (!quiet) {
    emit(h.id, HG_NONE32);
    n++;
  }
  uint32_t first = 0, last = 0;
  hg_comb_feed_range(feed, nfeed, h.id, &first, &last);
  for (uint32_t k = first; k < last; k++) {
    const HgComb &c = combs[feed[nfeed + k]];
    if (!hg_comb_at(c, words, hits, lo, hi, h.to)) continue;
    emit(c.id, c.pattern);
    n++;
  }
  return n;
}
