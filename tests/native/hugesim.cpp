// TEST-ONLY placement accessor of the huge automata (never shipped): for a compiled set, what decides the routine of
// hg_huge.hip each huge expression runs in (huge_prepare: the staged-table need against the staging cap, and nw against the 256
// words of the register-resident routine), and the shape of its exception edges (sources, target ranges, whether a target lies
// below its source, whether a range crosses a slab of 64 words).  It labels test cells and asserts placement: it never produces
// an expected hit.  Compiled together with hostsim.cpp for hgsim_compile / hgsim_free.
#include "hostsim.cpp"

namespace {
constexpr uint32_t HUGE_WORDS = 16;
}

extern "C" {

// head[0..3] = huge_max_nw, huge_stage_words, nhuge, nslow_huge.  Returns the number of huge expressions and fills
// min(that, cap) records of HUGE_WORDS words:
//   0 expression index   1 tier   2 confirm mode   3 nw   4 ncls   5 ctxfree   6 init_hi   7 exception sources   8 target ranges
//   9 widest range in words   10 some target word lies below its source's word   11 some range crosses a multiple of 64 words
//   12 single   13 highest target word   14 nnodes
uint32_t hugesim_exprs(void *h, uint32_t *head, uint32_t *out, uint32_t cap) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const uint32_t *pool = db->pool.data();
  head[0] = db->huge_max_nw;
  head[1] = db->huge_stage_words;
  head[2] = db->nhuge;
  head[3] = db->nslow_huge;
  uint32_t n = 0;
  for (uint32_t pi = 0; pi < db->patterns.size(); pi++) {
    const HgPattern &p = db->patterns[pi];
    if (p.nw <= HG_MAX_W) continue;
    if (n < cap) {
      uint32_t *o = out + static_cast<size_t>(n) * HUGE_WORDS;
      std::fill(o, o + HUGE_WORDS, 0u);
      const HgHugeHeader *hd = reinterpret_cast<const HgHugeHeader *>(pool + p.follow_off);
      const HgHugeView v = hg_huge_view(pool, p);
      o[0] = pi;
      o[1] = p.tier;
      o[2] = hg_confirm_mode(p);
      o[3] = p.nw;
      o[4] = v.ncls;
      o[5] = v.ctxfree;
      o[6] = v.init_hi;
      o[7] = hd->nsources;
      o[8] = hd->nranges;
      o[12] = p.single;
      o[14] = p.nnodes;
      for (uint32_t w = 0; w < p.nw; w++)
        for (uint32_t x = v.xsrc[w]; x; x &= x - 1) {
          const uint32_t k = v.xrank[w] + hg_popc(v.xsrc[w] & ((1u << hg_ctz(x)) - 1u));
          for (uint32_t r = v.xlist[k]; r < v.xlist[k + 1]; r++) {
            const uint32_t w0 = v.xt[2 * r] >> 5, w1 = v.xt[2 * r + 1] >> 5;
            o[9] = std::max(o[9], w1 - w0 + 1u);
            if (w0 < w) o[10] = 1;
            if ((w0 >> 6) != (w1 >> 6)) o[11] = 1;
            o[13] = std::max(o[13], w1);
          }
        }
    }
    n++;
  }
  return n;
}

}  // extern "C"
