// TEST-ONLY placement accessor of the always-on tier (never shipped): for a compiled set, the units of
// hg_always_on_fast_kernel in kernel order (the groups, then the other entries of the fast part of the always-on list), then
// the entries of the scalar kernel, each with what decides the routine it runs in.  One half of that is in HgDb (slow order,
// nslow_fast, nslow_grouped, groups, simple / nw / nnodes / max_len / single); the other half the device computes from the
// tables when it stages a unit, and is replicated here.  The replica labels test cells and asserts placement: it never
// produces an expected hit.  Compiled together with hostsim.cpp for hgsim_compile / hgsim_free.
#include "hostsim.cpp"

namespace {

constexpr uint32_t AO_UNIT_WORDS = 40;
constexpr uint32_t AO_NONE = 0xFFFFFFFFu;

struct Shift64 {
  uint64_t M[4] = {0, 0, 0, 0}, F[2] = {0, 0};
  uint32_t nexc = 0, src[2] = {0, 0};
};

// One state word.  Mirrors always_on_stage (hg_always_on.hip), "the shift form of the follow step, if the unit has one":
// the block `if (tid == 0) { uint32_t M[4] ... tab[CT_SHIFT + 7] = F[1]; }`.
Shift64 shift_one_word(const uint32_t *follow, uint32_t nnodes) {
  Shift64 s;
  for (uint32_t i = 0; i < nnodes; i++) {
    uint32_t f = follow[i];
    for (uint32_t k = 0; k < 4 && i + k < 32; k++)
      if (f >> (i + k) & 1u) {
        s.M[k] |= 1u << i;
        f &= ~(1u << (i + k));
      }
    if (f) {
      if (s.nexc < 2) { s.src[s.nexc] = i; s.F[s.nexc] = f; }
      s.nexc++;
    }
  }
  return s;
}

// Two state words.  Mirrors always_on_stage, the `if (!one_word)` block: the loop over the nodes that fills M0..M3, F0, F1.
Shift64 shift_two_words(const uint32_t *follow, uint32_t nnodes) {
  Shift64 s;
  for (uint32_t i = 0; i < nnodes; i++) {
    uint64_t f = follow[2 * i] | (static_cast<uint64_t>(follow[2 * i + 1]) << 32);
    const uint64_t self = 1ull << i;
    if (f & self) { s.M[0] |= self; f &= ~self; }
    if (i + 1 < 64 && (f >> (i + 1) & 1ull)) { s.M[1] |= self; f &= ~(1ull << (i + 1)); }
    if (i + 2 < 64 && (f >> (i + 2) & 1ull)) { s.M[2] |= self; f &= ~(1ull << (i + 2)); }
    if (i + 3 < 64 && (f >> (i + 3) & 1ull)) { s.M[3] |= self; f &= ~(1ull << (i + 3)); }
    if (f) {
      if (s.nexc == 0) { s.src[0] = i; s.F[0] = f; }
      if (s.nexc == 1) { s.src[1] = i; s.F[1] = f; }
      s.nexc++;
    }
  }
  return s;
}

void put_shift(uint32_t *o, const Shift64 &s) {
  o[14] = s.nexc;
  o[15] = (s.M[0] ? 1u : 0u) | (s.M[1] ? 2u : 0u) | (s.M[2] ? 4u : 0u) | (s.M[3] ? 8u : 0u);
  o[16] = s.nexc > 0 ? s.src[0] : AO_NONE;
  o[17] = s.nexc > 1 ? s.src[1] : AO_NONE;
  for (uint32_t k = 0; k < 4; k++) {
    o[24 + 2 * k] = static_cast<uint32_t>(s.M[k]);
    o[25 + 2 * k] = static_cast<uint32_t>(s.M[k] >> 32);
  }
  for (uint32_t k = 0; k < 2; k++) {
    o[32 + 2 * k] = static_cast<uint32_t>(s.F[k]);
    o[33 + 2 * k] = static_cast<uint32_t>(s.F[k] >> 32);
  }
}

}  // namespace

extern "C" {

// out[0..3] = ngroups, nslow_fast, nslow_grouped, entries of the always-on list.  Returns the number of units and fills
// min(units, cap) records of AO_UNIT_WORDS words:
//   0 kind (0 group, 1 single of the fast kernel, 2 scalar kernel, 3 huge)   1 nmembers   2..9 members (expression indices)
//   10 ctx   11 state words   12 nnodes   13 nt   14 exception nodes (raw count)   15 bit k: Mk != 0   16, 17 exception sources
//   18 max_len (0 = unbounded)   19 nl_accepts != 0   20 two words: lean-eligible   21 single_mask   22 one word: shift form taken
//   24..31 M0..M3 (lo, hi)   32..35 F0, F1 (lo, hi)
uint32_t aosim_units(void *h, uint32_t *head, uint32_t *out, uint32_t cap) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const uint32_t *pool = db->pool.data();
  const uint32_t ngroups = static_cast<uint32_t>(db->groups.size());
  head[0] = ngroups;
  head[1] = db->nslow_fast;
  head[2] = db->nslow_grouped;
  head[3] = static_cast<uint32_t>(db->slow.size());
  const uint32_t nfast_units = ngroups + (db->nslow_fast - db->nslow_grouped);  // nunits of hg_always_on_fast_kernel
  const uint32_t nunits = nfast_units + (head[3] - db->nslow_fast);
  for (uint32_t u = 0; u < nunits && u < cap; u++) {
    uint32_t *o = out + static_cast<size_t>(u) * AO_UNIT_WORDS;
    std::fill(o, o + AO_UNIT_WORDS, 0u);
    o[16] = o[17] = AO_NONE;
    if (u < ngroups) {  // always_on_stage: `if (u < ngroups)`
      const HgSlowGroup &g = db->groups[u];
      o[0] = 0;
      o[1] = g.nmembers;
      for (uint32_t m = 0; m < g.nmembers; m++) o[2 + m] = g.member[m];
      o[10] = g.ctx_off != 0;
      o[11] = 1;
      o[12] = g.nnodes;
      o[13] = (g.nnodes + 7u) >> 3;
      o[18] = g.max_len;
      o[21] = g.single_mask;
      const Shift64 s = shift_one_word(pool + g.follow_off, g.nnodes);
      put_shift(o, s);
      o[22] = o[13] >= 2 && s.nexc <= 2;  // hg_always_on_fast_kernel: shift_form
      // CT_NL_ACCEPTS: reach['\n'] & acc_all, or with conditions & acc[HG_PC_NL][HG_NC_END]
      o[19] = (pool[g.reach_off + '\n'] & (g.ctx_off ? pool[g.ctx_off + 16 + HG_PC_NL * 5 + HG_NC_END] : g.acc_all)) != 0;
      continue;
    }
    const uint32_t j = u < nfast_units ? db->nslow_grouped + (u - ngroups) : db->nslow_fast + (u - nfast_units);
    const uint32_t pi = db->slow[j];
    const HgPattern &p = db->patterns[pi];
    o[1] = 1;
    o[2] = pi;
    o[10] = !p.simple;
    o[11] = p.nw;
    o[12] = p.nnodes;
    o[18] = p.max_len;
    o[21] = p.single ? 1u : 0u;
    if (u >= nfast_units) {
      o[0] = p.nw > HG_MAX_W ? 3u : 2u;
      continue;
    }
    o[0] = 1;
    if (p.simple || p.nw == 1) {
      o[11] = 1;
      o[13] = (p.nnodes + 7u) >> 3;
      const Shift64 s = shift_one_word(pool + p.follow_off, p.nnodes);
      put_shift(o, s);
      o[22] = o[13] >= 2 && s.nexc <= 2;
      o[19] = (pool[p.reach_off + '\n'] & (p.simple ? p.acc_all : pool[p.acc_off + HG_PC_NL * 5 + HG_NC_END])) != 0;
    } else {  // two words: always_on_stage, `if (!one_word)`
      const uint32_t *am = pool + p.amask_off, *ac = pool + p.acc_off, *reach = pool + p.reach_off;
      bool same = true;
      for (uint32_t k = 1; k < 16; k++) same = same && am[2 * k] == am[0] && am[2 * k + 1] == am[1];
      for (uint32_t k = 1; k < 20; k++) same = same && ac[2 * k] == ac[0] && ac[2 * k + 1] == ac[1];
      const uint32_t nl0 = reach[2 * '\n'] & am[0] & ac[0], nl1 = reach[2 * '\n' + 1] & am[1] & ac[1];
      const Shift64 s = shift_two_words(pool + p.follow_off, p.nnodes);
      put_shift(o, s);
      o[10] = !same;
      o[19] = (nl0 | nl1) != 0;
      o[20] = same && !(nl0 | nl1) && s.nexc <= 2;
    }
  }
  return nunits;
}

}  // extern "C"
