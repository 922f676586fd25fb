// TEST-ONLY host harness for min_length (never shipped): compiles the product's pattern compiler (hgc_compile_ext), the
// forward scalar routine of hg_core.h (hg_nfa_scan), the match-length and start-of-match references of hg_som.h
// (hg_nfa_minlen, hg_hit_som) and the scalar routines of the combination pass (hg_comb.h) for x86.  One call scans one
// trimmed line piece with every expression in the order of the GPU passes: raw reports, offset bounds, the match-length
// filter, the report rules, the combination pass and its report rules, then `from`.  That is what the GPU must deliver.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_comb.h"
#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_post.h"
#include "../../hypergrep_amd/csrc/hg_som.h"

namespace {
struct Rec {
  HgHit h;
  uint32_t pattern;
};
// order by (id, to, single-after-multi) and apply the report rules, as the compact finalize does
std::vector<Rec> report_rules(const HgDb &db, std::vector<Rec> raw) {
  auto single = [&](const Rec &r) { return hg_report_single(db.patterns[r.pattern]); };
  std::stable_sort(raw.begin(), raw.end(), [&](const Rec &a, const Rec &b) { return hg_sort_key(a.h, single(a)) < hg_sort_key(b.h, single(b)); });
  std::vector<Rec> out;
  for (size_t i = 0; i < raw.size(); i++)
    if (hg_keep_hit_at([&](size_t j) { return raw[j].h; }, [&](size_t j) { return single(raw[j]); }, i)) out.push_back(raw[i]);
  return out;
}
}  // namespace

extern "C" {

void *minlensim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, const hs_expr_ext_t *const *ext, unsigned n, char *err,
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
void minlensim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// {expressions with a filtering min_length, nsom, pool words} and, per expression i, out[3 + 4 i ..] = {min_length, single,
// som_follow_off != 0, tier}
void minlensim_info(void *h, uint32_t *out) {
  const HgDb *db = static_cast<const HgDb *>(h);
  uint32_t nf = 0;
  for (uint32_t v : db->min_lengths) nf += v ? 1 : 0;
  out[0] = nf;
  out[1] = db->nsom;
  out[2] = static_cast<uint32_t>(db->pool.size());
  for (uint32_t i = 0; i < db->patterns.size(); i++) {
    out[3 + 4 * i] = db->min_lengths.empty() ? 0u : db->min_lengths[i];
    out[4 + 4 * i] = db->patterns[i].single;
    out[5 + 4 * i] = db->patterns[i].som_follow_off != 0;
    out[6 + 4 * i] = db->patterns[i].tier;
  }
}

// hg_nfa_minlen for one (expression, to, length)
int minlensim_long_enough(void *h, uint32_t pattern, const uint8_t *data, uint32_t len, uint32_t to, uint32_t min_len) {
  const HgDb *db = static_cast<const HgDb *>(h);
  return hg_nfa_minlen(db->pool.data(), db->patterns[pattern], data, len, to, min_len) ? 1 : 0;
}

// The delivered reports of one piece data[0, len) in (id, to) order.  out: {id, to, from, pattern} per report; *n_raw: the
// reports before the filter.  Returns the count, -1 if cap is too small.
long minlensim_piece(void *h, const uint8_t *data, uint32_t len, uint32_t *out, size_t cap, uint32_t *n_raw) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const uint32_t *ml = db->min_lengths.empty() ? nullptr : db->min_lengths.data();
  std::vector<Rec> raw;
  *n_raw = 0;
  for (uint32_t i = 0; i < db->patterns.size(); i++) {
    const HgPattern &p = db->patterns[i];
    if (p.tier == HG_TIER_COMB) continue;
    hg_nfa_scan(db->pool.data(), p, data, len, [&](uint32_t to) {
      if (!db->bounds.empty() && (to < db->bounds[2 * i] || (to > db->bounds[2 * i + 1] && db->bounds[2 * i + 1] != HG_BOUND_NONE))) return;
      ++*n_raw;
      if (ml && ml[i] && !hg_nfa_minlen(db->pool.data(), p, data, len, to, ml[i])) return;
      raw.push_back({HgHit{0, p.id, to}, i});
    });
  }
  std::vector<Rec> kept = report_rules(*db, raw);
  if (db->comb_pass()) {
    std::vector<HgHit> hits;
    for (const Rec &r : kept) hits.push_back(r.h);
    std::vector<Rec> fed;
    const uint32_t m = static_cast<uint32_t>(kept.size());
    for (uint32_t i = 0; i < m; i++) {
      const bool quiet = (db->patterns[kept[i].pattern].flags & HG_FLAG_QUIET) != 0;
      hg_comb_hit(db->combs.data(), db->comb_words.data(), db->comb_feed.data(), static_cast<uint32_t>(db->comb_feed.size() / 2), hits.data(), 0, m, i, quiet,
                  [&](uint32_t id, uint32_t pattern) { fed.push_back({HgHit{0, id, hits[i].to}, pattern != HG_NONE32 ? pattern : kept[i].pattern}); });
    }
    kept = report_rules(*db, fed);
  }
  if (kept.size() > cap) return -1;
  for (size_t i = 0; i < kept.size(); i++) {
    out[4 * i] = kept[i].h.id;
    out[4 * i + 1] = kept[i].h.to;
    out[4 * i + 2] = hg_hit_som(db->pool.data(), db->patterns.data(), kept[i].pattern, data, len, kept[i].h.to, ml);
    out[4 * i + 3] = kept[i].pattern;
  }
  return static_cast<long>(kept.size());
}

}  // extern "C"
