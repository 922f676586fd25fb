// TEST-ONLY host harness for the start-of-match pass (never shipped): compiles the product's pattern compiler, the forward
// scalar routine of hg_core.h (hg_nfa_scan) and the start-of-match reference of hg_som.h (hg_hit_som) for x86.  One call
// scans one trimmed line piece with every expression, applies the report rules and gives each report its `from`, which is
// what the GPU pass (hg_som.hip) must reproduce.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_som.h"

extern "C" {

void *somsim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, unsigned n, char *err, size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  if (hgc_compile(exprs, flags, ids, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
void somsim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// pool words and {nsom, tier of expression 0, nw of expression 0, literal_only of expression 0}
uint64_t somsim_info(void *h, uint32_t *out) {
  const HgDb *db = static_cast<const HgDb *>(h);
  out[0] = db->nsom;
  out[1] = db->patterns[0].tier;
  out[2] = db->patterns[0].nw;
  out[3] = db->patterns[0].literal_only;
  return db->pool.size();
}

// The reports of one piece data[0, len) in (id, to) order: SINGLEMATCH expressions sharing an id give one report (the smallest
// end), the others every distinct end, an identical (id, to) once.  out: {id, to, from, pattern} per report.  Returns the count.
long somsim_piece(void *h, const uint8_t *data, uint32_t len, uint32_t *out, size_t cap) {
  const HgDb *db = static_cast<const HgDb *>(h);
  struct Rec { uint32_t id, to, single, pattern; };
  std::vector<Rec> recs;
  for (uint32_t i = 0; i < db->patterns.size(); i++) {
    const HgPattern &p = db->patterns[i];
    hg_nfa_scan(db->pool.data(), p, data, len, [&](uint32_t to) { recs.push_back({p.id, to, p.single, i}); });
  }
  std::sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) {
    if (a.id != b.id) return a.id < b.id;
    if (a.to != b.to) return a.to < b.to;
    return a.single < b.single;
  });
  size_t n = 0;
  bool seen_single = false;
  for (size_t i = 0; i < recs.size(); i++) {
    if (i == 0 || recs[i].id != recs[i - 1].id) seen_single = false;
    const bool dup = i > 0 && recs[i].id == recs[i - 1].id && recs[i].to == recs[i - 1].to;
    const bool keep = !dup && !(recs[i].single && seen_single);
    if (recs[i].single) seen_single = true;
    if (!keep) continue;
    if (n >= cap) return -1;
    out[4 * n] = recs[i].id;
    out[4 * n + 1] = recs[i].to;
    out[4 * n + 2] = hg_hit_som(db->pool.data(), db->patterns.data(), recs[i].pattern, data, len, recs[i].to);
    out[4 * n + 3] = recs[i].pattern;
    n++;
  }
  return static_cast<long>(n);
}

// hg_hit_som for one given (expression, to): what the GPU pass computes for a hit record
uint32_t somsim_start(void *h, uint32_t pattern, const uint8_t *data, uint32_t len, uint32_t to) {
  const HgDb *db = static_cast<const HgDb *>(h);
  return hg_hit_som(db->pool.data(), db->patterns.data(), pattern, data, len, to);
}

}  // extern "C"
