// TEST-ONLY host harness for the combination pass (never shipped): compiles the product's pattern compiler and the scalar
// routines of hg_comb.h / hg_post.h for x86.  One call takes one piece's reports (after the report rules, in (id, to)
// order), hands every report to hg_comb_hit exactly as a lane of hg_comb.hip does, then orders the union and applies the
// report rules as the compact finalize does (hg_keep_hit_at): what the GPU delivers for the piece.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_comb.h"
#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_post.h"

namespace {
template <typename T>
void put(std::string &s, const std::vector<T> &v) {
  const uint64_t n = v.size();
  s.append(reinterpret_cast<const char *>(&n), sizeof n);
  if (n) s.append(reinterpret_cast<const char *>(v.data()), n * sizeof(T));
}
template <typename T>
void put1(std::string &s, const T &v) {
  s.append(reinterpret_cast<const char *>(&v), sizeof v);
}
}  // namespace

extern "C" {

void *combsim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, unsigned n, char *err, size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  if (hgc_compile(exprs, flags, ids, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
void combsim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// {ncomb, nquiet, combination records, feed pairs}
void combsim_info(void *h, uint32_t *out) {
  const HgDb *db = static_cast<const HgDb *>(h);
  out[0] = db->ncomb;
  out[1] = db->nquiet;
  out[2] = static_cast<uint32_t>(db->combs.size());
  out[3] = static_cast<uint32_t>(db->comb_feed.size() / 2);
}

// tier of expression i
uint32_t combsim_tier(void *h, uint32_t i) { return static_cast<const HgDb *>(h)->patterns[i].tier; }

// Everything the scan passes read about expressions [0, n_keep): their pattern records and all tables, filter and tier
// lists of the database (the combination tables excluded).  Returns the size; copies min(size, cap) bytes to out.
size_t combsim_digest(void *h, uint32_t n_keep, uint8_t *out, size_t cap) {
  const HgDb *db = static_cast<const HgDb *>(h);
  std::string s;
  put(s, std::vector<HgPattern>(db->patterns.begin(), db->patterns.begin() + n_keep));
  put(s, db->pool);
  put(s, db->factors);
  put(s, db->windows);
  put(s, db->bucket_off);
  put(s, db->disc);
  put(s, db->bucket_off2);
  put(s, db->windows2);
  put(s, db->wtab);
  put(s, db->filter);
  put(s, db->ext);
  put(s, db->slow);
  put(s, db->groups);
  for (uint32_t v : {db->nreal_factors, db->wtab_mask, db->shared_windows, db->wtab_first, db->filter_log2, db->filter_wide, db->window_bytes, db->window_mask,
                     db->weights_c, db->dense, db->weights_a, db->weights_b, db->nslow_fast, db->nslow_grouped, db->fold_mask, db->max_nw, db->nhuge,
                     db->huge_max_nw, db->huge_stage_words, db->nslow_huge, db->nsom})
    put1(s, v);
  for (uint32_t m = 0; m < HG_CONFIRM_MODES; m++) put1(s, db->n_confirm_mode[m]);
  std::memcpy(out, s.data(), std::min(s.size(), cap));
  return s.size();
}

// The formula of combination record k evaluated for operand statuses `status` (bit s: slot s), and its operand ids.
int combsim_eval(void *h, uint32_t k, uint64_t status) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const HgComb &c = db->combs[k];
  return hg_comb_eval(db->comb_words.data() + c.prog_off, c.prog_len, status) ? 1 : 0;
}
uint32_t combsim_operands(void *h, uint32_t k, uint32_t *ids, uint32_t *pattern) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const HgComb &c = db->combs[k];
  for (uint32_t s = 0; s < c.nops; s++) ids[s] = db->comb_words[c.ops_off + s];
  *pattern = c.pattern;
  return c.nops;
}

// One piece: in = {id, to, pattern} x m, the piece's reports after the report rules in (id, to) order.  out = the delivered
// reports {id, to, pattern}, in (id, to) order.  Returns their number, -1 if cap is too small.
long combsim_piece(void *h, const uint32_t *in, uint32_t m, uint32_t *out, size_t cap) {
  const HgDb *db = static_cast<const HgDb *>(h);
  std::vector<HgHit> hits(m);
  std::vector<uint32_t> pat(m);
  for (uint32_t i = 0; i < m; i++) {
    hits[i] = HgHit{0, in[3 * i], in[3 * i + 1]};
    pat[i] = in[3 * i + 2];
  }
  struct Rec {
    HgHit h;
    uint32_t pattern;
  };
  std::vector<Rec> raw;
  for (uint32_t i = 0; i < m; i++) {
    const bool quiet = (db->patterns[pat[i]].flags & HG_FLAG_QUIET) != 0;
    hg_comb_hit(db->combs.data(), db->comb_words.data(), db->comb_feed.data(), static_cast<uint32_t>(db->comb_feed.size() / 2), hits.data(), 0, m, i, quiet,
                [&](uint32_t id, uint32_t pattern) { raw.push_back({HgHit{0, id, hits[i].to}, pattern != HG_NONE32 ? pattern : pat[i]}); });
  }
  auto single = [&](const Rec &r) { return db->patterns[r.pattern].single; };
  std::stable_sort(raw.begin(), raw.end(), [&](const Rec &a, const Rec &b) { return hg_sort_key(a.h, single(a)) < hg_sort_key(b.h, single(b)); });
  size_t n = 0;
  for (size_t i = 0; i < raw.size(); i++) {
    if (!hg_keep_hit_at([&](size_t j) { return raw[j].h; }, [&](size_t j) { return single(raw[j]) != 0; }, i)) continue;
    if (n >= cap) return -1;
    out[3 * n] = raw[i].h.id;
    out[3 * n + 1] = raw[i].h.to;
    out[3 * n + 2] = raw[i].pattern;
    n++;
  }
  return static_cast<long>(n);
}

}  // extern "C"
