// TEST-ONLY host harness for extended parameters (never shipped): the whole-pipeline host replay of hostsim.cpp (hgsim_*),
// compiled together with hgc_compile_ext, so that databases with approximate expressions run through the same scalar stages
// (stream filter, confirm windows, always-on, report rules) as the plain ones.  Plus a byte-for-byte digest of a database,
// for the rule that a set without parameters compiles to the same database with or without `ext`, and a per-piece run
// of every automaton with the start-of-match reference of hg_som.h.
#include "hostsim.cpp"

#include "../../hypergrep_amd/csrc/hg_som.h"

namespace {
template <typename T>
void put_vec(std::string &s, const std::vector<T> &v) {
  const uint64_t n = v.size();
  s.append(reinterpret_cast<const char *>(&n), sizeof n);
  if (n) s.append(reinterpret_cast<const char *>(v.data()), n * sizeof(T));
}
template <typename T>
void put_one(std::string &s, const T &v) {
  s.append(reinterpret_cast<const char *>(&v), sizeof v);
}
}  // namespace

extern "C" {

// ext_mode 0: hgc_compile; 1: hgc_compile_ext with the given array (entries may be NULL); 2: hgc_compile_ext with ext == NULL
void *extsim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, const hs_expr_ext_t *const *ext, unsigned n, int ext_mode,
                     char *err, size_t errlen, int *bad) {
  HgDb *db = nullptr;
  std::string e;
  *bad = -1;
  const int rc = ext_mode == 0 ? hgc_compile(exprs, flags, ids, n, &db, &e, bad)
                               : hgc_compile_ext(exprs, flags, ids, ext_mode == 1 ? ext : nullptr, n, &db, &e, bad);
  if (rc != 0) {
    if (err && errlen) snprintf(err, errlen, "%s", e.c_str());
    return nullptr;
  }
  return db;
}

// Every table and scalar of the database that a scan reads.  Returns the size; copies min(size, cap) bytes to out.
size_t extsim_digest(void *h, uint8_t *out, size_t cap) {
  const HgDb *db = static_cast<const HgDb *>(h);
  std::string s;
  put_vec(s, db->patterns);
  put_vec(s, db->pool);
  put_vec(s, db->factors);
  put_one(s, db->nreal_factors);
  put_vec(s, db->windows);
  put_vec(s, db->bucket_off);
  put_vec(s, db->disc);
  put_vec(s, db->bucket_off2);
  put_vec(s, db->windows2);
  put_vec(s, db->wtab);
  put_one(s, db->wtab_mask);
  put_one(s, db->shared_windows);
  put_one(s, db->wtab_first);
  put_vec(s, db->filter);
  put_one(s, db->filter_log2);
  put_one(s, db->filter_wide);
  put_one(s, db->window_bytes);
  put_one(s, db->window_mask);
  put_one(s, db->weights_c);
  put_one(s, db->dense);
  put_one(s, db->weights_a);
  put_one(s, db->weights_b);
  put_vec(s, db->ext);
  put_vec(s, db->slow);
  put_one(s, db->nslow_fast);
  put_vec(s, db->groups);
  put_one(s, db->nslow_grouped);
  put_one(s, db->fold_mask);
  put_one(s, db->max_nw);
  put_one(s, db->nhuge);
  put_one(s, db->huge_max_nw);
  put_one(s, db->huge_stage_words);
  put_one(s, db->nslow_huge);
  put_one(s, db->max_id);
  put_one(s, db->nsom);
  put_one(s, db->ncomb);
  put_one(s, db->nquiet);
  put_vec(s, db->combs);
  put_vec(s, db->comb_words);
  put_vec(s, db->comb_feed);
  put_one(s, db->n_confirm_mode);
  put_vec(s, db->bounds);
  std::memcpy(out, s.data(), std::min(cap, s.size()));
  return s.size();
}

// {tier, nw, nnodes, max_len, lit_lead, literal_only, confirm mode, single, bound lo, bound hi} of expression i
void extsim_pattern(void *h, uint32_t i, uint32_t *out) {
  const HgPattern &p = static_cast<const HgDb *>(h)->patterns[i];
  out[0] = p.tier;
  out[1] = p.nw;
  out[2] = p.nnodes;
  out[3] = p.max_len;
  out[4] = p.lit_lead;
  out[5] = p.literal_only;
  out[6] = hg_confirm_mode(p);
  out[7] = p.single;
  const HgDb *db = static_cast<const HgDb *>(h);
  out[8] = db->bounds.empty() ? 0u : db->bounds[2 * i];
  out[9] = db->bounds.empty() ? HG_BOUND_NONE : db->bounds[2 * i + 1];
}

// Expression i's automaton over one trimmed piece: every end (emission-time SINGLEMATCH rule included) with its
// start-of-match (hg_nfa_som; 0 unless the expression has HS_FLAG_SOM_LEFTMOST).  out: {to, from} pairs.  Returns the count.
long extsim_nfa(void *h, uint32_t i, const uint8_t *data, uint32_t len, uint32_t *out, size_t cap) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const HgPattern &p = db->patterns[i];
  size_t n = 0;
  bool over = false;
  hg_nfa_scan(db->pool.data(), p, data, len, [&](uint32_t to) {
    if (n >= cap) { over = true; return; }
    out[2 * n] = to;
    out[2 * n + 1] = (p.flags & HG_FLAG_SOM_LEFTMOST) ? hg_nfa_som(db->pool.data(), p, data, len, to) : 0u;
    n++;
  });
  return over ? -1 : static_cast<long>(n);
}

}  // extern "C"
