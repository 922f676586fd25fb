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

// The same with hs_expr_ext_t parameters (min_length): the handle serves every call of this file.
void *somsim_compile_ext(const char *const *exprs, const unsigned *flags, const unsigned *ids, const hs_expr_ext_t *const *ext, unsigned n, char *err,
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

// Per-expression read-out: {nw, max_len, literal_only, som_next, flags, min_length, tier, reverse tables present}
void somsim_pattern(void *h, uint32_t i, uint32_t *out) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const HgPattern &p = db->patterns[i];
  out[0] = p.nw;
  out[1] = p.max_len;
  out[2] = p.literal_only;
  out[3] = p.som_next;
  out[4] = p.flags;
  out[5] = db->min_lengths.empty() ? 0u : db->min_lengths[i];
  out[6] = p.tier;
  out[7] = p.som_follow_off != 0;
}

// hg_nfa_som / hg_nfa_minlen for one (expression, to): the scalar loops the restatement below is held to
uint32_t somsim_nfa_som(void *h, uint32_t pattern, const uint8_t *data, uint32_t len, uint32_t to) {
  const HgDb *db = static_cast<const HgDb *>(h);
  return hg_nfa_som(db->pool.data(), db->patterns[pattern], data, len, to);
}
int somsim_nfa_minlen(void *h, uint32_t pattern, const uint8_t *data, uint32_t len, uint32_t to, uint32_t min_len) {
  const HgDb *db = static_cast<const HgDb *>(h);
  return hg_nfa_minlen(db->pool.data(), db->patterns[pattern], data, len, to, min_len) ? 1 : 0;
}

// A host RESTATEMENT of som_walk (hg_som.hip): the same decomposition written again, not the kernel's code.  The text is
// walked backwards from top = a + to - 1 in aligned 16-byte chunks, the chunks of a 64-byte line "loaded" together (a load
// that the kernel clamps is not counted: it re-reads a visited chunk), one pending position, finish() with hg_own_ctx /
// hg_prev_ctx, the piece start finalised behind the loop unless the walk stopped.  `text` has text_len bytes; a chunk may
// reach past it (bytes there read as 0 and are skipped by `at > top`).  early: the match-length mode with `limit`.
// out: {result, exit (0 state died, 1 q == lo, 2 piece start, 3 early exit), lowest loaded offset, highest loaded offset,
// 64-byte rounds}.
void somsim_walk(void *h, uint32_t pattern, const uint8_t *text, uint64_t text_len, uint64_t a, uint32_t len, uint32_t to, int early, uint32_t limit,
                 uint64_t *out) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const HgPattern &p = db->patterns[pattern];
  const uint32_t *pool = db->pool.data();
  const uint32_t nw = p.nw;
  const uint32_t *reach = pool + p.reach_off, *rfollow = pool + p.som_follow_off, *init = pool + p.init_off;
  const uint32_t *amask = pool + p.amask_off, *acc = pool + p.acc_off;
  const uint32_t lo = (p.max_len && to > p.max_len) ? to - p.max_len : 0u;
  const uint32_t floor = lo ? lo - 1 : 0u;
  auto byte_at = [&](uint64_t off) -> uint32_t { return off < text_len ? text[off] : 0u; };
  const uint32_t nc = to == len ? static_cast<uint32_t>(HG_NC_END) : hg_own_ctx(byte_at(a + to), to + 1 == len);
  std::vector<uint32_t> R(nw), T(nw);
  const uint32_t *ac = acc + (hg_prev_ctx(byte_at(a + to - 1)) * 5 + nc) * nw;
  for (uint32_t w = 0; w < nw; w++) R[w] = ac[w];
  uint32_t best = HG_NONE32, q = to - 1, cq = 0, exit_taken = 0;
  bool stopped = false;
  auto finish = [&](uint32_t pc) {
    const uint32_t *r = reach + cq * nw, *m = amask + (pc * 4 + hg_own_ctx(cq, q + 1 == len)) * nw;
    uint32_t any = 0, start = 0;
    for (uint32_t w = 0; w < nw; w++) {
      R[w] &= r[w] & m[w];
      any |= R[w];
      start |= R[w] & init[w];
    }
    if (early) {
      if (start && q <= limit) {
        best = q;
        exit_taken = 3;
        return false;
      }
    } else if (start) {
      best = q;
    }
    if (!any) {
      exit_taken = 0;
      return false;
    }
    if (q == lo) {
      exit_taken = 1;
      return false;
    }
    return true;
  };
  const uint64_t top = a + to - 1, bottom = a + floor, lowest = bottom & ~15ull;
  uint64_t chunk = top & ~15ull, lo_load = ~0ull, hi_load = 0, rounds = 0;
  bool more = true;
  while (more) {
    const uint64_t base = chunk & ~63ull;
    rounds++;
    uint8_t line[64];
    for (uint32_t j = 0; j < 4; j++) {
      const uint64_t c = base + 16u * j;
      const bool visited = !(c > chunk || c < lowest);
      if (visited) {
        lo_load = std::min(lo_load, c);
        hi_load = std::max(hi_load, c + 15);
      }
      for (uint32_t i = 0; i < 16; i++) line[16 * j + i] = visited ? static_cast<uint8_t>(byte_at(c + i)) : 0xEE;  // (a clamped load's bytes are never used)
    }
    for (int j = 3; j >= 0 && more; j--) {
      const uint64_t c = base + 16u * static_cast<uint32_t>(j);
      if (c > chunk) continue;
      if (c < lowest) {
        more = false;
        break;
      }
      for (int i = 15; i >= 0; i--) {
        const uint64_t at = c + static_cast<uint32_t>(i);
        const uint32_t b = line[16 * j + i];
        if (at > top) continue;
        if (at < bottom) {
          more = false;
          break;
        }
        if (at == top) {
          cq = b;
          continue;
        }
        if (!finish(hg_prev_ctx(b))) {
          stopped = true;
          more = false;
          break;
        }
        std::fill(T.begin(), T.end(), 0u);
        for (uint32_t w = 0; w < nw; w++)
          for (uint32_t x = R[w]; x; x &= x - 1) {
            const uint32_t *f = rfollow + (w * 32 + hg_ctz(x)) * nw;
            for (uint32_t k = 0; k < nw; k++) T[k] |= f[k];
          }
        R = T;
        q--;
        cq = b;
      }
    }
    if (base <= lowest) break;
    chunk = base - 16u;
  }
  if (!stopped && q == 0) {
    exit_taken = 2;  // the piece start: unless finish() says otherwise below (an early exit AT the piece start)
    const uint32_t before = exit_taken;
    finish(HG_PC_START);
    if (exit_taken != 3) exit_taken = before;
  }
  out[0] = best;
  out[1] = exit_taken;
  out[2] = lo_load;
  out[3] = hi_load;
  out[4] = rounds;
}

}  // extern "C"
