// TEST-ONLY host harness for the batched block scan (never shipped): compiles the product's pattern compiler and
// hypergrep_amd/csrc/hg_batch.h for x86 and replays what hg_scan_blocks and hg_block_batch_kernel do with them: the items
// packed into one staging area plus an item table (hg_batch_pack), per group of expressions and shard of items the rounds,
// teams, passes and slices of hg_batch.h, every lane's hg_nfa_scan_slice over the team's share of the text tile with the
// bitmap of ends, then the per-item report rules (hg_block_rules).  batchsim_block runs hg_nfa_scan over one item alone.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_batch.h"
#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"

extern "C" {

void *batchsim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, unsigned n, char *err, size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  if (hgc_compile_ext(exprs, flags, ids, nullptr, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
void batchsim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// Raw ends of every expression over data[0, len) as one block: out[2 k] = expression, out[2 k + 1] = end.
long batchsim_block(void *h, const uint8_t *data, uint32_t len, uint32_t *out, size_t cap) {
  const HgDb &db = *static_cast<HgDb *>(h);
  size_t n = 0;
  for (uint32_t p = 0; p < db.patterns.size(); p++)
    hg_nfa_scan(db.pool.data(), db.patterns[p], data, len, [&](uint32_t to) {
      if (n < cap) out[2 * n] = p, out[2 * n + 1] = to;
      n++;
    });
  return static_cast<long>(n);
}

// The batch blob[offs[i], offs[i] + lens[i]) for i < nitems, scanned as hg_scan_blocks scans it with workgroups of `lanes`
// lanes (a power of two), `ppw` expressions per group and `nshards` shards.  out[3 k] = item, id, to: per item in delivery
// order, items ascending.  Negative: a bound of the geometry was violated (-2 text share, -3 bitmap share, -4 lane map,
// -5 an item visited other than once per group).
long batchsim_run(void *h, const uint8_t *blob, const uint64_t *offs, const uint32_t *lens, uint32_t nitems, uint32_t lanes, uint32_t ppw, uint32_t nshards,
                  uint32_t *out, size_t cap) {
  const HgDb &db = *static_cast<HgDb *>(h);
  const uint32_t *pool = db.pool.data();
  const uint32_t np = static_cast<uint32_t>(db.patterns.size());
  // the host's part: non-empty items picked and packed
  std::vector<const char *> data(nitems);
  std::vector<uint32_t> pick;
  for (uint32_t i = 0; i < nitems; i++) {
    data[i] = reinterpret_cast<const char *>(blob + offs[i]);
    if (lens[i] && lens[i] <= HG_BATCH_ITEM_MAX) pick.push_back(i);
  }
  const uint32_t n = static_cast<uint32_t>(pick.size());
  std::vector<uint8_t> text(hg_batch_bytes(lens, pick.data(), n) + 16, 0xEE);
  std::vector<HgBatchItem> items(n);
  if (hg_batch_pack(data.data(), lens, pick.data(), n, text.data(), items.data()) + 16 != text.size()) return -2;
  std::vector<std::vector<HgHit>> per(n);
  std::vector<uint32_t> visits(n, 0u);
  const uint32_t ngroups = (np + ppw - 1) / ppw;
  std::vector<uint8_t> s_text(HG_BATCH_ITEM_MAX);
  std::vector<uint32_t> s_seen(HG_BATCH_SEEN_WORDS);
  for (uint32_t group = 0; group < ngroups; group++) {
    const uint32_t first = group * ppw, npat = std::min(first + ppw, np) - first;
    for (uint32_t shard = 0; shard < nshards; shard++) {
      const uint32_t mine = shard < n ? (n - shard + nshards - 1) / nshards : 0u;
      for (uint32_t cur = 0; cur < mine;) {
        const uint32_t avail = std::min(mine - cur, HG_BATCH_MAX_TEAMS);
        uint32_t s_len[HG_BATCH_MAX_TEAMS];
        for (uint32_t t = 0; t < avail; t++) s_len[t] = items[shard + static_cast<size_t>(cur + t) * nshards].len;
        uint32_t ts;
        const uint32_t taken = hg_batch_round(s_len, avail, npat, lanes, &ts);
        const uint32_t teams = lanes / ts;
        if (taken == 0 || taken > teams || taken > avail || teams > HG_BATCH_MAX_TEAMS) return -4;
        std::fill(s_text.begin(), s_text.end(), 0xDD);
        for (uint32_t team = 0; team < taken; team++) {  // every team stages before any lane scans
          const HgBatchItem &it = items[shard + static_cast<size_t>(cur + team) * nshards];
          if (hg_batch_pad16(it.len) > hg_batch_text_share(teams) || (team + 1) * hg_batch_text_share(teams) > HG_BATCH_ITEM_MAX || (it.text_off & 15)) return -2;
          std::memcpy(s_text.data() + team * hg_batch_text_share(teams), text.data() + it.text_off, hg_batch_pad16(it.len));
        }
        for (uint32_t team = 0; team < taken; team++) {
          const uint32_t k = shard + (cur + team) * nshards, len = s_len[team];
          if (group == 0) visits[k]++;
          const uint8_t *txt = s_text.data() + team * hg_batch_text_share(teams);
          uint32_t *seen = s_seen.data() + team * hg_batch_seen_share(teams);
          const HgBatchGeom g = hg_batch_geom(npat, len, ts, teams);
          if (g.epp == 0 || g.epp * g.words > hg_batch_seen_share(teams) || (team + 1) * hg_batch_seen_share(teams) > HG_BATCH_SEEN_WORDS) return -3;
          std::vector<uint32_t> covered(npat, 0u);
          for (uint32_t pass = 0; pass < g.passes; pass++) {
            std::fill(seen, seen + g.epp * g.words, 0u);
            for (uint32_t tl = 0; tl < ts; tl++) {
              uint32_t e, slot, from, upto;
              if (!hg_batch_lane(g, npat, len, pass, tl, &e, &slot, &from, &upto)) continue;
              if (e >= npat || slot >= g.epp || from >= upto || upto > len) return -4;
              covered[e] += upto - from;
              const HgPattern &pat = db.patterns[first + e];
              uint32_t *bits = seen + slot * g.words;
              hg_nfa_scan_slice(pool, pat, txt, len, from, upto, [&](uint32_t to) {
                if (g.nslices > 1) {
                  if (bits[to >> 5] >> (to & 31) & 1u) return;
                  bits[to >> 5] |= 1u << (to & 31);
                }
                per[k].push_back(HgHit{k, pat.id, to | (pat.single ? HG_BATCH_SINGLE_BIT : 0u)});
              });
            }
          }
          for (uint32_t e = 0; e < npat; e++)
            if (covered[e] != len) return -4;  // every start position of every expression exactly once
        }
        cur += taken;
      }
    }
  }
  for (uint32_t k = 0; k < n; k++)
    if (visits[k] != 1) return -5;
  size_t m = 0;
  for (uint32_t k = 0; k < n; k++) {
    hg_block_rules(per[k]);
    for (const HgHit &x : per[k]) {
      if (m < cap) out[3 * m] = pick[k], out[3 * m + 1] = x.id, out[3 * m + 2] = x.to;
      m++;
    }
  }
  return static_cast<long>(m);
}

}  // extern "C"
