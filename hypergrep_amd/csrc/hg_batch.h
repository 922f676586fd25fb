// Batched block scan (hg_scan_blocks): what the host, hg_block_batch_kernel (hg_batch.hip) and the tests' replay
// (tests/native/batchsim.cpp, compiled for x86) share: the packing of a launch's items, the geometry of a workgroup's walk
// over its shard (rounds, teams, passes, slices), one lane's work, and the host report rules of a short block (hs_scan's
// one-launch path and every item of a batch run the same ones).  DESIGN.md §8f.
//
// A workgroup serves one group of expressions (HgScanner's grouping of short blocks: 32 per workgroup while 64 groups hold
// the set) and one shard of the launch's items: items shard, shard + nshards, ...  It walks them in ROUNDS.  In a round the
// workgroup's lanes are cut into equal TEAMS (a power of two of lanes, HG_BATCH_MIN_TEAM at least) and each team takes one
// item, so that short items on few expressions still fill the lanes: the team is sized by the round's first item
// (expressions x slices of HG_BATCH_MIN_SLICE start positions), and the round takes the following items of the shard while
// they fit a team's share of the text tile.  A team's lanes are (expression, slice by start position), hg_nfa_scan_slice
// unchanged; an end found from two slices is emitted once through a bitmap of ends per expression.  The bitmaps of a team hold
// HG_BATCH_SEEN_WORDS / teams words, so a long item's expressions run in several PASSES of `epp` expressions.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/hypergrep_amd.h"
#include "hg_core.h"

constexpr uint32_t HG_BATCH_ITEM_MAX = 8192;   // bytes of an item the kernel takes (= HG_BLOCK_SMALL_MAX, hg_engine.h) and of its text tile
// Words of end bitmaps per workgroup, split evenly over the round's teams.  A team runs epp = min(expressions of the group,
// lanes of the team, share / words of one bitmap) expressions per pass (hg_batch_geom): e.g. one team, 32 expressions: all 32 up
// to ends 0 .. 4127, 16 per pass for longer items; 16 teams of 512-byte items: 15 per pass; groups of 256 expressions: more passes.
constexpr uint32_t HG_BATCH_SEEN_WORDS = 4128;
constexpr uint32_t HG_BATCH_MIN_SLICE = 8;      // start positions per slice at least (as hg_block_small_kernel)
constexpr uint32_t HG_BATCH_MIN_TEAM = 16;      // lanes per team at least: at most 256 / 16 items per round
constexpr uint32_t HG_BATCH_MAX_TEAMS = 16;
constexpr uint32_t HG_BATCH_REPS = 512;         // reports of a round a workgroup gathers in LDS before its one global atomic
constexpr uint32_t HG_BATCH_SINGLE_BIT = 0x80000000u;  // (= HG_HIT_SINGLE_BIT) bit 31 of a raw record's `to`: a SINGLEMATCH expression

// One item of a launch.  Its bytes are text[text_off, text_off + len), text_off a multiple of 16, readable up to len rounded
// up to 16; 0 < len <= HG_BATCH_ITEM_MAX.
struct HgBatchItem {
  uint64_t text_off;
  uint32_t len;
  uint32_t reserved;
};

HG_HD uint32_t hg_batch_pad16(uint32_t len) { return (len + 15u) & ~15u; }
// bytes of the text tile / words of end bitmaps one of `teams` teams owns
HG_HD uint32_t hg_batch_text_share(uint32_t teams) { return (HG_BATCH_ITEM_MAX / teams) & ~15u; }
HG_HD uint32_t hg_batch_seen_share(uint32_t teams) { return HG_BATCH_SEEN_WORDS / teams; }

// Lanes of a team in a round whose first item has `len` bytes, for a workgroup of `lanes` lanes (a power of two) and `npat`
// expressions: enough for every (expression, slice of HG_BATCH_MIN_SLICE), and few enough teams for the item's text.
HG_HD uint32_t hg_batch_team(uint32_t npat, uint32_t len, uint32_t lanes) {
  const uint32_t want = npat * ((len + HG_BATCH_MIN_SLICE - 1) / HG_BATCH_MIN_SLICE);
  uint32_t ts = lanes < HG_BATCH_MIN_TEAM ? lanes : HG_BATCH_MIN_TEAM;
  while (ts < lanes && (ts < want || hg_batch_text_share(lanes / ts) < hg_batch_pad16(len))) ts <<= 1;
  return ts;
}

// The round that starts at an item of lens[0] bytes when lens[0, avail) are the next items of the shard: *team = lanes per
// team; returns how many items the round takes (1 .. lanes / *team): the leading ones that fit a team's text share.
HG_HD uint32_t hg_batch_round(const uint32_t *lens, uint32_t avail, uint32_t npat, uint32_t lanes, uint32_t *team) {
  const uint32_t ts = hg_batch_team(npat, lens[0], lanes), teams = lanes / ts;
  const uint32_t share = hg_batch_text_share(teams);
  uint32_t m = 1;
  while (m < teams && m < avail && hg_batch_pad16(lens[m]) <= share) m++;
  *team = ts;
  return m;
}

// How one team of `ts` lanes (one of `teams`) walks an item of `len` bytes under `npat` expressions.
struct HgBatchGeom {
  uint32_t words;      // words of one expression's end bitmap: ends 0 .. len
  uint32_t epp;        // expressions per pass
  uint32_t passes;
  uint32_t slice_len;  // start positions per slice
  uint32_t nslices;
};
HG_HD HgBatchGeom hg_batch_geom(uint32_t npat, uint32_t len, uint32_t ts, uint32_t teams) {
  HgBatchGeom g;
  g.words = (len >> 5) + 1;
  const uint32_t room = hg_batch_seen_share(teams) / g.words;  // (at least 1: the item fits the team's text share)
  g.epp = npat < ts ? npat : ts;
  if (g.epp > room) g.epp = room;
  g.passes = (npat + g.epp - 1) / g.epp;
  const uint32_t most = ts / g.epp;
  const uint32_t even = (len + most - 1) / most;
  g.slice_len = even < HG_BATCH_MIN_SLICE ? HG_BATCH_MIN_SLICE : even;
  g.nslices = (len + g.slice_len - 1) / g.slice_len;
  return g;
}

// Lane `tl` of a team in pass `pass`: which expression of the group and which start positions [*from, *upto); false: idle.
HG_HD bool hg_batch_lane(const HgBatchGeom &g, uint32_t npat, uint32_t len, uint32_t pass, uint32_t tl, uint32_t *expr, uint32_t *slot, uint32_t *from,
                                uint32_t *upto) {
  const uint32_t e0 = pass * g.epp;
  const uint32_t ne = npat - e0 < g.epp ? npat - e0 : g.epp;
  const uint32_t j = tl % ne, k = tl / ne;
  if (k >= g.nslices) return false;
  *expr = e0 + j;
  *slot = j;  // the expression's bitmap in the team's share: words [j * g.words, (j + 1) * g.words)
  *from = k * g.slice_len;
  *upto = *from + g.slice_len < len ? *from + g.slice_len : len;
  return true;
}

// ---- host only ------------------------------------------------------------------------------------------------------------
// Packs items (data[i], lengths[i]) for i in `pick` into `text` (each padded with zeros to 16 bytes) and fills `table`;
// returns the bytes used.  hg_batch_bytes: the same sum without copying.
inline uint64_t hg_batch_bytes(const unsigned int *lengths, const uint32_t *pick, size_t n) {
  uint64_t at = 0;
  for (size_t k = 0; k < n; k++) at += hg_batch_pad16(lengths[pick[k]]);
  return at;
}
inline uint64_t hg_batch_pack(const char *const *data, const unsigned int *lengths, const uint32_t *pick, size_t n, uint8_t *text, HgBatchItem *table) {
  uint64_t at = 0;
  for (size_t k = 0; k < n; k++) {
    const uint32_t len = lengths[pick[k]], padded = hg_batch_pad16(len);
    table[k] = HgBatchItem{at, len, 0u};
    std::memcpy(text + at, data[pick[k]], len);
    std::memset(text + at + len, 0, padded - len);
    at += padded;
  }
  return at;
}

// The report rules of a short block over its raw records {_, id, to | HG_BATCH_SINGLE_BIT} (hg_post.h, restated on the raw
// records): SINGLEMATCH expressions sharing an id give one report (the smallest end offset), the others every distinct end
// offset, an identical (id, to) once; what is left, the bit cleared, in delivery order (to, id).
inline void hg_block_rules(std::vector<HgHit> &h) {
  auto to_of = [](const HgHit &x) { return x.to & ~HG_BATCH_SINGLE_BIT; };
  auto single_of = [](const HgHit &x) { return (x.to & HG_BATCH_SINGLE_BIT) != 0; };
  std::sort(h.begin(), h.end(), [&](const HgHit &a, const HgHit &b) {
    if (a.id != b.id) return a.id < b.id;
    if (to_of(a) != to_of(b)) return to_of(a) < to_of(b);
    return single_of(a) < single_of(b);
  });
  size_t kept = 0;
  bool seen_single = false;
  for (size_t i = 0; i < h.size(); i++) {
    if (i == 0 || h[i].id != h[i - 1].id) seen_single = false;
    const bool dup = i > 0 && h[i].id == h[i - 1].id && to_of(h[i]) == to_of(h[i - 1]);
    const bool single = single_of(h[i]);
    const bool keep = !dup && !(single && seen_single);
    if (single) seen_single = true;
    if (keep) {
      HgHit out = h[i];
      out.to = to_of(h[i]);
      h[kept++] = out;
    }
  }
  h.resize(kept);
  std::sort(h.begin(), h.end(), [](const HgHit &a, const HgHit &b) { return a.to != b.to ? a.to < b.to : a.id < b.id; });
}
