// TEST-ONLY host harness (never shipped, never loaded by the product): compiles the product's pattern
// compiler and hg_core.h for x86 and replays the GPU pipeline's stages in scalar form —
//   stream pass (newline summaries + window fingerprint filter + literal verify)  ~ hg_stream_kernel
//   tile scan                                                          ~ hg_tile_scan_*
//   confirm / always-on                                                ~ hg_confirm_kernel / hg_always_on_kernel
//   order + dedupe                                                     ~ hg_finalize
// so the compiler's tables and the shared device logic can be checked against the oracle without a GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_post.h"

extern "C" {

struct SimHit {
  uint64_t line_no;
  uint32_t id, to;
  uint64_t start;
  uint32_t len, pattern;
};

void *hgsim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, unsigned n, char *err, size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  if (hgc_compile(exprs, flags, ids, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
int hgsim_tune(void *h, const uint8_t *sample, size_t n) {  // the handle keeps its identity: the tuned copy's tables move in
  std::string e;
  HgDb *tuned = nullptr;
  int rc = hgc_tune(static_cast<const HgDb *>(h), sample, n, &tuned, &e);
  if (rc != 0) return rc;
  *static_cast<HgDb *>(h) = std::move(*tuned);
  hgc_free(tuned);
  return 0;
}
void hgsim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

void hgsim_info(void *h, uint32_t *out) {  // npatterns, nfactors, nwindows, nslow, fold_mask, max_nw
  HgDb *db = static_cast<HgDb *>(h);
  out[0] = db->patterns.size();
  out[1] = db->nreal_factors;
  out[2] = db->nreal_factors ? db->windows.size() : 0;
  out[3] = db->slow.size();
  out[4] = db->fold_mask;
  out[5] = db->max_nw;
}
static HgDbView view_of(HgDb *db);
// Invariants of the compiled prefilter, checked on the tables themselves (no text): every window of every literal
//  (1) passes the first level at its own slot, (2) passes the second level when the literal's own bytes surround it,
//  (3) is found by the verify pass's discriminated bucket lookup when the literal itself is the text.
// Returns the number of violations; out[0] = filter log2, out[1] = wide, out[2] = slots holding more than two values,
// out[3] = byte-aligned probing step (0: dword windows), out[6] = window bytes (3 or 4).
uint32_t hgsim_selfcheck(void *h, uint32_t *out) {  // out[7]
  HgDb *db = static_cast<HgDb *>(h);
  const HgDbView v = view_of(db);
  uint32_t bad = 0, many = 0;
  const uint32_t byte_mask = ((1u << db->filter_log2) - 1u) << 2;
  if (!db->filter_wide)
    for (const HgSlotInfo &s : db->ext) many += s.many ? 1 : 0;
  for (size_t wi = 0; wi < db->windows.size() && db->nreal_factors; wi++) {
    const HgWindow &w = db->windows[wi];
    const HgFactor &f = db->factors[w.factor_off >> 8];
    const uint32_t off = w.factor_off & 0xff;
    const uint32_t key = hg_hash_window(w.value);
    // the literal as a text of its own, lower-cased where it is case-insensitive (what folding maps both cases to)
    std::vector<uint8_t> text(f.lit, f.lit + f.len);
    if (f.len < db->window_bytes) text.push_back(static_cast<uint8_t>(w.value >> 24));  // enumerated byte after a 3-byte literal
    auto dword_at = [&](int64_t p) {
      uint32_t x = 0;
      for (int b = 0; b < 4; b++)
        if (p + b >= 0 && p + b < static_cast<int64_t>(text.size())) x |= static_cast<uint32_t>(text[p + b]) << (8 * b);
      return x;
    };
    if (db->filter_wide) {
      const uint32_t a = hg_dot4(w.value, db->weights_a), b = hg_dot4(w.value, db->weights_b), fp = key & 0xFFFFu;
      const uint32_t ta = db->filter[hg_slot_wide(a, b, byte_mask) >> 2], tb = db->filter[hg_slot_wide(b, a, byte_mask) >> 2];
      if (!((ta & 0xFFFFu) == fp || (ta >> 16) == fp || (tb & 0xFFFFu) == fp || (tb >> 16) == fp)) bad++;
    } else {
      const uint32_t sl = hg_slot(w.value, db->weights_a, byte_mask) >> 2;
      if (!hg_slot_match(db->filter[sl], key)) bad++;
      const uint32_t prev = dword_at(static_cast<int64_t>(off) - 4) | db->fold_mask, next = dword_at(static_cast<int64_t>(off) + db->window_bytes) | db->fold_mask;
      // bytes outside the literal are unknown in a real text: try both extremes
      for (uint32_t fill : {0u, 0xFFFFFFFFu}) {
        uint32_t p2 = prev, n2 = next;
        for (int b = 0; b < 4; b++) {
          if (static_cast<int>(off) - 4 + b < 0) p2 = (p2 & ~(0xFFu << (8 * b))) | (fill & (0xFFu << (8 * b)));
          if (off + db->window_bytes + b >= f.len) n2 = (n2 & ~(0xFFu << (8 * b))) | (fill & (0xFFu << (8 * b)));
        }
        if (!hg_slot_pass(db->ext[sl], w.value, p2 | db->fold_mask, n2 | db->fold_mask, 0xFFFFFFFFu, 0xFFFFFFFFu)) bad++;
      }
    }
    uint32_t j0, j1;
    hg_disc_range(v, text.data(), text.size(), off, w.value, &j0, &j1);
    bool found = false;
    for (uint32_t j = j0; j < j1; j++) found = found || (db->windows2[j].value == w.value && db->windows2[j].factor_off == w.factor_off);
    if (!found) bad++;
    // (4) the direct table holds the window's value; with one owner it names exactly this (literal, offset)
    const uint32_t owner = hg_wtab_find(db->wtab.data(), db->wtab_mask, w.value);
    if (owner == HG_WTAB_EMPTY || (owner != HG_WTAB_SHARED && owner != w.factor_off)) bad++;
  }
  if (out) { out[0] = db->filter_log2; out[1] = db->filter_wide; out[2] = many; out[3] = db->dense; }
  // the table's buckets fill front to back and are never more than half full over all
  size_t used = 0;
  for (const HgWinBucket &b : db->wtab)
    for (uint32_t k = 0; k < HG_WTAB_WAYS; k++) {
      used += b.factor_off[k] != HG_WTAB_EMPTY ? 1 : 0;
      if (k && b.factor_off[k] != HG_WTAB_EMPTY && b.factor_off[k - 1] == HG_WTAB_EMPTY) bad++;
    }
  if (used * 2 > db->wtab.size() * HG_WTAB_WAYS || db->wtab.size() != static_cast<size_t>(db->wtab_mask) + 1) bad++;
  if (out) { out[4] = db->shared_windows; out[5] = db->wtab_first; out[6] = db->window_bytes; }
  return bad;
}
uint32_t hgsim_pattern_tier(void *h, uint32_t i) { return static_cast<HgDb *>(h)->patterns[i].tier; }
uint32_t hgsim_pattern_nodes(void *h, uint32_t i) { return static_cast<HgDb *>(h)->patterns[i].nnodes; }

// Run one pattern's automaton over one already-trimmed piece; returns number of reports, fills tos[<=cap].
size_t hgsim_nfa(void *h, uint32_t pattern, const uint8_t *data, size_t len, uint32_t *tos, size_t cap) {
  HgDb *db = static_cast<HgDb *>(h);
  size_t n = 0;
  hg_nfa_scan(db->pool.data(), db->patterns[pattern], data, len, [&](uint32_t to) {
    if (n < cap) tos[n] = to;
    n++;
  });
  return n;
}

static HgDbView view_of(HgDb *db) {
  HgDbView v{};
  v.patterns = db->patterns.data();
  v.pool = db->pool.data();
  v.factors = db->factors.data();
  v.windows = db->windows.data();
  v.bucket_off = db->bucket_off.data();
  v.disc = db->disc.data();
  v.bucket_off2 = db->bucket_off2.data();
  v.windows2 = db->windows2.data();
  v.wtab = db->wtab.data();
  v.wtab_mask = db->wtab_mask;
  v.wtab_first = db->wtab_first;
  v.slow = db->slow.data();
  v.npatterns = db->patterns.size();
  v.nslow = db->slow.size();
  v.nslow_fast = db->nslow_fast;
  v.nslow_grouped = 0;  // (the host replay runs every always-on expression on its own)
  v.nslow_huge = db->nslow_huge;
  v.ngroups = 0;
  v.groups = nullptr;
  v.fold_mask = db->fold_mask;
  v.window_mask = db->window_mask;
  return v;
}

// Whole pipeline on a memory buffer.  Returns number of hits (after dedupe); *out is malloc'ed.
// stats[4] = hits surviving the neighbour-dword check; stats[0] = window fingerprint filter hits, stats[1] = verified candidates, stats[2] = raw hits before dedupe, stats[3] = pieces
long hgsim_scan(void *h, const uint8_t *data, uint64_t nbytes, int buffer_size, SimHit **out, uint64_t *stats) {
  HgDb *db = static_cast<HgDb *>(h);
  HgDbView v = view_of(db);
  if (buffer_size < 2) { *out = nullptr; return 0; }
  uint64_t bs1 = static_cast<uint64_t>(buffer_size) - 1;
  uint64_t ntiles = (nbytes + HG_TILE_BYTES - 1) / HG_TILE_BYTES;
  std::vector<HgTileSum> sums(ntiles ? ntiles : 1);
  std::vector<HgTileBase> bases(ntiles + 1);
  std::vector<HgCand> cands;
  uint64_t bitmap_hits = 0, level2_hits = 0;
  std::map<uint32_t, uint64_t> l1_hist;
  // ---- stream pass
  for (uint64_t t = 0; t < ntiles; t++) {
    uint64_t base = t * HG_TILE_BYTES;
    HgTileSum s{0, HG_NONE32, HG_NONE32, 0};
    const uint32_t step = 1;  // newlines are counted byte by byte; windows are probed every `probe_step` bytes
    const uint32_t probe_step = db->dense ? db->dense : 4;
    for (uint32_t d = 0; d < HG_TILE_BYTES / step; d++) {
      uint64_t pos = base + static_cast<uint64_t>(d) * step;
      if (pos >= nbytes) break;
      uint32_t w = 0;
      uint64_t avail = nbytes - pos < 4 ? nbytes - pos : 4;
      std::memcpy(&w, data + pos, avail);  // bytes past the end read as zero, as the kernel masks them
      uint32_t rank_here = s.nl_count;
      uint32_t m = hg_newline_mask(w);
      m &= 0x80u;  // only the byte at pos itself
      if (m) {
        for (uint32_t b = 0; b < 4; b++)
          if (m >> (8 * b + 7) & 1) {
            if (s.first_nl == HG_NONE32) s.first_nl = d * step + b;
            s.last_nl = d * step + b;
          }
        s.nl_count += hg_popc(m);
      }
      if (pos % probe_step) continue;  // windows start every probe_step bytes (absolute offsets: chunks are 16-byte aligned)
      const uint32_t folded = (w | v.fold_mask) & db->window_mask, byte_mask = ((1u << db->filter_log2) - 1u) << 2;
      // bytes outside the text read as zero, like the kernel's masked tail
      auto dword_at = [&](int64_t p) -> uint32_t {
        uint32_t x = 0;
        for (int b = 0; b < 4; b++)
          if (p + b >= 0 && static_cast<uint64_t>(p + b) < nbytes) x |= static_cast<uint32_t>(data[p + b]) << (8 * b);
        return x;
      };
      // first level: window hash
      const uint32_t key0 = hg_hash_window(folded);
      uint32_t sla = hg_slot(folded, db->weights_a, byte_mask) >> 2, slb = hg_slot(folded, db->weights_b, byte_mask) >> 2;
      if (db->filter_wide) {
        const uint32_t a = hg_dot4(folded, db->weights_a), b = hg_dot4(folded, db->weights_b);
        sla = hg_slot_wide(a, b, byte_mask) >> 2, slb = hg_slot_wide(b, a, byte_mask) >> 2;
      }
      bool ha = hg_slot_match(db->filter[sla], key0), hb = false;  // single probe (slot A)
      if (db->filter_wide) {
        const uint32_t fp = key0 & 0xFFFFu, ta = db->filter[sla], tb = db->filter[slb];
        ha = (ta & 0xFFFFu) == fp || (ta >> 16) == fp;
        hb = (tb & 0xFFFFu) == fp || (tb >> 16) == fp;
      }
      if (ha || hb) {
        bitmap_hits++;
        if (getenv("HGSIM_DUMP")) l1_hist[folded]++;
        const uint32_t pf = dword_at(static_cast<int64_t>(pos) - 4) | v.fold_mask, nf = dword_at(static_cast<int64_t>(pos) + db->window_bytes) | v.fold_mask;
        // the kernel cannot see across its 16 KiB tile edge or the first/last lane of a 1 KiB segment: treat as pass there
        const bool edge_prev = !db->dense && (pos % 1024) == 0, edge_next = !db->dense && (pos % 1024) == 1020;
        auto pass = [&](uint32_t sl) {
          // the last lane sees at most its own dword's top byte
          return hg_slot_pass(db->ext[sl], folded, pf, nf, edge_prev ? 0u : 0xFFFFFFFFu, edge_next ? (HG_WINDOW_BYTES == 4 ? 0u : 0xFFu) : 0xFFFFFFFFu);
        };
        if (!db->filter_wide && !((ha && pass(sla)) || (hb && pass(slb)))) continue;
        level2_hits++;
        cands.push_back(HgCand{pos, w, rank_here});
      }
    }
    s.inner = s.nl_count ? s.nl_count - 1 : 0;
    if (bs1 < HG_TILE_BYTES && s.nl_count >= 2)  // ~ hg_tile_inner_kernel
      s.inner = static_cast<uint32_t>(hg_inner_pieces(data, base + s.first_nl + 1, base + s.last_nl + 1, bs1));
    sums[t] = s;
  }
  if (getenv("HGSIM_DUMP")) {
    std::vector<std::pair<uint64_t, uint32_t>> top;
    for (auto &kv : l1_hist) top.push_back({kv.second, kv.first});
    std::sort(top.rbegin(), top.rend());
    for (size_t i = 0; i < top.size() && i < 12; i++) {
      uint32_t x = top[i].second;
      fprintf(stderr, "L1 window '%c%c%c%c' x%llu\n", x & 0xff, (x >> 8) & 0xff, (x >> 16) & 0xff, x >> 24, (unsigned long long)top[i].first);
    }
  }
  // ---- tile scan
  HgTileBase st{0, 0};
  for (uint64_t t = 0; t < ntiles; t++) {
    bases[t] = st;
    st = hg_tile_apply(st, hg_tile_elem(sums[t], t * HG_TILE_BYTES), bs1);
  }
  bases[ntiles] = st;
  uint64_t pieces = st.L + (nbytes > st.cs ? hg_pieces(nbytes - st.cs, bs1) : 0);
  // ---- confirm
  std::vector<HgHit> hits;
  std::vector<HgHitAux> aux;
  uint64_t verified = 0;
  std::set<std::pair<uint64_t, uint32_t>> huge_done;  // (piece start, expression) pairs a huge automaton has run on
  for (auto &c : cands) {
    hg_verify_window(v, data, nbytes, c.pos, c.word, [&](uint32_t pattern, uint64_t fs, uint32_t) {
      verified++;
      auto emit = [&](uint64_t line_no, uint32_t to, uint64_t a, uint32_t len) {
        hits.push_back(HgHit{line_no, db->patterns[pattern].id, to});
        aux.push_back(HgHitAux{a, len, pattern});
      };
      // SINGLEMATCH automata of <= 2 state words are confirmed by window on the device (confirm modes 1 and 2): the same here
      const uint32_t mode = hg_confirm_mode(db->patterns[pattern]);
      if ((mode == 1 || mode == 2) && !getenv("HGSIM_NO_WINDOW")) {
        hg_confirm_window(v, data, nbytes, sums.data(), bases.data(), bs1, c.pos, fs, pattern, c.rank, emit);
      } else if (mode == 4) {
        // huge automata: ONE run per (expression, piece), whichever occurrence of the literal comes first — the device claims
        // the pair in a hash table (hg_huge.hip); a literal that overlaps itself (a{32767}) gives a candidate per byte
        bool fresh = false;
        hg_confirm(v, data, nbytes, sums.data(), bases.data(), bs1, c.pos, pattern, c.rank, emit,
                   [&](uint64_t ps) { return fresh = huge_done.insert({ps, pattern}).second; });
        (void)fresh;
      } else {
        hg_confirm(v, data, nbytes, sums.data(), bases.data(), bs1, c.pos, pattern, c.rank, emit);
      }
    });
  }
  // ---- always-on tier: every line start
  if (v.nslow) {
    for (uint64_t t = 0; t < ntiles; t++) {
      uint64_t base = t * HG_TILE_BYTES, end = std::min<uint64_t>(base + HG_TILE_BYTES, nbytes);
      uint32_t rank = 0;
      for (uint64_t s = base; s < end; s++) {
        bool starts = (s == 0) || data[s - 1] == '\n';
        if (starts)
          hg_scan_line_always_on(v, data, nbytes, sums.data(), bases.data(), bs1, s, rank, 0u, v.nslow,
                                 [&](uint32_t pi, uint64_t line_no, uint32_t to, uint64_t a, uint32_t len) {
                                   hits.push_back(HgHit{line_no, db->patterns[pi].id, to});
                                   aux.push_back(HgHitAux{a, len, pi});
                                 });
        if (data[s] == '\n') rank++;
      }
    }
  }
  uint64_t raw = hits.size();
  // ---- order + dedupe
  std::vector<uint32_t> order(hits.size());
  for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    uint64_t kx = hg_sort_key(hits[x], db->patterns[aux[x].pattern].single), ky = hg_sort_key(hits[y], db->patterns[aux[y].pattern].single);
    if (hits[x].line_no != hits[y].line_no) return hits[x].line_no < hits[y].line_no;
    return kx < ky;
  });
  std::vector<HgHit> sh(hits.size());
  std::vector<HgHitAux> sa(hits.size());
  for (size_t i = 0; i < order.size(); i++) { sh[i] = hits[order[i]]; sa[i] = aux[order[i]]; }
  std::vector<SimHit> kept;
  for (size_t i = 0; i < sh.size(); i++) {
    if (!hg_keep_hit(sh.data(), sa.data(), v.patterns, i)) continue;
    kept.push_back(SimHit{sh[i].line_no, sh[i].id, sh[i].to, sa[i].start, sa[i].len, sa[i].pattern});
  }
  SimHit *res = static_cast<SimHit *>(malloc(sizeof(SimHit) * (kept.size() ? kept.size() : 1)));
  std::memcpy(res, kept.data(), sizeof(SimHit) * kept.size());
  *out = res;
  if (stats) { stats[0] = bitmap_hits; stats[1] = verified; stats[2] = raw; stats[3] = pieces; stats[4] = level2_hits; }
  return static_cast<long>(kept.size());
}
void hgsim_free_hits(SimHit *p) { free(p); }

// ---- verify pass: placement read-out and the buckets-only path (tests/verify_cells.py) ----------------------------------------
// One record of 12 words per window of every literal, in the order of db->windows:
//   0 factor index, 1 offset of the window in the literal, 2 value (folded), 3 table state (0 absent, 1 this window is the direct
//   owner, 2 shared), 4 buckets probed before the value's (0: its home bucket), 5 way in that bucket, 6 discriminator delta
//   (int8 as a byte), 7 discriminator byte-select bits, 8 size of the discriminated bucket this window lies in (found with the
//   literal itself as the text), 9 literal length, 10 pattern index, 11 the literal's case bits.
// Returns the number of windows (records beyond cap are not written).
uint32_t hgsim_windows(void *h, uint32_t *out, uint32_t cap) {
  HgDb *db = static_cast<HgDb *>(h);
  const HgDbView v = view_of(db);
  if (!db->nreal_factors) return 0;
  uint32_t n = 0;
  for (const HgWindow &w : db->windows) {
    if (n < cap) {
      uint32_t *r = out + static_cast<size_t>(n) * 12;
      const HgFactor &f = db->factors[w.factor_off >> 8];
      const uint32_t off = w.factor_off & 0xff;
      r[0] = w.factor_off >> 8;
      r[1] = off;
      r[2] = w.value;
      r[3] = 0, r[4] = 0, r[5] = 0;
      uint32_t probes = 0;
      for (uint32_t b = hg_wtab_bucket(w.value, db->wtab_mask);; b = (b + 1u) & db->wtab_mask, probes++) {
        const HgWinBucket &e = db->wtab[b];
        bool stop = false;
        for (uint32_t k = 0; k < HG_WTAB_WAYS && !stop; k++) {
          if (e.factor_off[k] == HG_WTAB_EMPTY) stop = true;
          else if (e.value[k] == w.value) {
            r[3] = e.factor_off[k] == HG_WTAB_SHARED ? 2u : (e.factor_off[k] == w.factor_off ? 1u : 3u);
            r[4] = probes;
            r[5] = k;
            stop = true;
          }
        }
        if (stop) break;
      }
      const uint32_t d = db->disc[hg_hash_window(w.value)];
      r[6] = d & 0xFFu;
      r[7] = d >> 8;
      std::vector<uint8_t> text(f.lit, f.lit + f.len);
      if (f.len < db->window_bytes) text.push_back(static_cast<uint8_t>(w.value >> 24));
      uint32_t j0, j1;
      hg_disc_range(v, text.data(), text.size(), off, w.value, &j0, &j1);
      r[8] = j1 - j0;
      r[9] = f.len;
      r[10] = f.pattern;
      r[11] = f.casebits;
    }
    n++;
  }
  return n;
}

// The literal compare of the verify kernel (literal_occurs in hg_kernels.hip) restated: dwords under hg_factor_mask_dword while
// 16 / 32 bytes from fs are readable, bytes in the buffer's last 16 / 32.
static bool sim_literal_occurs(const HgFactor &f, const uint8_t *text, uint64_t fs, uint64_t readable) {
  const uint32_t len = f.len, cb = f.casebits;
  uint32_t diff = 0;
  if (fs + (len > 16 ? 32u : 16u) <= readable) {
    for (uint32_t j = 0; j < (len > 16 ? 8u : 4u); j++) {
      uint32_t x, l;
      std::memcpy(&x, text + fs + 4 * j, 4);
      std::memcpy(&l, f.lit + 4 * j, 4);
      diff |= (x ^ l) & hg_factor_mask_dword(cb, len, j);
    }
  } else {
    for (uint32_t b = 0; b < len; b++) diff |= (text[fs + b] ^ f.lit[b]) & (((cb >> b) & 1u) ? 0xDFu : 0xFFu);
  }
  return diff == 0;
}

// The verify pass over EVERY probe position of a text, three ways:
//   A  hg_verify_window: the direct table first (what the host replay and the block-mode kernel run);
//   B  the buckets-only path, what the verify kernel does for a set without wtab_first: the discriminated bucket of every
//      position, the value compare inside it, the kernel's position checks and its literal compare (sim_literal_occurs);
//   C  brute force: every window of every literal against the text's dword, every literal byte by byte, no table.
// `text` must be readable up to nbytes rounded up to 16.  Each answer is the multiset of (pattern, literal start) per position;
// out[0] positions, out[1..3] emits of A, B, C, out[4] positions where the three differ, out[5] positions the table ends
// (value absent), out[6] positions whose bucket is not empty but holds no window of the value, out[7] the largest bucket met,
// out[8] positions with a negative discriminator address (at < 0) whose selected bytes lie inside the text, out[9] positions
// whose selected bytes lie outside the text, out[10] positions verified through a byte compare at the buffer's end,
// out[11] windows whose literal would start before the text (pos < off), out[12] occurrences with another byte behind the
// literal than its record holds there, inside a compared dword (the tail mask decides), out[13] the first differing position.
void hgsim_verify3(void *h, const uint8_t *text, uint64_t nbytes, uint64_t *out) {
  HgDb *db = static_cast<HgDb *>(h);
  const HgDbView v = view_of(db);
  for (int i = 0; i < 14; i++) out[i] = 0;
  out[13] = ~0ull;
  if (!db->nreal_factors) return;
  const uint32_t step = db->dense ? db->dense : 4;
  const uint64_t readable = (nbytes + 15) & ~15ull;
  typedef std::vector<std::pair<uint32_t, uint64_t>> Answer;
  for (uint64_t pos = 0; pos < nbytes; pos += step) {
    uint32_t w = 0;
    std::memcpy(&w, text + pos, nbytes - pos < 4 ? nbytes - pos : 4);
    const uint32_t folded = (w | v.fold_mask) & v.window_mask;
    Answer a, b, c;
    hg_verify_window(v, text, nbytes, pos, w, [&](uint32_t pattern, uint64_t fs, uint32_t) { a.push_back({pattern, fs}); });
    if (hg_wtab_find(v.wtab, v.wtab_mask, folded) == HG_WTAB_EMPTY) out[5]++;
    {  // B
      const uint32_t hh = hg_hash_window(folded), d = v.disc[hh], sel = d >> 8;
      uint32_t key = 0, j0 = 0, cnt = 0;
      bool inside = true;
      if (sel) {
        const int64_t at = static_cast<int64_t>(pos) + static_cast<int8_t>(d & 0xFFu);
        const uint32_t lo = hg_ctz(sel), hi = 31u - hg_clz32(sel);
        inside = at + static_cast<int64_t>(lo) >= 0 && static_cast<uint64_t>(at + hi) < nbytes;
        if (!inside) out[9]++;
        if (inside && at < 0) out[8]++;
        if (inside) {
          uint32_t x = 0;
          if (at >= 0 && (at & 3) == 0) std::memcpy(&x, text + at, 4);  // (ends before the size rounded up to 4)
          else
            for (uint32_t q = lo; q <= hi; q++) x |= static_cast<uint32_t>(text[at + static_cast<int64_t>(q)]) << (8u * q);
          key = (x | v.fold_mask) & hg_disc_bytes(sel);
        }
      }
      if (inside) {
        const uint32_t h2 = hg_disc_bucket(hh, key);
        j0 = v.bucket_off2[h2];
        cnt = v.bucket_off2[h2 + 1] - j0;
      }
      if (cnt > out[7]) out[7] = cnt;
      bool value_seen = false;
      for (uint32_t t = 0; t < cnt; t++) {
        const HgWindow win = v.windows2[j0 + t];
        if (win.value != folded) continue;
        value_seen = true;
        const uint32_t off = win.factor_off & 0xffu;
        const HgFactor &f = v.factors[win.factor_off >> 8];
        if (pos < off) { out[11]++; continue; }
        if (pos - off + f.len > nbytes) continue;
        const uint64_t fs = pos - off;
        if (fs + (f.len > 16 ? 32u : 16u) > readable) out[10]++;
        if (sim_literal_occurs(f, text, fs, readable)) b.push_back({f.pattern, fs});
      }
      if (cnt && !value_seen) out[6]++;
    }
    for (const HgWindow &win : db->windows) {  // C
      if (win.value != folded) continue;
      const uint32_t off = win.factor_off & 0xffu;
      const HgFactor &f = db->factors[win.factor_off >> 8];
      if (pos < off || pos - off + f.len > nbytes) continue;
      bool same = true;
      for (uint32_t q = 0; q < f.len && same; q++) {
        const uint8_t x = text[pos - off + q], l = f.lit[q];
        same = ((f.casebits >> q) & 1u) ? ((x | 0x20) == (l | 0x20)) : (x == l);
      }
      if (!same) continue;
      c.push_back({f.pattern, pos - off});
      // the byte behind the literal differs from the record's byte there, in a dword the compare loads: the tail mask decides
      const uint64_t fs = pos - off;
      if (f.len < HG_FACTOR_MAX && (f.len & 3u) && fs + (f.len > 16 ? 32u : 16u) <= readable && text[fs + f.len] != f.lit[f.len]) out[12]++;
    }
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    std::sort(c.begin(), c.end());
    out[0]++;
    out[1] += a.size();
    out[2] += b.size();
    out[3] += c.size();
    if (a != b || a != c) {
      out[4]++;
      if (out[13] == ~0ull) out[13] = pos;
    }
  }
}

// The stream pass's filter at one probe position, as hgsim_scan applies it (both levels): does `pos` become a candidate?
static bool sim_filter_pass(HgDb *db, const HgDbView &v, const uint8_t *data, uint64_t nbytes, uint64_t pos, uint32_t w) {
  const uint32_t folded = (w | v.fold_mask) & db->window_mask, byte_mask = ((1u << db->filter_log2) - 1u) << 2;
  auto dword_at = [&](int64_t p) -> uint32_t {
    uint32_t x = 0;
    for (int b = 0; b < 4; b++)
      if (p + b >= 0 && static_cast<uint64_t>(p + b) < nbytes) x |= static_cast<uint32_t>(data[p + b]) << (8 * b);
    return x;
  };
  const uint32_t key0 = hg_hash_window(folded);
  uint32_t sla = hg_slot(folded, db->weights_a, byte_mask) >> 2, slb = hg_slot(folded, db->weights_b, byte_mask) >> 2;
  if (db->filter_wide) {
    const uint32_t a = hg_dot4(folded, db->weights_a), b = hg_dot4(folded, db->weights_b);
    sla = hg_slot_wide(a, b, byte_mask) >> 2, slb = hg_slot_wide(b, a, byte_mask) >> 2;
  }
  bool ha = hg_slot_match(db->filter[sla], key0), hb = false;
  if (db->filter_wide) {
    const uint32_t fp = key0 & 0xFFFFu, ta = db->filter[sla], tb = db->filter[slb];
    ha = (ta & 0xFFFFu) == fp || (ta >> 16) == fp;
    hb = (tb & 0xFFFFu) == fp || (tb >> 16) == fp;
  }
  if (!ha && !hb) return false;
  if (db->filter_wide) return true;
  const uint32_t pf = dword_at(static_cast<int64_t>(pos) - 4) | v.fold_mask, nf = dword_at(static_cast<int64_t>(pos) + db->window_bytes) | v.fold_mask;
  const bool edge_prev = !db->dense && (pos % 1024) == 0, edge_next = !db->dense && (pos % 1024) == 1020;
  auto pass = [&](uint32_t sl) {
    return hg_slot_pass(db->ext[sl], folded, pf, nf, edge_prev ? 0u : 0xFFFFFFFFu, edge_next ? (HG_WINDOW_BYTES == 4 ? 0u : 0xFFu) : 0xFFFFFFFFu);
  };
  return (ha && pass(sla)) || (hb && pass(slb));
}

// What the verify pass meets at the CANDIDATES of a text (the positions the filter lets through: what the device kernel sees),
// and per candidate its class.  cls[i] for the i-th candidate at pos[i] (up to cap): bit 0 the direct table holds no such
// value, bit 1 the discriminated bucket is empty or skipped (zero pairs on the buckets-only path), bit 2 the bucket is not
// empty and holds no window of the value, bit 3 a selected discriminator byte lies before the text (at + lo < 0), bit 4 one
// lies at or behind nbytes, bit 5 at < 0 with every selected byte inside, bit 6 some literal verifies here.
// out[0] candidates, out[1..7] candidates with each bit.  Returns the number of candidates.
uint64_t hgsim_candidates(void *h, const uint8_t *text, uint64_t nbytes, uint64_t *out, uint64_t *pos_out, uint8_t *cls_out, uint64_t cap) {
  HgDb *db = static_cast<HgDb *>(h);
  const HgDbView v = view_of(db);
  for (int i = 0; i < 8; i++) out[i] = 0;
  if (!db->nreal_factors) return 0;
  const uint32_t step = db->dense ? db->dense : 4;
  uint64_t n = 0;
  for (uint64_t pos = 0; pos < nbytes; pos += step) {
    uint32_t w = 0;
    std::memcpy(&w, text + pos, nbytes - pos < 4 ? nbytes - pos : 4);
    if (!sim_filter_pass(db, v, text, nbytes, pos, w)) continue;
    const uint32_t folded = (w | v.fold_mask) & v.window_mask;
    uint8_t cls = 0;
    if (hg_wtab_find(v.wtab, v.wtab_mask, folded) == HG_WTAB_EMPTY) cls |= 1;
    const uint32_t hh = hg_hash_window(folded), d = v.disc[hh], sel = d >> 8;
    uint32_t key = 0, cnt = 0, j0 = 0;
    bool inside = true;
    if (sel) {
      const int64_t at = static_cast<int64_t>(pos) + static_cast<int8_t>(d & 0xFFu);
      const uint32_t lo = hg_ctz(sel), hi = 31u - hg_clz32(sel);
      if (at + static_cast<int64_t>(lo) < 0) cls |= 8;
      if (static_cast<uint64_t>(at + hi) >= nbytes && at + static_cast<int64_t>(hi) >= 0) cls |= 16;
      inside = !(cls & 24);
      if (inside && at < 0) cls |= 32;
      if (inside) {
        uint32_t x = 0;
        for (uint32_t q = lo; q <= hi; q++) x |= static_cast<uint32_t>(text[at + static_cast<int64_t>(q)]) << (8u * q);
        key = (x | v.fold_mask) & hg_disc_bytes(sel);
      }
    }
    if (inside) {
      const uint32_t h2 = hg_disc_bucket(hh, key);
      j0 = v.bucket_off2[h2];
      cnt = v.bucket_off2[h2 + 1] - j0;
    }
    bool seen = false;
    for (uint32_t t = 0; t < cnt; t++) seen = seen || v.windows2[j0 + t].value == folded;
    if (cnt == 0) cls |= 2;
    if (cnt && !seen) cls |= 4;
    bool any = false;
    hg_verify_window(v, text, nbytes, pos, w, [&](uint32_t, uint64_t, uint32_t) { any = true; });
    if (any) cls |= 64;
    out[0]++;
    for (int b = 0; b < 7; b++)
      if (cls >> b & 1) out[1 + b]++;
    if (n < cap) {
      pos_out[n] = pos;
      cls_out[n] = cls;
    }
    n++;
  }
  return n;
}
}
