// TEST-ONLY host harness (never shipped): the stream pass's first level with one byte of context (HgDb::filter_ctx,
// hg_db.h hg_slot_match_ctx) against the first + second level it stands in front of (HgDb::filter, hg_slot_pass), on the
// compiled tables and on texts.  The scalar mirror of Probe<LOG2, false> and drain_batch in hg_stream.hip.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"

extern "C" {

void *ctxsim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, unsigned n, char *err, size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  if (hgc_compile(exprs, flags, ids, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
int ctxsim_tune(void *h, const uint8_t *sample, size_t n) {
  std::string e;
  HgDb *tuned = nullptr;
  int rc = hgc_tune(static_cast<const HgDb *>(h), sample, n, &tuned, &e);
  if (rc != 0) return rc;
  *static_cast<HgDb *>(h) = std::move(*tuned);
  hgc_free(tuned);
  return 0;
}
void ctxsim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// out: filter_log2, wide, dense, fold_mask, windows, has filter_ctx, used slots, used slots that care about the context byte,
// filter_use_ctx (the stream pass runs the kernels with the context byte)
void ctxsim_info(void *h, uint32_t *out) {
  HgDb *db = static_cast<HgDb *>(h);
  out[0] = db->filter_log2;
  out[1] = db->filter_wide;
  out[2] = db->dense;
  out[3] = db->fold_mask;
  out[4] = db->nreal_factors ? static_cast<uint32_t>(db->windows.size()) : 0;
  out[5] = db->filter_ctx.size() == db->filter.size() && !db->filter.empty() ? 1 : 0;
  out[6] = out[7] = 0;
  out[8] = db->filter_use_ctx;
  if (out[5])
    for (size_t s = 0; s < db->filter_ctx.size(); s++) {
      if (!db->ext[s].nvalues) continue;
      out[6]++;
      if ((db->filter_ctx[s] >> 16) & ~HG_CTX_LOW) out[7]++;
    }
}

// Every window of every literal at its own offset passes the context test (1) with the literal's own bytes after it — in
// either case where the literal is caseless there —, (2) with every value of a byte that lies outside the literal and
// arbitrary bytes after it, (3) at a row edge, where the kernel has no next dword.  Returns the violations; *checks = tests made.
uint32_t ctxsim_windows(void *h, uint64_t *checks) {
  HgDb *db = static_cast<HgDb *>(h);
  uint32_t bad = 0;
  uint64_t n = 0;
  if (db->filter_ctx.size() != db->filter.size()) return 0xFFFFFFFFu;
  const uint32_t byte_mask = ((1u << db->filter_log2) - 1u) << 2;
  for (size_t wi = 0; wi < db->windows.size() && db->nreal_factors; wi++) {
    const HgWindow &w = db->windows[wi];
    const HgFactor &f = db->factors[w.factor_off >> 8];
    const uint32_t off = w.factor_off & 0xff;
    const uint32_t word = db->filter_ctx[hg_slot(w.value, db->weights_a, byte_mask) >> 2];
    const uint32_t key = hg_hash_window(w.value);
    // the candidates for each of the four bytes after the window
    std::vector<uint32_t> first;  // byte 0: the context byte
    if (off + 4 < f.len) {
      first.push_back(f.lit[off + 4]);
      if (hg_factor_cmask(f, off + 4) != 0xFF) first.push_back(f.lit[off + 4] ^ 0x20u);  // (stored in lower case)
    } else {
      for (uint32_t b = 0; b < 256; b++) first.push_back(b);
    }
    for (uint32_t b0 : first)
      for (uint32_t fill : {0u, 0xFFFFFF00u, 0x5A3C9600u}) {
        uint32_t next = b0 | fill;
        for (uint32_t b = 1; b < 4; b++)  // the literal's own bytes where it goes on
          if (off + 4 + b < f.len) next = (next & ~(0xFFu << (8 * b))) | (static_cast<uint32_t>(f.lit[off + 4 + b]) << (8 * b));
        n++;
        if (!hg_slot_match_ctx(word, key, next | db->fold_mask, true)) bad++;
      }
    for (uint32_t next : {0u, 0xFFFFFFFFu, 0x12345678u, 0x20202020u}) {
      n++;
      if (!hg_slot_match_ctx(word, key, next | db->fold_mask, false)) bad++;
    }
  }
  if (checks) *checks = n;
  return bad;
}

// The stream pass's filter levels over a text, dword by dword as the kernel sees them (rows of 1 KiB; bytes past the text
// read as zero; with filters of up to 16 KiB the drain has no neighbour across a row's edge and skips the condition there).
// out[0] dwords probed            out[1] pass the old first level        out[2] pass the new first level
// out[3] old first + second level (the parent's candidates)              out[4] the new path's candidates (drain_batch)
// out[5] VIOLATIONS: old first + second level pass, new first level rejects
// out[6] rows (wave-iterations)   out[7] rows with an old first-level match   out[8] rows with a new first-level match
// out[9] pass the old first level and not the new one (what the context byte is for; the new one also passes dwords the old
//        one does not: it keeps fewer bits of hash C)
void ctxsim_scan(void *h, const uint8_t *data, uint64_t nbytes, uint64_t *out) {
  HgDb *db = static_cast<HgDb *>(h);
  for (int i = 0; i < 10; i++) out[i] = 0;
  if (db->filter_ctx.size() != db->filter.size() || db->filter_wide || db->dense) { out[5] = ~0ull; return; }
  const uint32_t byte_mask = ((1u << db->filter_log2) - 1u) << 2, fold = db->fold_mask;
  const bool stash = db->filter_log2 <= 12;
  auto dword_at = [&](int64_t p) -> uint32_t {
    uint32_t x = 0;
    for (int b = 0; b < 4; b++)
      if (p + b >= 0 && static_cast<uint64_t>(p + b) < nbytes) x |= static_cast<uint32_t>(data[p + b]) << (8 * b);
    return x;
  };
  bool row_old = false, row_new = false;
  for (uint64_t pos = 0; pos < nbytes; pos += 4) {
    const uint32_t f = dword_at(static_cast<int64_t>(pos)) | fold;
    const uint32_t pf = dword_at(static_cast<int64_t>(pos) - 4) | fold, nf = dword_at(static_cast<int64_t>(pos) + 4) | fold;
    const uint32_t sl = hg_slot(f, db->weights_a, byte_mask) >> 2, key = hg_hash_window(f);
    const bool edge_prev = stash && pos % 1024 == 0, edge_next = stash && pos % 1024 == 1020;
    const bool l1_old = hg_slot_match(db->filter[sl], key);
    // (the hot loop has no right neighbour in a row's last lane whatever the filter's size; the drain decides)
    const bool l1_hot = hg_slot_match_ctx(db->filter_ctx[sl], key, nf, pos % 1024 != 1020);
    const bool l1_new = hg_slot_match_ctx(db->filter_ctx[sl], key, nf, !edge_next);
    const bool l2 = hg_slot_pass(db->ext[sl], f, pf, nf, edge_prev ? 0u : 0xFFFFFFFFu, edge_next ? 0u : 0xFFFFFFFFu);
    // drain_batch: a dword that is none of the slot's exact values (a crowded slot's `rest`) also answers to the old slot word
    const HgSlotInfo &info = db->ext[sl];
    const bool exact = (info.nvalues > 0 && info.value[0] == f) || (info.nvalues > 1 && info.value[1] == f);
    const bool cand_new = l1_hot && l1_new && (exact || l1_old) && l2;
    out[0]++;
    out[1] += l1_old;
    out[2] += l1_hot;
    out[3] += l1_old && l2;
    out[4] += cand_new;
    out[5] += (l1_old && l2 && !(l1_new && l1_hot)) ? 1 : 0;
    out[9] += (l1_old && !l1_hot) ? 1 : 0;
    row_old = row_old || l1_old;
    row_new = row_new || l1_hot;
    if (pos % 1024 == 1020 || pos + 4 >= nbytes) {
      out[6]++;
      out[7] += row_old;
      out[8] += row_new;
      row_old = row_new = false;
    }
  }
}
}
