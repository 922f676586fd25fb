// TEST-ONLY host harness for the per-file parts stage (never shipped): compiles the product's pattern compiler, the scalar
// rules of hg_segparts.h (head, address, first_part) and the walk of hg_parts.h for x86, and replays the stage's steps over
// the surviving, file-relative records of a segment pass: count per record, exclusive scan, ordered write, first_part.  What
// the GPU stage (hg_segparts.hip) must reproduce; its lane logic (ballots, LDS state) is covered by the GPU tests only.
// With -DSEGPARTSSIM_MAIN the file is a program of its own over a fixed case (a sanitized run: each piece is walked in a heap
// block of its exact size, so a read outside [0, len) is the sanitizer's to catch).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_parts.h"
#include "../../hypergrep_amd/csrc/hg_segparts.h"

extern "C" {

void *segpartssim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, unsigned n, char *err, size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  if (hgc_compile_ext(exprs, flags, ids, nullptr, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
void segpartssim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// recs: n surviving records {line, id, to, start, len} (file-relative, uint64 each), seg_of their segments; seg_start, first_record
// (n_seg + 1) as the segment stage leaves them.  out: {line, from, to, pattern, segment} per part (uint64 each, room for cap);
// first_part: n_seg + 1.  exact != 0: every piece is copied into a heap block of its exact size before it is walked.
// Returns the number of parts, -1 if out is too small, -2 if the write pass disagrees with the count pass.
long segpartssim_run(void *h, const uint8_t *text, const uint64_t *recs, const uint32_t *seg_of, uint64_t n, const uint64_t *seg_start, uint64_t n_seg,
                     const uint64_t *first_record, uint64_t *out, uint64_t cap, uint64_t *first_part, int exact) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const uint32_t npatterns = static_cast<uint32_t>(db->patterns.size());
  std::vector<HgHit> hits(n + 1);
  std::vector<HgHitAux> aux(n + 1);
  for (uint64_t i = 0; i < n; i++) {
    hits[i] = HgHit{recs[5 * i], static_cast<uint32_t>(recs[5 * i + 1]), static_cast<uint32_t>(recs[5 * i + 2])};
    aux[i] = HgHitAux{recs[5 * i + 3], static_cast<uint32_t>(recs[5 * i + 4]), 0};
  }
  std::vector<uint64_t> count(n + 1, 0), pos(n + 1, 0);
  for (int write = 0; write < 2; write++) {
    for (uint64_t i = 0; i < n; i++) {
      if (!hg_segparts_head(hits.data(), seg_of, i)) continue;
      const uint32_t s = seg_of[i], len = aux[i].len;
      const uint8_t *data = text + hg_segparts_offset(seg_start, s, aux[i]);
      std::vector<uint8_t> block;
      if (exact) {
        block.assign(data, data + len);
        block.shrink_to_fit();
        data = block.data();
      }
      uint64_t k = 0;
      uint32_t cursor = 0, from, to, pattern;
      while (cursor < len && hg_parts_next(db->pool.data(), db->patterns.data(), npatterns, data, len, cursor, &from, &to, &pattern)) {
        if (write) {
          if (pos[i] + k >= cap) return -1;
          uint64_t *o = out + 5 * (pos[i] + k);
          o[0] = hits[i].line_no;
          o[1] = from;
          o[2] = to;
          o[3] = pattern;
          o[4] = s;
        }
        k++;
        cursor = to;
      }
      if (write && k != count[i]) return -2;
      count[i] = k;
    }
    if (!write) {
      uint64_t sum = 0;
      for (uint64_t i = 0; i <= n; i++) {
        pos[i] = sum;
        sum += count[i];
      }
    }
  }
  for (uint64_t s = 0; s <= n_seg; s++) first_part[s] = hg_segparts_first(pos.data(), first_record, s);
  return static_cast<long>(pos[n]);
}

}  // extern "C"

#ifdef SEGPARTSSIM_MAIN
// Two one-line files that both match on their line 0, an unterminated file with its pad, and a file whose second line matches.
int main() {
  const char *exprs[] = {"abc$", "q+"};
  const unsigned flags[] = {10, 14}, ids[] = {1, 2};
  char err[256] = "";
  void *h = segpartssim_compile(exprs, flags, ids, 2, err, sizeof err);
  if (!h) {
    printf("compile failed: %s\n", err);
    return 1;
  }
  const std::string text = std::string("abc\n") + "abc\n" + "qq abc" + std::string("\0\n", 2) + "x\nqabc\n";
  const uint64_t seg_start[] = {0, 4, 8, 16}, first_record[] = {0, 1, 2, 4, 6};
  // {line, id, to, start, len}
  const uint64_t recs[] = {0, 1, 4, 0, 4, 0, 1, 4, 0, 4, 0, 2, 2, 0, 6, 0, 1, 6, 0, 6, 1, 2, 1, 2, 5, 1, 1, 5, 2, 5};
  const uint32_t seg_of[] = {0, 1, 2, 2, 3, 3};
  const uint64_t want[][5] = {{0, 0, 3, 0, 0}, {0, 0, 3, 0, 1}, {0, 0, 2, 1, 2}, {0, 3, 6, 0, 2}, {1, 0, 1, 1, 3}, {1, 1, 4, 0, 3}};
  const uint64_t want_first[] = {0, 1, 2, 4, 6};
  std::vector<uint8_t> heap(text.begin(), text.end());
  uint64_t out[5 * 16], first_part[5];
  const long n = segpartssim_run(h, heap.data(), recs, seg_of, 6, seg_start, 4, first_record, out, 16, first_part, 1);
  int bad = n != 6;
  for (long i = 0; !bad && i < n; i++)
    for (int k = 0; k < 5; k++) bad |= out[5 * i + k] != want[i][k];
  for (int s = 0; !bad && s < 5; s++) bad |= first_part[s] != want_first[s];
  if (bad) {
    printf("got %ld parts:", n);
    for (long i = 0; i < n && i < 16; i++) printf(" {%llu [%llu,%llu)#%llu seg %llu}", (unsigned long long)out[5 * i], (unsigned long long)out[5 * i + 1],
                                                  (unsigned long long)out[5 * i + 2], (unsigned long long)out[5 * i + 3], (unsigned long long)out[5 * i + 4]);
    printf("\nFAILED\n");
  } else {
    printf("segparts case ok\n");
  }
  segpartssim_free(h);
  return bad;
}
#endif
