// TEST-ONLY host harness for the parts stage (never shipped): compiles the product's pattern compiler and the scalar
// reference routines of hg_parts.h for x86.  One call gives the parts of one trimmed line piece over all expressions of a
// database, which is what the GPU stage (hg_parts.hip) must reproduce for every piece that has a hit.
// With -DPARTSSIM_MAIN the file is a program of its own over a fixed table (the sanitized run of tests/test_parts_host.py).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_compile.h"
#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_parts.h"

extern "C" {

// ext_min_offset (or NULL): per expression, a non-zero value compiles it with hs_expr_ext_t{HS_EXT_FLAG_MIN_OFFSET, value}
void *partssim_compile(const char *const *exprs, const unsigned *flags, const unsigned *ids, const unsigned long long *ext_min_offset, unsigned n, char *err,
                       size_t errlen) {
  HgDb *db = nullptr;
  std::string e;
  int bad = -1;
  std::vector<hs_expr_ext_t> ext(n);
  std::vector<const hs_expr_ext_t *> extp(n, nullptr);
  for (unsigned i = 0; ext_min_offset && i < n; i++)
    if (ext_min_offset[i]) {
      ext[i] = hs_expr_ext_t{HS_EXT_FLAG_MIN_OFFSET, ext_min_offset[i], 0, 0, 0, 0};
      extp[i] = &ext[i];
    }
  if (hgc_compile_ext(exprs, flags, ids, ext_min_offset ? extp.data() : nullptr, n, &db, &e, &bad) != 0) {
    if (err && errlen) snprintf(err, errlen, "%d: %s", bad, e.c_str());
    return nullptr;
  }
  return db;
}
void partssim_free(void *h) { hgc_free(static_cast<HgDb *>(h)); }

// why the stage is not offered for the database (the engine's text), or NULL
const char *partssim_refusal(void *h) {
  const HgDb *db = static_cast<const HgDb *>(h);
  return hg_parts_refusal(db->nhuge, db->ncomb, db->nquiet, db->n_ext != 0);
}

// {max state words, simple of expression 0, nodes of expression 0}
void partssim_info(void *h, uint32_t *out) {
  const HgDb *db = static_cast<const HgDb *>(h);
  out[0] = db->max_nw;
  out[1] = db->patterns[0].simple;
  out[2] = db->patterns[0].nnodes;
}

// The parts of one piece data[0, len): out = {from, to, pattern} per part, in order.  Returns the count, -1 if out is too small.
long partssim_piece(void *h, const uint8_t *data, uint32_t len, uint32_t *out, size_t cap) {
  const HgDb *db = static_cast<const HgDb *>(h);
  size_t n = 0;
  uint32_t cursor = 0, from, to, pattern;
  while (hg_parts_next(db->pool.data(), db->patterns.data(), static_cast<uint32_t>(db->patterns.size()), data, len, cursor, &from, &to, &pattern)) {
    if (n >= cap) return -1;
    out[3 * n] = from;
    out[3 * n + 1] = to;
    out[3 * n + 2] = pattern;
    n++;
    cursor = to;
  }
  return static_cast<long>(n);
}

// {state words, simple, nodes} of expression `index`; returns the number of expressions (out untouched when index is past it)
uint32_t partssim_pattern_info(void *h, uint32_t index, uint32_t *out) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const uint32_t n = static_cast<uint32_t>(db->patterns.size());
  if (index < n) {
    out[0] = db->patterns[index].nw;
    out[1] = db->patterns[index].simple;
    out[2] = db->patterns[index].nnodes;
  }
  return n;
}

// The kernels' decomposition of one piece, replayed lane by lane: groups of 64 candidate starts from `base`; per start
// hg_parts_at over the expressions the first-byte rule admits (some word of init & reach[data[s]] is not empty: restated here
// from the tables, the engine's copy builds the device bitmap), in ascending order; then the ballot / cursor / base loop as
// hg_parts.hip and hg_segparts.hip write it.
//   out    {from, to, pattern, tie} per part; tie = 1 when an expression of ANOTHER 32-expression bitmap word reaches the same end
//   trace  {base, ballot rounds, outrun} per group; outrun = starts of the group that had a match, were never taken and whose
//          match ends behind the accepted end that hid them
// Returns the parts, -1 if out is too small, -2 if trace is; *n_groups = groups walked.
long partssim_piece_grouped(void *h, const uint8_t *data, uint32_t len, uint32_t *out, size_t cap, uint32_t *trace, size_t trace_cap, uint32_t *n_groups) {
  const HgDb *db = static_cast<const HgDb *>(h);
  const uint32_t *pool = db->pool.data();
  const uint32_t np = static_cast<uint32_t>(db->patterns.size());
  size_t n = 0, g = 0;
  uint32_t cursor = 0;
  std::vector<HgPattern> admitted;
  std::vector<uint32_t> index;
  for (uint32_t base = 0; base < len;) {
    uint32_t to[64], pattern[64], tie[64];
    bool taken[64];
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint32_t s = base + lane;
      to[lane] = pattern[lane] = tie[lane] = 0;
      taken[lane] = false;
      if (s >= len) continue;
      admitted.clear();
      index.clear();
      for (uint32_t j = 0; j < np; j++) {
        const HgPattern &p = db->patterns[j];
        if (p.nw == 0 || p.nw > HG_MAX_W) continue;
        const uint32_t *init = pool + p.init_off, *reach = pool + p.reach_off + data[s] * p.nw;
        uint32_t any = 0;
        for (uint32_t w = 0; w < p.nw; w++) any |= init[w] & reach[w];
        if (any) {
          admitted.push_back(p);
          index.push_back(j);
        }
      }
      uint32_t e = 0, who = 0;
      if (admitted.empty() || !hg_parts_at(pool, admitted.data(), static_cast<uint32_t>(admitted.size()), data, len, s, &e, &who)) continue;
      to[lane] = e;
      pattern[lane] = index[who];
      for (size_t k = 0; k < admitted.size(); k++) {
        uint32_t e1 = 0, w1 = 0;
        if ((index[k] >> 5) != (pattern[lane] >> 5) && hg_parts_at(pool, &admitted[k], 1, data, len, s, &e1, &w1) && e1 == e) tie[lane] = 1;
      }
    }
    uint32_t rounds = 0, outrun = 0;
    uint32_t shadow[64];  // the accepted end that hides the lane's start, 0 while nothing does
    for (uint32_t lane = 0; lane < 64; lane++) shadow[lane] = base + lane < cursor ? cursor : 0;
    for (;;) {
      int w = -1;  // the ballot over to != 0 && s >= cursor, and its lowest lane
      for (int lane = 0; lane < 64 && w < 0; lane++)
        if (to[lane] != 0 && base + static_cast<uint32_t>(lane) >= cursor) w = lane;
      if (w < 0) break;
      if (n >= cap) return -1;
      out[4 * n] = base + static_cast<uint32_t>(w);
      out[4 * n + 1] = to[w];
      out[4 * n + 2] = pattern[w];
      out[4 * n + 3] = tie[w];
      n++;
      rounds++;
      taken[w] = true;
      cursor = to[w];
      for (uint32_t lane = static_cast<uint32_t>(w) + 1; lane < 64 && base + lane < cursor; lane++)
        if (!shadow[lane]) shadow[lane] = cursor;
    }
    for (int lane = 0; lane < 64; lane++) outrun += to[lane] != 0 && !taken[lane] && to[lane] > shadow[lane];
    if (g >= trace_cap) return -2;
    trace[3 * g] = base;
    trace[3 * g + 1] = rounds;
    trace[3 * g + 2] = outrun;
    g++;
    base = cursor > base + 64 ? cursor : base + 64;
  }
  *n_groups = static_cast<uint32_t>(g);
  return static_cast<long>(n);
}

}  // extern "C"

#ifdef PARTSSIM_MAIN
namespace {
struct Case {
  std::vector<const char *> exprs;
  std::vector<unsigned> flags;
  std::string piece;
  std::vector<std::vector<uint32_t>> want;  // {from, to, pattern}
};

int run(const Case &c, int index) {
  char err[256] = "";
  std::vector<unsigned> ids(c.exprs.size(), 0);
  void *h = partssim_compile(c.exprs.data(), c.flags.data(), ids.data(), nullptr, static_cast<unsigned>(c.exprs.size()), err, sizeof err);
  if (!h) {
    printf("case %d: compile failed: %s\n", index, err);
    return 1;
  }
  // (the piece in a heap block of its exact size: a read past either end is the sanitizer's to catch)
  std::vector<uint8_t> data(c.piece.begin(), c.piece.end());
  std::vector<uint32_t> out(3 * (data.size() + 1));
  const long n = partssim_piece(h, data.data(), static_cast<uint32_t>(data.size()), out.data(), data.size() + 1);
  int bad = n != static_cast<long>(c.want.size());
  for (long i = 0; !bad && i < n; i++)
    for (int k = 0; k < 3; k++) bad |= out[3 * i + k] != c.want[i][k];
  if (bad) {
    printf("case %d: got %ld parts:", index, n);
    for (long i = 0; i < n; i++) printf(" [%u,%u)#%u", out[3 * i], out[3 * i + 1], out[3 * i + 2]);
    printf("\n");
  }
  // the grouped replay of the same piece, its outputs in heap blocks of their exact sizes too
  std::vector<uint32_t> gout(4 * (data.size() + 1)), trace(3 * (data.size() + 1));
  uint32_t groups = 0;
  const long gn = partssim_piece_grouped(h, data.data(), static_cast<uint32_t>(data.size()), gout.data(), data.size() + 1, trace.data(), data.size() + 1, &groups);
  int gbad = gn != static_cast<long>(c.want.size());
  for (long i = 0; !gbad && i < gn; i++)
    for (int k = 0; k < 3; k++) gbad |= gout[4 * i + k] != c.want[i][k];
  if (gbad) {
    printf("case %d, grouped: got %ld parts in %u groups:", index, gn, groups);
    for (long i = 0; i < gn; i++) printf(" [%u,%u)#%u", gout[4 * i], gout[4 * i + 1], gout[4 * i + 2]);
    printf("\n");
  }
  bad |= gbad;
  partssim_free(h);
  return bad;
}
}  // namespace

int main() {
  const unsigned A = 6, S = 8;  // DOTALL | MULTILINE, SINGLEMATCH
  std::string longrun(1000, 'q');
  // Ten pieces after cells of tests/parts_cells.py, restated here (the hit line alone, without the cell's lines around it;
  // the cell each follows stands behind it).  They are this program's own table: the cells themselves are compared with
  // both replays, unsanitized, by tests/test_parts_cells.py.
  const std::string dots5(5, '.'), dots63(63, '.');
  auto kz = [](size_t n) { return "k" + std::string(n - 2, 'a') + "z"; };
  std::vector<std::vector<uint32_t>> ones65, seam;
  for (uint32_t i = 0; i < 65; i++) ones65.push_back({i, i + 1, 0});
  std::string xy40;
  for (uint32_t i = 0; i < 40; i++) {
    seam.push_back({2 * i, 2 * i + 2, 0});
    xy40 += "XY";
  }
  std::vector<Case> cases = {
      {{"k[a-z]{0,50}z", "XY"}, {A, A}, std::string(20, '.') + kz(52) + "XY", {{20, 72, 0}, {72, 74, 1}}},  // A1/R2: a part of the tier's longest length, XY at the cursor
      {{"k[a-z]{0,70}z", "XY"}, {A, A}, dots63 + kz(66) + "XY.." + kz(66), {{63, 129, 0}, {129, 131, 1}, {133, 199, 0}}},  // A2/L3 66 from 63, second at +0
      {{"k[a-z]{0,1000}z", "XY"}, {A, A}, dots5 + kz(200) + dots63 + "XY..." + kz(129) + ".kaz", {{5, 205, 0}, {268, 270, 1}, {273, 402, 0}, {403, 406, 0}}},  // A2 200 from 5, second at +63, with L32 itself
      {{"ab{6}", "bbbx", "xq"}, {A, A, A}, "abbbbbbxq bbbx", {{0, 7, 0}, {7, 9, 2}, {10, 14, 1}}},  // A3/S
      {{"q|XY|k[a-z]{0,70}z"}, {A}, std::string(65, 'q'), ones65},  // A4/L3 65 adjacent
      {{"q|XY|k[a-z]{0,70}z"}, {A}, xy40, seam},  // A4/L3 two-byte parts, seam on the edge
      {{"foo\\b"}, {A}, "xxx foo", {{4, 7, 0}}},  // B1/foo\\b: piece ends before a word byte (its first piece)
      {{"foo[a-z]{0,70}$"}, {2}, "xfooab", {{1, 6, 0}}},  // B2/foo[a-z]{0,70}$ flags 2: dollar at an unterminated end
      {{"^f$"}, {A}, "f", {{0, 1, 0}}},  // B3/^f$: one-byte last line
      {{"\\Bf"}, {A}, "f", {}},  // B3/\\Bf: one-byte last line
  };
  cases.insert(cases.end(), {
      {{"a|aaa"}, {A}, "aaaa\n", {{0, 3, 0}, {3, 4, 0}}},
      {{"abcd", "bc"}, {A, A}, "xabcdx\n", {{1, 5, 0}}},
      {{"ab", "abc"}, {A, A}, "abcab\n", {{0, 3, 1}, {3, 5, 0}}},
      {{"abc", "ab|abc"}, {A, A}, "abcab\n", {{0, 3, 0}, {3, 5, 1}}},
      {{"ab"}, {A}, "ababab\n", {{0, 2, 0}, {2, 4, 0}, {4, 6, 0}}},
      {{"^a"}, {A}, "aaa\n", {{0, 1, 0}}},
      {{"\\bfoo"}, {A}, "foo xfoo foofoo\n", {{0, 3, 0}, {9, 12, 0}}},
      {{"a+$"}, {A}, "baaa\n", {{1, 4, 0}}},
      {{"a+$"}, {2}, "baaa\n", {{1, 4, 0}}},
      {{"a+$"}, {2}, "baaa", {{1, 4, 0}}},
      {{"hello"}, {A | 1}, "HeLLo hello\n", {{0, 5, 0}, {6, 11, 0}}},
      {{"foo.*"}, {A}, "xfoo bar\n", {{1, 9, 0}}},
      {{"foo.*"}, {4}, "xfoo bar\n", {{1, 8, 0}}},
      {{"x\\d{2,40}y"}, {A}, "x12y x1y x123456789012y\n", {{0, 4, 0}, {9, 23, 0}}},
      {{"[a-z]{1000}x"}, {A}, longrun + "x\n", {{0, 1001, 0}}},
      {{"[a-z]{1000}x"}, {A}, longrun.substr(1) + "x\n", {}},
      {{"foo", "o+"}, {A | S, A | S}, "foo boo\n", {{0, 3, 0}, {5, 7, 1}}},
      {{"b"}, {A}, "b", {{0, 1, 0}}},
      {{"zz"}, {A}, "z\n", {}},
  });
  int failed = 0;
  for (size_t i = 0; i < cases.size(); i++) failed += run(cases[i], static_cast<int>(i));
  if (failed) {
    printf("%d cases FAILED\n", failed);
    return 1;
  }
  printf("%zu cases ok\n", cases.size());
  return 0;
}
#endif
