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
  partssim_free(h);
  return bad;
}
}  // namespace

int main() {
  const unsigned A = 6, S = 8;  // DOTALL | MULTILINE, SINGLEMATCH
  std::string longrun(1000, 'q');
  const std::vector<Case> cases = {
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
  };
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
