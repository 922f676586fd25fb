// TEST-ONLY host replay of the tile scan (hg_tile_reduce / spine / apply_kernel, hypergrep_amd/csrc/hg_kernels.hip) with
// the functions of hg_post.h themselves: the kernels' decomposition restated thread by thread, so that hg_tile_combine and the
// structure built on it run under a CPU test.
//
//   4 tiles a thread (identity elements behind tile_end), a Hillis-Steele scan over the block's 256 threads with identity
//   padding on the left, the last thread's value as the block aggregate; the spine's rounds of 256 aggregates with the state
//   carried from round to round and chained through *state; the apply pass from each block's base.
//
// Every "thread" of a scan step reads the values the previous step left (the kernels separate the read and the write of a step
// with barriers): the replay keeps the old array beside the new one.
//
// tilesim_walk is the sequential walk every other host mirror uses (hg_tile_apply tile by tile).
// With -DTILESIM_MAIN the file is a program of its own: seeded synthetic summaries of up to 600 blocks (three spine rounds),
// ranges that begin on any tile, small scan buffers; the replay against the walk.  It is built with the sanitizers by
// tests/test_tile_cells.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_post.h"

namespace {
constexpr int TS_THREADS = 256;
constexpr int TS_PER_THREAD = 4;
constexpr uint64_t TS_BLOCK_TILES = TS_THREADS * TS_PER_THREAD;

HgTileElem identity_elem() {
  HgTileElem e;
  e.k1 = e.d = e.new_cs = 0;
  e.has_nl = 0;
  e.pad = 0;
  return e;
}

// block_scan of the kernels: sh[] holds every thread's inclusive value on return.
void block_scan(std::vector<HgTileElem> &sh, uint64_t bs1) {
  std::vector<HgTileElem> old(TS_THREADS);
  for (int o = 1; o < TS_THREADS; o <<= 1) {
    old = sh;  // (what the threads read before the step's barrier)
    for (int t = 0; t < TS_THREADS; t++) {
      HgTileElem left = identity_elem();
      if (t >= o) left = old[t - o];
      if (t >= o) sh[t] = hg_tile_combine(left, old[t], bs1);
    }
  }
}

HgTileElem thread_elems(const HgTileSum *sums, uint64_t tile_end, uint64_t first, uint64_t bs1, HgTileElem *each) {
  HgTileElem acc = identity_elem();
  for (int k = 0; k < TS_PER_THREAD; k++) {
    const uint64_t t = first + k;
    HgTileElem e = identity_elem();
    if (t < tile_end) e = hg_tile_elem(sums[t], t << HG_TILE_SHIFT);
    if (each) each[k] = e;
    acc = hg_tile_combine(acc, e, bs1);
  }
  return acc;
}

void reduce_block(const HgTileSum *sums, uint64_t tile_begin, uint64_t tile_end, uint64_t bs1, uint32_t block, HgTileElem *agg) {
  std::vector<HgTileElem> sh(TS_THREADS);
  for (int t = 0; t < TS_THREADS; t++) sh[t] = thread_elems(sums, tile_end, tile_begin + (static_cast<uint64_t>(block) * TS_THREADS + t) * TS_PER_THREAD, bs1, nullptr);
  block_scan(sh, bs1);
  agg[block] = sh[TS_THREADS - 1];
}

void spine(const HgTileElem *agg, uint32_t nblocks, uint64_t bs1, HgTileBase *block_base, HgTileBase *state) {
  HgTileBase carry = *state;
  std::vector<HgTileElem> sh(TS_THREADS);
  for (uint32_t base = 0; base < nblocks; base += TS_THREADS) {
    for (int t = 0; t < TS_THREADS; t++) {
      const uint32_t i = base + t;
      sh[t] = i < nblocks ? agg[i] : identity_elem();
    }
    block_scan(sh, bs1);
    const HgTileBase st = carry;
    for (int t = 0; t < TS_THREADS; t++) {
      const uint32_t i = base + t;
      HgTileElem excl = identity_elem();
      if (t > 0) excl = sh[t - 1];
      if (i < nblocks) block_base[i] = hg_tile_apply(st, excl, bs1);
    }
    carry = hg_tile_apply(st, sh[TS_THREADS - 1], bs1);
  }
  *state = carry;
}

void apply_block(const HgTileSum *sums, uint64_t tile_begin, uint64_t tile_end, uint64_t bs1, uint32_t block, const HgTileBase *block_base, HgTileBase *bases) {
  std::vector<HgTileElem> sh(TS_THREADS), each(static_cast<size_t>(TS_THREADS) * TS_PER_THREAD);
  for (int t = 0; t < TS_THREADS; t++)
    sh[t] = thread_elems(sums, tile_end, tile_begin + (static_cast<uint64_t>(block) * TS_THREADS + t) * TS_PER_THREAD, bs1, &each[static_cast<size_t>(t) * TS_PER_THREAD]);
  block_scan(sh, bs1);
  for (int t = 0; t < TS_THREADS; t++) {
    const uint64_t first = tile_begin + (static_cast<uint64_t>(block) * TS_THREADS + t) * TS_PER_THREAD;
    HgTileElem excl = identity_elem();
    if (t > 0) excl = sh[t - 1];
    HgTileBase st = hg_tile_apply(block_base[block], excl, bs1);
    for (int k = 0; k < TS_PER_THREAD; k++) {
      const uint64_t tt = first + k;
      if (tt < tile_end) bases[tt] = st;
      st = hg_tile_apply(st, each[static_cast<size_t>(t) * TS_PER_THREAD + k], bs1);
    }
  }
}
}  // namespace

extern "C" {

// The three launches over the tiles [tile_begin, tile_end) of `sums` (indexed by absolute tile, as are `bases`): state[0] = cs,
// state[1] = L at tile_begin on entry, at tile_end on return.  Returns the number of blocks.
uint32_t tilesim_scan(const HgTileSum *sums, uint64_t tile_begin, uint64_t tile_end, uint64_t bs1, uint64_t *state, HgTileBase *bases) {
  const uint32_t nblocks = static_cast<uint32_t>((tile_end - tile_begin + TS_BLOCK_TILES - 1) / TS_BLOCK_TILES);
  std::vector<HgTileElem> agg(nblocks);
  std::vector<HgTileBase> block_base(nblocks);
  for (uint32_t b = 0; b < nblocks; b++) reduce_block(sums, tile_begin, tile_end, bs1, b, agg.data());
  HgTileBase st{state[0], state[1]};
  spine(agg.data(), nblocks, bs1, block_base.data(), &st);
  for (uint32_t b = 0; b < nblocks; b++) apply_block(sums, tile_begin, tile_end, bs1, b, block_base.data(), bases);
  state[0] = st.cs;
  state[1] = st.L;
  return nblocks;
}

// The sequential walk: the state at each tile's start, tile after tile.
void tilesim_walk(const HgTileSum *sums, uint64_t tile_begin, uint64_t tile_end, uint64_t bs1, uint64_t *state, HgTileBase *bases) {
  HgTileBase st{state[0], state[1]};
  for (uint64_t t = tile_begin; t < tile_end; t++) {
    bases[t] = st;
    st = hg_tile_apply(st, hg_tile_elem(sums[t], t << HG_TILE_SHIFT), bs1);
  }
  state[0] = st.cs;
  state[1] = st.L;
}

// Combines the elements of tiles [a, b) in the tree order `split` chooses (0: left to right; otherwise halves, recursively)
// and applies the result to `state`: any bracketing of an associative operation gives the walk's result.
static HgTileElem tree(const HgTileSum *sums, uint64_t a, uint64_t b, uint64_t bs1, uint32_t split) {
  if (b == a) return identity_elem();
  if (b - a == 1) return hg_tile_elem(sums[a], a << HG_TILE_SHIFT);
  const uint64_t mid = split ? a + 1 + (static_cast<uint64_t>(split) * 2654435761u + a) % (b - a - 1) : b - 1;
  return hg_tile_combine(tree(sums, a, mid, bs1, split), tree(sums, mid, b, bs1, split), bs1);
}
void tilesim_tree(const HgTileSum *sums, uint64_t a, uint64_t b, uint64_t bs1, uint32_t split, uint64_t *state) {
  const HgTileBase st = hg_tile_apply(HgTileBase{state[0], state[1]}, tree(sums, a, b, bs1, split), bs1);
  state[0] = st.cs;
  state[1] = st.L;
}

void tilesim_sizes(uint32_t *out) {
  out[0] = sizeof(HgTileSum);
  out[1] = sizeof(HgTileBase);
  out[2] = sizeof(HgTileElem);
  out[3] = HG_TILE_BYTES;
}
}  // extern "C"

#ifdef TILESIM_MAIN
namespace {
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return static_cast<uint32_t>(rng_state >> 24);
}

// Summaries of a text nobody wrote out: per tile none, one, two or a few newlines; long runs of tiles without one (whole
// blocks, and once more than a spine round of blocks).  bs1 >= tile: inner = nl_count - 1.  bs1 < tile: the inner lines are
// given lengths here, and `inner` is their pieces.
std::vector<HgTileSum> synth(uint64_t ntiles, uint64_t bs1, uint32_t density) {
  std::vector<HgTileSum> s(ntiles);
  uint64_t run = 0;
  for (uint64_t t = 0; t < ntiles; t++) {
    HgTileSum &x = s[t];
    if (run == 0 && rnd() % 997 == 0) run = (rnd() % 4 == 0) ? 1024ull * (1 + rnd() % 300) + rnd() % 5 : 1 + rnd() % 1030;
    if (run || rnd() % 100 >= density) {
      if (run) run--;
      x = HgTileSum{0, HG_NONE32, HG_NONE32, 0};
      continue;
    }
    const uint32_t kind = rnd() % 4;
    if (kind == 0) {
      const uint32_t at = rnd() % 3 == 0 ? (rnd() % 2 ? 0u : HG_TILE_BYTES - 1) : rnd() % HG_TILE_BYTES;
      x = HgTileSum{1, at, at, 0};
    } else {
      uint32_t first = rnd() % (HG_TILE_BYTES / 2), last = HG_TILE_BYTES / 2 + rnd() % (HG_TILE_BYTES / 2);
      if (rnd() % 5 == 0) first = 0;
      if (rnd() % 5 == 0) last = HG_TILE_BYTES - 1;
      // inner lines: the stretch (first, last] cut into `more + 1` lines
      const uint32_t span = last - first, more = span > 8 ? rnd() % 4 : 0;
      uint64_t inner = 0;
      uint32_t left = span;
      for (uint32_t i = 0; i < more; i++) {
        const uint32_t len = 1 + rnd() % (left - (more - i));
        inner += hg_pieces(len, bs1);
        left -= len;
      }
      inner += hg_pieces(left, bs1);
      x = HgTileSum{more + 2, first, last, static_cast<uint32_t>(bs1 >= HG_TILE_BYTES ? more + 1 : inner)};
    }
  }
  return s;
}

int check(const std::vector<HgTileSum> &s, uint64_t tile_begin, uint64_t tile_end, uint64_t bs1, uint64_t cs0, uint64_t L0, const char *what) {
  // heap blocks of exactly the tiles the range covers: a read or write outside [tile_begin, tile_end) is the sanitizer's
  const uint64_t n = tile_end - tile_begin;
  std::vector<HgTileSum> own(s.begin() + tile_begin, s.begin() + tile_end);
  std::vector<HgTileBase> a(n), b(n);
  uint64_t sa[2] = {cs0, L0}, sb[2] = {cs0, L0}, sc[2] = {cs0, L0};
  tilesim_scan(own.data() - tile_begin, tile_begin, tile_end, bs1, sa, a.data() - tile_begin);
  tilesim_walk(own.data() - tile_begin, tile_begin, tile_end, bs1, sb, b.data() - tile_begin);
  tilesim_tree(own.data() - tile_begin, tile_begin, tile_end, bs1, 1 + rnd() % 1000, sc);
  if (sa[0] != sb[0] || sa[1] != sb[1] || sc[0] != sb[0] || sc[1] != sb[1]) {
    std::printf("%s: final state differs: scan (%llu, %llu), walk (%llu, %llu), tree (%llu, %llu)\n", what, (unsigned long long)sa[0], (unsigned long long)sa[1],
                (unsigned long long)sb[0], (unsigned long long)sb[1], (unsigned long long)sc[0], (unsigned long long)sc[1]);
    return 1;
  }
  for (uint64_t i = 0; i < n; i++)
    if (a[i].cs != b[i].cs || a[i].L != b[i].L) {
      std::printf("%s: tile %llu: scan (%llu, %llu), walk (%llu, %llu)\n", what, (unsigned long long)(tile_begin + i), (unsigned long long)a[i].cs, (unsigned long long)a[i].L,
                  (unsigned long long)b[i].cs, (unsigned long long)b[i].L);
      return 1;
    }
  return 0;
}
}  // namespace

int main() {
  int cases = 0;
  const uint64_t sizes[] = {1, 2, 3, 4, 5, 8, 9, 1023, 1024, 1025, 2047, 2048, 2049, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, 258 * 1024 + 5, 512 * 1024 + 1, 600 * 1024};
  const uint64_t bs1s[] = {8, 1000, 16383, 16384, 16385, 40000, 262139};
  for (uint64_t ntiles : sizes)
    for (uint64_t bs1 : bs1s) {
      if (ntiles > 300000 && bs1 != 262139 && bs1 != 1000 && bs1 != 16384) continue;
      for (uint32_t density : {3u, 60u, 100u}) {
        if (ntiles > 300000 && density == 60u) continue;
        const std::vector<HgTileSum> s = synth(ntiles, bs1, density);
        char what[128];
        std::snprintf(what, sizeof what, "%llu tiles, bs1 %llu, density %u", (unsigned long long)ntiles, (unsigned long long)bs1, density);
        if (check(s, 0, ntiles, bs1, 0, (1ull << 33) + 5, what)) return 1;
        cases++;
      }
    }
  // a text without a newline, and ranges in the middle of a text (a segment of a segmented scan: the state is the walk's)
  {
    std::vector<HgTileSum> none(3000, HgTileSum{0, HG_NONE32, HG_NONE32, 0});
    if (check(none, 0, 3000, 16384, 0, 7, "no newline")) return 1;
    cases++;
    const std::vector<HgTileSum> s = synth(5000, 40000, 50);
    std::vector<HgTileBase> walk(5000);
    uint64_t st[2] = {0, 0};
    tilesim_walk(s.data(), 0, 5000, 40000, st, walk.data());
    for (uint64_t begin : {1ull, 2ull, 3ull, 5ull, 16ull, 528ull, 1023ull, 1040ull, 2049ull}) {
      std::vector<HgTileBase> a(5000);
      uint64_t sa[2] = {walk[begin].cs, walk[begin].L};
      tilesim_scan(s.data(), begin, 5000, 40000, sa, a.data());
      for (uint64_t t = begin; t < 5000; t++)
        if (a[t].cs != walk[t].cs || a[t].L != walk[t].L) {
          std::printf("range from %llu: tile %llu differs\n", (unsigned long long)begin, (unsigned long long)t);
          return 1;
        }
      if (sa[0] != st[0] || sa[1] != st[1]) return 1;
      cases++;
    }
  }
  std::printf("%d cases ok\n", cases);
  return 0;
}
#endif
