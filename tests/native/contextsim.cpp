// TEST-ONLY host harness for the context stage (never shipped): compiles the scalar routines of hg_context.h for x86 and
// replays the stage over tiles of ANY size: the tile summaries and prefix states the scan would leave (hg_post.h's monoid, one
// tile after the other), the textless count of each tile from those states and the hit lines alone, then the piece walk of the
// tile with the class of each piece and the trim rule.  The two must agree tile by tile; the records are what the GPU must
// write.  With -DCONTEXTSIM_MAIN it is a stand-alone program (for a sanitized build) that runs corner cases against a
// piece-by-piece restatement of the definition.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_context.h"
#include "../../hypergrep_amd/csrc/hg_post.h"

extern "C" {

// text[0, nbytes) in tiles of `tile` bytes, pieces of at most bs1 bytes numbered from line_base; hit_lines: the line numbers
// of the call's records, ascending, repeats allowed.  out receives {line_number, start, len, id, to, pattern} per context or
// tail piece; info = {owed_after, n_tail, n_pieces}.  Returns the number of records; -1: cap too small; -2: a tile's count
// (from the states) and its walk disagree; -3: the tiles' first piece numbers and the piece total disagree; -4: the counted
// tail records and the walked ones disagree.
long contextsim_run(const uint8_t *text, uint64_t nbytes, uint64_t tile, uint64_t bs1, uint64_t line_base, const uint64_t *hit_lines, uint64_t n_hits,
                    uint32_t before, uint32_t after, uint64_t carry_after, int tail, uint64_t *out, uint64_t cap, uint64_t *info) {
  const uint64_t ntiles = (nbytes + tile - 1) / tile;
  std::vector<HgHit> hits(n_hits);
  for (uint64_t i = 0; i < n_hits; i++) hits[i] = HgHit{hit_lines[i], 7, 1};
  std::vector<HgTileSum> sums(ntiles);
  std::vector<HgTileBase> bases(ntiles + 1);
  HgTileBase st{0, line_base};
  for (uint64_t t = 0; t < ntiles; t++) {
    const uint64_t t0 = t * tile, t1 = t0 + tile < nbytes ? t0 + tile : nbytes;
    HgTileSum s{0, HG_NONE32, HG_NONE32, 0};
    for (uint64_t i = t0; i < t1; i++)
      if (text[i] == '\n') {
        if (!s.nl_count++) s.first_nl = static_cast<uint32_t>(i - t0);
        s.last_nl = static_cast<uint32_t>(i - t0);
      }
    if (s.nl_count) s.inner = static_cast<uint32_t>(hg_inner_pieces(text, t0 + s.first_nl + 1, t0 + s.last_nl + 1, bs1));
    sums[t] = s;
    bases[t] = st;
    st = hg_tile_apply(st, hg_tile_elem(s, t0), bs1);
  }
  const uint64_t n_pieces = st.L - line_base + (nbytes > st.cs ? hg_pieces(nbytes - st.cs, bs1) : 0);  // (as HgScanner::run_once)
  const HgContextWin w = hg_context_win(line_base, n_pieces, before, after, carry_after, tail != 0);
  info[0] = hg_context_owed(n_hits, n_hits ? hits[n_hits - 1].line_no : 0, line_base, n_pieces, after, carry_after);
  info[1] = 0;
  info[2] = n_pieces;
  auto bounds = [&](uint64_t t, uint64_t *t0, uint64_t *t1) {
    *t0 = t * tile;
    *t1 = *t0 + tile < nbytes ? *t0 + tile : nbytes;
  };
  auto first_piece = [&](uint64_t t) {
    uint64_t t0, t1;
    bounds(t, &t0, &t1);
    return hg_invert_first_piece(bases[t], sums[t], t0, t1, bs1);
  };
  uint64_t n = 0, expect_first = line_base, tails_counted = 0, tails_walked = 0;
  for (uint64_t t = 0; t < ntiles; t++) {
    uint64_t t0, t1;
    bounds(t, &t0, &t1);
    const uint64_t f0 = first_piece(t), f1 = t + 1 < ntiles ? first_piece(t + 1) : w.end_piece;
    if (f0 != expect_first || f1 < f0) return -3;
    expect_first = f1;
    // the count pass of hg_context_count_kernel, one record after the other
    const HgContextTile ct = hg_context_tile(hits.data(), n_hits, f0, f1, w);
    int64_t sum = 0, sum_plain = 0;
    for (uint64_t i = ct.r0; i < ct.r1; i++) {
      sum += hg_context_contrib(hits.data(), i, ct, ct.whi, w);
      sum_plain += hg_context_contrib(hits.data(), i, ct, f1, w);
    }
    const uint64_t count = hg_context_count(ct, ct.whi, sum);
    if (ct.whi < f1) tails_counted += count - hg_context_count(ct, f1, sum_plain);
    uint64_t walked = 0;
    bool full = false;
    hg_context_walk_tile(text, bases[t], sums[t], t0, t1, bs1, hits.data(), n_hits, w, [&](uint64_t q, uint64_t ps, uint32_t cls) {
      walked++;
      tails_walked += cls == HG_CTX_TAIL ? 1 : 0;
      if (n >= cap) {
        full = true;
        return;
      }
      uint64_t a, z;
      hg_trim_piece(text, ps, ps + bs1 < nbytes ? ps + bs1 : nbytes, a, z);
      HgHit h;
      HgHitAux x;
      hg_context_record(q, a, z, cls, &h, &x);
      uint64_t *o = out + 6 * n++;
      o[0] = h.line_no, o[1] = x.start, o[2] = x.len, o[3] = h.id, o[4] = h.to, o[5] = x.pattern;
    });
    if (full) return -1;
    if (walked != count) return -2;
  }
  if (ntiles == 0 && w.end_piece != line_base) return -3;
  if (tails_counted != tails_walked) return -4;
  info[1] = tails_walked;
  return static_cast<long>(n);
}

}  // extern "C"

#ifdef CONTEXTSIM_MAIN
#include <algorithm>
#include <cstdio>
#include <string>

// The definition, piece by piece: is q (not a match) context, tail, or nothing?
static uint32_t class_by_definition(const std::vector<uint64_t> &lines, uint64_t q, uint64_t line_base, uint64_t n_pieces, uint64_t before, uint64_t after,
                                    uint64_t carry_after, bool tail) {
  const auto at = std::lower_bound(lines.begin(), lines.end(), q);  // (ascending) the first line at or after q
  if (at != lines.end() && *at == q) return HG_CTX_MATCH;
  if (at != lines.end() && *at - q <= before) return HG_CTX_CONTEXT;
  if (at != lines.begin() && q - *(at - 1) <= after) return HG_CTX_CONTEXT;
  if (q - line_base < carry_after) return HG_CTX_CONTEXT;
  if (tail && line_base + n_pieces - q <= before) return HG_CTX_TAIL;
  return HG_CTX_NONE;
}

int main() {
  std::string text;
  for (int i = 0; i < 120; i++) {  // empty lines, NULs, a line longer than every tile below, no final newline
    if (i % 7 == 3) text += "\n";
    else if (i % 11 == 5) text += std::string("a\0b\0\0c", 6) + "\n";
    else if (i == 60) text += std::string(300, 'x') + "\n";
    else text += "line " + std::to_string(i) + "\n";
  }
  text += "tail without newline";
  const uint8_t *data = reinterpret_cast<const uint8_t *>(text.data());
  const uint64_t nbytes = text.size();
  std::vector<uint64_t> out(6 * (nbytes + 1));
  long cases = 0;
  for (uint64_t bs1 : {2ull, 7ull, 63ull, 1024ull})
    for (uint64_t tile : {4ull, 7ull, 64ull, 16384ull})
      for (uint64_t line_base : {0ull, (1ull << 33) + 7})
        for (auto ba : {std::pair<uint32_t, uint32_t>{0, 0}, {1, 0}, {0, 1}, {2, 3}, {5, 1}, {1000, 1000}, {0xFFFFFFFFu, 0xFFFFFFFFu}})
          for (uint64_t carry : {0ull, 1ull, 100000ull})
            for (int tail = 0; tail < 2; tail++)
              for (int set = 0; set < 6; set++) {
                uint64_t info[3];
                // the piece count first (no hits), then the hit set from it
                long n = contextsim_run(data, nbytes, tile, bs1, line_base, nullptr, 0, 0, 0, 0, 0, out.data(), nbytes + 1, info);
                if (n != 0) return std::printf("piece count failed: %ld\n", n), 1;
                const uint64_t n_pieces = info[2];
                std::vector<uint64_t> lines;
                for (uint64_t q = 0; q < n_pieces; q++) {
                  const bool hit = set == 0 ? false : set == 1 ? true : set == 2 ? q == 0 : set == 3 ? q + 1 == n_pieces : set == 4 ? q % 17 == 4 || q % 17 == 9 : q % 3 != 1;
                  if (hit) lines.push_back(line_base + q);
                  if (hit && set == 4) lines.push_back(line_base + q);  // several records per line
                }
                n = contextsim_run(data, nbytes, tile, bs1, line_base, lines.data(), lines.size(), ba.first, ba.second, carry, tail, out.data(), nbytes + 1, info);
                if (n < 0) return std::printf("replay failed: %ld (bs1 %llu tile %llu set %d)\n", n, (unsigned long long)bs1, (unsigned long long)tile, set), 1;
                uint64_t k = 0;
                for (uint64_t q = line_base; q < line_base + n_pieces; q++) {
                  const uint32_t cls = class_by_definition(lines, q, line_base, n_pieces, ba.first, ba.second, carry, tail != 0);
                  if (cls != HG_CTX_CONTEXT && cls != HG_CTX_TAIL) continue;
                  if (k >= static_cast<uint64_t>(n) || out[6 * k] != q || out[6 * k + 3] != (cls == HG_CTX_TAIL ? HG_CTX_ID_TAIL : HG_CTX_ID_CONTEXT))
                    return std::printf("record %llu differs (bs1 %llu tile %llu set %d)\n", (unsigned long long)k, (unsigned long long)bs1, (unsigned long long)tile, set), 1;
                  k++;
                }
                if (k != static_cast<uint64_t>(n)) return std::printf("%ld records, %llu expected\n", n, (unsigned long long)k), 1;
                cases++;
              }
  std::printf("contextsim: %ld cases ok\n", cases);
  return 0;
}
#endif
