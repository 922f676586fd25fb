// TEST-ONLY host harness for the per-file context stage (never shipped): compiles the scalar routines of hg_segctx.h for x86
// and replays the stage over tiles of ANY size: the tile states the scan would leave (hg_post.h's monoid), the segments' line
// bases by a plain piece walk (how the device finds them is segsim.cpp's subject), their runs (hg_seg_run), then what
// hg_segctx.hip does: the kept records in packed piece numbers with their segments' windows, the textless count of each tile
// (hg_segctx_contrib) next to the piece walk of the tile with the class of each piece (hg_segctx_walk_tile) — the two must
// agree tile by tile —, the records made file-relative and the per-segment offsets.  With -DSEGCTXSIM_MAIN it is a
// stand-alone program (for a sanitized build) that runs packs against a piece-by-piece restatement of the rules.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_core.h"
#include "../../hypergrep_amd/csrc/hg_post.h"
#include "../../hypergrep_amd/csrc/hg_segctx.h"

extern "C" {

// text[0, nbytes) in tiles of `tile` bytes, pieces of at most bs1 bytes.  recs: the packed scan's ordered records, six words
// each {line_number, id, to, start, len, pattern}.  Outputs: out (six words {line_number, id, to, start, len, pattern} per
// context record, file-relative, segment after segment), out_seg, first_context[n_seg + 1], and info = {kept records,
// tiles whose text the write pass reads}.  Returns the context records; -1: cap too small; -2: a tile's count and its walk
// disagree; -3: the tiles do not chain or a segment got no base; -4: the records' segments do not ascend; -5: malformed segments.
long segctxsim_run(const uint8_t *text, uint64_t nbytes, uint64_t tile, uint64_t bs1, const uint64_t *recs, uint64_t n, const uint64_t *seg_start,
                   const uint64_t *seg_end, uint64_t n_seg, uint64_t limit, int invert, uint32_t before, uint32_t after, uint64_t *out, uint32_t *out_seg,
                   uint64_t cap, uint64_t *first_context, uint64_t *info) {
  for (uint64_t s = 0; s < n_seg; s++)
    if (hg_seg_check(text, nbytes, seg_start, seg_end, n_seg, s)) return -5;
  const uint64_t ntiles = (nbytes + tile - 1) / tile;
  std::vector<HgHit> hits(n);
  std::vector<HgHitAux> aux(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t *r = recs + 6 * i;
    hits[i] = HgHit{r[0], static_cast<uint32_t>(r[1]), static_cast<uint32_t>(r[2])};
    aux[i] = HgHitAux{r[3], static_cast<uint32_t>(r[4]), static_cast<uint32_t>(r[5])};
  }
  std::vector<HgTileSum> sums(ntiles);
  std::vector<HgTileBase> bases(ntiles + 1);
  HgTileBase st{0, 0};
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
  const uint64_t end_piece = st.L + (nbytes > st.cs ? hg_pieces(nbytes - st.cs, bs1) : 0);  // (as HgScanner::run_once)
  auto bounds = [&](uint64_t t, uint64_t *t0, uint64_t *t1) {
    *t0 = t * tile;
    *t1 = *t0 + tile < nbytes ? *t0 + tile : nbytes;
  };
  auto first_piece = [&](uint64_t t) {
    if (t >= ntiles) return end_piece;
    uint64_t t0, t1;
    bounds(t, &t0, &t1);
    return hg_invert_first_piece(bases[t], sums[t], t0, t1, bs1);
  };
  // the line bases: the number of the first piece that starts at or after each boundary (one walk of the whole text)
  std::vector<uint64_t> starts_of;  // piece number -> piece start
  for (uint64_t t = 0; t < ntiles; t++) {
    uint64_t t0, t1;
    bounds(t, &t0, &t1);
    if (first_piece(t) != starts_of.size()) return -3;
    hg_invert_walk_tile(text, bases[t], sums[t], t0, t1, bs1, [&](uint64_t, uint64_t ps) { starts_of.push_back(ps); });
  }
  if (starts_of.size() != end_piece) return -3;
  auto piece_at = [&](uint64_t b) {
    uint64_t lo = 0, hi = end_piece;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (starts_of[mid] < b) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  std::vector<uint64_t> B(n_seg + 1), E(n_seg + 1), r0(n_seg + 1), kept(n_seg + 1);
  std::vector<HgHit> K;
  std::vector<HgSegCtxWin> W;
  for (uint64_t s = 0; s < n_seg; s++) {
    B[s] = piece_at(seg_start[s]);
    E[s] = piece_at(seg_end[s]);
    uint64_t a, z;
    hg_seg_run(hits.data(), aux.data(), n, B[s], E[s], seg_end[s], invert != 0, limit, &a, &z);
    r0[s] = a;
    kept[s] = z - a;
    // (hg_segctx_prep_kernel)
    const uint64_t stop = hg_segctx_stop(hits.data(), aux.data(), n, B[s], E[s], seg_end[s], invert != 0, limit, a, z - a);
    for (uint64_t i = a; i < z; i++) K.push_back(hits[i]), W.push_back(HgSegCtxWin{B[s], stop});
  }
  info[0] = K.size();
  info[1] = 0;
  const HgContextWin w = hg_context_win(0, end_piece, 0, 0, 0, false);
  uint64_t total = 0;
  for (uint64_t t = 0; t < ntiles; t++) {
    uint64_t t0, t1;
    bounds(t, &t0, &t1);
    // the count pass of hg_segctx_count_kernel, one record after the other
    const HgContextTile ct = hg_context_tile(K.data(), K.size(), first_piece(t), first_piece(t + 1), w);
    int64_t count = 0;
    for (uint64_t i = ct.r0; i < ct.r1; i++) count += hg_segctx_contrib(K.data(), W.data(), i, ct, before, after);
    uint64_t walked = 0;
    bool full = false;
    hg_segctx_walk_tile(text, bases[t], sums[t], t0, t1, bs1, K.data(), W.data(), K.size(), before, after, [&](uint64_t q, uint64_t ps) {
      walked++;
      if (total >= cap) {
        full = true;
        return;
      }
      uint64_t a, z;
      hg_trim_piece(text, ps, ps + bs1 < nbytes ? ps + bs1 : nbytes, a, z);
      HgHit h;
      HgHitAux x;
      hg_context_record(q, a, z, HG_CTX_CONTEXT, &h, &x);
      // (hg_segctx_map_kernel)
      out_seg[total] = hg_segctx_map_record(B.data(), seg_start, seg_end, n_seg, &h, &x);
      uint64_t *o = out + 6 * total++;
      o[0] = h.line_no, o[1] = h.id, o[2] = h.to, o[3] = x.start, o[4] = x.len, o[5] = x.pattern;
    });
    if (full) return -1;
    if (count < 0 || walked != static_cast<uint64_t>(count)) return -2;
    if (walked) info[1]++;
  }
  for (uint64_t j = 1; j < total; j++)
    if (out_seg[j] < out_seg[j - 1]) return -4;
  for (uint64_t s = 0; s <= n_seg; s++) first_context[s] = hg_segctx_first(out_seg, total, s);  // (hg_segctx_first_kernel)
  return static_cast<long>(total);
}

}  // extern "C"

#ifdef SEGCTXSIM_MAIN
#include <algorithm>
#include <cstdio>
#include <string>

// The rules, file by file and piece by piece, on the file's own bytes: its pieces (split at '\n', cut at bs1), its matching
// pieces kept under the limit, and for every other piece whether a kept one lies within reach.
static std::vector<uint64_t> piece_starts(const std::string &f, uint64_t bs1) {
  std::vector<uint64_t> ps;
  uint64_t ls = 0;
  for (uint64_t i = 0; i <= f.size(); i++)
    if (i == f.size() || f[i] == '\n') {
      const uint64_t e = i < f.size() ? i + 1 : i;
      for (uint64_t p = ls; p < e; p += bs1) ps.push_back(p);
      ls = e;
    }
  return ps;
}

int main() {
  long cases = 0;
  for (uint64_t bs1 : {3ull, 7ull, 63ull})
    for (uint64_t tile : {4ull, 16ull, 17ull, 64ull, 16384ull})
      for (int shape = 0; shape < 4; shape++) {
        // the files: terminated, unterminated (pad), empty, NUL tails, a long line, lengths around multiples of bs1
        std::vector<std::string> files;
        for (int i = 0; i < 24; i++) {
          std::string f;
          const int lines = shape == 0 ? 1 : shape == 1 ? (i % 5) : shape == 2 ? 1 + (i * 7) % 9 : 6;
          for (int l = 0; l < lines; l++) f += (l * 3 + i) % 4 == 0 ? "xab\n" : (l + i) % 7 == 3 ? std::string(2 * bs1 + 1, 'q') + "\n" : "zz\n";
          if (i % 3 == 1 && !f.empty()) f.pop_back();                      // unterminated
          if (i % 6 == 2) f += std::string(3, '\0');                        // a last piece of NULs only
          if (i % 8 == 5) f = std::string(static_cast<size_t>(bs1) * 2 - (i % 3), 'a');  // k * bs1 + {0, -1, -2}
          files.push_back(f);
        }
        std::string text;
        std::vector<uint64_t> ss, se;
        for (const std::string &f : files) {
          ss.push_back(text.size());
          text += f;
          se.push_back(text.size());
          if (!f.empty() && f.back() != '\n') text += std::string("\0\n", 2);
        }
        ss.push_back(0), se.push_back(0);  // (never read: n_seg entries are)
        const uint64_t n_seg = files.size();
        // the packed records: a piece "matches" when its scanned bytes hold "ab" (or, inverted, when they do not), computed on
        // the PACKED text piece by piece; pad hits cannot arise (a pad holds no "ab")
        const uint8_t *data = reinterpret_cast<const uint8_t *>(text.data());
        const std::vector<uint64_t> pstarts = piece_starts(text, bs1);
        for (int invert = 0; invert < 2; invert++)
          for (uint64_t limit : {0ull, 1ull, 2ull})
            for (auto ba : {std::pair<uint32_t, uint32_t>{1, 0}, {0, 1}, {2, 3}, {1000, 1000}, {0xFFFFFFFFu, 0xFFFFFFFFu}}) {
              std::vector<uint64_t> recs;
              auto matches = [&](const uint8_t *base, uint64_t limit_end, uint64_t ps) {
                uint64_t a, z;
                hg_trim_piece(base, ps, ps + bs1 < limit_end ? ps + bs1 : limit_end, a, z);
                bool hit = false;
                for (uint64_t i = a; i + 1 < z; i++) hit |= base[i] == 'a' && base[i + 1] == 'b';
                return std::pair<bool, std::pair<uint64_t, uint64_t>>{hit != (invert != 0), {a, z}};
              };
              for (uint64_t q = 0; q < pstarts.size(); q++) {
                const auto m = matches(data, text.size(), pstarts[q]);
                if (m.first) recs.insert(recs.end(), {q, invert ? 0xFFFFFFFFull : 1ull, 0ull, m.second.first, m.second.second - m.second.first, invert ? 0xFFFFFFFFull : 0ull});
              }
              const uint64_t cap = pstarts.size() + 1;
              std::vector<uint64_t> out(6 * cap), first(n_seg + 1);
              std::vector<uint32_t> out_seg(cap);
              uint64_t info[2];
              const long n = segctxsim_run(data, text.size(), tile, bs1, recs.data(), recs.size() / 6, ss.data(), se.data(), n_seg, limit, invert, ba.first, ba.second,
                                           out.data(), out_seg.data(), cap, first.data(), info);
              if (n < 0) return std::printf("replay failed: %ld (bs1 %llu tile %llu shape %d)\n", n, (unsigned long long)bs1, (unsigned long long)tile, shape), 1;
              uint64_t k = 0;
              for (uint64_t s = 0; s < n_seg; s++) {
                if (first[s] != k) return std::printf("first_context[%llu] differs\n", (unsigned long long)s), 1;
                const uint8_t *fd = reinterpret_cast<const uint8_t *>(files[s].data());
                const std::vector<uint64_t> ps = piece_starts(files[s], bs1);
                std::vector<uint64_t> kept;  // the file's matching pieces under the limit; `next`: the first one removed
                uint64_t next = ps.size();
                for (uint64_t q = 0; q < ps.size(); q++)
                  if (matches(fd, files[s].size(), ps[q]).first) {
                    if (limit && kept.size() >= limit) {
                      next = q;
                      break;
                    }
                    kept.push_back(q);
                  }
                for (uint64_t q = 0; q < next; q++) {
                  if (std::binary_search(kept.begin(), kept.end(), q)) continue;
                  bool ctx = false;
                  for (uint64_t m : kept) ctx |= m > q ? m - q <= ba.first : q - m <= ba.second;
                  if (!ctx) continue;
                  const auto m = matches(fd, files[s].size(), ps[q]);
                  if (k >= static_cast<uint64_t>(n) || out_seg[k] != s || out[6 * k] != q || out[6 * k + 1] != HG_CTX_ID_CONTEXT || out[6 * k + 3] != m.second.first ||
                      out[6 * k + 4] != m.second.second - m.second.first)
                    return std::printf("record %llu differs (bs1 %llu tile %llu shape %d invert %d limit %llu)\n", (unsigned long long)k, (unsigned long long)bs1,
                                       (unsigned long long)tile, shape, invert, (unsigned long long)limit), 1;
                  k++;
                }
              }
              if (k != static_cast<uint64_t>(n) || first[n_seg] != k) return std::printf("%ld records, %llu expected\n", n, (unsigned long long)k), 1;
              cases++;
            }
      }
  std::printf("segctxsim: %ld cases ok\n", cases);
  return 0;
}
#endif
