// Wave64 building blocks of the stages that walk a tile's line pieces with one wavefront (hg_invert.hip, hg_context.hip):
// prefix sums over the lanes, the newline / NUL bits of a lane's 16 bytes, a piece trimmed by the whole wave, and the write
// pass both stages run over a tile (wave_write_tile).
#pragma once
#include <hip/hip_runtime.h>

#include "hg_invert.h"

static __device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o, 64);
    if (lane >= static_cast<uint32_t>(o)) v += u;
  }
  return v;
}
static __device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {  // set bits of a ballot below this lane
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}
// bit b of the result: byte b of the dword is marked (0x80) in m
static __device__ __forceinline__ uint32_t pack4(uint32_t m) { return (((m >> 7) * 0x00204081u) >> 21) & 0xFu; }
static __device__ __forceinline__ uint32_t pack16(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return pack4(a) | (pack4(b) << 4) | (pack4(c) << 8) | (pack4(d) << 12); }
static __device__ __forceinline__ uint32_t newline_bits16(const uint4 &v) { return pack16(hg_newline_mask(v.x), hg_newline_mask(v.y), hg_newline_mask(v.z), hg_newline_mask(v.w)); }
static __device__ __forceinline__ uint32_t zero_bits16(const uint4 &v) { return pack16(hg_zero_bytes(v.x), hg_zero_bytes(v.y), hg_zero_bytes(v.z), hg_zero_bytes(v.w)); }

// The first position in [from, limit) whose byte stops the search (STOP: a NUL or a '\n'; else: any byte but NUL), or limit.
// The wave reads 1 KiB per step in aligned 16-byte chunks; arguments and result are wave-uniform.
template <bool STOP>
static __device__ uint64_t wave_find(const uint8_t *text, uint64_t from, uint64_t limit, uint32_t lane) {
  for (uint64_t base = from & ~static_cast<uint64_t>(15); base < limit; base += 1024) {
    const uint64_t p = base + lane * 16u;
    uint32_t m = 0;
    if (p < limit) {  // (limit <= nbytes and p is 16-byte aligned: the chunk lies in the text rounded up to 16)
      const uint4 v = *reinterpret_cast<const uint4 *>(text + p);
      m = STOP ? (zero_bits16(v) | newline_bits16(v)) : (~zero_bits16(v) & 0xFFFFu);
      if (p < from) m &= 0xFFFFu << (from - p);
      if (limit - p < 16) m &= (1u << (limit - p)) - 1u;
    }
    const uint64_t any = __builtin_amdgcn_ballot_w64(m != 0);
    if (any) {
      const uint32_t l = __builtin_ctzll(any);
      return base + l * 16u + hg_ctz(__shfl(m, l, 64));
    }
  }
  return limit;
}
// hg_trim_piece by the whole wave (a piece that may be megabytes long)
static __device__ inline void wave_trim_piece(const uint8_t *text, uint64_t ps, uint64_t limit, uint32_t lane, uint64_t &a, uint64_t &z) {
  a = wave_find<false>(text, ps, limit, lane);
  z = a;
  if (a >= limit) return;
  z = wave_find<true>(text, a, limit, lane);
  if (z < limit && text[z] == '\n') z++;
}

constexpr uint32_t HG_WALK_SKIP = 0;  // wave_write_tile's selector: no record for this piece (the records' ids are HG_ID_* values, never 0)

// The write pass of one tile by one wavefront: stream the tile once (16 B per lane, 1 KiB per row), find the newlines with
// ballots, number the pieces that start in the tile, ask sel(h, piece number) for each (h: a hit index with only smaller line
// numbers below it) and write the two 16-byte records {piece, id, 0} / {start, len, 0xFFFFFFFF} of those for which it returns
// an id, in order, to out_*[pos[t] .. pos[t + 1]).  A tile whose share of the output is empty is left without touching its text.
template <typename Sel>
static __device__ __forceinline__ void wave_write_tile(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t t, const HgTileBase *bases, const HgTileSum *sums,
                                                       const HgHit *hits, uint64_t n_hits, const uint64_t *pos, HgHit *out_hits, HgHitAux *out_aux, uint32_t lane, Sel sel) {
  uint64_t o = pos[t];  // the next record of this tile; wave-uniform, like s, q and h below
  const uint64_t o_end = pos[t + 1];
  if (o == o_end) return;  // nothing to write for this tile: its text is not read
  const uint64_t t0 = t << HG_TILE_SHIFT, t1 = t0 + HG_TILE_BYTES < nbytes ? t0 + HG_TILE_BYTES : nbytes;
  uint64_t s = bases[t].cs;  // start of the line that is open at the current row
  uint64_t q = hg_invert_first_piece(bases[t], sums[t], t0, t1, bs1);  // number of the next piece
  uint64_t h = hg_invert_lower_bound(hits, 0, n_hits, q);               // first hit at or after it
  uint32_t nul_end = 0;  // tile-relative end of the last NUL of the rows so far (0: none)
  auto store = [&](uint64_t at, uint64_t piece, uint64_t pa, uint64_t pz, uint32_t id) {
    if (at >= o_end) return;  // (never, unless the count pass and this walk disagree: stay inside the tile's share)
    out_hits[at] = HgHit{piece, id, 0u};
    out_aux[at] = HgHitAux{pa, static_cast<uint32_t>(pz - pa), HG_NONE32};
  };
  for (uint32_t row = 0; row < HG_TILE_BYTES && t0 + row < t1; row += 1024) {
    const uint64_t p = t0 + row + lane * 16u;  // this lane's 16 bytes
    uint32_t nlm = 0, zm = 0;
    if (p < t1) {
      const uint4 v = *reinterpret_cast<const uint4 *>(text + p);
      const uint32_t valid = t1 - p < 16 ? (1u << (t1 - p)) - 1u : 0xFFFFu;
      nlm = newline_bits16(v) & valid;
      zm = zero_bits16(v) & valid;
    }
    // what the lanes below hand on: the end of the last newline (the start of the line open at this lane) and of the last NUL
    const uint32_t rel = row + lane * 16u;
    const uint32_t my_nl_end = nlm ? rel + 32u - hg_clz32(nlm) : 0u, my_nul_end = zm ? rel + 32u - hg_clz32(zm) : 0u;
    const uint64_t nl_lanes = __builtin_amdgcn_ballot_w64(nlm != 0), nul_lanes = __builtin_amdgcn_ballot_w64(zm != 0);
    const uint64_t below = lane ? ~0ull >> (64u - lane) : 0ull;
    const uint64_t nl_below = nl_lanes & below, nul_below = nul_lanes & below;
    const uint32_t nl_from = __shfl(my_nl_end, nl_below ? 63 - __builtin_clzll(nl_below) : 0, 64);
    const uint32_t nul_from = __shfl(my_nul_end, nul_below ? 63 - __builtin_clzll(nul_below) : 0, 64);
    const uint64_t s_in = nl_below ? t0 + nl_from : s;
    const uint32_t nul_in = nul_below ? nul_from : nul_end;
    if (nul_lanes) nul_end = __shfl(my_nul_end, 63 - __builtin_clzll(nul_lanes), 64);
    if (!nl_lanes) continue;  // no line ends in this row
    // the lines that END in this lane's bytes: fn(piece number, piece start, line end, the newline's bit) per piece that
    // starts in the tile
    auto each_piece = [&](uint64_t number, auto &&fn) {
      uint64_t ls = s_in, k0, k1;
      for (uint32_t m = nlm; m; m &= m - 1) {
        const uint32_t b = hg_ctz(m);
        const uint64_t e = p + b + 1;
        hg_invert_cuts(ls, e, t0, bs1, &k0, &k1);
        for (uint64_t k = k0; k < k1; k++) fn(number++, ls + k * bs1, e, b);
        ls = e;
      }
    };
    uint32_t npieces = 0;
    {
      uint64_t ls = s_in, k0, k1;
      for (uint32_t m = nlm; m; m &= m - 1) {
        const uint64_t e = p + hg_ctz(m) + 1;
        hg_invert_cuts(ls, e, t0, bs1, &k0, &k1);
        npieces += static_cast<uint32_t>(k1 - k0);  // (pieces of 1 byte at least, all inside the tile)
        ls = e;
      }
    }
    const uint32_t pieces_incl = wave_inclusive_scan(npieces, lane);
    const uint64_t my_q = q + (pieces_incl - npieces);
    uint32_t nsel = 0;
    each_piece(my_q, [&](uint64_t number, uint64_t, uint64_t, uint32_t) { nsel += sel(h, number) != HG_WALK_SKIP ? 1u : 0u; });
    const uint32_t sel_incl = wave_inclusive_scan(nsel, lane);
    uint64_t at = o + (sel_incl - nsel);
    if (nsel)
      each_piece(my_q, [&](uint64_t number, uint64_t ps, uint64_t e, uint32_t b) {
        const uint32_t id = sel(h, number);
        if (id == HG_WALK_SKIP) return;
        // no NUL between the piece's start and the line's end: the piece is its bytes up to the cut or the newline
        const uint32_t z_low = zm & ((1u << b) - 1u);
        const uint64_t last_nul_end = t0 + (z_low ? rel + 32u - hg_clz32(z_low) : nul_in);
        uint64_t pa = ps, pz = ps + bs1 < e ? ps + bs1 : e;
        if (last_nul_end > ps) hg_trim_piece(text, ps, pz, pa, pz);
        store(at++, number, pa, pz, id);
      });
    s = t0 + __shfl(my_nl_end, 63 - __builtin_clzll(nl_lanes), 64);
    q += __shfl(pieces_incl, 63, 64);
    o += __shfl(sel_incl, 63, 64);
    h = hg_invert_lower_bound(hits, h, n_hits, q);
  }
  // the line still open at the tile's end: its pieces that start in the tile may reach far beyond it
  uint64_t k0, k1;
  hg_invert_cuts(s, t1, t0, bs1, &k0, &k1);
  if (bs1 <= HG_TILE_BYTES) {  // short pieces, maybe many: a lane each
    for (uint64_t kb = k0; kb < k1; kb += 64) {
      const uint64_t k = kb + lane;
      const uint32_t id = k < k1 ? sel(h, q + (k - k0)) : HG_WALK_SKIP;
      const uint64_t sel_lanes = __builtin_amdgcn_ballot_w64(id != HG_WALK_SKIP);
      if (id != HG_WALK_SKIP) {
        const uint64_t ps = s + k * bs1;
        uint64_t pa, pz;
        hg_trim_piece(text, ps, ps + bs1 < nbytes ? ps + bs1 : nbytes, pa, pz);
        store(o + lanes_below(sel_lanes), q + (k - k0), pa, pz, id);
      }
      o += __popcll(sel_lanes);
    }
  } else {  // long pieces, two at most: the wave trims each
    for (uint64_t k = k0; k < k1; k++) {
      const uint32_t id = sel(h, q + (k - k0));
      if (id == HG_WALK_SKIP) continue;
      const uint64_t ps = s + k * bs1;
      uint64_t pa, pz;
      wave_trim_piece(text, ps, ps + bs1 < nbytes ? ps + bs1 : nbytes, lane, pa, pz);
      if (lane == 0) store(o, q + (k - k0), pa, pz, id);
      o++;
    }
  }
}
