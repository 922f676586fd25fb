// TEST-ONLY host harness for the gather stage (never shipped): compiles the scalar rules of hypergrep_amd/csrc/hg_gather.h for
// x86 and replays the stage's steps: head flags, their exclusive scan, the entry pass, the exclusive scan of the sizes, the
// span pass and the copy pass over output spans of `tile` bytes, 16 bytes at a time, as the lanes of hg_gather_copy_kernel do it.  What the GPU
// stage (hg_gather.hip) must reproduce; only its launch geometry is left to the GPU tests.
// The text is read through a checked view: every byte and dword read must lie inside [0, nbytes rounded up to 4) and inside
// the heap block that holds exactly those bytes, and `base` (any value, above 2^32 in one test) is added to every record's
// start by the caller and subtracted on access, so the 64-bit offset arithmetic is exercised without gigabytes of text.
// With -DGATHERSIM_MAIN the file is a program of its own (a sanitized run).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_gather.h"

namespace {

struct CheckedText {
  const uint8_t *p;  // a heap block of exactly `readable` bytes
  uint64_t base, readable;
  bool *bad;
  uint8_t byte(uint64_t o) const {
    if (o < base || o - base >= readable) {
      *bad = true;
      return 0;
    }
    return p[o - base];
  }
  uint32_t dword(uint64_t o) const {
    if ((o & 3) || o < base || o - base + 4 > readable) {
      *bad = true;
      return 0;
    }
    uint32_t v;
    memcpy(&v, p + (o - base), 4);
    return v;
  }
};

void exclusive_scan(const std::vector<uint64_t> &in, std::vector<uint64_t> &out) {
  uint64_t sum = 0;
  for (size_t i = 0; i < in.size(); i++) {
    out[i] = sum;
    sum += in[i];
  }
}

}  // namespace

extern "C" {

// recs: {line, id, start, len, segment} per record (uint64 each): n_main main records, then n_ctx context records; every
// start already has `base` added, and base is a multiple of 4 (the device's text is 16-byte aligned).  seg_start / first_record
// / first_context: n_seg + 1 each or NULL (no segments).  out_bytes: room for cap_bytes; entry_off: n + 1; line_number, kind,
// segment: n each; first_entry: n_seg + 1.  totals: {n_entries, n_bytes}.
// Returns 0, -1 if an output is too small, -2 if a read left the readable range, -3 if two lanes' chunks disagree with the
// byte-by-byte definition (hg_gather_byte over every entry).
long gathersim_run(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_main, uint64_t n_ctx, int segments, const uint64_t *seg_start,
                   const uint64_t *first_record, const uint64_t *first_context, uint64_t n_seg, uint32_t flags, uint64_t tile, uint8_t *out_bytes, uint64_t cap_bytes,
                   uint64_t *entry_off, uint64_t *line_number, uint32_t *kind, uint32_t *segment, uint64_t *first_entry, uint64_t *totals) {
  const uint64_t n = n_main + n_ctx, readable = (nbytes + 3) & ~uint64_t{3};
  std::vector<uint8_t> block(readable, 0);  // (exactly the readable bytes: a read past them is the sanitizer's to catch, too)
  if (nbytes) memcpy(block.data(), text, nbytes);
  bool bad = false;
  const CheckedText view{block.data(), base, readable, &bad};
  std::vector<HgHit> hits(n + 1);
  std::vector<HgHitAux> aux(n + 1);
  std::vector<uint32_t> seg_of(n + 1);
  for (uint64_t i = 0; i < n; i++) {
    hits[i] = HgHit{recs[5 * i], static_cast<uint32_t>(recs[5 * i + 1]), 0};
    aux[i] = HgHitAux{recs[5 * i + 2], static_cast<uint32_t>(recs[5 * i + 3]), 0xFFFFFFFFu};
    seg_of[i] = static_cast<uint32_t>(recs[5 * i + 4]);
  }
  std::vector<uint64_t> head(n + 1, 0), F(n + 1, 0), size(n + 1, 0), off(n + 1, 0), first(n_seg + 1, 0);
  std::vector<HgGatherEntry> entries(n + 1);
  HgGatherArgs a{};
  a.main = HgGatherList{hits.data(), aux.data(), segments ? seg_of.data() : nullptr, n_main};
  a.ctx = HgGatherList{hits.data() + n_main, aux.data() + n_main, segments ? seg_of.data() + n_main : nullptr, n_ctx};
  a.seg_start = segments ? seg_start : nullptr;
  a.first_record = segments ? first_record : nullptr;
  a.first_context = segments ? first_context : nullptr;
  a.n_seg = n_seg;
  a.flags = flags;
  a.head = head.data();
  a.F = F.data();
  a.size = size.data();
  a.entries = entries.data();
  a.line_number = line_number;
  a.kind = kind;
  a.segment = segments ? segment : nullptr;
  a.first_entry = first.data();
  a.off = off.data();
  for (uint64_t r = 0; r < n; r++) head[r] = hg_gather_flag(a, r);
  exclusive_scan(head, F);
  for (uint64_t r = 0; r < n; r++) hg_gather_entry(a, view, r);
  if (segments)
    for (uint64_t s = 0; s <= n_seg; s++) first_entry[s] = hg_gather_first(a, s);
  exclusive_scan(size, off);
  a.n_entries = F[n];
  a.n_bytes = off[n];
  totals[0] = a.n_entries;
  totals[1] = a.n_bytes;
  for (uint64_t j = 0; j <= a.n_entries; j++) entry_off[j] = off[j];
  if (bad) return -2;
  const uint64_t padded = (a.n_bytes + 15) & ~uint64_t{15};
  if (padded > cap_bytes) return -1;
  std::vector<uint8_t> out(padded + 1, 0xEE);
  const uint64_t n_spans = (a.n_bytes + tile - 1) / tile;
  std::vector<uint64_t> span(n_spans + 1, 0);
  for (uint64_t t = 0; a.n_bytes && t <= n_spans; t++) span[t] = hg_gather_span(a, tile, t);
  for (uint64_t t0 = 0; t0 < a.n_bytes; t0 += tile) {  // a workgroup
    const uint64_t tile_last = (t0 + tile < a.n_bytes ? t0 + tile : a.n_bytes) - 1;
    const uint64_t j_lo = span[t0 / tile], j_hi = span[t0 / tile + 1];
    for (uint64_t pos = t0; pos <= tile_last; pos += 16) {  // a lane's chunk
      const uint64_t j = hg_gather_find(a.off, j_lo, j_hi, pos);
      const HgGatherChunk c = hg_gather_chunk(a, view, pos, j, off[j], off[j + 1]);
      const uint32_t w[4] = {c.w0, c.w1, c.w2, c.w3};
      memcpy(out.data() + pos, w, 16);
    }
  }
  if (bad) return -2;
  if (out[padded] != 0xEE) return -3;
  // the definition, byte by byte
  for (uint64_t j = 0; j < a.n_entries; j++)
    for (uint64_t k = 0; k < off[j + 1] - off[j]; k++)
      if (out[off[j] + k] != hg_gather_byte(view, entries[j], k)) return -3;
  for (uint64_t p = a.n_bytes; p < padded; p++)
    if (out[p] != 0) return -3;
  if (bad) return -2;
  if (a.n_bytes) memcpy(out_bytes, out.data(), a.n_bytes);
  return 0;
}

uint32_t gathersim_digits(uint64_t v) { return hg_gather_digits(v); }
uint32_t gathersim_tile() { return HG_GATHER_TILE; }

}  // extern "C"

#ifdef GATHERSIM_MAIN
// A text of four lines (the last unterminated), hits on lines 0 and 3 (two reports on line 0), context on 1 and 2 (2 a tail),
// every flag combination, tiles of 16 and 64 bytes, and a base above 2^32; then two one-line files that both match on line 0.
int main() {
  const std::string text = "alpha abc\nbeta\ngamma gamma gamma gamma\ndelta abc";
  const uint64_t base = (uint64_t{1} << 32) + 64;
  // {line, id, start, len, segment}
  const uint64_t recs[] = {0, 1, base + 0, 10, 0, 0, 2, base + 0, 10, 0, 3, 1, base + 39, 9, 0, 1, 0xFFFFFFFEu, base + 10, 5, 0, 2, 0xFFFFFFFDu, base + 15, 24, 0};
  const char *want[16] = {nullptr};
  want[0] = "alpha abc\ndelta abc";
  want[1] = "alpha abc\nbeta\ngamma gamma gamma gamma\ndelta abc";
  want[2] = "alpha abc\ndelta abc\n";
  want[4] = "1:alpha abc\n4:delta abc";
  want[8] = "alpha abc\n--\ndelta abc";
  want[15] = "1:alpha abc\n2-beta\n3-gamma gamma gamma gamma\n4:delta abc\n";
  want[14] = "1:alpha abc\n--\n4:delta abc\n";
  int bad = 0, cases = 0;
  for (uint32_t flags = 0; flags < 16; flags++)
    for (uint64_t tile : {16, 64}) {
      uint8_t out[256];
      uint64_t entry_off[8], line_number[8], totals[2];
      uint32_t kind[8];
      const long rc = gathersim_run(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs, 3, (flags & 1) ? 2 : 0, 0, nullptr, nullptr, nullptr, 0, flags,
                                    tile, out, sizeof out, entry_off, line_number, kind, nullptr, nullptr, totals);
      const std::string got(reinterpret_cast<const char *>(out), rc == 0 ? totals[1] : 0);
      const bool ok = rc == 0 && totals[0] == ((flags & 1) ? 4u : 2u) && (!want[flags] || got == want[flags]);
      if (!ok) printf("flags %u tile %llu: rc %ld, %llu entries, \"%s\"\n", flags, (unsigned long long)tile, rc, (unsigned long long)totals[0], got.c_str());
      bad |= !ok;
      cases++;
    }
  {
    const std::string files = "abc\nabc\n";
    const uint64_t frecs[] = {0, 1, 0, 4, 0, 0, 1, 0, 4, 1};
    const uint64_t seg_start[] = {0, 4, 8}, first_record[] = {0, 1, 2};
    uint8_t out[64];
    uint64_t entry_off[4], line_number[4], totals[2], first_entry[3];
    uint32_t kind[4], segment[4];
    const long rc = gathersim_run(reinterpret_cast<const uint8_t *>(files.data()), files.size(), 0, frecs, 2, 0, 1, seg_start, first_record, nullptr, 2,
                                  HG_GATHER_SEPARATOR | HG_GATHER_NUMBER, 16, out, sizeof out, entry_off, line_number, kind, segment, first_entry, totals);
    const std::string got(reinterpret_cast<const char *>(out), rc == 0 ? totals[1] : 0);
    const bool ok = rc == 0 && totals[0] == 2 && got == "1:abc\n--\n1:abc\n" && first_entry[0] == 0 && first_entry[1] == 1 && first_entry[2] == 2 && segment[1] == 1;
    if (!ok) printf("files: rc %ld \"%s\"\n", rc, got.c_str());
    bad |= !ok;
    cases++;
  }
  bad |= hg_gather_digits(9999999999999999999ull) != 19 || hg_gather_digits(10000000000000000000ull) != 20 || hg_gather_digits(0) != 1;
  printf(bad ? "FAILED\n" : "%d cases ok\n", cases);
  return bad;
}
#endif
