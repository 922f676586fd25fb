// TEST-ONLY host harness for the parts gather (never shipped): compiles the scalar rules of hypergrep_amd/csrc/hg_partlines.h
// for x86 and replays the stage's steps: the entry pass, the exclusive scan of the sizes, the span pass and the copy pass over
// output spans of `tile` bytes, 16 bytes at a time, as the lanes of hg_partlines_copy_kernel do it.  What the GPU stage
// (hg_partlines.hip) must reproduce; only its launch geometry is left to the GPU tests.
// The text is read through a checked view: every byte and dword read must lie inside [0, nbytes rounded up to 4) and inside
// the heap block that holds exactly those bytes, and `base` (any multiple of 4, above 2^32 in one test) is added to every
// record's start by the caller and subtracted on access, so the 64-bit offset arithmetic is exercised without gigabytes of text.
// With -DPARTLINESIM_MAIN the file is a program of its own (a sanitized run).
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_partlines.h"
#include "../../include/hypergrep_amd.h"

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

}  // namespace

extern "C" {

// recs: {line, start, len, segment} per final record, in order; parts: {line, from, to, pattern, segment} per part, in order
// (uint64 each).  Every start (seg_start with segments) already has `base` added.  seg_start: n_seg values or NULL (no
// segments).  out_bytes: room for cap_bytes; entry_off: n_parts + 1; line_number, kind, pattern, segment: n_parts each.
// totals: {n_entries, n_bytes}.
// Returns 0, -1 if an output is too small, -2 if a read left the readable range, -3 if the lanes' chunks disagree with the
// byte-by-byte definition (hg_partlines_byte over every entry).
long partlinesim_run(const uint8_t *text, uint64_t nbytes, uint64_t base, const uint64_t *recs, uint64_t n_recs, const uint64_t *parts, uint64_t n_parts, int segments,
                     const uint64_t *seg_start, uint32_t flags, uint64_t byte_base, const uint8_t *mark_on, uint32_t on_len, const uint8_t *mark_off, uint32_t off_len,
                     uint64_t tile, uint8_t *out_bytes, uint64_t cap_bytes, uint64_t *entry_off, uint64_t *line_number, uint32_t *kind, uint32_t *pattern, uint32_t *segment,
                     uint64_t *totals) {
  const uint64_t readable = (nbytes + 3) & ~uint64_t{3};
  uint8_t *block = static_cast<uint8_t *>(calloc(readable ? readable : 1, 1));  // (exactly the readable bytes: a read past them is the sanitizer's to catch, too)
  if (nbytes) memcpy(block, text, nbytes);
  bool bad = false;
  const CheckedText view{block, base, readable, &bad};
  std::vector<HgHit> hits(n_recs + 1);
  std::vector<HgHitAux> aux(n_recs + 1);
  std::vector<uint32_t> seg_of(n_recs + 1), part_seg(n_parts + 1), part_pattern(n_parts + 1);
  std::vector<HgPart> rows(n_parts + 1);
  for (uint64_t i = 0; i < n_recs; i++) {
    hits[i] = HgHit{recs[4 * i], 1, 0};
    aux[i] = HgHitAux{recs[4 * i + 1], static_cast<uint32_t>(recs[4 * i + 2]), 0};
    seg_of[i] = static_cast<uint32_t>(recs[4 * i + 3]);
  }
  for (uint64_t q = 0; q < n_parts; q++) {
    rows[q] = HgPart{parts[5 * q], static_cast<uint32_t>(parts[5 * q + 1]), static_cast<uint32_t>(parts[5 * q + 2])};
    part_pattern[q] = static_cast<uint32_t>(parts[5 * q + 3]);
    part_seg[q] = static_cast<uint32_t>(parts[5 * q + 4]);
  }
  std::vector<uint64_t> size(n_parts + 1, 0), off(n_parts + 1, 0);
  std::vector<HgPartLinesEntry> entries(n_parts + 1);
  HgPartLinesArgs a{};
  a.recs = HgGatherList{hits.data(), aux.data(), segments ? seg_of.data() : nullptr, n_recs};
  a.parts = rows.data();
  a.part_pattern = part_pattern.data();
  a.part_seg = segments ? part_seg.data() : nullptr;
  a.n_parts = n_parts;
  a.seg_start = segments ? seg_start : nullptr;
  a.flags = flags;
  a.byte_base = byte_base;
  a.marks = hg_partlines_marks(mark_on, on_len, mark_off, off_len);
  a.size = size.data();
  a.entries = entries.data();
  a.line_number = line_number;
  a.kind = kind;
  a.pattern = pattern;
  a.segment = segments ? segment : nullptr;
  a.off = off.data();
  for (uint64_t q = 0; q < n_parts; q++) hg_partlines_entry(a, view, q);
  uint64_t sum = 0;
  for (uint64_t q = 0; q <= n_parts; q++) {
    off[q] = sum;
    sum += size[q];
  }
  a.n_entries = n_parts;
  a.n_bytes = off[n_parts];
  totals[0] = a.n_entries;
  totals[1] = a.n_bytes;
  for (uint64_t j = 0; j <= a.n_entries; j++) entry_off[j] = off[j];
  const uint64_t padded = (a.n_bytes + 15) & ~uint64_t{15};
  long rc = 0;
  if (bad) rc = -2;
  else if (padded > cap_bytes) rc = -1;
  if (!rc) {
    std::vector<uint8_t> out(padded + 1, 0xEE);
    const uint64_t n_spans = (a.n_bytes + tile - 1) / tile;
    std::vector<uint64_t> span(n_spans + 1, 0);
    a.span = span.data();
    for (uint64_t t = 0; a.n_bytes && t <= n_spans; t++) span[t] = hg_partlines_span(a, tile, t);
    for (uint64_t t0 = 0; t0 < a.n_bytes; t0 += tile) {  // a workgroup
      const uint64_t tile_last = (t0 + tile < a.n_bytes ? t0 + tile : a.n_bytes) - 1;
      const uint64_t j_lo = span[t0 / tile], j_hi = span[t0 / tile + 1];
      for (uint64_t pos = t0; pos <= tile_last; pos += 16) {  // a lane's chunk
        const uint64_t j = hg_gather_find(a.off, j_lo, j_hi, pos);
        const HgGatherChunk c = hg_partlines_chunk(a, view, pos, j, off[j], off[j + 1]);
        const uint32_t w[4] = {c.w0, c.w1, c.w2, c.w3};
        memcpy(out.data() + pos, w, 16);
      }
    }
    if (out[padded] != 0xEE) rc = -3;
    // the definition, byte by byte
    for (uint64_t j = 0; j < a.n_entries && !rc; j++) {
      if (off[j + 1] - off[j] != hg_partlines_size(entries[j], a.marks) && off[j + 1] != off[j]) rc = -3;
      for (uint64_t k = 0; k < off[j + 1] - off[j]; k++)
        if (out[off[j] + k] != hg_partlines_byte(view, entries[j], a.marks, k)) rc = -3;
    }
    for (uint64_t p = a.n_bytes; p < padded; p++)
      if (out[p] != 0) rc = -3;
    if (bad) rc = -2;
    if (!rc && a.n_bytes) memcpy(out_bytes, out.data(), a.n_bytes);
  }
  free(block);
  return rc;
}

uint32_t partlinesim_digits(uint64_t v) { return hg_gather_digits(v); }

// {sizeof params, sizeof result, offsets of the params' fields, offsets of the result's fields, sizeof(HgPartLinesEntry), tile, mark max}
void partlinesim_sizes(uint32_t *out) {
  const uint32_t v[] = {sizeof(hg_part_lines_params_t),
                        sizeof(hg_part_lines_result_t),
                        offsetof(hg_part_lines_params_t, flags),
                        offsetof(hg_part_lines_params_t, byte_base),
                        offsetof(hg_part_lines_params_t, mark_on_len),
                        offsetof(hg_part_lines_params_t, mark_off_len),
                        offsetof(hg_part_lines_params_t, mark_on),
                        offsetof(hg_part_lines_params_t, mark_off),
                        offsetof(hg_part_lines_result_t, n_entries),
                        offsetof(hg_part_lines_result_t, n_bytes),
                        offsetof(hg_part_lines_result_t, d_bytes),
                        offsetof(hg_part_lines_result_t, d_entry_off),
                        offsetof(hg_part_lines_result_t, d_line_number),
                        offsetof(hg_part_lines_result_t, d_kind),
                        offsetof(hg_part_lines_result_t, d_pattern),
                        offsetof(hg_part_lines_result_t, d_segment),
                        offsetof(hg_part_lines_result_t, d_first_entry),
                        offsetof(hg_part_lines_result_t, gather_us),
                        sizeof(HgPartLinesEntry),
                        HG_GATHER_TILE,
                        HG_PARTS_MARK_MAX};
  memcpy(out, v, sizeof v);
}

}  // extern "C"

#ifdef PARTLINESIM_MAIN
// `foo abc bar abc` and a second, unterminated line: parts mode with number, offset and terminator, line mode with grep's colour
// escapes, every flag combination at tiles of 16 and 64 bytes with a base above 2^32, and two one-line files that both hold
// line 0.  The text sits in an exactly sized allocation inside partlinesim_run.
int main() {
  const std::string text = "foo abc bar abc\nno\nxabc";
  const uint64_t base = (uint64_t{1} << 32) + 64;
  const uint64_t recs[] = {0, base + 0, 16, 0, 0, base + 0, 16, 0, 2, base + 19, 4, 0};  // (two reports on line 0)
  const uint64_t parts[] = {0, 4, 7, 0, 0, 0, 12, 15, 0, 0, 2, 1, 4, 0, 0};
  const uint8_t on[] = "\x1b[01;31m\x1b[K", off[] = "\x1b[m\x1b[K";
  int bad = 0, cases = 0;
  for (uint32_t flags = 0; flags < 16; flags++)
    for (uint64_t tile : {16, 64})
      for (int marks = 0; marks < 2; marks++) {
        uint8_t out[512];
        uint64_t entry_off[8], line_number[8], totals[2];
        uint32_t kind[8], pattern[8];
        const long rc = partlinesim_run(reinterpret_cast<const uint8_t *>(text.data()), text.size(), base, recs, 3, parts, 3, 0, nullptr, flags, 0 - base, on, marks ? 11 : 0, off,
                                        marks ? 6 : 0, tile, out, sizeof out, entry_off, line_number, kind, pattern, nullptr, totals);
        const std::string got(reinterpret_cast<const char *>(out), rc == 0 ? totals[1] : 0);
        const char *want = nullptr;
        if (!marks && flags == 7) want = "1:4:abc\n1:12:abc\n3:20:abc\n";
        if (!marks && flags == 0) want = "abcabcabc";
        if (!marks && flags == 8) want = "foo abc bar abc\nxabc";
        if (marks && flags == 12) want = "foo \x1b[01;31m\x1b[Kabc\x1b[m\x1b[K bar \x1b[01;31m\x1b[Kabc\x1b[m\x1b[K\nx\x1b[01;31m\x1b[Kabc\x1b[m\x1b[K\n";
        if (!marks && flags == 15) want = "1:0:foo abc bar abc\n3:19:xabc\n";
        const bool ok = rc == 0 && totals[0] == 3 && kind[0] == 1 && kind[1] == 2 && kind[2] == 3 && (!want || got == want);
        if (!ok) printf("flags %u tile %llu marks %d: rc %ld \"%s\"\n", flags, (unsigned long long)tile, marks, rc, got.c_str());
        bad |= !ok;
        cases++;
      }
  {
    const std::string files = "abc\nabc\n";
    const uint64_t frecs[] = {0, 0, 4, 0, 0, 0, 4, 1}, fparts[] = {0, 0, 3, 0, 0, 0, 0, 3, 0, 1}, seg_start[] = {base + 0, base + 4};
    uint8_t out[64];
    uint64_t entry_off[4], line_number[4], totals[2];
    uint32_t kind[4], pattern[4], segment[4];
    const long rc = partlinesim_run(reinterpret_cast<const uint8_t *>(files.data()), files.size(), base, frecs, 2, fparts, 2, 1, seg_start, 15, 0, on, 0, off, 0, 16, out, sizeof out,
                                    entry_off, line_number, kind, pattern, segment, totals);
    const std::string got(reinterpret_cast<const char *>(out), rc == 0 ? totals[1] : 0);
    const bool ok = rc == 0 && got == "1:0:abc\n1:0:abc\n" && kind[0] == 3 && kind[1] == 3 && segment[1] == 1;
    if (!ok) printf("files: rc %ld \"%s\"\n", rc, got.c_str());
    bad |= !ok;
    cases++;
  }
  bad |= hg_gather_digits(18446744073709551615ull) != 20 || hg_gather_digit(18446744073709551615ull, 20, 19) != '5' || hg_gather_digit(4294967296ull, 10, 9) != '6';
  printf(bad ? "FAILED\n" : "%d cases ok\n", cases);
  return bad;
}
#endif
