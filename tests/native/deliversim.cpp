// TEST-ONLY host harness for Face B's delivery (never shipped): a C face over hypergrep_amd/csrc/hg_deliver.h (the result ring,
// the line routines, the per-chunk state object HgDelivery) and over the cut rule of hg_reader.h.  The caller plays scan_file's
// loop: it asks for the context parameters of the next chunk, hands over that chunk's records, and stops when told to; the
// event callback appends (id, line_number, bytes) and the batch sizes to lists the caller reads back.
// With -DDELIVERSIM_MAIN it is a stand-alone program (for a sanitized build) that replays recorded calls from a file of
// 64-bit words and prints what was delivered.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../hypergrep_amd/csrc/hg_deliver.h"
#include "../../hypergrep_amd/csrc/hg_reader.h"

namespace {
struct Sim {
  Ring ring;
  std::unique_ptr<HgDelivery> delivery;
  bool parts = false;
  std::vector<uint64_t> rows;  // {id, line_number, len} per result
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> batches;
};
// rows of 64-bit words -> the records: hits {line, id, to, start, len}, ctx {line, id, start, len}, parts {line, from, to, pattern}
struct Lists {
  std::vector<HgHit> hits, ctx_hits;
  std::vector<HgHitAux> aux, ctx_aux;
  std::vector<HgPart> parts;
  std::vector<uint32_t> part_pattern;
  std::vector<HgPattern> patterns;
  HgChunkRecords view(const uint8_t *base, uint64_t n_pieces, uint64_t owed_after) const {
    HgChunkRecords r;
    r.base = base;
    r.hits = hits.data(), r.aux = aux.data(), r.n_hits = hits.size();
    r.ctx_hits = ctx_hits.data(), r.ctx_aux = ctx_aux.data(), r.n_ctx = ctx_hits.size();
    r.parts = parts.data(), r.part_pattern = part_pattern.data(), r.n_parts = parts.size();
    r.patterns = patterns.data();
    r.n_pieces = n_pieces;
    r.owed_after = owed_after;
    return r;
  }
};
Lists make_lists(const uint64_t *hits, uint64_t n_hits, const uint64_t *ctx, uint64_t n_ctx, const uint64_t *parts, uint64_t n_parts, const uint32_t *pattern_ids, uint32_t n_patterns) {
  Lists l;
  for (uint64_t i = 0; i < n_hits; i++) {
    const uint64_t *h = hits + 5 * i;
    l.hits.push_back(HgHit{h[0], static_cast<uint32_t>(h[1]), static_cast<uint32_t>(h[2])});
    l.aux.push_back(HgHitAux{h[3], static_cast<uint32_t>(h[4]), HG_NONE32});
  }
  for (uint64_t i = 0; i < n_ctx; i++) {
    const uint64_t *c = ctx + 4 * i;
    l.ctx_hits.push_back(HgHit{c[0], static_cast<uint32_t>(c[1]), 0});
    l.ctx_aux.push_back(HgHitAux{c[2], static_cast<uint32_t>(c[3]), HG_NONE32});
  }
  for (uint64_t i = 0; i < n_parts; i++) {
    const uint64_t *p = parts + 4 * i;
    l.parts.push_back(HgPart{p[0], static_cast<uint32_t>(p[1]), static_cast<uint32_t>(p[2])});
    l.part_pattern.push_back(static_cast<uint32_t>(p[3]));
  }
  l.patterns.resize(n_patterns);
  for (uint32_t i = 0; i < n_patterns; i++) {
    std::memset(&l.patterns[i], 0, sizeof(HgPattern));
    l.patterns[i].id = pattern_ids[i];
  }
  return l;
}
}  // namespace

extern "C" {

void *deliversim_new(int parts, uint32_t before, uint32_t after, uint64_t max_match_count, int buffer_count, int buffer_size) {
  Sim *s = new Sim;
  s->parts = parts != 0;
  s->ring.init(buffer_count, buffer_size, [s](hyperscanner_result_t *r, int n) {
    s->batches.push_back(static_cast<uint64_t>(n));
    for (int i = 0; i < n; i++) {
      const size_t len = std::strlen(r[i].line);  // (the test's lines hold no NUL)
      s->rows.insert(s->rows.end(), {r[i].id, r[i].line_number, len});
      s->bytes.insert(s->bytes.end(), r[i].line, r[i].line + len);
    }
  });
  s->delivery = std::make_unique<HgDelivery>(s->ring, s->parts, before, after, max_match_count);
  return s;
}
void deliversim_free(void *h) { delete static_cast<Sim *>(h); }
// out = {before, after, carry_after, tail} of the next chunk's context stage
void deliversim_context_params(void *h, uint64_t *out) {
  const HgContextParams p = static_cast<Sim *>(h)->delivery->context_params();
  out[0] = p.before, out[1] = p.after, out[2] = p.carry_after, out[3] = p.tail;
}
uint64_t deliversim_line_base(void *h) { return static_cast<Sim *>(h)->delivery->line_base(); }
// One chunk through the state object; 1: the call stops.
int deliversim_chunk(void *h, const uint8_t *base, const uint64_t *hits, uint64_t n_hits, const uint64_t *ctx, uint64_t n_ctx, const uint64_t *parts, uint64_t n_parts,
                     const uint32_t *pattern_ids, uint32_t n_patterns, uint64_t n_pieces, uint64_t owed_after) {
  const Lists l = make_lists(hits, n_hits, ctx, n_ctx, parts, n_parts, pattern_ids, n_patterns);
  return static_cast<Sim *>(h)->delivery->chunk(l.view(base, n_pieces, owed_after)) ? 1 : 0;
}
// A whole file through the line routines, as the packed route delivers it; the ring is flushed behind it.
void deliversim_file(void *h, const uint8_t *base, const uint64_t *hits, uint64_t n_hits, const uint64_t *ctx, uint64_t n_ctx, const uint64_t *parts, uint64_t n_parts,
                     const uint32_t *pattern_ids, uint32_t n_patterns) {
  Sim *s = static_cast<Sim *>(h);
  const Lists l = make_lists(hits, n_hits, ctx, n_ctx, parts, n_parts, pattern_ids, n_patterns);
  hg_deliver_file(s->ring, l.view(base, 0, 0), s->parts);
  s->ring.flush();
}
void deliversim_flush(void *h) { static_cast<Sim *>(h)->ring.flush(); }
// sizes = {results, bytes, batches}; then the lists themselves
void deliversim_sizes(void *h, uint64_t *sizes) {
  Sim *s = static_cast<Sim *>(h);
  sizes[0] = s->rows.size() / 3, sizes[1] = s->bytes.size(), sizes[2] = s->batches.size();
}
void deliversim_read(void *h, uint64_t *rows, uint8_t *bytes, uint64_t *batches) {
  Sim *s = static_cast<Sim *>(h);
  if (!s->rows.empty()) std::memcpy(rows, s->rows.data(), s->rows.size() * 8);
  if (!s->bytes.empty()) std::memcpy(bytes, s->bytes.data(), s->bytes.size());
  if (!s->batches.empty()) std::memcpy(batches, s->batches.data(), s->batches.size() * 8);
}
uint64_t deliversim_cut(const uint8_t *buf, uint64_t have, uint64_t bs1) { return hg_chunk_cut(buf, have, bs1); }

}  // extern "C"

#ifdef DELIVERSIM_MAIN
#include <cstdio>

// The file: calls, one after the other, as 64-bit words.  A call: 1, parts, before, after, max_match_count, buffer_count,
// buffer_size, n_patterns, their ids, n_chunks; a chunk: n_bytes, the bytes (a word each), n_hits, hit rows, n_ctx, context rows,
// n_parts, part rows, n_pieces, owed_after.  A chunk behind the one that stopped the call is an error.  One line per call:
// "id:line:hex ..." then "|" and the batch sizes.
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint64_t> w;
  uint64_t v;
  while (std::fread(&v, 8, 1, f) == 1) w.push_back(v);
  std::fclose(f);
  size_t at = 0;
  auto take = [&](size_t n) {
    if (at + n > w.size()) std::exit(3);
    const uint64_t *p = w.data() + at;
    at += n;
    return p;
  };
  long calls = 0;
  while (at < w.size()) {
    const uint64_t *head = take(8);
    if (head[0] != 1) return 3;
    const uint32_t n_patterns = static_cast<uint32_t>(head[7]);
    std::vector<uint32_t> ids(n_patterns);
    for (uint32_t i = 0; i < n_patterns; i++) ids[i] = static_cast<uint32_t>(*take(1));
    void *h = deliversim_new(static_cast<int>(head[1]), static_cast<uint32_t>(head[2]), static_cast<uint32_t>(head[3]), head[4], static_cast<int>(head[5]), static_cast<int>(head[6]));
    const uint64_t n_chunks = *take(1);
    bool stopped = false;
    for (uint64_t c = 0; c < n_chunks; c++) {
      if (stopped) return 4;
      const uint64_t n_bytes = *take(1);
      const uint64_t *b = take(n_bytes);
      std::vector<uint8_t> base(b, b + n_bytes);  // (exactly the chunk's bytes: a read past them is the sanitizer's to find)
      const uint64_t n_hits = *take(1), *hits = take(5 * n_hits), n_ctx = *take(1), *ctx = take(4 * n_ctx), n_parts = *take(1), *parts = take(4 * n_parts), *tail = take(2);
      stopped = deliversim_chunk(h, base.data(), hits, n_hits, ctx, n_ctx, parts, n_parts, ids.data(), n_patterns, tail[0], tail[1]) != 0;
    }
    deliversim_flush(h);
    const Sim *s = static_cast<const Sim *>(h);
    size_t byte_at = 0;
    for (size_t i = 0; i < s->rows.size(); i += 3) {
      std::printf("%llu:%llu:", static_cast<unsigned long long>(s->rows[i]), static_cast<unsigned long long>(s->rows[i + 1]));
      for (uint64_t j = 0; j < s->rows[i + 2]; j++) std::printf("%02x", s->bytes[byte_at++]);
      std::printf(" ");
    }
    std::printf("|");
    for (uint64_t n : s->batches) std::printf(" %llu", static_cast<unsigned long long>(n));
    std::printf("\n");
    deliversim_free(h);
    calls++;
  }
  std::fprintf(stderr, "deliversim: %ld calls replayed\n", calls);
  return 0;
}
#endif
