// hg_* entry points of include/hypergrep_amd.h: thin C wrappers over HgDb / HgScanner, plus the
// synthetic-log generator kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/hypergrep_amd.h"
#include "hg_compile.h"
#include "hg_engine.h"
#include "hg_synth.h"

struct hg_database {
  std::shared_ptr<const HgDb> db;  // scanners share it; hg_db_tune swaps in a tuned copy, scanners made before keep theirs
};
struct hg_scanner {
  HgScanner *sc;
  hg_scan_result_t last;
  const uint32_t *d_from;  // the last scan's hit starts (SOM databases), else nullptr: every start is 0
  hg_context_result_t last_ctx;  // the last scan's context records (hg_scan_device_context), else zeroes
  hg_segment_result_t last_seg;  // the last scan's per-segment arrays (hg_scan_device_segments), else zeroes
  uint32_t last_n_seg;
  hg_parts_result_t last_parts;  // the last scan's parts (hg_scan_device_parts), else zeroes
  HgSegCtxOutput last_segctx;    // the last scan's per-segment context arrays (hg_scan_device_segments_context), else zeroes
  HgSegPartsOutput last_segparts;  // the last scan's per-segment parts arrays (hg_scan_device_segments_parts), else zeroes
  // what hg_gather_lines needs of the last successful scan (scanned == false: none yet, or the last one failed), the stage's
  // own buffers (made by the first gather), and the last gather's result (zeroes after a scan)
  bool scanned;
  const void *last_text;
  uint64_t last_nbytes;
  const uint64_t *last_seg_start;
  HgGather *gather;
  hg_lines_result_t last_lines;
  // what hg_count_records needs beside them: whether the last scan was inverted; the stage's own buffers and running totals
  // (made by the first count), and the last count's result (its matrices are gone after a scan)
  bool last_invert;
  HgCounts *counts;
  hg_counts_result_t last_counts;
  // what hg_gather_parts needs beside them: whether the last scan was one with parts (zero parts leave last_parts empty); the
  // stage's own buffers (made by the first parts gather), and the last parts gather's result (zeroes after a scan)
  bool last_with_parts = false;
  HgPartLines *partlines = nullptr;
  hg_part_lines_result_t last_part_lines = {};
  // the values stage's own buffers (made by the first hg_count_values) and its last result (zeroes after a scan)
  HgValues *values = nullptr;
  hg_values_result_t last_values = {};
  // the rank stage's own buffers (made by the first hg_rank_values) and its last result (zeroes after a scan)
  HgRank *rank = nullptr;
  hg_rank_result_t last_rank = {};
  // the value store (made by the first hg_accumulate_values; it survives scans) and its last ranking (zeroes after an accumulate
  // or a reset)
  HgValueStore *store = nullptr;
  hg_acc_rank_result_t last_acc_rank = {};
};

static_assert(HG_ID_CONTEXT == HG_CTX_ID_CONTEXT && HG_ID_CONTEXT_TAIL == HG_CTX_ID_TAIL, "the context records carry the ids the header names");
static_assert(sizeof(hg_part_t) == sizeof(HgPart) && sizeof(hg_parts_result_t) == 32, "ABI records mirror the device records");
static_assert(sizeof(hg_hit_t) == sizeof(HgHit) && sizeof(hg_hit_aux_t) == sizeof(HgHitAux), "ABI records mirror the device records");
static_assert(HG_LINES_CONTEXT == HG_GATHER_CONTEXT && HG_LINES_TERMINATE == HG_GATHER_TERMINATE && HG_LINES_NUMBER == HG_GATHER_NUMBER &&
                  HG_LINES_SEPARATOR == HG_GATHER_SEPARATOR && HG_LINE_MATCH == HG_GATHER_MATCH && HG_LINE_CONTEXT == HG_GATHER_KIND_CONTEXT &&
                  HG_LINE_TAIL == HG_GATHER_KIND_TAIL && sizeof(hg_lines_result_t) == 72,
              "the gather stage's flags and kinds are the header's");
static_assert(HG_COUNTS_ACCUMULATE == HG_COUNTS_F_ACCUMULATE && HG_COUNTS_PER_SEGMENT == HG_COUNTS_F_PER_SEGMENT && HG_COUNTS_LDS_BINS == HG_COUNTS_LDS_MAX &&
                  sizeof(hg_counts_result_t) == 64,
              "the counts stage's flags and limit are the header's");
static_assert(HG_PARTS_NUMBER == HG_PARTLINES_NUMBER && HG_PARTS_BYTE_OFFSET == HG_PARTLINES_BYTE_OFFSET && HG_PARTS_TERMINATE == HG_PARTLINES_TERMINATE &&
                  HG_PARTS_LINE == HG_PARTLINES_LINE && HG_PART_FIRST == HG_PARTLINES_FIRST && HG_PART_LAST == HG_PARTLINES_LAST &&
                  HG_PARTS_MARK_MAX == HG_PARTLINES_MARK_MAX && sizeof(hg_part_lines_params_t) == 56 && sizeof(hg_part_lines_result_t) == 80,
              "the parts gather's flags, kinds and limit are the header's");
static_assert(HG_VALUES_BY_PATTERN == HG_VALUES_F_BY_PATTERN && sizeof(hg_values_params_t) == 16 && sizeof(hg_values_result_t) == 88, "the values stage's flag is the header's");
static_assert(HG_RANK_BY_PATTERN == HG_RANK_F_BY_PATTERN && HG_RANK_PER_SEGMENT == HG_RANK_F_PER_SEGMENT && sizeof(hg_rank_params_t) == 24 && sizeof(hg_rank_result_t) == 128,
              "the rank stage's flags are the header's");
static_assert(HG_ACC_BY_PATTERN == HG_VALSTORE_F_BY_PATTERN && sizeof(hg_acc_params_t) == 16 && sizeof(hg_acc_result_t) == 56 && sizeof(hg_acc_rank_result_t) == 88,
              "the value store's flag is the header's");

static void put_err(char *err, size_t errlen, const std::string &msg) {
  if (err && errlen) std::snprintf(err, errlen, "%s", msg.c_str());
}

extern "C" {

int hg_db_compile(const char *const *expressions, const unsigned int *flags, const unsigned int *ids, unsigned int n,
                  hg_database_t **db, char *err, size_t errlen) {
  return hg_db_compile_ext(expressions, flags, ids, nullptr, n, db, err, errlen);
}

int hg_db_compile_ext(const char *const *expressions, const unsigned int *flags, const unsigned int *ids, const hs_expr_ext_t *const *ext,
                      unsigned int n, hg_database_t **db, char *err, size_t errlen) {
  if (!db) return HG_ERR_ARG;
  *db = nullptr;
  HgDb *d = nullptr;
  std::string msg;
  int bad = -1;
  int rc = hgc_compile_ext(expressions, flags, ids, ext, n, &d, &msg, &bad);
  if (rc != 0) {
    put_err(err, errlen, std::to_string(bad) + ": " + msg);
    return rc == -2 ? HG_ERR_NOMEM : (rc == -1 ? HG_ERR_ARG : HG_ERR_COMPILE);
  }
  *db = new hg_database{std::shared_ptr<const HgDb>(d, [](const HgDb *x) { hgc_free(const_cast<HgDb *>(x)); })};
  return HG_OK;
}

int hg_db_tune(hg_database_t *db, const void *sample, size_t nbytes) {
  if (!db || (!sample && nbytes)) return HG_ERR_ARG;
  std::string err;
  HgDb *tuned = nullptr;
  if (hgc_tune(db->db.get(), static_cast<const uint8_t *>(sample), nbytes, &tuned, &err) != 0) return HG_ERR_COMPILE;  // (the database is unchanged)
  db->db = std::shared_ptr<const HgDb>(tuned, [](const HgDb *x) { hgc_free(const_cast<HgDb *>(x)); });
  return HG_OK;
}

void hg_db_release(hg_database_t *db) {
  delete db;  // (scanners created from it keep the compiled tables alive)
}

int hg_db_info(const hg_database_t *db, hg_db_info_t *info) {
  if (!db || !info) return HG_ERR_ARG;
  const HgDb &d = *db->db;
  info->n_patterns = static_cast<uint32_t>(d.patterns.size());
  info->n_always_on = static_cast<uint32_t>(d.slow.size());
  info->n_literal_anchored = info->n_patterns - info->n_always_on - d.ncomb;  // (combinations are neither: no automaton)
  info->n_factors = d.nreal_factors;
  info->n_windows = d.nreal_factors ? static_cast<uint32_t>(d.windows.size()) : 0;
  info->fold_mask = d.fold_mask;
  info->max_state_words = d.max_nw;
  info->table_bytes = static_cast<uint32_t>(d.pool.size() * 4);
  info->byte_windows = d.dense;
  return HG_OK;
}

int hg_scanner_create(const hg_database_t *db, int device, hg_scanner_t **scanner, char *err, size_t errlen) {
  if (!db || !scanner) return HG_ERR_ARG;
  *scanner = nullptr;
  HgScanner *sc = nullptr;
  std::string msg;
  int rc = HgScanner::create(db->db, device, &sc, &msg);
  if (rc != HG_OK) {
    put_err(err, errlen, msg);
    return rc;
  }
  *scanner = new hg_scanner{sc, {}, nullptr, {}, {}, 0, {}, {}, {}, false, nullptr, 0, nullptr, nullptr, {}, false, nullptr, {}};
  return HG_OK;
}

void hg_scanner_destroy(hg_scanner_t *scanner) {
  if (!scanner) return;
  delete scanner->gather;
  delete scanner->counts;
  delete scanner->partlines;
  delete scanner->values;
  delete scanner->rank;
  delete scanner->store;
  delete scanner->sc;
  delete scanner;
}

const char *hg_scanner_error(const hg_scanner_t *scanner) { return scanner ? scanner->sc->last_error().c_str() : "null scanner"; }

static int scan_device(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, void *stream,
                       hg_scan_result_t *result, bool invert, const hg_context_t *context = nullptr, hg_context_result_t *context_result = nullptr,
                       const hg_segments_t *segments = nullptr, hg_segment_result_t *segment_result = nullptr, hg_parts_result_t *parts_result = nullptr,
                       hg_segment_parts_result_t *segment_parts = nullptr) {
  if (!scanner || !result) return HG_ERR_ARG;
  HgScanOutput o{};
  HgPartsOutput pt{};
  scanner->scanned = false;
  scanner->last_lines = hg_lines_result_t{};
  scanner->last_part_lines = hg_part_lines_result_t{};
  scanner->last_values = hg_values_result_t{};
  scanner->last_rank = hg_rank_result_t{};
  scanner->last_with_parts = false;
  scanner->last_counts.n_seg = 0;  // (the totals stay: HG_COUNTS_ACCUMULATE adds the next scan's)
  scanner->last_counts.d_seg_lines = scanner->last_counts.d_seg_reports = nullptr;
  scanner->last_parts = hg_parts_result_t{};
  HgContextOutput c{};
  HgSegOutput g{};
  int rc;
  scanner->last_seg = hg_segment_result_t{};
  scanner->last_n_seg = 0;
  scanner->last_segctx = HgSegCtxOutput{};
  HgSegCtxOutput sx{};
  scanner->last_segparts = HgSegPartsOutput{};
  HgSegPartsOutput sp{};
  if (segments) {
    const HgSegParams params{segments->d_seg_start, segments->d_seg_end, segments->n_seg, segments->max_per_segment};
    if (parts_result)  // (hg_scan_device_segments_parts: per-file parts, never inverted)
      rc = scanner->sc->scan_packed_parts(d_text, nbytes, buffer_size, static_cast<hipStream_t>(stream), params, &o, &g, &pt, &sp);
    else if (context)  // (hg_scan_device_segments_context: per-file context, no carry and no tail)
      rc = scanner->sc->scan_packed_context(d_text, nbytes, buffer_size, static_cast<hipStream_t>(stream), params, context->before, context->after, invert, &o, &g, &c, &sx);
    else
      rc = scanner->sc->scan_packed(d_text, nbytes, buffer_size, static_cast<hipStream_t>(stream), params, invert, &o, &g);
    if (rc != HG_OK) {  // (nothing was scanned, or the scan failed: no records to copy)
      scanner->last = hg_scan_result_t{};
      scanner->d_from = nullptr;
    }
  } else if (context) {
    const HgContextParams params{context->before, context->after, context->carry_after, (context->flags & HG_CONTEXT_TAIL) != 0};
    rc = scanner->sc->scan_context(d_text, nbytes, buffer_size, line_base, static_cast<hipStream_t>(stream), params, invert, &o, &c);
  } else if (parts_result) {
    rc = scanner->sc->scan_parts(d_text, nbytes, buffer_size, line_base, static_cast<hipStream_t>(stream), &o, &pt);
  } else {
    rc = scanner->sc->scan(d_text, nbytes, buffer_size, line_base, static_cast<hipStream_t>(stream), &o, invert);
  }
  if (rc != HG_OK) return rc;
  if (parts_result) {
    scanner->last_parts = hg_parts_result_t{pt.n_parts, reinterpret_cast<const hg_part_t *>(pt.d_parts), pt.d_pattern, static_cast<uint32_t>(pt.ms_parts * 1000.0f + 0.5f), 0};
    *parts_result = scanner->last_parts;
  }
  scanner->last_ctx = hg_context_result_t{c.n_context, c.n_tail, c.owed_after, reinterpret_cast<const hg_hit_t *>(c.d_hits), reinterpret_cast<const hg_hit_aux_t *>(c.d_aux),
                                          static_cast<uint32_t>(c.ms_context * 1000.0f + 0.5f), 0};
  if (context_result) *context_result = scanner->last_ctx;
  if (segments) {
    scanner->last_seg = hg_segment_result_t{g.d_record_segment, g.d_first_record, g.d_n_lines, g.d_n_selected, static_cast<uint32_t>(g.ms_segments * 1000.0f + 0.5f), 0};
    scanner->last_n_seg = segments->n_seg;
    *segment_result = scanner->last_seg;
    scanner->last_segctx = sx;
    scanner->last_segparts = sp;
    if (segment_parts) *segment_parts = hg_segment_parts_result_t{sp.d_part_segment, sp.d_first_part};
  }
  result->n_hits = o.n_hits;
  result->n_lines = o.n_pieces;
  result->n_candidates = o.n_cands;
  result->n_raw_hits = o.n_raw_hits;
  result->d_hits = reinterpret_cast<const hg_hit_t *>(o.d_hits);
  result->d_aux = reinterpret_cast<const hg_hit_aux_t *>(o.d_aux);
  result->ms_stream = o.ms_stream;
  result->ms_total = o.ms_total;
  result->reruns = o.reruns;
  result->stream_launches = o.stream_launches;
  result->joiner_tiles = o.joiner_tiles;
  result->joiner_launches = o.joiner_launches;
  result->invert_us = static_cast<uint32_t>(o.ms_invert * 1000.0f + 0.5f);
  scanner->last = *result;
  scanner->d_from = o.d_from;
  scanner->scanned = true;
  scanner->last_invert = invert;
  scanner->last_with_parts = parts_result != nullptr;
  scanner->last_text = d_text;
  scanner->last_nbytes = nbytes;
  scanner->last_seg_start = segments ? segments->d_seg_start : nullptr;
  return HG_OK;
}

int hg_scan_device(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, void *stream,
                   hg_scan_result_t *result) {
  return scan_device(scanner, d_text, nbytes, buffer_size, line_base, stream, result, false);
}

int hg_scan_device_invert(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, void *stream,
                          hg_scan_result_t *result) {
  return scan_device(scanner, d_text, nbytes, buffer_size, line_base, stream, result, true);
}

int hg_scan_device_context(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, void *stream,
                           const hg_context_t *context, int invert, hg_scan_result_t *result, hg_context_result_t *context_result) {
  if (!context || !context_result || (context->flags & ~HG_CONTEXT_TAIL)) return HG_ERR_ARG;
  return scan_device(scanner, d_text, nbytes, buffer_size, line_base, stream, result, invert != 0, context, context_result);
}

int hg_scan_device_segments(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, void *stream, const hg_segments_t *segments, int invert,
                            hg_scan_result_t *result, hg_segment_result_t *segment_result) {
  if (!segments || !segment_result) return HG_ERR_ARG;
  *segment_result = hg_segment_result_t{};
  return scan_device(scanner, d_text, nbytes, buffer_size, 0, stream, result, invert != 0, nullptr, nullptr, segments, segment_result);
}

int hg_scan_device_segments_context(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, void *stream, const hg_segments_t *segments,
                                    uint32_t before, uint32_t after, int invert, hg_scan_result_t *result, hg_segment_result_t *segment_result,
                                    hg_context_result_t *context_result) {
  if (!segments || !segment_result || !context_result) return HG_ERR_ARG;
  *segment_result = hg_segment_result_t{};
  *context_result = hg_context_result_t{};
  const hg_context_t context{before, after, 0, 0};
  return scan_device(scanner, d_text, nbytes, buffer_size, 0, stream, result, invert != 0, &context, context_result, segments, segment_result);
}

int hg_scan_device_parts(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, void *stream, hg_scan_result_t *result,
                         hg_parts_result_t *parts) {
  if (!parts) return HG_ERR_ARG;
  *parts = hg_parts_result_t{};
  return scan_device(scanner, d_text, nbytes, buffer_size, line_base, stream, result, false, nullptr, nullptr, nullptr, nullptr, parts);
}

int hg_scan_device_segments_parts(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, void *stream, const hg_segments_t *segments,
                                  hg_scan_result_t *result, hg_segment_result_t *segment_result, hg_parts_result_t *parts, hg_segment_parts_result_t *segment_parts) {
  if (!segments || !segment_result || !parts || !segment_parts) return HG_ERR_ARG;
  *segment_result = hg_segment_result_t{};
  *parts = hg_parts_result_t{};
  *segment_parts = hg_segment_parts_result_t{};
  return scan_device(scanner, d_text, nbytes, buffer_size, 0, stream, result, false, nullptr, nullptr, segments, segment_result, parts, segment_parts);
}

int hg_gather_lines(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, uint32_t flags, void *stream, hg_lines_result_t *result) {
  if (!scanner) return HG_ERR_ARG;
  if (result) *result = hg_lines_result_t{};
  const char *why = !result                                                                      ? "hg_gather_lines: result is NULL"
                    : !scanner->scanned                                                          ? "hg_gather_lines: no successful scan to gather the lines of"
                    : (d_text != scanner->last_text || nbytes != scanner->last_nbytes)           ? "hg_gather_lines: d_text and nbytes are not those of the last scan"
                    : (flags & ~(HG_LINES_CONTEXT | HG_LINES_TERMINATE | HG_LINES_NUMBER | HG_LINES_SEPARATOR)) ? "hg_gather_lines: unknown flag bits"
                                                                                                 : nullptr;
  if (why) return scanner->sc->set_error(HG_ERR_ARG, why);
  scanner->last_lines = hg_lines_result_t{};
  if (!scanner->gather) scanner->gather = new HgGather(scanner->sc->device());
  const bool seg = scanner->last_seg.d_first_record != nullptr, ctx = (flags & HG_LINES_CONTEXT) && scanner->last_ctx.n_context;
  HgGatherInput in{};
  in.text = static_cast<const uint8_t *>(d_text);
  in.main = HgGatherList{reinterpret_cast<const HgHit *>(scanner->last.d_hits), reinterpret_cast<const HgHitAux *>(scanner->last.d_aux),
                         seg ? scanner->last_seg.d_record_segment : nullptr, scanner->last.n_hits};
  if (ctx)
    in.ctx = HgGatherList{reinterpret_cast<const HgHit *>(scanner->last_ctx.d_ctx_hits), reinterpret_cast<const HgHitAux *>(scanner->last_ctx.d_ctx_aux),
                          seg ? scanner->last_segctx.d_context_segment : nullptr, scanner->last_ctx.n_context};
  if (seg) {
    in.seg_start = scanner->last_seg_start;
    in.first_record = scanner->last_seg.d_first_record;
    in.first_context = ctx ? scanner->last_segctx.d_first_context : nullptr;
    in.n_seg = scanner->last_n_seg;
  }
  in.flags = flags;
  HgGatherOutput o{};
  std::string err;
  const int rc = scanner->gather->run(in, static_cast<hipStream_t>(stream), &o, &err);
  if (rc != HG_OK) return scanner->sc->set_error(rc, err);
  scanner->last_lines = hg_lines_result_t{o.n_entries, o.n_bytes, o.d_bytes, o.d_entry_off, o.d_line_number, o.d_kind, o.d_segment, o.d_first_entry,
                                          static_cast<uint32_t>(o.ms_gather * 1000.0f + 0.5f), 0};
  *result = scanner->last_lines;
  return HG_OK;
}

int hg_copy_lines(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *entry_off, uint64_t *line_number, uint32_t *kind, uint32_t *segment,
                  uint64_t max_entries) {
  if (!scanner) return HG_ERR_ARG;
  const hg_lines_result_t &g = scanner->last_lines;
  if (!g.d_entry_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_lines: no gather since the last scan");
  if (segment && !g.d_segment) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_lines: the last scan had no segments");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t nb = std::min(g.n_bytes, max_bytes), ne = std::min(g.n_entries, max_entries);
  if (bytes && nb && hipMemcpy(bytes, g.d_bytes, nb, hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (entry_off && hipMemcpy(entry_off, g.d_entry_off, (ne + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (line_number && ne && hipMemcpy(line_number, g.d_line_number, ne * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (kind && ne && hipMemcpy(kind, g.d_kind, ne * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (segment && ne && hipMemcpy(segment, g.d_segment, ne * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_lines_first(hg_scanner_t *scanner, uint64_t *first_entry) {
  if (!scanner || !first_entry) return HG_ERR_ARG;
  const hg_lines_result_t &g = scanner->last_lines;
  if (!g.d_first_entry) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_lines_first: no gather after a scan with segments");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  return hipMemcpy(first_entry, g.d_first_entry, (scanner->last_n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_copy_lines_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  const hg_lines_result_t &g = scanner->last_lines;
  if (!g.d_entry_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_lines_device: no gather since the last scan");
  const uint64_t nb = std::min(g.n_bytes, max_bytes);
  if (!nb) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  return hipMemcpyAsync(d_dst, g.d_bytes, nb, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_gather_parts(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, const hg_part_lines_params_t *params, void *stream, hg_part_lines_result_t *result) {
  if (!scanner) return HG_ERR_ARG;
  if (result) *result = hg_part_lines_result_t{};
  const bool seg = scanner->last_seg.d_first_record != nullptr;
  const char *why = !result                                                                    ? "hg_gather_parts: result is NULL"
                    : !params                                                                  ? "hg_gather_parts: params is NULL"
                    : !scanner->scanned                                                        ? "hg_gather_parts: no successful scan to gather the parts of"
                    : (d_text != scanner->last_text || nbytes != scanner->last_nbytes)         ? "hg_gather_parts: d_text and nbytes are not those of the last scan"
                    : !scanner->last_with_parts                                                ? "hg_gather_parts: the last scan was not one with parts (hg_scan_device_parts, hg_scan_device_segments_parts)"
                    : (params->flags & ~(HG_PARTS_NUMBER | HG_PARTS_BYTE_OFFSET | HG_PARTS_TERMINATE | HG_PARTS_LINE)) ? "hg_gather_parts: unknown flag bits"
                    : (params->mark_on_len > HG_PARTS_MARK_MAX || params->mark_off_len > HG_PARTS_MARK_MAX) ? "hg_gather_parts: a mark of more than 16 bytes"
                    : (seg && params->byte_base)                                               ? "hg_gather_parts: byte_base must be 0 after a scan with segments (the starts are file-relative)"
                                                                                               : nullptr;
  if (why) return scanner->sc->set_error(HG_ERR_ARG, why);
  scanner->last_part_lines = hg_part_lines_result_t{};
  if (!scanner->partlines) scanner->partlines = new HgPartLines(scanner->sc->device());
  HgPartLinesInput in{};
  in.text = static_cast<const uint8_t *>(d_text);
  in.recs = HgGatherList{reinterpret_cast<const HgHit *>(scanner->last.d_hits), reinterpret_cast<const HgHitAux *>(scanner->last.d_aux),
                         seg ? scanner->last_seg.d_record_segment : nullptr, scanner->last.n_hits};
  in.parts = reinterpret_cast<const HgPart *>(scanner->last_parts.d_parts);
  in.part_pattern = scanner->last_parts.d_part_pattern;
  in.n_parts = scanner->last_parts.n_parts;
  if (seg) {
    in.part_seg = scanner->last_segparts.d_part_segment;
    in.seg_start = scanner->last_seg_start;
    in.first_part = scanner->last_segparts.d_first_part;
    in.n_seg = scanner->last_n_seg;
  }
  in.flags = params->flags;
  in.byte_base = params->byte_base;
  in.marks = hg_partlines_marks(params->mark_on, params->mark_on_len, params->mark_off, params->mark_off_len);
  HgPartLinesOutput o{};
  std::string err;
  const int rc = scanner->partlines->run(in, static_cast<hipStream_t>(stream), &o, &err);
  if (rc != HG_OK) return scanner->sc->set_error(rc, err);
  scanner->last_part_lines = hg_part_lines_result_t{o.n_entries, o.n_bytes, o.d_bytes, o.d_entry_off, o.d_line_number, o.d_kind, o.d_pattern, o.d_segment, o.d_first_entry,
                                                    static_cast<uint32_t>(o.ms_gather * 1000.0f + 0.5f), 0};
  *result = scanner->last_part_lines;
  return HG_OK;
}

int hg_copy_part_lines(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *entry_off, uint64_t *line_number, uint32_t *kind, uint32_t *pattern,
                       uint32_t *segment, uint64_t max_entries) {
  if (!scanner) return HG_ERR_ARG;
  const hg_part_lines_result_t &g = scanner->last_part_lines;
  if (!g.d_entry_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_part_lines: no parts gather since the last scan");
  if (segment && !g.d_segment) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_part_lines: the last scan had no segments");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t nb = std::min(g.n_bytes, max_bytes), ne = std::min(g.n_entries, max_entries);
  if (bytes && nb && hipMemcpy(bytes, g.d_bytes, nb, hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (entry_off && hipMemcpy(entry_off, g.d_entry_off, (ne + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (line_number && ne && hipMemcpy(line_number, g.d_line_number, ne * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (kind && ne && hipMemcpy(kind, g.d_kind, ne * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (pattern && ne && hipMemcpy(pattern, g.d_pattern, ne * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (segment && ne && hipMemcpy(segment, g.d_segment, ne * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_part_lines_first(hg_scanner_t *scanner, uint64_t *first_entry) {
  if (!scanner || !first_entry) return HG_ERR_ARG;
  const hg_part_lines_result_t &g = scanner->last_part_lines;
  if (!g.d_first_entry) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_part_lines_first: no parts gather after a scan with segments");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  return hipMemcpy(first_entry, g.d_first_entry, (scanner->last_n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_copy_part_lines_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  const hg_part_lines_result_t &g = scanner->last_part_lines;
  if (!g.d_entry_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_part_lines_device: no parts gather since the last scan");
  const uint64_t nb = std::min(g.n_bytes, max_bytes);
  if (!nb) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  return hipMemcpyAsync(d_dst, g.d_bytes, nb, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_count_values(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, const hg_values_params_t *params, void *stream, hg_values_result_t *result) {
  if (!scanner) return HG_ERR_ARG;
  if (result) *result = hg_values_result_t{};
  scanner->last_values = hg_values_result_t{};  // (a refused call leaves no earlier count behind for hg_copy_values)
  const hg_values_params_t p = params ? *params : hg_values_params_t{0, 0, 0, 0};
  const bool seg = scanner->last_seg.d_first_record != nullptr;
  const uint64_t n_parts = scanner->last_with_parts ? scanner->last_parts.n_parts : 0;
  const char *why = !result                                                            ? "hg_count_values: result is NULL"
                    : !scanner->scanned                                                ? "hg_count_values: no successful scan to count the values of"
                    : (d_text != scanner->last_text || nbytes != scanner->last_nbytes) ? "hg_count_values: d_text and nbytes are not those of the last scan"
                    : !scanner->last_with_parts                                        ? "hg_count_values: the last scan was not one with parts (hg_scan_device_parts, hg_scan_device_segments_parts)"
                    : (p.flags & ~HG_VALUES_BY_PATTERN)                                ? "hg_count_values: unknown flag bits"
                    : p.hash_bits > 64                                                 ? "hg_count_values: hash_bits above 64"
                    : p.table_log2 > HG_VALUES_MAX_TABLE_LOG2                          ? "hg_count_values: table_log2 above 40"
                    : (p.table_log2 && (uint64_t{1} << p.table_log2) <= n_parts)       ? "hg_count_values: 2^table_log2 must exceed the number of parts"
                    : (!p.table_log2 && hg_values_default_log2(n_parts) > HG_VALUES_MAX_TABLE_LOG2) ? "hg_count_values: more parts than a table of 2^40 slots serves"
                                                                                       : nullptr;
  if (why) return scanner->sc->set_error(HG_ERR_ARG, why);
  if (!scanner->values) scanner->values = new HgValues(scanner->sc->device());
  HgValuesInput in{};
  in.text = static_cast<const uint8_t *>(d_text);
  in.recs = HgGatherList{reinterpret_cast<const HgHit *>(scanner->last.d_hits), reinterpret_cast<const HgHitAux *>(scanner->last.d_aux),
                         seg ? scanner->last_seg.d_record_segment : nullptr, scanner->last.n_hits};
  in.parts = reinterpret_cast<const HgPart *>(scanner->last_parts.d_parts);
  in.part_pattern = scanner->last_parts.d_part_pattern;
  in.n_parts = n_parts;
  if (seg) {
    in.part_seg = scanner->last_segparts.d_part_segment;
    in.seg_start = scanner->last_seg_start;
  }
  in.flags = p.flags;
  in.hash_bits = p.hash_bits ? p.hash_bits : 64;
  in.table_log2 = p.table_log2 ? p.table_log2 : hg_values_default_log2(n_parts);
  HgValuesOutput o{};
  std::string err;
  const int rc = scanner->values->run(in, static_cast<hipStream_t>(stream), &o, &err);
  if (rc != HG_OK) return scanner->sc->set_error(rc, err);
  scanner->last_values = hg_values_result_t{o.n_values, o.n_parts, o.n_bytes, o.d_bytes, o.d_off, o.d_count, o.d_first, o.d_pattern, o.d_line_number, o.d_segment,
                                            o.table_log2, static_cast<uint32_t>(o.ms_values * 1000.0f + 0.5f)};
  *result = scanner->last_values;
  return HG_OK;
}

int hg_copy_values(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number,
                   uint32_t *segment, uint64_t max_values) {
  if (!scanner) return HG_ERR_ARG;
  const hg_values_result_t &g = scanner->last_values;
  if (!g.d_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_values: no value count since the last scan");
  if (segment && !g.d_segment) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_values: the last scan had no segments");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t nb = std::min(g.n_bytes, max_bytes), nv = std::min(g.n_values, max_values);
  if (bytes && nb && hipMemcpy(bytes, g.d_bytes, nb, hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (off && hipMemcpy(off, g.d_off, (nv + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (count && nv && hipMemcpy(count, g.d_count, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (first && nv && hipMemcpy(first, g.d_first, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (pattern && nv && hipMemcpy(pattern, g.d_pattern, nv * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (line_number && nv && hipMemcpy(line_number, g.d_line_number, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (segment && nv && hipMemcpy(segment, g.d_segment, nv * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_values_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  const hg_values_result_t &g = scanner->last_values;
  if (!g.d_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_values_device: no value count since the last scan");
  const uint64_t nb = std::min(g.n_bytes, max_bytes);
  if (!nb) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  return hipMemcpyAsync(d_dst, g.d_bytes, nb, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_rank_values(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, const hg_rank_params_t *params, void *stream, hg_rank_result_t *result) {
  if (!scanner) return HG_ERR_ARG;
  if (result) *result = hg_rank_result_t{};
  scanner->last_rank = hg_rank_result_t{};  // (a refused call leaves no earlier ranking behind for hg_copy_ranked_values)
  const hg_rank_params_t p = params ? *params : hg_rank_params_t{0, 0, 0, 0, 0};
  const bool seg = scanner->last_seg.d_first_record != nullptr;
  const uint64_t n_parts = scanner->last_with_parts ? scanner->last_parts.n_parts : 0;
  const char *why = !result                                                            ? "hg_rank_values: result is NULL"
                    : !scanner->scanned                                                ? "hg_rank_values: no successful scan to rank the values of"
                    : (d_text != scanner->last_text || nbytes != scanner->last_nbytes) ? "hg_rank_values: d_text and nbytes are not those of the last scan"
                    : !scanner->last_with_parts                                        ? "hg_rank_values: the last scan was not one with parts (hg_scan_device_parts, hg_scan_device_segments_parts)"
                    : (p.flags & ~(HG_RANK_BY_PATTERN | HG_RANK_PER_SEGMENT))          ? "hg_rank_values: unknown flag bits"
                    : ((p.flags & HG_RANK_PER_SEGMENT) && !seg)                        ? "hg_rank_values: HG_RANK_PER_SEGMENT after a scan without segments"
                    : p.hash_bits > 64                                                 ? "hg_rank_values: hash_bits above 64"
                    : p.table_log2 > HG_VALUES_MAX_TABLE_LOG2                          ? "hg_rank_values: table_log2 above 40"
                    : (p.table_log2 && (uint64_t{1} << p.table_log2) <= n_parts)       ? "hg_rank_values: 2^table_log2 must exceed the number of parts"
                    : (!p.table_log2 && hg_values_default_log2(n_parts) > HG_VALUES_MAX_TABLE_LOG2) ? "hg_rank_values: more parts than a table of 2^40 slots serves"
                                                                                       : nullptr;
  if (why) return scanner->sc->set_error(HG_ERR_ARG, why);
  if (!scanner->rank) scanner->rank = new HgRank(scanner->sc->device());
  HgRankInput in{};
  in.values.text = static_cast<const uint8_t *>(d_text);
  in.values.recs = HgGatherList{reinterpret_cast<const HgHit *>(scanner->last.d_hits), reinterpret_cast<const HgHitAux *>(scanner->last.d_aux),
                                seg ? scanner->last_seg.d_record_segment : nullptr, scanner->last.n_hits};
  in.values.parts = reinterpret_cast<const HgPart *>(scanner->last_parts.d_parts);
  in.values.part_pattern = scanner->last_parts.d_part_pattern;
  in.values.n_parts = n_parts;
  if (seg) {
    in.values.part_seg = scanner->last_segparts.d_part_segment;
    in.values.seg_start = scanner->last_seg_start;
  }
  in.values.flags = p.flags;
  in.values.hash_bits = p.hash_bits ? p.hash_bits : 64;
  in.values.table_log2 = p.table_log2 ? p.table_log2 : hg_values_default_log2(n_parts);
  in.n_seg = seg ? scanner->last_n_seg : 0;
  in.top = p.top;
  HgRankOutput o{};
  std::string err;
  const int rc = scanner->rank->run(in, static_cast<hipStream_t>(stream), &o, &err);
  if (rc != HG_OK) return scanner->sc->set_error(rc, err);
  scanner->last_rank = hg_rank_result_t{o.n_values, o.n_distinct, o.n_parts, o.n_bytes, o.d_bytes, o.d_off, o.d_count, o.d_first, o.d_pattern, o.d_line_number, o.d_segment,
                                        o.d_first_value, o.d_seg_distinct, o.d_seg_parts, o.n_seg, o.table_log2, static_cast<uint32_t>(o.ms_rank * 1000.0f + 0.5f), 0};
  *result = scanner->last_rank;
  return HG_OK;
}

int hg_copy_ranked_values(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number,
                          uint32_t *segment, uint64_t max_values) {
  if (!scanner) return HG_ERR_ARG;
  const hg_rank_result_t &g = scanner->last_rank;
  if (!g.d_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_ranked_values: no ranking since the last scan");
  if (segment && !g.d_segment) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_ranked_values: the last scan had no segments");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t nb = std::min(g.n_bytes, max_bytes), nv = std::min(g.n_values, max_values);
  if (bytes && nb && hipMemcpy(bytes, g.d_bytes, nb, hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (off && hipMemcpy(off, g.d_off, (nv + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (count && nv && hipMemcpy(count, g.d_count, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (first && nv && hipMemcpy(first, g.d_first, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (pattern && nv && hipMemcpy(pattern, g.d_pattern, nv * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (line_number && nv && hipMemcpy(line_number, g.d_line_number, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (segment && nv && hipMemcpy(segment, g.d_segment, nv * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_ranked_segments(hg_scanner_t *scanner, uint64_t *first_value, uint64_t *seg_distinct, uint64_t *seg_parts) {
  if (!scanner) return HG_ERR_ARG;
  const hg_rank_result_t &g = scanner->last_rank;
  if (!g.d_first_value) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_ranked_segments: no ranking with HG_RANK_PER_SEGMENT since the last scan");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t ns = g.n_seg;
  if (first_value && hipMemcpy(first_value, g.d_first_value, (ns + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (seg_distinct && ns && hipMemcpy(seg_distinct, g.d_seg_distinct, ns * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (seg_parts && ns && hipMemcpy(seg_parts, g.d_seg_parts, ns * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_ranked_values_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  const hg_rank_result_t &g = scanner->last_rank;
  if (!g.d_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_ranked_values_device: no ranking since the last scan");
  const uint64_t nb = std::min(g.n_bytes, max_bytes);
  if (!nb) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  return hipMemcpyAsync(d_dst, g.d_bytes, nb, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_accumulate_values(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, const hg_acc_params_t *params, void *stream, hg_acc_result_t *result) {
  if (!scanner) return HG_ERR_ARG;
  if (result) *result = hg_acc_result_t{};
  const hg_acc_params_t p = params ? *params : hg_acc_params_t{0, 0, 0, 0};
  const bool seg = scanner->last_seg.d_first_record != nullptr, reset = (p.flags & HG_ACC_RESET) != 0;
  const uint64_t n_parts = scanner->last_with_parts ? scanner->last_parts.n_parts : 0;
  const uint32_t hash_bits = p.hash_bits ? p.hash_bits : 64;
  const char *why = !result                                                            ? "hg_accumulate_values: result is NULL"
                    : !scanner->scanned                                                ? "hg_accumulate_values: no successful scan to accumulate the values of"
                    : (d_text != scanner->last_text || nbytes != scanner->last_nbytes) ? "hg_accumulate_values: d_text and nbytes are not those of the last scan"
                    : !scanner->last_with_parts                                        ? "hg_accumulate_values: the last scan was not one with parts (hg_scan_device_parts, hg_scan_device_segments_parts)"
                    : (p.flags & ~(HG_ACC_BY_PATTERN | HG_ACC_RESET))                  ? "hg_accumulate_values: unknown flag bits"
                    : p.hash_bits > 64                                                 ? "hg_accumulate_values: hash_bits above 64"
                    : p.table_log2 > HG_VALUES_MAX_TABLE_LOG2                          ? "hg_accumulate_values: table_log2 above 40"
                    : (p.table_log2 && (uint64_t{1} << p.table_log2) <= n_parts)       ? "hg_accumulate_values: 2^table_log2 must exceed the number of parts"
                    : (!p.table_log2 && hg_values_default_log2(n_parts) > HG_VALUES_MAX_TABLE_LOG2) ? "hg_accumulate_values: more parts than a table of 2^40 slots serves"
                    : p.store_log2 > HG_VALUES_MAX_TABLE_LOG2                          ? "hg_accumulate_values: store_log2 above 40"
                                                                                       : nullptr;
  if (why) return scanner->sc->set_error(HG_ERR_ARG, why);
  if (scanner->store) {
    if (const char *differs = scanner->store->mismatch(p.flags & HG_ACC_BY_PATTERN, hash_bits, reset)) return scanner->sc->set_error(HG_ERR_ARG, std::string("hg_accumulate_values: ") + differs);
  } else {
    scanner->store = new HgValueStore(scanner->sc->device());
  }
  HgValStoreInput in{};
  in.values.text = static_cast<const uint8_t *>(d_text);
  in.values.recs = HgGatherList{reinterpret_cast<const HgHit *>(scanner->last.d_hits), reinterpret_cast<const HgHitAux *>(scanner->last.d_aux),
                                seg ? scanner->last_seg.d_record_segment : nullptr, scanner->last.n_hits};
  in.values.parts = reinterpret_cast<const HgPart *>(scanner->last_parts.d_parts);
  in.values.part_pattern = scanner->last_parts.d_part_pattern;
  in.values.n_parts = n_parts;
  if (seg) {
    in.values.part_seg = scanner->last_segparts.d_part_segment;
    in.values.seg_start = scanner->last_seg_start;
  }
  in.values.flags = p.flags & HG_ACC_BY_PATTERN;
  in.values.hash_bits = hash_bits;
  in.values.table_log2 = p.table_log2 ? p.table_log2 : hg_values_default_log2(n_parts);
  in.store_log2 = p.store_log2;
  in.reset = reset;
  HgValStoreOutput o{};
  std::string err;
  const int rc = scanner->store->accumulate(in, static_cast<hipStream_t>(stream), &o, &err);
  if (rc != HG_OK) {  // (the store is as it was, and so is its last ranking; after a HIP error it may be empty)
    if (!scanner->store->began()) scanner->last_acc_rank = hg_acc_rank_result_t{};
    return scanner->sc->set_error(rc, err);
  }
  scanner->last_acc_rank = hg_acc_rank_result_t{};
  *result = hg_acc_result_t{o.n_distinct, o.n_added, o.n_groups, o.n_parts, o.n_parts_total, o.n_bytes, o.store_log2, static_cast<uint32_t>(o.ms_acc * 1000.0f + 0.5f)};
  return HG_OK;
}

int hg_rank_accumulated(hg_scanner_t *scanner, uint64_t top, uint32_t flags, void *stream, hg_acc_rank_result_t *result) {
  if (!scanner) return HG_ERR_ARG;
  if (result) *result = hg_acc_rank_result_t{};
  const char *why = !result                                        ? "hg_rank_accumulated: result is NULL"
                    : (flags & ~HG_ACC_ORDER_FIRST)                ? "hg_rank_accumulated: unknown flag bits"
                    : (!scanner->store || !scanner->store->began()) ? "hg_rank_accumulated: no accumulation since the last reset"
                                                                   : nullptr;
  if (why) return scanner->sc->set_error(HG_ERR_ARG, why);
  scanner->last_acc_rank = hg_acc_rank_result_t{};
  HgValRankOutput o{};
  std::string err;
  const int rc = scanner->store->rank(top, (flags & HG_ACC_ORDER_FIRST) != 0, static_cast<hipStream_t>(stream), &o, &err);
  if (rc != HG_OK) return scanner->sc->set_error(rc, err);
  scanner->last_acc_rank = hg_acc_rank_result_t{o.n_values, o.n_distinct, o.n_parts, o.n_bytes, o.d_bytes, o.d_off, o.d_count, o.d_first, o.d_pattern, o.d_line_number,
                                                o.store_log2, static_cast<uint32_t>(o.ms_rank * 1000.0f + 0.5f)};
  *result = scanner->last_acc_rank;
  return HG_OK;
}

int hg_copy_accumulated(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *off, uint64_t *count, uint64_t *first, uint32_t *pattern, uint64_t *line_number,
                        uint64_t max_values) {
  if (!scanner) return HG_ERR_ARG;
  if (!scanner->store || !scanner->store->began()) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_accumulated: no accumulation since the last reset");
  const hg_acc_rank_result_t &g = scanner->last_acc_rank;
  if (!g.d_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_accumulated: no ranking since the last accumulation");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t nb = std::min(g.n_bytes, max_bytes), nv = std::min(g.n_values, max_values);
  if (bytes && nb && hipMemcpy(bytes, g.d_bytes, nb, hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (off && hipMemcpy(off, g.d_off, (nv + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (count && nv && hipMemcpy(count, g.d_count, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (first && nv && hipMemcpy(first, g.d_first, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (pattern && nv && hipMemcpy(pattern, g.d_pattern, nv * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (line_number && nv && hipMemcpy(line_number, g.d_line_number, nv * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_accumulated_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  if (!scanner->store || !scanner->store->began()) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_accumulated_device: no accumulation since the last reset");
  const hg_acc_rank_result_t &g = scanner->last_acc_rank;
  if (!g.d_off) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_accumulated_device: no ranking since the last accumulation");
  const uint64_t nb = std::min(g.n_bytes, max_bytes);
  if (!nb) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  return hipMemcpyAsync(d_dst, g.d_bytes, nb, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_reset_accumulated(hg_scanner_t *scanner) {
  if (!scanner) return HG_ERR_ARG;
  if (scanner->store) scanner->store->reset();
  scanner->last_acc_rank = hg_acc_rank_result_t{};
  return HG_OK;
}

int hg_db_report_ids(const hg_database_t *db, uint32_t *ids, uint32_t max, uint32_t *n_bins) {
  if (!db || !n_bins) return HG_ERR_ARG;
  const std::vector<uint32_t> &r = db->db->report_ids;
  *n_bins = static_cast<uint32_t>(r.size());
  if (ids) std::copy(r.begin(), r.begin() + std::min<size_t>(r.size(), max), ids);
  return HG_OK;
}

int hg_count_records(hg_scanner_t *scanner, uint32_t flags, void *stream, hg_counts_result_t *result) {
  if (!scanner) return HG_ERR_ARG;
  if (result) *result = hg_counts_result_t{};
  const bool seg = scanner->last_seg.d_first_record != nullptr, per_seg = (flags & HG_COUNTS_PER_SEGMENT) != 0;
  const uint64_t n_bins = scanner->sc->database()->report_ids.size();
  const char *why = !result                                                        ? "hg_count_records: result is NULL"
                    : !scanner->scanned                                            ? "hg_count_records: no successful scan to count the records of"
                    : scanner->last_invert                                         ? "hg_count_records: the last scan was inverted (its records carry no expression)"
                    : (flags & ~(HG_COUNTS_ACCUMULATE | HG_COUNTS_PER_SEGMENT))    ? "hg_count_records: unknown flag bits"
                    : (per_seg && !seg)                                            ? "hg_count_records: HG_COUNTS_PER_SEGMENT after a scan without segments"
                    : (per_seg && scanner->last_n_seg * n_bins > HG_COUNTS_MAX_CELLS) ? "hg_count_records: more than 2^28 cells (n_seg * n_bins)"
                                                                                   : nullptr;
  if (why) return scanner->sc->set_error(HG_ERR_ARG, why);
  if (!scanner->counts) scanner->counts = new HgCounts(scanner->sc->device(), *scanner->sc->database());
  HgCountsInput in{};
  in.list = HgCountsList{reinterpret_cast<const HgHit *>(scanner->last.d_hits), seg ? scanner->last_seg.d_record_segment : nullptr, scanner->last.n_hits};
  in.n_seg = per_seg ? scanner->last_n_seg : 0;
  in.flags = flags;
  HgCountsOutput o{};
  std::string err;
  const int rc = scanner->counts->run(in, static_cast<hipStream_t>(stream), &o, &err);
  if (rc != HG_OK) return scanner->sc->set_error(rc, err);
  scanner->last_counts = hg_counts_result_t{o.n_bins, o.n_seg, o.n_records, o.d_ids, o.d_n_lines, o.d_n_reports, o.d_seg_lines, o.d_seg_reports,
                                            static_cast<uint32_t>(o.ms_counts * 1000.0f + 0.5f), 0};
  *result = scanner->last_counts;
  return HG_OK;
}

int hg_copy_counts(hg_scanner_t *scanner, uint32_t *ids, uint64_t *n_lines, uint64_t *n_reports, uint32_t max_bins) {
  if (!scanner) return HG_ERR_ARG;
  const hg_counts_result_t &c = scanner->last_counts;
  if (!c.d_ids) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_counts: no count on this scanner");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint32_t n = std::min(c.n_bins, max_bins);
  if (ids && n && hipMemcpy(ids, c.d_ids, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (n_lines && n && hipMemcpy(n_lines, c.d_n_lines, n * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (n_reports && n && hipMemcpy(n_reports, c.d_n_reports, n * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_segment_counts(hg_scanner_t *scanner, uint32_t *seg_lines, uint32_t *seg_reports, uint32_t first_seg, uint32_t n) {
  if (!scanner) return HG_ERR_ARG;
  const hg_counts_result_t &c = scanner->last_counts;
  if (!c.d_seg_lines) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_segment_counts: no count with HG_COUNTS_PER_SEGMENT since the last scan");
  if (first_seg > c.n_seg || n > c.n_seg - first_seg) return scanner->sc->set_error(HG_ERR_ARG, "hg_copy_segment_counts: rows out of range");
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t off = static_cast<uint64_t>(first_seg) * c.n_bins, cells = static_cast<uint64_t>(n) * c.n_bins;
  if (seg_lines && cells && hipMemcpy(seg_lines, c.d_seg_lines + off, cells * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (seg_reports && cells && hipMemcpy(seg_reports, c.d_seg_reports + off, cells * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_segment_parts(hg_scanner_t *scanner, uint32_t *part_segment, uint64_t *first_part) {
  if (!scanner) return HG_ERR_ARG;
  const HgSegPartsOutput &x = scanner->last_segparts;
  if (!x.d_first_part) return HG_ERR_ARG;  // the last scan was not hg_scan_device_segments_parts
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t n = scanner->last_parts.n_parts, n_seg = scanner->last_n_seg;
  if (part_segment && n && hipMemcpy(part_segment, x.d_part_segment, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (first_part && hipMemcpy(first_part, x.d_first_part, (n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_parts(hg_scanner_t *scanner, hg_part_t *parts, uint32_t *pattern, uint64_t max) {
  if (!scanner || !parts) return HG_ERR_ARG;
  uint64_t n = scanner->last_parts.n_parts < max ? scanner->last_parts.n_parts : max;
  if (!n) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  if (hipMemcpy(parts, scanner->last_parts.d_parts, n * sizeof(hg_part_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (pattern && hipMemcpy(pattern, scanner->last_parts.d_part_pattern, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_parts_device(hg_scanner_t *scanner, void *d_dst, uint64_t max, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  uint64_t n = scanner->last_parts.n_parts < max ? scanner->last_parts.n_parts : max;
  if (!n) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  if (hipMemcpyAsync(d_dst, scanner->last_parts.d_parts, n * sizeof(hg_part_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) != hipSuccess)
    return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_segments(hg_scanner_t *scanner, uint32_t *record_segment, uint64_t *first_record, uint64_t *n_lines, uint64_t *n_selected) {
  if (!scanner) return HG_ERR_ARG;
  const hg_segment_result_t &g = scanner->last_seg;
  if (!g.d_first_record) return HG_ERR_ARG;  // the last scan had no segments
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t n = scanner->last.n_hits, n_seg = scanner->last_n_seg;
  if (record_segment && n && hipMemcpy(record_segment, g.d_record_segment, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (first_record && hipMemcpy(first_record, g.d_first_record, (n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (n_lines && n_seg && hipMemcpy(n_lines, g.d_n_lines, n_seg * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (n_selected && n_seg && hipMemcpy(n_selected, g.d_n_selected, n_seg * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_segment_context(hg_scanner_t *scanner, uint32_t *context_segment, uint64_t *first_context) {
  if (!scanner) return HG_ERR_ARG;
  const HgSegCtxOutput &x = scanner->last_segctx;
  if (!x.d_first_context) return HG_ERR_ARG;  // the last scan was not hg_scan_device_segments_context
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const uint64_t n = scanner->last_ctx.n_context, n_seg = scanner->last_n_seg;
  if (context_segment && n && hipMemcpy(context_segment, x.d_context_segment, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (first_context && hipMemcpy(first_context, x.d_first_context, (n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_context(hg_scanner_t *scanner, hg_hit_t *hits, hg_hit_aux_t *aux, uint64_t max) {
  if (!scanner || !hits) return HG_ERR_ARG;
  uint64_t n = scanner->last_ctx.n_context < max ? scanner->last_ctx.n_context : max;
  if (!n) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  if (hipMemcpy(hits, scanner->last_ctx.d_ctx_hits, n * sizeof(hg_hit_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (aux && hipMemcpy(aux, scanner->last_ctx.d_ctx_aux, n * sizeof(hg_hit_aux_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_context_device(hg_scanner_t *scanner, void *d_dst, uint64_t max, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  uint64_t n = scanner->last_ctx.n_context < max ? scanner->last_ctx.n_context : max;
  if (!n) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  if (hipMemcpyAsync(d_dst, scanner->last_ctx.d_ctx_hits, n * sizeof(hg_hit_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) != hipSuccess)
    return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_hits(hg_scanner_t *scanner, hg_hit_t *hits, hg_hit_aux_t *aux, uint64_t max) {
  if (!scanner || !hits) return HG_ERR_ARG;
  uint64_t n = scanner->last.n_hits < max ? scanner->last.n_hits : max;
  if (!n) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  if (hipMemcpy(hits, scanner->last.d_hits, n * sizeof(hg_hit_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  if (aux && hipMemcpy(aux, scanner->last.d_aux, n * sizeof(hg_hit_aux_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_hits_device(hg_scanner_t *scanner, void *d_dst, uint64_t max, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  uint64_t n = scanner->last.n_hits < max ? scanner->last.n_hits : max;
  if (!n) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  if (hipMemcpyAsync(d_dst, scanner->last.d_hits, n * sizeof(hg_hit_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) != hipSuccess)
    return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_hit_starts(hg_scanner_t *scanner, uint32_t *from, uint64_t max) {
  if (!scanner || !from) return HG_ERR_ARG;
  uint64_t n = scanner->last.n_hits < max ? scanner->last.n_hits : max;
  if (!n) return HG_OK;
  if (!scanner->d_from) {  // no SOM expression in the database
    std::memset(from, 0, n * sizeof(uint32_t));
    return HG_OK;
  }
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  if (hipMemcpy(from, scanner->d_from, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HG_ERR_HIP;
  return HG_OK;
}

int hg_copy_hit_starts_device(hg_scanner_t *scanner, void *d_dst, uint64_t max, void *stream) {
  if (!scanner || !d_dst) return HG_ERR_ARG;
  uint64_t n = scanner->last.n_hits < max ? scanner->last.n_hits : max;
  if (!n) return HG_OK;
  if (hipSetDevice(scanner->sc->device()) != hipSuccess) return HG_ERR_HIP;
  const hipError_t e = scanner->d_from ? hipMemcpyAsync(d_dst, scanner->d_from, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream))
                                       : hipMemsetAsync(d_dst, 0, n * sizeof(uint32_t), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? HG_OK : HG_ERR_HIP;
}

}  // extern "C"

// ---------------------------------------------------------------- guarded buffers (diagnostics / tests)
// A device buffer whose END is followed by reserved but UNMAPPED address space: any read or write past the buffer's size
// rounded up to 16 bytes is a GPU memory fault, wherever ordinary allocations would let it pass silently because the next
// bytes happen to be mapped.  (Round 1's one GPU fault was such a read: it took ~50 live contexts before a text buffer
// ended at the edge of a mapping.)  Built on the HIP virtual-memory API: reserve mapped + guard, map only the first part.
struct hg_guarded {
  void *base;
  size_t mapped, reserved;
  hipMemGenericAllocationHandle_t handle;
};
extern "C" {

int hg_debug_alloc_guarded(uint64_t nbytes, int device, void **d_ptr, void **guard_handle) {
  if (!d_ptr || !guard_handle) return HG_ERR_ARG;
  *d_ptr = *guard_handle = nullptr;
  if (hipSetDevice(device) != hipSuccess) return HG_ERR_HIP;
  hipMemAllocationProp prop{};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || !gran) return HG_ERR_HIP;
  const size_t usable = (static_cast<size_t>(nbytes) + 15) & ~static_cast<size_t>(15);
  auto g = std::make_unique<hg_guarded>();
  g->mapped = std::max<size_t>((usable + gran - 1) / gran * gran, gran);
  g->reserved = g->mapped + gran;
  if (hipMemAddressReserve(&g->base, g->reserved, gran, nullptr, 0) != hipSuccess) return HG_ERR_HIP;
  if (hipMemCreate(&g->handle, g->mapped, &prop, 0) != hipSuccess) {
    (void)hipMemAddressFree(g->base, g->reserved);
    return HG_ERR_HIP;
  }
  hipMemAccessDesc access{};
  access.location = prop.location;
  access.flags = hipMemAccessFlagsProtReadWrite;
  if (hipMemMap(g->base, g->mapped, 0, g->handle, 0) != hipSuccess || hipMemSetAccess(g->base, g->mapped, &access, 1) != hipSuccess) {
    (void)hipMemRelease(g->handle);
    (void)hipMemAddressFree(g->base, g->reserved);
    return HG_ERR_HIP;
  }
  *d_ptr = static_cast<char *>(g->base) + (g->mapped - usable);  // 16-byte aligned; [d_ptr, d_ptr + usable) ends at the guard
  *guard_handle = g.release();
  return HG_OK;
}

void hg_debug_free_guarded(void *guard_handle) {
  hg_guarded *g = static_cast<hg_guarded *>(guard_handle);
  if (!g) return;
  (void)hipDeviceSynchronize();
  (void)hipMemUnmap(g->base, g->mapped);
  (void)hipMemRelease(g->handle);
  (void)hipMemAddressFree(g->base, g->reserved);
  delete g;
}

int hg_debug_finalize_info(hg_scanner_t *scanner, hg_finalize_info_t *info, uint32_t *fill, uint32_t max_fill) {
  if (!scanner || !info) return HG_ERR_ARG;
  const HgScanner::FinInfo &f = scanner->sc->finalize_info();
  *info = hg_finalize_info_t{f.path, f.fin_shift, f.fin_nb, f.fin_cap, f.id_bits, f.to_bits, f.early_buckets, f.early_beside_stream, f.scan_blocks, scanner->sc->left_bucketed() ? 1u : 0u, 0u, 0u};
  return fill ? scanner->sc->copy_fin_fill(fill, max_fill, &info->n_fill) : HG_OK;
}

int hg_debug_upload(void *d_dst, const void *src, uint64_t nbytes) {
  if (!nbytes) return HG_OK;
  if (!d_dst || !src) return HG_ERR_ARG;
  return hipMemcpy(d_dst, src, nbytes, hipMemcpyHostToDevice) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_debug_download(void *dst, const void *d_src, uint64_t nbytes) {
  if (!nbytes) return HG_OK;
  if (!dst || !d_src) return HG_ERR_ARG;
  return hipMemcpy(dst, d_src, nbytes, hipMemcpyDeviceToHost) == hipSuccess ? HG_OK : HG_ERR_HIP;
}

}  // extern "C"

// ---------------------------------------------------------------- synthetic log
__global__ void hg_synth_kernel(uint8_t *text, uint64_t nbytes, HgSynthSpec sp) {
  uint64_t nblocks = (nbytes + HG_SYNTH_BLOCK - 1) / HG_SYNTH_BLOCK;
  for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; b < nblocks;
       b += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
    uint64_t off = b * HG_SYNTH_BLOCK;
    uint32_t len = static_cast<uint32_t>(nbytes - off < HG_SYNTH_BLOCK ? nbytes - off : HG_SYNTH_BLOCK);
    hg_synth_block(sp, sp.first_block + b, text + off, len);
  }
}

extern "C" {

int hg_synth_device(void *d_text, uint64_t nbytes, const hg_synth_spec_t *spec, int device, void *stream) {
  if (!d_text || !spec) return HG_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return HG_ERR_HIP;
  uint32_t total = spec->n_needles ? spec->needle_off[spec->n_needles] : 0;
  uint8_t *d_needles = nullptr;
  uint32_t *d_off = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&d_needles), total + 16) != hipSuccess) return HG_ERR_HIP;
  if (hipMalloc(reinterpret_cast<void **>(&d_off), (spec->n_needles + 1) * 4 + 16) != hipSuccess) return HG_ERR_HIP;
  if (total) (void)hipMemcpy(d_needles, spec->needles, total, hipMemcpyHostToDevice);
  if (spec->n_needles) (void)hipMemcpy(d_off, spec->needle_off, (spec->n_needles + 1) * 4, hipMemcpyHostToDevice);
  HgSynthSpec sp{spec->seed, spec->first_block, spec->hit_per_million, spec->n_needles, d_needles, d_off};
  uint64_t nblocks = (nbytes + HG_SYNTH_BLOCK - 1) / HG_SYNTH_BLOCK;
  uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((nblocks + 63) / 64, 65536));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (nblocks) hipLaunchKernelGGL(hg_synth_kernel, dim3(grid), dim3(64), 0, st, static_cast<uint8_t *>(d_text), nbytes, sp);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d_needles);
  (void)hipFree(d_off);
  return e == hipSuccess ? HG_OK : HG_ERR_HIP;
}

int hg_synth_host(uint8_t *text, uint64_t nbytes, const hg_synth_spec_t *spec) {
  if (!text || !spec) return HG_ERR_ARG;
  HgSynthSpec sp{spec->seed, spec->first_block, spec->hit_per_million, spec->n_needles, spec->needles, spec->needle_off};
  uint64_t nblocks = (nbytes + HG_SYNTH_BLOCK - 1) / HG_SYNTH_BLOCK;
  for (uint64_t b = 0; b < nblocks; b++) {
    uint64_t off = b * HG_SYNTH_BLOCK;
    uint32_t len = static_cast<uint32_t>(nbytes - off < HG_SYNTH_BLOCK ? nbytes - off : HG_SYNTH_BLOCK);
    hg_synth_block(sp, sp.first_block + b, text + off, len);
  }
  return HG_OK;
}

}  // extern "C"
