// Host side of the device scanner: uploads the compiled database, owns the workspace in HBM and issues
// the launch sequence (stream pass -> tile scan -> confirm / always-on -> order + de-duplicate).
// There is no CPU scan path here: any HIP failure is reported as HG_ERR_HIP.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "hg_engine.h"
#include "hg_mem.h"

#include <rocprim/rocprim.hpp>

// kernels (hg_kernels.hip)
bool hg_launch_stream(const HgStreamArgs &a, uint32_t grid, hipStream_t stream);
bool hg_launch_stream_join(const HgStreamArgs &a, uint32_t grid, hipStream_t stream);
int hg_stream_blocks_per_cu(uint32_t filter_log2, uint32_t filter_wide, uint32_t dense);
__global__ void hg_tile_reduce_kernel(const HgTileSum *sums, uint64_t tile_begin, uint64_t tile_end, uint64_t bs1, HgTileElem *agg);
__global__ void hg_tile_spine_kernel(const HgTileElem *agg, uint32_t nblocks, uint64_t bs1, HgTileBase *block_base, HgTileBase *state);
__global__ void hg_tile_apply_kernel(const HgTileSum *sums, uint64_t tile_begin, uint64_t tile_end, uint64_t bs1, const HgTileBase *block_base,
                                     HgTileBase *bases);
__global__ void hg_tile_inner_kernel(const uint8_t *text, HgTileSum *sums, uint64_t tile_begin, uint64_t tile_end, uint64_t bs1);
__global__ void hg_verify_kernel(HgConfirmArgs a);
__global__ void hg_confirm_fast_kernel(HgConfirmArgs a, uint32_t blocks_per_mode);
__global__ void hg_confirm_generic_kernel(HgConfirmArgs a);
__global__ void hg_always_on_kernel(HgConfirmArgs a, uint32_t first, uint32_t last);
__global__ void hg_always_on_fast_kernel(HgConfirmArgs a);
__global__ void hg_always_on_finish_kernel(HgConfirmArgs a);
__global__ void hg_block_mark_kernel(HgConfirmArgs a, uint32_t *pattern_flags);
__global__ void hg_block_scan_kernel(HgConfirmArgs a, const uint32_t *pattern_flags);
__global__ void hg_block_small_kernel(HgDbView db, const uint8_t *h_text, uint32_t length, HgHit *h_out, uint32_t seg_cap, uint32_t *h_counts, uint32_t *d_done,
                                      uint32_t *h_flag, uint32_t seq, uint32_t ppw);
__global__ void hg_reset_kernel(uint32_t *state, uint32_t state_words, HgTileBase *final_state, uint64_t carry_start, uint64_t first_piece, uint32_t *fill, uint32_t nb, uint32_t *defer_count,
                                uint32_t ndefer);
__global__ void hg_fin_sort_small_kernel(const HgHit *hits, uint32_t *idx, const uint32_t *fill, uint32_t b_lo, uint32_t b_hi, uint32_t cap, uint32_t id_bits,
                                         uint32_t to_bits, uint32_t *kept_count, uint32_t *big_list, uint32_t *big_count, uint32_t big_stride);
template <uint32_t LCAP, bool IN_LDS>
__global__ void hg_fin_sort_big_kernel(const HgHit *hits, uint32_t *idx, const uint32_t *fill, const uint32_t *big_list, const uint32_t *big_count, uint32_t cap,
                                       uint32_t id_bits, uint32_t to_bits, uint32_t *kept_count, uint32_t *overflow, uint64_t *scratch_key, uint32_t *scratch_idx);
template <uint32_t THREADS>
__global__ void hg_fin_scan_kernel(uint32_t *kept_count, uint32_t b_lo, uint32_t b_hi, uint32_t *total, const uint32_t *fill, uint32_t cap, uint32_t *part, uint32_t epoch);
__global__ void hg_confirm_literal_kernel(HgConfirmArgs a);
__global__ void hg_verify_lean_kernel(HgConfirmArgs a);
__global__ void hg_fin_gather_kernel(const HgHit *hits, const HgHitAux *aux, const uint32_t *idx, const uint32_t *kept_base, const uint32_t *total, uint32_t b_lo,
                                     uint32_t b_hi, uint32_t cap, HgHit *oh, HgHitAux *oa);
__global__ void hg_key_kernel(const HgHit *hits, const HgHitAux *aux, const HgPattern *patterns, uint32_t n, uint64_t *key, uint32_t *idx);
__global__ void hg_line_key_kernel(const HgHit *hits, const uint32_t *perm, uint32_t n, uint64_t *key);
__global__ void hg_offset_kernel(uint32_t *idx, uint32_t n, uint32_t add);
__global__ void hg_key_packed_kernel(const HgHit *hits, const HgHitAux *aux, const HgPattern *patterns, uint32_t n, uint32_t id_bits, uint32_t to_bits,
                                     uint64_t *key, uint32_t *idx);
__global__ void hg_keep_kernel(const HgHit *hits, const HgHitAux *aux, const uint32_t *perm, const HgPattern *patterns, uint32_t n, uint8_t *keep);
__global__ void hg_scatter_kernel(const HgHit *hits, const HgHitAux *aux, const uint32_t *perm, const uint8_t *keep, const uint32_t *pos, uint32_t n,
                                  HgHit *oh, HgHitAux *oa, uint32_t *count);

// huge automata (hg_huge.hip)
size_t hg_huge_lds_bytes(uint32_t nw_max, uint32_t stage_cap);
bool hg_launch_confirm_huge(const HgConfirmArgs &a, uint32_t grid, uint32_t nw_max, uint32_t stage_cap, void *claim, uint32_t claim_mask, hipStream_t stream);
bool hg_launch_always_on_huge(const HgConfirmArgs &a, uint32_t grid, uint32_t nw_max, uint32_t stage_cap, uint32_t first, uint32_t last, hipStream_t stream);
bool hg_launch_block_huge(const HgConfirmArgs &a, uint32_t grid, uint32_t nw_max, uint32_t stage_cap, const uint32_t *pattern_flags, hipStream_t stream);

namespace {
constexpr int TS_BLOCK_TILES = 1024;  // must match hg_kernels.hip (256 threads x 4 tiles)
constexpr int STREAM_WG_WAVES = HG_STREAM_WG_WAVES;

template <typename T>
hipError_t upload(void **dst, const std::vector<T> &src, const char *name) {
  size_t bytes = std::max<size_t>(src.size() * sizeof(T), 16);
  hipError_t e = hgmem::dev_alloc(dst, bytes, name);
  if (e != hipSuccess) return e;
  if (!src.empty()) e = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}
// frees ptr and allocates `count` elements (16 bytes at least) in its place
template <typename T>
hipError_t realloc_dev(T *&ptr, size_t count, const char *name) {
  hgmem::dev_free(ptr, name);
  ptr = nullptr;
  return hgmem::dev_alloc(&ptr, std::max<size_t>(count * sizeof(T), 16), name);
}
uint32_t bits_for(uint64_t v) {
  uint32_t b = 1;
  while (b < 64 && (v >> b)) b++;
  return b;
}
// compact finalize: line, id, `to` and the single bit in ONE 64-bit key (else two sorts)
bool compact_key_packed(uint64_t line_bound, uint32_t id_bits, uint32_t to_bits) { return bits_for(line_bound) + id_bits + to_bits + 1 <= 64; }
}  // namespace

// (members of HgScanner) a failed HIP call: its message in err_, HG_ERR_HIP to the caller
#define HG_TRY(call, what) \
  do { if (fail((call), what)) return HG_ERR_HIP; } while (0)

HgEngineKnobs HgEngineKnobs::from_env() {
  HgEngineKnobs k;
  auto num = [](const char *name, uint64_t dflt) -> uint64_t {
    const char *env = std::getenv(name);
    return env ? std::strtoull(env, nullptr, 10) : dflt;
  };
  k.fin_target = std::max<uint64_t>(4, num("HG_FIN_TARGET", 48));
  k.no_bucket_finalize = std::getenv("HG_NO_BUCKET_FINALIZE") != nullptr;
  k.chunk_tiles = num("HG_CHUNK_TILES", 0);
  k.max_chunks = static_cast<uint32_t>(std::min<uint64_t>(num("HG_MAX_CHUNKS", 0), 1u << 20));
  if (const char *env = std::getenv("HG_CHUNK_WEIGHTS")) {  // e.g. "10,10,8,4"
    for (const char *q = env; *q;) {
      char *e = nullptr;
      const double v = std::strtod(q, &e);
      if (e == q) break;
      if (v > 0) k.chunk_weights.push_back(v);
      q = *e ? e + 1 : e;
    }
  }
  k.stream_wgs_per_cu = static_cast<long>(num("HG_STREAM_WGS_PER_CU", 0));
  if (const char *env = std::getenv("HG_JOINER")) k.joiner = std::max(0l, std::min(2l, std::strtol(env, nullptr, 10)));
  k.joiner_ahead = std::getenv("HG_JOINER_AHEAD") != nullptr;
  k.no_early_finalize = std::getenv("HG_NO_EARLY_FINALIZE") != nullptr;
#ifdef HG_PROFILE_CONFIRM
  if (const char *env = std::getenv("HG_DEBUG_CONFIRM_MODES")) k.confirm_mode_mask = static_cast<uint32_t>(std::strtoul(env, nullptr, 0));
#endif
  k.confirm_blocks_per_cu = static_cast<long>(std::min<uint64_t>(num("HG_CONFIRM_BLOCKS_PER_CU", 0), 16));
  k.hit_limit = num("HG_HIT_LIMIT", 0);
  k.cand_limit = num("HG_CAND_LIMIT", 0);
  k.verbose = std::getenv("HG_VERBOSE") != nullptr;
  return k;
}

bool HgScanner::fail(hipError_t e, const char *what) {
  if (e == hipSuccess) return false;
  err_ = std::string(what) + ": " + hipGetErrorString(e);
  return true;
}

int HgScanner::create(std::shared_ptr<const HgDb> db, int device, HgScanner **out, std::string *err) {
  *out = nullptr;
  std::unique_ptr<HgScanner> s(new HgScanner());
  s->device_ = device;
  s->db_ = std::move(db);
  if (int rc = s->init()) {
    if (err) *err = s->err_;
    return rc;
  }
  *out = s.release();
  return HG_OK;
}

// Uploads the database and allocates what every scan needs.
int HgScanner::init() {
  if (!db_) return error(HG_ERR_ARG, "no database");
  int count = 0;
  const hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) return error(HG_ERR_HIP, std::string("no HIP device available (") + hipGetErrorString(e) + "); the scan path has no CPU fallback");
  if (device_ < 0 || device_ >= count) return error(HG_ERR_ARG, "device index out of range");
  knobs_ = HgEngineKnobs::from_env();
  const HgDb &db = *db_;
  HG_TRY(hipSetDevice(device_), "hipSetDevice");
  hipDeviceProp_t prop;
  HG_TRY(hipGetDeviceProperties(&prop, device_), "hipGetDeviceProperties");
  num_cus_ = prop.multiProcessorCount;
  HG_TRY(upload(&d_patterns_, db.patterns, "d_patterns_"), "upload patterns");
  HG_TRY(upload(&d_pool_, db.pool, "d_pool_"), "upload tables");
  HG_TRY(upload(&d_factors_, db.factors, "d_factors_"), "upload factors");
  HG_TRY(upload(&d_windows_, db.windows, "d_windows_"), "upload windows");
  HG_TRY(upload(&d_bucket_, db.bucket_off, "d_bucket_"), "upload buckets");
  HG_TRY(upload(&d_disc_, db.disc, "d_disc_"), "upload discriminators");
  HG_TRY(upload(&d_bucket2_, db.bucket_off2, "d_bucket2_"), "upload buckets");
  HG_TRY(upload(&d_windows2_, db.windows2, "d_windows2_"), "upload windows");
  HG_TRY(upload(&d_wtab_, db.wtab, "d_wtab_"), "upload window table");
  if (db.filter_use_ctx) {
    // single probe: the stream kernel stages the slots with the context byte in LDS; the slot words of hash C alone follow
    // the slots' conditions in HBM (drain_batch asks them about the dwords a crowded slot judges by `rest`)
    // (drain_batch finds HgDb::filter's word of slot s at ext + (1 << filter_log2), word s: both arrays have 1 << filter_log2 entries)
    if (db.filter_wide || db.dense || db.filter_ctx.size() != (size_t(1) << db.filter_log2) || db.ext.size() != db.filter_ctx.size() || db.filter.size() != db.filter_ctx.size())
      return error(HG_ERR_ARG, "the database's single-probe filter has no context slots");
    HG_TRY(upload(&d_filter_, db.filter_ctx, "d_filter_"), "upload filter");
    std::vector<uint32_t> ext_words(db.ext.size() * (sizeof(HgSlotInfo) / 4) + db.filter.size());
    std::memcpy(ext_words.data(), db.ext.data(), db.ext.size() * sizeof(HgSlotInfo));
    std::memcpy(ext_words.data() + db.ext.size() * (sizeof(HgSlotInfo) / 4), db.filter.data(), db.filter.size() * 4);
    HG_TRY(upload(&d_ext_, ext_words, "d_ext_"), "upload filter conditions");
  } else {
    HG_TRY(upload(&d_filter_, db.filter, "d_filter_"), "upload filter");
    HG_TRY(upload(&d_ext_, db.ext, "d_ext_"), "upload filter conditions");
  }
  HG_TRY(upload(&d_slow_, db.slow, "d_slow_"), "upload always-on list");
  HG_TRY(upload(&d_groups_, db.groups, "d_groups_"), "upload always-on groups");
  view_.patterns = static_cast<const HgPattern *>(d_patterns_);
  view_.pool = static_cast<const uint32_t *>(d_pool_);
  view_.factors = static_cast<const HgFactor *>(d_factors_);
  view_.windows = static_cast<const HgWindow *>(d_windows_);
  view_.bucket_off = static_cast<const uint32_t *>(d_bucket_);
  view_.disc = static_cast<const uint16_t *>(d_disc_);
  view_.bucket_off2 = static_cast<const uint32_t *>(d_bucket2_);
  view_.windows2 = static_cast<const HgWindow *>(d_windows2_);
  view_.wtab = static_cast<const HgWinBucket *>(d_wtab_);
  view_.wtab_mask = db.wtab_mask;
  view_.wtab_first = db.wtab_first;
  view_.slow = static_cast<const uint32_t *>(d_slow_);
  view_.npatterns = static_cast<uint32_t>(db.patterns.size());
  view_.nslow = static_cast<uint32_t>(db.slow.size());
  view_.nslow_fast = db.nslow_fast;
  view_.nslow_grouped = db.nslow_grouped;
  view_.nslow_huge = db.nslow_huge;
  view_.ngroups = static_cast<uint32_t>(db.groups.size());
  view_.groups = static_cast<const HgSlowGroup *>(d_groups_);
  if (!db.bounds.empty()) HG_TRY(upload(&d_bounds_, db.bounds, "d_bounds_"), "upload offset bounds");
  view_.bounds = static_cast<const uint32_t *>(d_bounds_);  // (nullptr: the database has no offset bounds)
  if (!db.min_lengths.empty()) HG_TRY(upload(reinterpret_cast<void **>(&d_min_lengths_), db.min_lengths, "d_min_lengths_"), "upload min_length");
  for (uint32_t i = 0; i < db.patterns.size(); i++) {
    const HgPattern &p = db.patterns[i];
    if (p.flags & HG_FLAG_SOM_LEFTMOST) som_max_nw_ = std::max(som_max_nw_, p.nw);
    if (!db.min_lengths.empty() && db.min_lengths[i]) minlen_max_nw_ = std::max(minlen_max_nw_, p.nw);
  }
  if (db.comb_pass()) {
    HG_TRY(upload(reinterpret_cast<void **>(&d_combs_), db.combs, "d_combs_"), "upload combinations");
    HG_TRY(upload(reinterpret_cast<void **>(&d_comb_words_), db.comb_words, "d_comb_words_"), "upload combinations");
    HG_TRY(upload(reinterpret_cast<void **>(&d_comb_feed_), db.comb_feed, "d_comb_feed_"), "upload combinations");
  }
  view_.fold_mask = db.fold_mask;
  view_.window_mask = db.window_mask;
  static_assert(HG_CNT_CURSORS == kMaxChunks, "one tile cursor per pipeline chunk");
  HG_TRY(hgmem::dev_alloc(&d_counters_, HG_ST_ALLOC_WORDS * 4, "d_state_"), "alloc state");  // the state block (hg_engine.h, HG_ST_*)
  HG_TRY(hipMemset(d_counters_, 0, HG_ST_ALLOC_WORDS * 4), "clear state");
  d_fin_total_ = d_counters_ + HG_ST_FIN_TOTAL;
  d_selected_ = d_counters_ + HG_ST_SELECTED;
  d_final_ = reinterpret_cast<HgTileBase *>(d_counters_ + HG_ST_FINAL);
  HG_TRY(hgmem::dev_alloc(&d_pflags_, db.patterns.size() * 4 + 16, "d_pflags_"), "alloc pattern flags");
  HG_TRY(hgmem::host_alloc(&h_counters_, (HG_CNT_WORDS + 4 + HG_DEFER_SHARDS) * 4, "h_counters_"), "alloc pinned");
  h_final_ = reinterpret_cast<HgTileBase *>(h_counters_ + HG_ST_FINAL);  // (the host copy of the state block)
  for (auto &ev : ev_) HG_TRY(hipEventCreate(&ev), "hipEventCreate");
  HG_TRY(hipStreamCreateWithFlags(&side_stream_, hipStreamNonBlocking), "hipStreamCreate");
  HG_TRY(hipEventCreateWithFlags(&ev_fin_early_, hipEventDisableTiming), "hipEventCreate");
  HG_TRY(hipEventCreateWithFlags(&ev_tile_done_, hipEventDisableTiming), "hipEventCreate");
  // (the bucket arrays of the finalize — 16 MiB — are allocated by the first pass that orders hits in buckets: a scratch that only
  // ever sees short hs_scan blocks never needs them)
  // (the per-chunk events of the two-stream pipeline are created by the first scan that is large enough to use it: a
  // process that keeps dozens of scanners for small files would otherwise hold thousands of events for nothing)
  return HG_OK;
}

HgScanner::~HgScanner() {
  (void)hipSetDevice(device_);
  void *ptrs[] = {d_patterns_, d_pool_, d_factors_, d_windows_, d_bucket_, d_filter_, d_ext_, d_slow_, d_sums_, d_bases_, d_block_base_,
                  d_agg_, d_cands_, d_hits_raw_, d_hits_out_, d_aux_raw_, d_aux_out_,
                  d_key_a_, d_key_b_, d_perm_a_, d_perm_b_, d_keep_, d_counters_, d_temp_, d_seg_count_, d_pflags_, d_deferred_, d_defer_count_, d_seg_count2_, d_cands2_, d_disc_, d_bucket2_, d_windows2_, d_groups_, d_acc_hits_, d_acc_aux_, d_huge_claim_, d_wtab_, d_from_, d_fin_fill_, d_fin_kept_, d_fin_big_,
                  d_combs_, d_comb_words_, d_comb_feed_, d_comb_count_, d_comb_pos_, d_comb_hits_, d_comb_aux_, d_comb_temp_, d_bounds_,
                  d_min_lengths_, d_minlen_hits_, d_minlen_aux_, d_inv_count_, d_inv_pos_, d_inv_temp_, d_inv_hits_, d_inv_aux_,
                  d_ctx_count_, d_ctx_pos_, d_ctx_temp_, d_ctx_hits_, d_ctx_aux_,
                  d_parts_first_, d_parts_count_, d_parts_pos_, d_parts_temp_, d_parts_, d_part_pattern_,
                  d_segw_, d_seg_flag_, d_seg_temp_, d_seg_hits_, d_seg_aux_, d_seg_of_, d_seg_from_, d_pad_keep_, d_pad_pos_,
                  d_segctx_first_, d_segctx_k_, d_segctx_win_, d_segctx_of_, d_segparts_first_, d_segparts_of_};
  for (void *p : ptrs) hgmem::dev_free(p, "scanner");
  hgmem::host_free(h_counters_, "h_counters_");
  for (auto &ev : ev_)
    if (ev) (void)hipEventDestroy(ev);
  for (int i = 0; i < kMaxChunks; i++) {
    if (ev_k1_begin_[i]) (void)hipEventDestroy(ev_k1_begin_[i]);
    if (ev_k1_end_[i]) (void)hipEventDestroy(ev_k1_end_[i]);
    if (ev_side_done_[i]) (void)hipEventDestroy(ev_side_done_[i]);
  }
  if (side_stream_) (void)hipStreamDestroy(side_stream_);
  if (ev_fin_early_) (void)hipEventDestroy(ev_fin_early_);
  if (ev_tile_done_) (void)hipEventDestroy(ev_tile_done_);
}

int HgScanner::alloc_cands(uint64_t n) {
  n = std::min<uint64_t>(n, 0x7FFFFFF0u);
  HG_TRY(realloc_dev(d_cands_, n, "d_cands_"), "workspace alloc (candidates)");
  HG_TRY(realloc_dev(d_cands2_, n, "d_cands2_"), "workspace alloc (candidates)");
  // verified occurrences: one set of sharded lists per confirm mode the database uses
  uint32_t modes = 0;
  for (uint32_t m = 0; m < HG_CONFIRM_MODES; m++) modes += db_->n_confirm_mode[m] ? 1 : 0;
  HG_TRY(realloc_dev(d_deferred_, std::max<uint64_t>(modes, 1) * n, "d_deferred_"), "workspace alloc (deferred)");
  // huge tier-0 expressions: the (piece, expression) claim table of hg_confirm_huge_kernel, two slots per occurrence a pass can hold
  hgmem::dev_free(d_huge_claim_, "d_huge_claim_");
  d_huge_claim_ = nullptr;
  huge_claim_slots_ = 0;
  if (db_->n_confirm_mode[4]) {
    uint64_t slots = 1u << 12;
    while (slots < 2 * n) slots <<= 1;
    HG_TRY(hgmem::dev_alloc(&d_huge_claim_, slots * 8, "d_huge_claim_"), "workspace alloc (claim table)");
    huge_claim_slots_ = slots;
  }
  cand_cap_ = static_cast<uint32_t>(n);
  return HG_OK;
}

int HgScanner::alloc_hits(uint64_t n64) {
  const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(n64, 0x7FFFFFF0u));
  auto re = [&](auto *&ptr, size_t count, const char *name) { return fail(realloc_dev(ptr, count, name), "workspace alloc (hits)"); };
  if (re(d_hits_raw_, n, "d_hits_raw_") || re(d_hits_out_, n, "d_hits_out_") || re(d_aux_raw_, n, "d_aux_raw_") || re(d_aux_out_, n, "d_aux_out_") ||
      re(d_key_a_, n, "d_key_a_") || re(d_key_b_, n, "d_key_b_") || re(d_perm_a_, n, "d_perm_a_") || re(d_perm_b_, n, "d_perm_b_") || re(d_keep_, n, "d_keep_"))
    return HG_ERR_HIP;
  hit_cap_ = n;
  size_t t1 = 0, t2 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t1, d_key_a_, d_key_b_, d_perm_a_, d_perm_b_, n, 0, 64, hipStream_t(nullptr));
  (void)rocprim::exclusive_scan(nullptr, t2, d_keep_, d_perm_a_, 0u, n, rocprim::plus<uint32_t>(), hipStream_t(nullptr));
  size_t t3 = 0;
  (void)rocprim::merge(nullptr, t3, d_key_a_, d_key_a_, d_key_b_, d_perm_a_, d_perm_a_, d_perm_b_, n, n, rocprim::less<uint64_t>(), hipStream_t(nullptr));
  size_t need = std::max(std::max(t1, t2), t3) + 256;
  if (need > temp_bytes_) {
    hgmem::dev_free(d_temp_, "d_temp_");
    d_temp_ = nullptr;
    HG_TRY(hgmem::dev_alloc(&d_temp_, need, "d_temp_"), "workspace alloc (sort)");
    temp_bytes_ = need;
  }
  return HG_OK;
}

int HgScanner::ensure(uint64_t nbytes) {
  uint64_t ntiles = std::max<uint64_t>((nbytes + HG_TILE_BYTES - 1) / HG_TILE_BYTES, 1);
  auto re = [&](auto *&ptr, size_t count, const char *name) { return fail(realloc_dev(ptr, count, name), "workspace alloc"); };
  if (ntiles > cap_tiles_) {
    uint64_t nblocks = (ntiles + TS_BLOCK_TILES - 1) / TS_BLOCK_TILES;
    if (re(d_sums_, ntiles, "d_sums_") || re(d_bases_, ntiles + 1, "d_bases_") || re(d_agg_, nblocks, "d_agg_") || re(d_block_base_, nblocks, "d_block_base_")) return HG_ERR_HIP;
    cap_tiles_ = ntiles;
  }
  if (!d_seg_count_) {
    max_segs_ = static_cast<uint32_t>(num_cus_) * 16;
    if (re(d_seg_count_, max_segs_, "d_seg_count_") || re(d_seg_count2_, max_segs_, "d_seg_count2_") || re(d_defer_count_, HG_CONFIRM_MODES * HG_DEFER_SHARDS, "d_defer_count_")) return HG_ERR_HIP;
  }
  // one candidate / hit per KiB of text to start with; grows (and the pass repeats) on overflow
  uint64_t want = std::max<uint64_t>(nbytes / 1024, 1u << 16);
  if (cand_cap_ < want && alloc_cands(want)) return HG_ERR_HIP;
  if (hit_cap_ < want && alloc_hits(want)) return HG_ERR_HIP;
  return HG_OK;
}

// (internal) results of a pass: HG_SPLIT, it would need more hit records or pipeline chunks than one pass may have (the caller
// scans in segments); HG_GROWN, a segment, a bucket or the compact hit array was too small and grew (the caller repeats the pass)
enum { HG_SPLIT = 1000, HG_GROWN = 1001 };

// What one pass does, worked out before it issues anything (plan_pass makes no HIP call); the launch stages read it and leave
// in it what later stages need.
struct HgScanner::PassPlan {
  const uint8_t *text;
  uint64_t nbytes, bs1, ntiles;
  PassRange range;
  bool block_mode, has_anchored;
  hipStream_t stream, side;  // side: the side passes' stream (the caller's unless piped)
  // finalize buckets (hg_fin_*): 2^fin_shift text bytes each by line start, fin_nb of them, fin_cap records of the hit arrays each
  uint32_t id_bits, to_bits, fin_shift = 10, fin_nb = 1, fin_cap;
  bool bucketed;  // (until the bucket arrays exist: whether the pass may order its hits in buckets)
  // pipeline chunks: chunk c = tiles [cut[c], cut[c + 1]); split: more of them than one pass may have
  uint32_t nchunks = 1;
  bool piped, split;
  uint64_t chunk_tiles;
  std::array<uint64_t, kMaxChunks + 1> cut;
  uint32_t wgs_alone, wgs_shared, joiner_wgs, wgs = 1;  // stream grids; wgs sizes the regrowth of the candidate segments
  uint32_t cand_seg_cap[2];  // records of a stream workgroup's candidate segment: chunk 0, later chunks
  HgStreamArgs sa;   // the fields every chunk shares
  HgConfirmArgs ca;
  // buckets finalized so far; the largest grid of the last chunk's side passes that stages hits (sizes their regrowth)
  uint32_t fin_done, stage_blocks = 1;
  uint32_t wgs_of(uint32_t c) const { return c == 0 ? wgs_alone : wgs_shared; }
  uint32_t joiners_of(uint32_t c) const { return c >= 1 ? joiner_wgs : 0u; }
  uint32_t set_of(uint32_t c) const { return piped ? (c & 1u) : 0u; }  // the candidate buffer set of chunk c
  // Buckets whose pieces all start before chunk c: a later hit's line starts less than bs1 bytes before it, so pieces that
  // start below (chunk start - bs1) have all their hits.
  uint32_t settled_buckets(uint32_t c) const {
    const uint64_t prev_end = std::min<uint64_t>(cut[c] << HG_TILE_SHIFT, nbytes);
    const uint64_t settled = prev_end > bs1 ? prev_end - bs1 : 0;
    return static_cast<uint32_t>(std::min<uint64_t>((settled > range.own_lo ? settled - range.own_lo : 0) >> fin_shift, fin_nb));
  }
};

HgScanner::PassPlan HgScanner::plan_pass(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, const PassRange &range, bool block_mode,
                                         hipStream_t stream) const {
  const uint64_t tile_lo = range.tile_lo, tile_hi = range.tile_hi, ntiles = tile_hi - tile_lo;
  PassPlan p{text, nbytes, bs1, ntiles, range, block_mode, db_->patterns.size() - db_->ncomb > db_->slow.size(), stream};
  // the bytes whose pieces this pass reports (buckets of the finalize count from own_lo)
  const uint64_t own_end = std::min<uint64_t>(range.own_hi, nbytes), own_len = own_end > range.own_lo ? own_end - range.own_lo : 0;
  // Bucketed emission + finalize (hg_fin_*): buckets of 2^fin_shift text bytes (1 KiB at least) by line start, at most
  // HG_FIN_MAX_BUCKETS of them, each a region of fin_cap records of the hit arrays.
  p.id_bits = bits_for(static_cast<uint64_t>(db_->max_id) + 1);
  p.to_bits = bits_for(bs1 + 1);
  // As many buckets as give ~30-50 records each (one wave orders up to 64 in registers; larger buckets go through LDS): from
  // the last pass's hits, else one hit per 8 KiB of text as a first guess.  (1 KiB buckets at least: a text with a report on
  // every line has ~10 per KiB)
  if (own_len) {
    const uint64_t expect = std::max<uint64_t>(fin_expect_hits_, own_len >> 13);
    uint64_t want_nb = 1;
    const uint64_t per_bucket = knobs_.fin_target;
    while (want_nb * per_bucket < expect && want_nb < HG_FIN_MAX_BUCKETS) want_nb <<= 1;
    while (((own_len - 1) >> p.fin_shift) >= want_nb) p.fin_shift++;
    p.fin_nb = static_cast<uint32_t>((own_len - 1) >> p.fin_shift) + 1;
  }
  p.fin_cap = hit_cap_ / p.fin_nb;
  // (sort key of a bucket: line start inside the bucket | id | to | single; the raw records carry that start in the top
  // 24 bits of the line number, so line numbers must stay below 2^40)
  p.bucketed = ntiles && p.fin_cap && p.fin_shift <= 64 - HG_HIT_REL_SHIFT && p.fin_shift + p.id_bits + p.to_bits + 1 <= 64 &&
               bits_for(line_base + nbytes + 1) <= HG_HIT_REL_SHIFT && !fin_fallback_ && !knobs_.no_bucket_finalize &&
               !view_.bounds &&     // (offset bounds: the compact finalize, whose report rule reads the SINGLEMATCH flag itself)
               !d_min_lengths_;     // (min_length: the same, and the match-length pass runs over the compact raw array)

  // Chunked pipeline (line mode, large buffers): the text is cut into tile-aligned chunks; the stream pass of chunk c+1
  // runs on the caller's stream while tile scan + verify + confirm of chunk c run on a side stream.  The stream pass
  // then leaves a quarter of the wave slots free so that the latency-bound side work is co-resident.
  uint32_t nchunks = 1;
  // measured on MI355X (32 GiB, 256 patterns): 8 GiB chunks 15.2 ms, 2 GiB chunks 20.8 ms, no chunking 17.6 ms per pass —
  // the latency-bound side kernels need a few hundred thousand candidates per launch to fill the chip
  constexpr uint64_t kChunkTiles = 8ull << (30 - HG_TILE_SHIFT);
  if (!block_mode && ntiles >= 2 * kChunkTiles) nchunks = static_cast<uint32_t>(std::min<uint64_t>(kMaxChunks, ntiles / kChunkTiles));
  uint64_t chunk_tiles = ((ntiles + nchunks - 1) / nchunks + TS_BLOCK_TILES - 1) / TS_BLOCK_TILES * TS_BLOCK_TILES;
  if (knobs_.chunk_tiles) {  // tests: force the chunked pipeline on small buffers
    const uint64_t v = knobs_.chunk_tiles;
    if (!block_mode && v >= TS_BLOCK_TILES) chunk_tiles = std::max<uint64_t>(v / TS_BLOCK_TILES * TS_BLOCK_TILES, (ntiles + kMaxChunks - 1) / kMaxChunks / TS_BLOCK_TILES * TS_BLOCK_TILES + TS_BLOCK_TILES);
  }
  if (!block_mode && chunk_limit_tiles_ && chunk_tiles > chunk_limit_tiles_) chunk_tiles = chunk_limit_tiles_;  // (a chunk's candidates did not fit before)
  nchunks = ntiles ? static_cast<uint32_t>((ntiles + chunk_tiles - 1) / chunk_tiles) : 1;
  uint32_t max_chunks = static_cast<uint32_t>(kMaxChunks);
  if (knobs_.max_chunks) max_chunks = std::max(1u, std::min<uint32_t>(kMaxChunks, knobs_.max_chunks));  // (tests)
  p.split = nchunks > max_chunks;  // (chunks that shrank for a dense text: fewer tiles per pass then)
  if (p.split) return p;
  for (uint32_t c = 0; c <= nchunks; c++) p.cut[c] = std::min<uint64_t>(tile_lo + static_cast<uint64_t>(c) * chunk_tiles, tile_hi);
  const std::vector<double> &w = knobs_.chunk_weights;  // experiment: relative chunk sizes
  if (!block_mode && w.size() >= 2 && w.size() <= static_cast<size_t>(kMaxChunks) && ntiles >= w.size() * TS_BLOCK_TILES * 2) {
    double total = 0, run = 0;
    for (double v : w) total += v;
    nchunks = static_cast<uint32_t>(w.size());
    chunk_tiles = 0;
    for (uint32_t c = 0; c < nchunks; c++) {
      run += w[c];
      uint64_t end = c + 1 == nchunks ? tile_hi : tile_lo + static_cast<uint64_t>(static_cast<double>(ntiles) * run / total) / TS_BLOCK_TILES * TS_BLOCK_TILES;
      end = std::min<uint64_t>(std::max<uint64_t>(end, p.cut[c] + TS_BLOCK_TILES), tile_hi);
      p.cut[c + 1] = end;
      chunk_tiles = std::max<uint64_t>(chunk_tiles, end - p.cut[c]);
    }
  }
  p.nchunks = nchunks;
  p.chunk_tiles = chunk_tiles;
  p.piped = nchunks > 1;
  p.side = p.piped ? side_stream_ : stream;

  if (ntiles) {
    uint32_t per_cu = p.piped ? std::max(1, stream_wgs_per_cu_ - 1) : stream_wgs_per_cu_;
    if (knobs_.stream_wgs_per_cu) {  // tuning knob: resident stream workgroups per CU
      const long v = knobs_.stream_wgs_per_cu;
      if (v >= 1 && v <= stream_wgs_per_cu_) per_cu = static_cast<uint32_t>(v);
    }
    auto grid_for = [&](uint32_t wgs_per_cu) {
      return static_cast<uint32_t>(std::min<uint64_t>((std::min<uint64_t>(chunk_tiles, ntiles) + STREAM_WG_WAVES - 1) / STREAM_WG_WAVES,
                                                      std::min<uint64_t>(static_cast<uint64_t>(num_cus_) * wgs_per_cu, max_segs_)));
    };
    p.wgs_shared = grid_for(per_cu);  // next to the side passes of the previous chunk
    // the first chunk streams alone: every workgroup slot (unless the grid was fixed by hand)
    p.wgs_alone = knobs_.stream_wgs_per_cu ? p.wgs_shared : grid_for(static_cast<uint32_t>(stream_wgs_per_cu_));
    // Joiners: the side passes of chunk c - 1 take about half as long as the stream pass of chunk c; behind them, on the side
    // stream, a second launch of the stream kernel (one more workgroup per CU, its own candidate segments) joins chunk c and
    // draws tiles from the same cursor until the chunk is used up.
    // (Only where a CU has room for it: the kernel's LDS allows three workgroups per CU and the shared launches use two;
    // and not when the last pass found the side passes to be the slower half (side_bound_: config 5).
    // Measured: 6.99 -> 6.84 ms per 32 GiB on config 3; HG_JOINER=0 turns it off.)
    // Not for texts so dense in candidates that the chunks had to shrink: their side passes are the slower half anyway, and
    // the joiner's segments would take workspace from the others.
    p.joiner_wgs = (p.piped && stream_wgs_per_cu_ >= 3 && per_cu < static_cast<uint32_t>(stream_wgs_per_cu_) && chunk_limit_tiles_ == 0 && !side_bound_) ? static_cast<uint32_t>(num_cus_) : 0u;
    if (knobs_.joiner >= 0) p.joiner_wgs = p.piped ? static_cast<uint32_t>(knobs_.joiner) * static_cast<uint32_t>(num_cus_) : 0u;
    if (p.wgs_shared + p.joiner_wgs > max_segs_ || db_->filter_wide || db_->filter_log2 > 13) p.joiner_wgs = 0;  // (hg_launch_stream_join's instantiations)
    p.wgs = std::max(p.wgs_shared + p.joiner_wgs, p.wgs_alone);
    // (the joiner's segments get a quarter of a stream workgroup's: it streams a few per cent of a chunk, and equal shares took a
    // third of the candidate workspace from the launch that fills it)
    for (uint32_t c = 0; c < std::min(nchunks, 2u); c++)
      p.cand_seg_cap[c] = static_cast<uint32_t>(static_cast<uint64_t>(cand_cap_) * 4 / (4ull * p.wgs_of(c) + p.joiners_of(c)));
  }
  HgStreamArgs &sa = p.sa;
  sa.text = text;
  sa.nbytes = nbytes;
  sa.db = view_;
  sa.filter = static_cast<const uint32_t *>(d_filter_);
  sa.filter_log2 = db_->filter_log2;
  sa.weights_a = db_->weights_a;
  sa.weights_b = db_->weights_b;
  sa.filter_wide = db_->filter_wide;
  sa.ctx = db_->filter_use_ctx;
  sa.dense = db_->dense;
  sa.weights_c = db_->weights_c;
  sa.ext = static_cast<const HgSlotInfo *>(d_ext_);
  sa.sums = d_sums_;
  sa.counters = d_counters_;
  HgConfirmArgs &ca = p.ca;
  ca.text = text;
  ca.nbytes = nbytes;
  ca.bs1 = bs1;
  ca.db = view_;
  ca.sums = d_sums_;
  ca.bases = d_bases_;
  ca.hits = d_hits_raw_;
  ca.aux = d_aux_raw_;
  ca.tmp_hits = d_hits_out_;  // free until the final select
  ca.tmp_aux = d_aux_out_;
  ca.hit_cap = hit_cap_;
  ca.hit_direct = hit_direct_ ? 1u : 0u;  // (bucket_cap / bucket_fill: set once the bucket arrays exist)
  ca.bucket_shift = p.fin_shift;
  ca.counters = d_counters_;
  ca.own_lo = range.own_lo;
  ca.own_hi = range.own_hi;
  if (!block_mode && p.has_anchored) {  // the verify / confirm passes' lists of verified occurrences
    const uint32_t mode_mask = knobs_.confirm_mode_mask;  // (all modes, except in profiling builds: HG_DEBUG_CONFIRM_MODES)
    ca.deferred = d_deferred_;
    ca.defer_count = d_defer_count_;
    ca.defer_shard_cap = cand_cap_ / HG_DEFER_SHARDS;
    for (uint32_t m = 0, next = 0; m < HG_CONFIRM_MODES; m++) {
      ca.mode_present[m] = (db_->n_confirm_mode[m] && ((mode_mask >> m) & 1u)) ? 1 : 0;
      ca.list_of_mode[m] = db_->n_confirm_mode[m] ? next++ : 0;
      ca.list_spread[m] = std::min<uint32_t>(HG_DEFER_SHARDS, std::max<uint32_t>(1, HG_DEFER_SHARDS / std::max<uint32_t>(1, db_->n_confirm_mode[m])) * defer_spread_boost_);
    }
  }
  return p;
}

// The finalize's bucket arrays, for nb buckets at least (64 K buckets at least, then by powers of two up to HG_FIN_MAX_BUCKETS).
int HgScanner::alloc_fin(uint32_t nb, hipStream_t stream) {
  uint32_t want = 1u << 16;
  while (want < nb) want <<= 1;
  fin_alloc_ = 0;
  HG_TRY(realloc_dev(d_fin_fill_, want, "d_fin_fill_"), "alloc finalize buckets");
  HG_TRY(realloc_dev(d_fin_kept_, want, "d_fin_kept_"), "alloc finalize buckets");
  HG_TRY(realloc_dev(d_fin_big_, 2 * static_cast<size_t>(want) + 3 * 128, "d_fin_big_"), "alloc finalize buckets");  // (two work lists + the scan's partial sums)
  HG_TRY(hipMemsetAsync(d_fin_big_ + 2 * static_cast<size_t>(want), 0, 3 * 128 * 4, stream), "clear scan flags");
  fin_alloc_ = want;
  return HG_OK;
}

// finalize of the buckets [lo, hi) on stream `s`: order each bucket, report rules, positions, gather (hg_fin_*)
int HgScanner::launch_fin(const PassPlan &p, hipStream_t s, uint32_t lo, uint32_t hi, bool beside_stream) {
  if (hi <= lo) return HG_OK;
  const uint32_t nbk = hi - lo, cu = static_cast<uint32_t>(num_cus_), fin_cap = p.fin_cap, id_bits = p.id_bits, to_bits = p.to_bits;
  HG_TRY(hipMemsetAsync(d_fin_total_ + 2, 0, 8, s), "memset work list");  // (larger buckets of this range: two size classes)
  hipLaunchKernelGGL(hg_fin_sort_small_kernel, dim3(std::min<uint32_t>((nbk + 3) / 4, cu * 8)), dim3(256), 0, s, d_hits_raw_, d_perm_a_, d_fin_fill_, lo, hi, fin_cap, id_bits, to_bits,
                     d_fin_kept_, d_fin_big_, d_fin_total_ + 2, fin_alloc_);
  hipLaunchKernelGGL((hg_fin_sort_big_kernel<HG_FIN_MEDIUM_CAP, true>), dim3(std::min<uint32_t>(nbk, cu * 4)), dim3(256), 0, s, d_hits_raw_, d_perm_a_, d_fin_fill_, d_fin_big_, d_fin_total_ + 2,
                     fin_cap, id_bits, to_bits, d_fin_kept_, d_selected_ + 1, static_cast<uint64_t *>(nullptr), static_cast<uint32_t *>(nullptr));
  // (scratch of the large class: the key / permutation arrays of the library sort, idle while the scanner emits into buckets)
  const uint32_t big_blocks = std::min<uint32_t>(std::min<uint32_t>(nbk, 64u), hit_cap_ / HG_FIN_BUCKET_CAP);
  if (big_blocks)
    hipLaunchKernelGGL((hg_fin_sort_big_kernel<HG_FIN_BUCKET_CAP, false>), dim3(big_blocks), dim3(256), 0, s, d_hits_raw_, d_perm_a_, d_fin_fill_, d_fin_big_ + fin_alloc_,
                       d_fin_total_ + 3, fin_cap, id_bits, to_bits, d_fin_kept_, d_selected_ + 1, d_key_a_, d_perm_b_);
  // (a block per 8192 buckets, 128 at most: their partial sums live behind the two work lists)
  const uint32_t scan_blocks = std::max<uint32_t>(1, std::min<uint32_t>(128, (nbk + 8191) / 8192));
  fin_info_.scan_blocks = std::max(fin_info_.scan_blocks, scan_blocks);
  uint32_t *part = d_fin_big_ + 2 * static_cast<size_t>(fin_alloc_);
  const uint32_t epoch = ++fin_epoch_ ? fin_epoch_ : ++fin_epoch_;  // (never 0: the flags start out zeroed)
  if (beside_stream) hipLaunchKernelGGL(hg_fin_scan_kernel<512u>, dim3(scan_blocks), dim3(512), 0, s, d_fin_kept_, lo, hi, d_fin_total_, d_fin_fill_, fin_cap, part, epoch);
  else hipLaunchKernelGGL(hg_fin_scan_kernel<1024u>, dim3(scan_blocks), dim3(1024), 0, s, d_fin_kept_, lo, hi, d_fin_total_, d_fin_fill_, fin_cap, part, epoch);
  hipLaunchKernelGGL(hg_fin_gather_kernel, dim3(std::min<uint32_t>((nbk + 3) / 4, cu * 8)), dim3(256), 0, s, d_hits_raw_, d_aux_raw_, d_perm_a_, d_fin_kept_, d_fin_total_, lo, hi, fin_cap,
                     d_hits_out_, d_aux_out_);
  HG_TRY(hipGetLastError(), "finalize launch");
  return HG_OK;
}

int HgScanner::copy_fin_fill(uint32_t *dst, uint32_t max, uint32_t *n) {
  *n = 0;
  if (fin_info_.path != 1u || !d_fin_fill_ || !dst) return HG_OK;
  const uint32_t count = std::min(max, fin_info_.fin_nb);
  HG_TRY(hipSetDevice(device_), "hipSetDevice");
  if (count) HG_TRY(hipMemcpy(dst, d_fin_fill_, static_cast<size_t>(count) * sizeof(uint32_t), hipMemcpyDeviceToHost), "copy bucket fill levels");
  *n = count;
  return HG_OK;
}

// Chunk c's stream launch on the caller's stream, with its joiner in front of it (tests) or behind it on the side stream.
int HgScanner::launch_stream(PassPlan &p, uint32_t c, HgScanOutput *out) {
  const uint32_t wgs_c = p.wgs_of(c), joiners_c = p.joiners_of(c);
  HgStreamArgs sa = p.sa;
  sa.tile_begin = p.cut[c];
  sa.tile_end = p.cut[c + 1];
  // the chunk's workgroups draw runs of consecutive tiles from a cursor (hg_stream_kernel): two tiles per wave and draw
  sa.cursor_slot = HG_CNT_CURSOR0 + c;  // (zeroed by hg_reset_kernel with the rest of the state block)
  sa.cands = p.set_of(c) ? d_cands2_ : d_cands_;
  sa.seg_count = p.set_of(c) ? d_seg_count2_ : d_seg_count_;
  sa.cand_seg_cap = p.cand_seg_cap[c ? 1 : 0];
  sa.alone = (c == 0 && wgs_c == p.wgs_alone && !knobs_.stream_wgs_per_cu) ? 1u : 0u;
  HgStreamArgs ja = sa;  // the joiner: its own candidate segments behind the stream launch's
  ja.cands = sa.cands + static_cast<uint64_t>(wgs_c) * sa.cand_seg_cap;
  ja.cand_seg_cap = sa.cand_seg_cap / 4;
  ja.seg_count = sa.seg_count + wgs_c;
  ja.alone = 0;
  auto launch_joiner = [&](hipStream_t s) -> int {
    if (!hg_launch_stream_join(ja, joiners_c, s)) return HG_ERR_ARG;
    out->joiner_launches++;
    HG_TRY(hipGetLastError(), "hg_stream_kernel launch (joiner)");
    return HG_OK;
  };
  HG_TRY(hipEventRecord(p.piped ? ev_k1_begin_[c] : ev_[1], p.stream), "event");
  if (joiners_c && knobs_.joiner_ahead)  // (tests: in front of the chunk's stream launch, it draws the chunk's tiles first)
    if (int rc = launch_joiner(p.stream)) return rc;
  if (!hg_launch_stream(sa, wgs_c, p.stream)) return error(HG_ERR_ARG, "no stream kernel for this database's filter size / mode");
  HG_TRY(hipGetLastError(), "hg_stream_kernel launch");
  HG_TRY(hipEventRecord(p.piped ? ev_k1_end_[c] : ev_[2], p.stream), "event");
  if (p.piped && p.bucketed && joiners_c && c + 1 == p.nchunks && !knobs_.no_early_finalize) {
    // The last chunk: the side stream is idle from the end of chunk c - 1's side passes to the end of this stream launch.
    // The buckets the earlier chunks have completed are finalized there, in front of the joiner (they used to be
    // finalized beside the last chunk's verify / confirm passes, competing with them for the chip: 430 us for what takes
    // 150 alone, and last to finish).
    const uint32_t lim = p.settled_buckets(c);
    if (lim > p.fin_done) {
      if (int rc = launch_fin(p, p.side, p.fin_done, lim, true)) return rc;
      fin_info_.early_buckets += lim - p.fin_done;
      fin_info_.early_beside_stream += lim - p.fin_done;
      p.fin_done = lim;
    }
  }
  if (joiners_c && !knobs_.joiner_ahead)  // (the side stream: behind the side passes of chunk c - 1, in front of those of chunk c)
    if (int rc = launch_joiner(p.side)) return rc;
  if (p.piped) HG_TRY(hipStreamWaitEvent(p.side, ev_k1_end_[c], 0), "stream wait");
  return HG_OK;
}

// Chunk c's side passes on the side stream: block mode's mark / scan passes, or line mode's tile scan, verify / confirm and
// always-on passes.
int HgScanner::launch_side(PassPlan &p, uint32_t c) {
  const uint64_t t0 = p.cut[c], t1 = p.cut[c + 1];
  const uint32_t segs_c = p.wgs_of(c) + p.joiners_of(c);  // candidate segments of the chunk: one per stream workgroup
  const hipStream_t side = p.side;
  HgConfirmArgs ca = p.ca;
  ca.tile_begin = t0;
  ca.tile_end = t1;
  uint32_t *seg_count = p.set_of(c) ? d_seg_count2_ : d_seg_count_;
  ca.cands = p.set_of(c) ? d_cands2_ : d_cands_;
  ca.seg_count = seg_count;
  ca.cand_seg_cap = p.cand_seg_cap[c ? 1 : 0];
  ca.join_seg0 = p.wgs_of(c);
  ca.join_seg_cap = ca.cand_seg_cap / 4;
  uint32_t confirm_blocks = 1, always_blocks = 1;
  if (p.block_mode) {
    HG_TRY(hipMemsetAsync(d_pflags_, 0, db_->patterns.size() * 4, side), "memset pattern flags");
    if (p.has_anchored) hipLaunchKernelGGL(hg_block_mark_kernel, dim3(segs_c), dim3(256), 0, side, ca, d_pflags_);
    always_blocks = std::max<uint32_t>(static_cast<uint32_t>((db_->patterns.size() + 255) / 256), std::min<uint32_t>(db_->nhuge, 1024u));
    ca.hit_seg_cap = hit_cap_ / always_blocks;
    hipLaunchKernelGGL(hg_block_scan_kernel, dim3(static_cast<uint32_t>((db_->patterns.size() + 255) / 256)), dim3(256), 0, side, ca, d_pflags_);
    if (db_->nhuge && !hg_launch_block_huge(ca, std::min<uint32_t>(db_->nhuge, 1024u), db_->huge_max_nw, db_->huge_stage_words, d_pflags_, side)) return huge_lds_error();
    HG_TRY(hipGetLastError(), "block-mode launch");
    p.stage_blocks = std::max(confirm_blocks, always_blocks);
    return HG_OK;
  }
  const uint64_t span = t1 - t0;
  const uint32_t nblocks = static_cast<uint32_t>((span + TS_BLOCK_TILES - 1) / TS_BLOCK_TILES);
  if (p.bs1 < HG_TILE_BYTES) {  // small-buffer mode: lines inside a tile can split, re-price the tile summaries
    uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((span + 255) / 256, 4096));
    hipLaunchKernelGGL(hg_tile_inner_kernel, dim3(blocks), dim3(256), 0, side, p.text, d_sums_, t0, t1, p.bs1);
  }
  hipLaunchKernelGGL(hg_tile_reduce_kernel, dim3(nblocks), dim3(256), 0, side, d_sums_, t0, t1, p.bs1, d_agg_);
  hipLaunchKernelGGL(hg_tile_spine_kernel, dim3(1), dim3(256), 0, side, d_agg_, nblocks, p.bs1, d_block_base_, d_final_);
  hipLaunchKernelGGL(hg_tile_apply_kernel, dim3(nblocks), dim3(256), 0, side, d_sums_, t0, t1, p.bs1, d_block_base_, d_bases_);
  HG_TRY(hipGetLastError(), "tile scan launch");
  if (p.piped && c + 1 == p.nchunks) HG_TRY(hipEventRecord(ev_tile_done_, side), "event");  // (the early finalize starts behind the tile scan)
  if (p.has_anchored) {
    const uint32_t verify_blocks = segs_c * HG_CONFIRM_SPLIT;  // HG_CONFIRM_SPLIT blocks share candidate segment b
    uint32_t fast_modes = 0;
    const uint32_t mode_mask = knobs_.confirm_mode_mask;
    for (uint32_t m = 0; m < 3; m++) fast_modes += (db_->n_confirm_mode[m] && ((mode_mask >> m) & 1u)) ? 1 : 0;
    // few, long-lived blocks per confirm routine (in units of 256 lanes per CU; 3 measured best next to the stream pass);
    // the last chunk's side passes have the chip to themselves
    uint32_t per_cu = c + 1 == p.nchunks ? 6 : 3;
    if (knobs_.confirm_blocks_per_cu) per_cu = static_cast<uint32_t>(knobs_.confirm_blocks_per_cu);
    const uint32_t mode_blocks = std::max<uint32_t>(HG_DEFER_SHARDS, static_cast<uint32_t>(num_cus_) * per_cu * (256 / HG_CONFIRM_THREADS));  // per_cu counts 256 lanes
    // huge automata (confirm mode 4): one-wave workgroups, as many per CU as their LDS allows (8 at most)
    const uint32_t huge_blocks = db_->n_confirm_mode[4] ? std::max<uint32_t>(HG_DEFER_SHARDS, static_cast<uint32_t>(num_cus_) * static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(8, (160u << 10) / std::max<size_t>(hg_huge_lds_bytes(db_->huge_max_nw, db_->huge_stage_words), 1))))) : 0u;
    confirm_blocks = std::max(std::max(mode_blocks * std::max(fast_modes, 1u), verify_blocks), huge_blocks);  // the largest grid that stages hits
    ca.hit_seg_cap = hit_cap_ / confirm_blocks;
    if (c > 0) HG_TRY(hipMemsetAsync(d_defer_count_, 0, HG_CONFIRM_MODES * HG_DEFER_SHARDS * 4, side), "memset deferred counts");  // (chunk 0: hg_reset_kernel)
    // (sets without automaton modes 1 / 2: the verify variant without the LDS staging area)
    if (ca.mode_present[1] || ca.mode_present[2]) hipLaunchKernelGGL(hg_verify_kernel, dim3(verify_blocks), dim3(256), 0, side, ca);
    else hipLaunchKernelGGL(hg_verify_lean_kernel, dim3(verify_blocks), dim3(256), 0, side, ca);
    const bool literal_only_set = ca.mode_present[0] && !ca.mode_present[1] && !ca.mode_present[2];
    if (literal_only_set) {
      hipLaunchKernelGGL(hg_confirm_literal_kernel, dim3(mode_blocks), dim3(256), 0, side, ca);  // (blocks of 256: as many lanes per CU as before)
    } else if (fast_modes) {
      hipLaunchKernelGGL(hg_confirm_fast_kernel, dim3(mode_blocks * fast_modes), dim3(HG_CONFIRM_THREADS), 0, side, ca, mode_blocks);
    }
    if (db_->n_confirm_mode[3]) hipLaunchKernelGGL(hg_confirm_generic_kernel, dim3(mode_blocks), dim3(256), 0, side, ca);
    if (huge_blocks && ((mode_mask >> 4) & 1u)) {
      HG_TRY(hipMemsetAsync(d_huge_claim_, 0, huge_claim_slots_ * 8, side), "memset claim table");
      if (!hg_launch_confirm_huge(ca, huge_blocks, db_->huge_max_nw, db_->huge_stage_words, d_huge_claim_, static_cast<uint32_t>(huge_claim_slots_ - 1), side)) return huge_lds_error();
    }
    HG_TRY(hipGetLastError(), "confirm launch");
  }
  if (!db_->slow.empty()) {
    always_blocks = static_cast<uint32_t>(std::min<uint64_t>((span + 3) / 4, static_cast<uint64_t>(num_cus_) * 8));
    // (huge automata: one-wave workgroups, four per SIMD — the routine is a chain of LDS reads and ballots per byte)
    const uint32_t huge_always_blocks = db_->nslow_huge ? static_cast<uint32_t>(std::min<uint64_t>(span, static_cast<uint64_t>(num_cus_) * 16)) : 0u;
    ca.hit_seg_cap = hit_cap_ / std::max(always_blocks, huge_always_blocks);
    const uint32_t nfast = db_->nslow_fast, nhuge = db_->nslow_huge, nall = static_cast<uint32_t>(db_->slow.size()) - nhuge;  // [fast | scalar | huge]
    if (nfast) {
      // the match list lives in the (by now idle) verified-occurrence lists: cand_cap_ entries at least, a segment per block
      ca.deferred = d_deferred_;
      ca.always_count = seg_count;  // this chunk's candidate segment counts were consumed by the verify pass
      ca.always_list_cap = cand_cap_ / always_blocks;
      hipLaunchKernelGGL(hg_always_on_fast_kernel, dim3(always_blocks), dim3(256), 0, side, ca);
      hipLaunchKernelGGL(hg_always_on_finish_kernel, dim3(always_blocks), dim3(256), 0, side, ca);
    }
    if (nall > nfast) hipLaunchKernelGGL(hg_always_on_kernel, dim3(always_blocks), dim3(256), 0, side, ca, nfast, nall);
    if (nhuge && !hg_launch_always_on_huge(ca, huge_always_blocks, db_->huge_max_nw, db_->huge_stage_words, nall, nall + nhuge, side)) return huge_lds_error();
    always_blocks = std::max(always_blocks, huge_always_blocks);
    HG_TRY(hipGetLastError(), "hg_always_on_kernel launch");
  }
  p.stage_blocks = std::max(confirm_blocks, always_blocks);
  return HG_OK;
}

// Behind the side passes of the last chunk c: the buckets that are left.
int HgScanner::finalize_last(PassPlan &p, uint32_t c) {
  bool fin_early = false;  // the buckets of all chunks but the last were finalized beside the last chunk's side passes
  if (p.piped && c >= 1 && !knobs_.no_early_finalize) {
    // The last stream launch is queued.  Behind it, on this stream, the buckets that the earlier chunks have completed
    // are finalized WHILE the side stream works through the last chunk's verify / confirm passes (both have the chip to
    // themselves by then); only the last chunk's buckets remain for after those.  (Finalizing a chunk's buckets beside
    // the NEXT chunk's stream pass was tried: it slowed the stream pass by more than it saved.)
    const uint32_t lim = p.settled_buckets(c);
    if (lim > p.fin_done) {
      HG_TRY(hipStreamWaitEvent(p.stream, ev_side_done_[c - 1], 0), "stream wait");  // the earlier chunks' hits are all in their buckets
      HG_TRY(hipStreamWaitEvent(p.stream, ev_tile_done_, 0), "stream wait");        // ... and the last chunk's tile scan (a one-block latency chain) is through
      if (int rc = launch_fin(p, p.stream, p.fin_done, lim)) return rc;
      HG_TRY(hipEventRecord(ev_fin_early_, p.stream), "event");
      fin_info_.early_buckets += lim - p.fin_done;
      p.fin_done = lim;
      fin_early = true;
    }
  }
  if (fin_early) HG_TRY(hipStreamWaitEvent(p.side, ev_fin_early_, 0), "stream wait");  // (shared totals / work list: one range at a time)
  return launch_fin(p, p.side, p.fin_done, p.fin_nb);
}

// The pass's counters are read back: grow what overflowed.  HG_OK: everything fit; HG_GROWN: the pass must be repeated;
// HG_SPLIT: the buffer is to be scanned in segments.
int HgScanner::regrow(const PassPlan &p, uint64_t n_raw) {
  const bool block_mode = p.block_mode, bucketed = p.bucketed;
  const uint64_t cand_need = h_counters_[HG_CNT_CAND_NEED], hit_need = h_counters_[HG_CNT_HIT_NEED];
  const uint64_t defer_need = h_counters_[HG_CNT_DEFER_NEED];
  const bool fin_overflow = bucketed && h_counters_[HG_ST_SELECTED + 1] != 0;  // a bucket beyond what one block sorts
  // Hit records one pass may hold (2^28: 8 GiB each of raw and ordered records); a buffer with more is scanned in segments
  // whose ordered hits are put one after the other (scan_segments).
  uint64_t kHitLimit = 1ull << 28;
  if (knobs_.hit_limit) kHitLimit = std::max<uint64_t>(1u << 10, knobs_.hit_limit);  // (tests)
  if (!block_mode && (n_raw > kHitLimit || h_counters_[HG_CNT_HITS_WRAPPED])) return HG_SPLIT;
  if (!(cand_need || defer_need || hit_need || fin_overflow || (!bucketed && n_raw > hit_cap_))) return HG_OK;
  if (cand_need || defer_need) {
    // Candidate segments fill evenly (the stream workgroups draw their tiles on demand) and so do the position-sharded
    // lists; a pattern-keyed list (automaton modes) overflows when ONE expression owns most occurrences: its occurrences
    // are then spread over more lists instead of sizing every list for it.
    if (defer_need && defer_spread_boost_ < HG_DEFER_SHARDS) defer_spread_boost_ *= 4;
    uint64_t want = std::max<uint64_t>((cand_need + cand_need / 4 + 64) * p.wgs, (defer_need + defer_need / 4 + 64) * HG_DEFER_SHARDS);
    want = std::max<uint64_t>(want, static_cast<uint64_t>(cand_cap_) * 2);
    // The workspace holds ONE chunk's candidates (two buffer sets): when that would pass 2^30 records (16 GiB a set) the
    // chunks get smaller instead — a text that fits in HBM always scans, a very dense one in more, smaller chunks.
    uint64_t kCandLimit = 1ull << 30;
    if (knobs_.cand_limit) kCandLimit = std::max<uint64_t>(1u << 16, knobs_.cand_limit);  // (tests)
    if (want > kCandLimit) {
      const uint64_t cur = (std::min<uint64_t>(p.chunk_tiles, p.ntiles) + TS_BLOCK_TILES - 1) / TS_BLOCK_TILES * TS_BLOCK_TILES;
      if (block_mode || cur <= TS_BLOCK_TILES) return error(HG_ERR_ARG, "the candidate limit is below what one 16 MiB chunk of this text produces");  // (only with HG_CAND_LIMIT lowered: 16 MiB hold 2^24 positions)
      chunk_limit_tiles_ = std::max<uint64_t>(TS_BLOCK_TILES, cur / 2 / TS_BLOCK_TILES * TS_BLOCK_TILES);
      want = std::min<uint64_t>(want / 2, kCandLimit);
    }
    if (want > cand_cap_)
      if (int rc = alloc_cands(want)) return rc;
  }
  if (bucketed && (hit_need || fin_overflow)) {
    // hit_need = the fullest bucket's demand.  Equal bucket regions are fine while the hits are spread; when one bucket
    // holds thousands of them (every match end of an all-matches expression on one long line) the scanner leaves bucketed
    // emission for good: compact array + library sort.
    const uint64_t want = (hit_need + hit_need / 4 + 16) * p.fin_nb;
    fin_expect_hits_ = std::max<uint64_t>(fin_expect_hits_ * 2, n_raw);  // (more, smaller buckets next time)
    if (fin_overflow || hit_need > HG_FIN_BUCKET_CAP || want > (128ull << 20)) {
      fin_fallback_ = true;
    } else if (int rc = alloc_hits(std::max<uint64_t>(want, static_cast<uint64_t>(hit_cap_) * 2))) {
      return rc;
    }
  } else if (hit_need || n_raw > hit_cap_) {
    uint64_t want = std::max<uint64_t>((hit_need + hit_need / 4 + 64) * p.stage_blocks, n_raw + n_raw / 4);
    // equal segments sized for the fullest block: fine while the hits are spread, absurd when one block holds most of them
    // (every match end of an all-matches expression on one very long line).  Past 64 M records (4 GiB of workspace) or 16
    // times the hits actually seen, the segments stop growing and full blocks append to the compact array directly.
    constexpr uint64_t kSegmentLimit = 64ull << 20;
    const uint64_t by_total = n_raw + n_raw / 4 + 4096;
    if (want > kSegmentLimit || want > 16 * by_total) {
      hit_direct_ = true;
      want = std::min<uint64_t>(want, std::max<uint64_t>(by_total, std::min<uint64_t>(16 * by_total, kSegmentLimit)));
    }
    const uint64_t most = kHitLimit + kHitLimit / 4 + 4096;
    want = std::max<uint64_t>(want, std::min<uint64_t>(static_cast<uint64_t>(hit_cap_) * 2, most));
    if (want > most && !block_mode) return HG_SPLIT;
    if (want > most) return error(HG_ERR_ARG, "more than 2^28 reports for one block");  // (block mode: one scan unit of at most 2 GiB, nothing to cut at)
    if (int rc = alloc_hits(want)) return rc;
  }
  return HG_GROWN;
}

// Compact array + library sort of the pass's n raw hits (scanners that left bucketed emission, keys wider than 64 bits):
// order by (line, id, to, single-after-multi), apply the report rules, and count the kept hits into d_selected_.  The line
// numbers stay below line_bound.
int HgScanner::finalize_compact(const HgHit *hits, const HgHitAux *aux, uint32_t n, uint32_t id_bits, uint32_t to_bits, uint64_t line_bound, hipStream_t stream) {
  const HgPattern *pats = static_cast<const HgPattern *>(d_patterns_);
  uint32_t blocks = (n + 255) / 256;
  // one radix sort over exactly the bits in use when they fit in 64, else two
  const uint32_t line_bits = bits_for(line_bound);
  const uint32_t *perm = nullptr;
  uint32_t *pos = nullptr;
  size_t tb = temp_bytes_;
  if (compact_key_packed(line_bound, id_bits, to_bits)) {
    hipLaunchKernelGGL(hg_key_packed_kernel, dim3(blocks), dim3(256), 0, stream, hits, aux, pats, n, id_bits, to_bits, d_key_a_, d_perm_a_);
    HG_TRY(rocprim::radix_sort_pairs(d_temp_, tb, d_key_a_, d_key_b_, d_perm_a_, d_perm_b_, n, 0, line_bits + id_bits + to_bits + 1, stream), "radix sort");
    perm = d_perm_b_;
    pos = d_perm_a_;
  } else {
    hipLaunchKernelGGL(hg_key_kernel, dim3(blocks), dim3(256), 0, stream, hits, aux, pats, n, d_key_a_, d_perm_a_);
    HG_TRY(rocprim::radix_sort_pairs(d_temp_, tb, d_key_a_, d_key_b_, d_perm_a_, d_perm_b_, n, 0, 64, stream), "radix sort (id, to)");
    hipLaunchKernelGGL(hg_line_key_kernel, dim3(blocks), dim3(256), 0, stream, hits, d_perm_b_, n, d_key_a_);
    tb = temp_bytes_;
    HG_TRY(rocprim::radix_sort_pairs(d_temp_, tb, d_key_a_, d_key_b_, d_perm_b_, d_perm_a_, n, 0, std::min<uint32_t>(64, line_bits), stream), "radix sort (line)");
    perm = d_perm_a_;
    pos = d_perm_b_;
  }
  hipLaunchKernelGGL(hg_keep_kernel, dim3(blocks), dim3(256), 0, stream, hits, aux, perm, pats, n, d_keep_);
  tb = temp_bytes_;
  HG_TRY(rocprim::exclusive_scan(d_temp_, tb, d_keep_, pos, 0u, n, rocprim::plus<uint32_t>(), stream), "scan");
  hipLaunchKernelGGL(hg_scatter_kernel, dim3(blocks), dim3(256), 0, stream, hits, aux, perm, d_keep_, pos, n, d_hits_out_, d_aux_out_, d_selected_);
  HG_TRY(hipGetLastError(), "finalize launch");
  HG_TRY(hipMemcpyAsync(h_counters_ + HG_ST_SELECTED, d_selected_, 4, hipMemcpyDeviceToHost, stream), "copy count");
  return HG_OK;
}

// The combination pass over a pass's final hits (databases with combinations or QUIET expressions): hg_comb.hip counts the
// records each hit hands on (itself unless QUIET, the reports of the combinations it makes true), an exclusive scan sizes the
// union, the second launch writes it, and the compact finalize orders it and applies the report rules into d_hits_out_.  *out
// then describes the delivered hits.  (The input may be d_hits_out_ itself: it is read completely before the finalize
// writes there.)
int HgScanner::comb_pass(HgScanOutput *out, uint64_t bs1, uint64_t line_bound, hipStream_t stream) {
  const uint64_t n = out->n_hits;
  if (n == 0) return HG_OK;
  if (n + 1 > comb_in_cap_) {
    const uint64_t cap = std::max<uint64_t>(n + n / 4 + 1, 4096);
    comb_in_cap_ = 0;
    HG_TRY(realloc_dev(d_comb_count_, cap, "d_comb_count_"), "alloc (combination pass)");
    HG_TRY(realloc_dev(d_comb_pos_, cap, "d_comb_pos_"), "alloc (combination pass)");
    size_t tb = 0;
    HG_TRY(rocprim::exclusive_scan(nullptr, tb, d_comb_count_, d_comb_pos_, uint64_t{0}, cap, rocprim::plus<uint64_t>(), stream), "scan (combination pass)");
    if (tb > comb_temp_bytes_) {
      comb_temp_bytes_ = 0;
      HG_TRY(realloc_dev(d_comb_temp_, tb, "d_comb_temp_"), "alloc (combination pass)");
      comb_temp_bytes_ = tb;
    }
    comb_in_cap_ = cap;
  }
  const HgDb &db = *db_;
  HgCombArgs a{out->d_hits, out->d_aux, n, static_cast<const HgPattern *>(d_patterns_), d_combs_, d_comb_words_, d_comb_feed_,
               static_cast<uint32_t>(db.comb_feed.size() / 2), d_comb_count_, d_comb_pos_, nullptr, nullptr};
  HG_TRY(hg_comb_launch(a, false, stream), "combination pass launch (count)");
  size_t tb = comb_temp_bytes_;
  HG_TRY(rocprim::exclusive_scan(d_comb_temp_, tb, d_comb_count_, d_comb_pos_, uint64_t{0}, n + 1, rocprim::plus<uint64_t>(), stream), "scan (combination pass)");
  uint64_t total = 0;
  HG_TRY(hipMemcpyAsync(&total, d_comb_pos_ + n, sizeof total, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (combination pass)");
  if (total > 0x7FFFFFF0u) return error(HG_ERR_NOMEM, "more than 2^31 reports with the combination reports of one pass");
  if (total == 0) {
    out->n_hits = 0;
    return HG_OK;
  }
  if (total > comb_out_cap_) {
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(total + total / 4, 4096), 0x7FFFFFF0u);
    comb_out_cap_ = 0;
    HG_TRY(realloc_dev(d_comb_hits_, cap, "d_comb_hits_"), "alloc (combination pass)");
    HG_TRY(realloc_dev(d_comb_aux_, cap, "d_comb_aux_"), "alloc (combination pass)");
    comb_out_cap_ = cap;
  }
  a.out_hits = d_comb_hits_;
  a.out_aux = d_comb_aux_;
  HG_TRY(hg_comb_launch(a, true, stream), "combination pass launch (emit)");
  if (total > hit_cap_) {  // the finalize's workspace (d_hits_out_ included: the input has been read by now)
    HG_TRY(hipStreamSynchronize(stream), "stream sync (combination pass)");
    if (int rc = alloc_hits(total)) return rc;
  }
  if (int rc = finalize_compact(d_comb_hits_, d_comb_aux_, static_cast<uint32_t>(total), bits_for(static_cast<uint64_t>(db.max_id) + 1), bits_for(bs1 + 1), line_bound, stream))
    return rc;
  HG_TRY(hipStreamSynchronize(stream), "stream sync (combination pass)");
  out->n_hits = h_counters_[HG_ST_SELECTED];
  out->d_hits = d_hits_out_;
  out->d_aux = d_aux_out_;
  return HG_OK;
}

// The match-length pass (hs_expr_ext_t min_length, hg_som.hip) over the *n raw reports of a pass in the compact array: the
// survivors go to a second raw array (allocated by the first pass that needs it) and *n becomes their number.  The count
// word was zeroed by the pass's reset launch.
int HgScanner::minlen_pass(const uint8_t *text, uint32_t *n, hipStream_t stream) {
  if (*n > minlen_cap_) {
    minlen_cap_ = 0;
    const uint64_t cap = std::max<uint64_t>(static_cast<uint64_t>(*n) + *n / 4, 4096);
    HG_TRY(realloc_dev(d_minlen_hits_, cap, "d_minlen_hits_"), "alloc (match-length pass)");
    HG_TRY(realloc_dev(d_minlen_aux_, cap, "d_minlen_aux_"), "alloc (match-length pass)");
    minlen_cap_ = cap;
  }
  HG_TRY(hg_minlen_launch(text, d_hits_raw_, d_aux_raw_, *n, static_cast<const HgPattern *>(d_patterns_), static_cast<const uint32_t *>(d_pool_), minlen_max_nw_,
                          d_min_lengths_, d_minlen_hits_, d_minlen_aux_, d_counters_ + HG_ST_MINLEN_KEPT, stream),
         "match-length launch");
  HG_TRY(hipMemcpyAsync(h_counters_ + HG_ST_MINLEN_KEPT, d_counters_ + HG_ST_MINLEN_KEPT, 4, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (match-length pass)");
  *n = h_counters_[HG_ST_MINLEN_KEPT];
  return HG_OK;
}

// The invert stage over a finished scan (*out: its final hits, ordered by line, and its piece count): the count pass over
// the scan's tile states and hits, an exclusive scan of the per-tile counts, and the write pass (hg_invert.hip).  *out then
// describes the selected pieces; its counters and timings stay the scan's.  A buffer that was scanned in segments is
// inverted here in one go: the segments leave the tile states of the whole buffer and their hits one after the other, so
// the result is the one of inverting segment by segment.
int HgScanner::invert_pass(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, hipStream_t stream, HgScanOutput *out) {
  const uint64_t ntiles = (nbytes + HG_TILE_BYTES - 1) / HG_TILE_BYTES;
  out->d_from = nullptr;  // (a selected piece has no match: its start reads 0)
  if (ntiles == 0) {
    out->n_hits = 0;
    return HG_OK;
  }
  if (ntiles + 1 > inv_tiles_cap_) {
    const uint64_t cap = std::max<uint64_t>(ntiles + ntiles / 4 + 1, 4096);
    inv_tiles_cap_ = 0;
    HG_TRY(realloc_dev(d_inv_count_, cap, "d_inv_count_"), "alloc (invert stage)");
    HG_TRY(realloc_dev(d_inv_pos_, cap, "d_inv_pos_"), "alloc (invert stage)");
    inv_tiles_cap_ = cap;
  }
  size_t tb = 0;  // the scan's scratch, asked for the size that is scanned
  HG_TRY(rocprim::exclusive_scan(nullptr, tb, d_inv_count_, d_inv_pos_, uint64_t{0}, ntiles + 1, rocprim::plus<uint64_t>(), stream), "scan (invert stage)");
  if (tb > inv_temp_bytes_ || !d_inv_temp_) {
    inv_temp_bytes_ = 0;
    HG_TRY(realloc_dev(d_inv_temp_, tb + tb / 4, "d_inv_temp_"), "alloc (invert stage)");
    inv_temp_bytes_ = tb + tb / 4;
  }
  HgInvertArgs a{text, nbytes, bs1, ntiles, line_base + out->n_pieces, d_sums_, d_bases_, out->d_hits, out->n_hits, d_inv_count_, d_inv_pos_, nullptr, nullptr};
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_TRY(hg_invert_launch(a, false, static_cast<uint32_t>(num_cus_), stream), "invert stage launch (count)");
  HG_TRY(rocprim::exclusive_scan(d_inv_temp_, tb, d_inv_count_, d_inv_pos_, uint64_t{0}, ntiles + 1, rocprim::plus<uint64_t>(), stream), "scan (invert stage)");
  uint64_t total = 0;
  HG_TRY(hipMemcpyAsync(&total, d_inv_pos_ + ntiles, sizeof total, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (invert stage)");
  if (total > out->n_pieces) return error(HG_ERR_HIP, "the invert stage counted more pieces than the buffer has");
  if (total > inv_cap_) {
    const uint64_t cap = std::max<uint64_t>(total + total / 4, 4096);
    inv_cap_ = 0;
    HG_TRY(realloc_dev(d_inv_hits_, cap, "d_inv_hits_"), "alloc (invert stage records)");
    HG_TRY(realloc_dev(d_inv_aux_, cap, "d_inv_aux_"), "alloc (invert stage records)");
    inv_cap_ = cap;
  }
  if (total) {
    a.out_hits = d_inv_hits_;
    a.out_aux = d_inv_aux_;
    HG_TRY(hg_invert_launch(a, true, static_cast<uint32_t>(num_cus_), stream), "invert stage launch (write)");
  }
  HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (invert stage)");
  (void)hipEventElapsedTime(&out->ms_invert, ev_[0], ev_[3]);
  out->n_hits = total;
  out->d_hits = d_inv_hits_;
  out->d_aux = d_inv_aux_;
  return HG_OK;
}

// The context stage over a finished call (`out`: its final records, ordered by line, and its piece count; untouched): the
// count pass over the scan's tile states and the records' lines, an exclusive scan of the per-tile counts, and the write pass
// (hg_context.hip).  For an inverted call the records are the selected pieces, so their context is matching pieces.  Like
// the invert stage it runs once over the whole buffer, however many segments or pipeline chunks the scan took.
int HgScanner::context_pass(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, const HgContextParams &params, hipStream_t stream,
                            const HgScanOutput &out, HgContextOutput *ctx) {
  const uint64_t ntiles = (nbytes + HG_TILE_BYTES - 1) / HG_TILE_BYTES;
  ctx->owed_after = hg_context_owed(0, 0, line_base, out.n_pieces, params.after, params.carry_after);
  if (ntiles == 0) return HG_OK;
  if (ntiles + 2 > ctx_tiles_cap_) {
    const uint64_t cap = std::max<uint64_t>(ntiles + ntiles / 4 + 2, 4096);
    ctx_tiles_cap_ = 0;
    HG_TRY(realloc_dev(d_ctx_count_, cap, "d_ctx_count_"), "alloc (context stage)");
    HG_TRY(realloc_dev(d_ctx_pos_, cap, "d_ctx_pos_"), "alloc (context stage)");
    ctx_tiles_cap_ = cap;
  }
  size_t tb = 0;  // the scan's scratch, asked for the size that is scanned
  HG_TRY(rocprim::exclusive_scan(nullptr, tb, d_ctx_count_, d_ctx_pos_, uint64_t{0}, ntiles + 1, rocprim::plus<uint64_t>(), stream), "scan (context stage)");
  if (tb > ctx_temp_bytes_ || !d_ctx_temp_) {
    ctx_temp_bytes_ = 0;
    HG_TRY(realloc_dev(d_ctx_temp_, tb + tb / 4, "d_ctx_temp_"), "alloc (context stage)");
    ctx_temp_bytes_ = tb + tb / 4;
  }
  uint64_t *d_n_tail = d_ctx_count_ + ntiles + 1;  // (behind the scanned words)
  HgContextArgs a{text, nbytes, bs1, ntiles, hg_context_win(line_base, out.n_pieces, params.before, params.after, params.carry_after, params.tail),
                  d_sums_, d_bases_, out.d_hits, out.n_hits, d_ctx_count_, d_n_tail, d_ctx_pos_, nullptr, nullptr};
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_TRY(hipMemsetAsync(d_n_tail, 0, sizeof(uint64_t), stream), "memset (context stage)");
  HG_TRY(hg_context_launch(a, false, static_cast<uint32_t>(num_cus_), stream), "context stage launch (count)");
  HG_TRY(rocprim::exclusive_scan(d_ctx_temp_, tb, d_ctx_count_, d_ctx_pos_, uint64_t{0}, ntiles + 1, rocprim::plus<uint64_t>(), stream), "scan (context stage)");
  uint64_t total = 0, n_tail = 0, last_line = 0;
  HG_TRY(hipMemcpyAsync(&total, d_ctx_pos_ + ntiles, sizeof total, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipMemcpyAsync(&n_tail, d_n_tail, sizeof n_tail, hipMemcpyDeviceToHost, stream), "copy count");
  if (out.n_hits) HG_TRY(hipMemcpyAsync(&last_line, &out.d_hits[out.n_hits - 1].line_no, sizeof last_line, hipMemcpyDeviceToHost, stream), "copy last line");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (context stage)");
  if (total > out.n_pieces || n_tail > total) return error(HG_ERR_HIP, "the context stage counted more pieces than the buffer has");
  if (total > ctx_cap_) {
    const uint64_t cap = std::max<uint64_t>(total + total / 4, 4096);
    ctx_cap_ = 0;
    HG_TRY(realloc_dev(d_ctx_hits_, cap, "d_ctx_hits_"), "alloc (context stage records)");
    HG_TRY(realloc_dev(d_ctx_aux_, cap, "d_ctx_aux_"), "alloc (context stage records)");
    ctx_cap_ = cap;
  }
  if (total) {
    a.out_hits = d_ctx_hits_;
    a.out_aux = d_ctx_aux_;
    HG_TRY(hg_context_launch(a, true, static_cast<uint32_t>(num_cus_), stream), "context stage launch (write)");
  }
  HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (context stage)");
  (void)hipEventElapsedTime(&ctx->ms_context, ev_[0], ev_[3]);
  ctx->n_context = total;
  ctx->n_tail = n_tail;
  ctx->owed_after = hg_context_owed(out.n_hits, last_line, line_base, out.n_pieces, params.after, params.carry_after);
  ctx->d_hits = d_ctx_hits_;
  ctx->d_aux = d_ctx_aux_;
  return HG_OK;
}

int HgScanner::scan_context(const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, hipStream_t stream, const HgContextParams &params, bool invert,
                            HgScanOutput *out, HgContextOutput *ctx) {
  if (!ctx) return error(HG_ERR_ARG, "invalid arguments");
  *ctx = HgContextOutput{};
  if (int rc = scan_impl(d_text, nbytes, buffer_size, line_base, false, invert, stream, out)) return rc;
  if (!params.any()) return HG_OK;  // no context asked for: the stage is skipped
  return context_pass(static_cast<const uint8_t *>(d_text), nbytes, static_cast<uint64_t>(buffer_size) - 1, line_base, params, stream, *out, ctx);
}

// The parts stage over a finished scan (`out`: its final hits, ordered by line; untouched): the count pass over the hits (a
// wave per piece that has a hit walks it), an exclusive scan of the per-hit counts, and the write pass (hg_parts.hip).  Like
// the invert stage it runs once over the whole buffer, however many segments or pipeline chunks the scan took.
int HgScanner::parts_pass(const uint8_t *text, hipStream_t stream, const HgScanOutput &out, HgPartsOutput *parts) {
  const uint64_t n = out.n_hits;
  if (n == 0) return HG_OK;
  size_t tb = 0;
  if (int rc = parts_alloc(n, &tb, stream)) return rc;
  const HgDb &db = *db_;
  const uint32_t npatterns = static_cast<uint32_t>(db.patterns.size()), first_words = (npatterns + 31) / 32;
  HgPartsArgs a{text, out.d_hits, out.d_aux, n, static_cast<const HgPattern *>(d_patterns_), static_cast<const uint32_t *>(d_pool_),
                npatterns, d_parts_first_, first_words, d_parts_count_, d_parts_pos_, nullptr, nullptr};
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_TRY(hg_parts_launch(a, false, db.max_nw, static_cast<uint32_t>(num_cus_), stream), "parts stage launch (count)");
  HG_TRY(rocprim::exclusive_scan(d_parts_temp_, tb, d_parts_count_, d_parts_pos_, uint64_t{0}, n + 1, rocprim::plus<uint64_t>(), stream), "scan (parts stage)");
  uint64_t total = 0;
  HG_TRY(hipMemcpyAsync(&total, d_parts_pos_ + n, sizeof total, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (parts stage)");
  if (int rc = parts_records(total)) return rc;
  if (total) {
    a.out = d_parts_;
    a.out_pattern = d_part_pattern_;
    HG_TRY(hg_parts_launch(a, true, db.max_nw, static_cast<uint32_t>(num_cus_), stream), "parts stage launch (write)");
  }
  HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (parts stage)");
  (void)hipEventElapsedTime(&parts->ms_parts, ev_[0], ev_[3]);
  parts->n_parts = total;
  parts->d_parts = d_parts_;
  parts->d_pattern = d_part_pattern_;
  return HG_OK;
}

// What the parts stage and the per-file parts stage share, for n records: the per-record counts and their scan, the scan's
// scratch (*tb: its size for n + 1 entries) and the first-byte bitmap over the expressions, built once per scanner.
int HgScanner::parts_alloc(uint64_t n, size_t *tb_out, hipStream_t stream) {
  if (n + 1 > parts_hits_cap_) {
    const uint64_t cap = std::max<uint64_t>(n + n / 4 + 1, 4096);
    parts_hits_cap_ = 0;
    HG_TRY(realloc_dev(d_parts_count_, cap, "d_parts_count_"), "alloc (parts stage)");
    HG_TRY(realloc_dev(d_parts_pos_, cap, "d_parts_pos_"), "alloc (parts stage)");
    parts_hits_cap_ = cap;
  }
  size_t tb = 0;  // the scan's scratch, asked for the size that is scanned
  HG_TRY(rocprim::exclusive_scan(nullptr, tb, d_parts_count_, d_parts_pos_, uint64_t{0}, n + 1, rocprim::plus<uint64_t>(), stream), "scan (parts stage)");
  if (tb > parts_temp_bytes_ || !d_parts_temp_) {
    parts_temp_bytes_ = 0;
    HG_TRY(realloc_dev(d_parts_temp_, tb + tb / 4, "d_parts_temp_"), "alloc (parts stage)");
    parts_temp_bytes_ = tb + tb / 4;
  }
  *tb_out = tb;
  if (!d_parts_first_) {  // which expressions can start with byte c: those whose init meets reach[c] (conditions left out: a superset)
    const HgDb &db = *db_;
    const uint32_t npatterns = static_cast<uint32_t>(db.patterns.size()), first_words = (npatterns + 31) / 32;
    std::vector<uint32_t> first(static_cast<size_t>(256) * first_words, 0u);
    for (uint32_t j = 0; j < npatterns; j++) {
      const HgPattern &p = db.patterns[j];
      if (p.nw == 0 || p.nw > HG_MAX_W) continue;
      const uint32_t *init = db.pool.data() + p.init_off, *reach = db.pool.data() + p.reach_off;
      for (uint32_t c = 0; c < 256; c++) {
        uint32_t any = 0;
        for (uint32_t w = 0; w < p.nw; w++) any |= init[w] & reach[c * p.nw + w];
        if (any) first[static_cast<size_t>(c) * first_words + (j >> 5)] |= 1u << (j & 31);
      }
    }
    HG_TRY(realloc_dev(d_parts_first_, first.size(), "d_parts_first_"), "alloc (parts stage)");
    HG_TRY(hipMemcpyAsync(d_parts_first_, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream), "copy (parts stage)");
    HG_TRY(hipStreamSynchronize(stream), "stream sync (parts stage)");  // (the host vector goes out of scope)
  }
  return HG_OK;
}

// Room for `total` parts with their expressions.
int HgScanner::parts_records(uint64_t total) {
  if (total > parts_cap_) {
    const uint64_t cap = std::max<uint64_t>(total + total / 4, 4096);
    parts_cap_ = 0;
    HG_TRY(realloc_dev(d_parts_, cap, "d_parts_"), "alloc (parts stage records)");
    HG_TRY(realloc_dev(d_part_pattern_, cap, "d_part_pattern_"), "alloc (parts stage records)");
    parts_cap_ = cap;
  }
  return HG_OK;
}

int HgScanner::scan_parts(const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, hipStream_t stream, HgScanOutput *out, HgPartsOutput *parts) {
  if (!parts) return error(HG_ERR_ARG, "invalid arguments");
  *parts = HgPartsOutput{};
  if (const char *why = hg_parts_refusal(db_->nhuge, db_->ncomb, db_->nquiet, db_->n_ext != 0)) return error(HG_ERR_ARG, why);
  if (int rc = scan_impl(d_text, nbytes, buffer_size, line_base, false, false, stream, out)) return rc;
  return parts_pass(static_cast<const uint8_t *>(d_text), stream, *out, parts);
}

// The per-segment arrays of the segment stage, for n_seg segments (n_seg + 1 words each).
int HgScanner::segment_alloc(uint64_t n_seg) {
  if (n_seg + 1 > seg_cap_) {
    const uint64_t cap = std::max<uint64_t>(n_seg + n_seg / 4 + 1, 4096);
    seg_cap_ = 0;
    HG_TRY(realloc_dev(d_segw_, 7 * cap, "d_segw_"), "alloc (segment stage)");
    seg_cap_ = cap;
  }
  if (!d_seg_flag_) HG_TRY(realloc_dev(d_seg_flag_, 4, "d_seg_flag_"), "alloc (segment stage)");
  size_t tb = 0;
  HG_TRY(rocprim::exclusive_scan(nullptr, tb, d_segw_, d_segw_, uint64_t{0}, n_seg + 1, rocprim::plus<uint64_t>(), hipStream_t(nullptr)), "scan (segment stage)");
  if (tb > seg_temp_bytes_ || !d_seg_temp_) {
    seg_temp_bytes_ = 0;
    HG_TRY(realloc_dev(d_seg_temp_, tb + tb / 4, "d_seg_temp_"), "alloc (segment stage)");
    seg_temp_bytes_ = tb + tb / 4;
  }
  return HG_OK;
}

// Room for n compacted records (with their segments and starts of match).
int HgScanner::segment_records(uint64_t n) {
  if (n > seg_rec_cap_) {
    const uint64_t cap = std::max<uint64_t>(n + n / 4, 4096);
    seg_rec_cap_ = 0;
    HG_TRY(realloc_dev(d_seg_hits_, cap, "d_seg_hits_"), "alloc (segment stage records)");
    HG_TRY(realloc_dev(d_seg_aux_, cap, "d_seg_aux_"), "alloc (segment stage records)");
    HG_TRY(realloc_dev(d_seg_of_, cap, "d_seg_of_"), "alloc (segment stage records)");
    HG_TRY(realloc_dev(d_seg_from_, cap, "d_seg_from_"), "alloc (segment stage records)");
    seg_rec_cap_ = cap;
  }
  return HG_OK;
}

// The pad filter of an inverted call, between the scan and the invert stage: the hits whose scanned bytes begin in a pad
// belong to no file and must not deselect a piece (hg_seg_pad_hit).  Flags, their exclusive scan, an ordered write; *out
// then describes the remaining hits (in the stage's record arrays: the invert stage reads them and writes its own).
int HgScanner::pad_filter(const HgSegArgs &checked, float *ms, hipStream_t stream, HgScanOutput *out) {
  const uint64_t n = out->n_hits;
  out->d_from = nullptr;
  if (!n) return HG_OK;
  if (int rc = segment_records(n)) return rc;
  if (n + 1 > pad_cap_) {
    const uint64_t cap = std::max<uint64_t>(n + n / 4 + 1, 4096);
    pad_cap_ = 0;
    HG_TRY(realloc_dev(d_pad_keep_, cap, "d_pad_keep_"), "alloc (pad filter)");
    HG_TRY(realloc_dev(d_pad_pos_, cap, "d_pad_pos_"), "alloc (pad filter)");
    pad_cap_ = cap;
  }
  size_t tb = 0;
  HG_TRY(rocprim::exclusive_scan(nullptr, tb, d_pad_keep_, d_pad_pos_, uint64_t{0}, n + 1, rocprim::plus<uint64_t>(), hipStream_t(nullptr)), "scan (pad filter)");
  if (tb > seg_temp_bytes_ || !d_seg_temp_) {
    seg_temp_bytes_ = 0;
    HG_TRY(realloc_dev(d_seg_temp_, tb + tb / 4, "d_seg_temp_"), "alloc (pad filter)");
    seg_temp_bytes_ = tb + tb / 4;
  }
  HgSegArgs a = checked;
  a.hits = out->d_hits;
  a.aux = out->d_aux;
  a.n_hits = n;
  a.pad_keep = d_pad_keep_;
  a.pad_pos = d_pad_pos_;
  a.out_hits = d_seg_hits_;
  a.out_aux = d_seg_aux_;
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_TRY(hg_segments_launch(a, HgSegStep::PadFlag, static_cast<uint32_t>(num_cus_), stream), "pad filter launch (flags)");
  HG_TRY(rocprim::exclusive_scan(d_seg_temp_, tb, d_pad_keep_, d_pad_pos_, uint64_t{0}, n + 1, rocprim::plus<uint64_t>(), stream), "scan (pad filter)");
  HG_TRY(hg_segments_launch(a, HgSegStep::PadWrite, static_cast<uint32_t>(num_cus_), stream), "pad filter launch (write)");
  uint64_t total = 0;
  HG_TRY(hipMemcpyAsync(&total, d_pad_pos_ + n, sizeof total, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (pad filter)");
  if (total > n) return error(HG_ERR_HIP, "the pad filter kept more hits than the scan has");
  float t = 0;
  (void)hipEventElapsedTime(&t, ev_[0], ev_[3]);
  *ms += t;
  out->n_hits = total;
  out->d_hits = d_seg_hits_;
  out->d_aux = d_seg_aux_;
  return HG_OK;
}

// The segment stage over a finished call (*out: its final records, ordered by line, with their starts of match if any): the
// segments' line bases from the scan's tile states (a wave per tile that holds a boundary), their runs of surviving records,
// an exclusive scan of the runs' lengths, and the ordered write of the file-relative records (hg_segments.hip).  *out then
// describes the surviving records; its counters and timings stay the packed scan's.
int HgScanner::segment_pass(const HgSegArgs &checked, float ms_check, hipStream_t stream, HgScanOutput *out, HgSegOutput *seg) {
  HgSegArgs a = checked;
  a.end_piece = out->n_pieces;
  a.sums = d_sums_;  // (the scan may have grown them: taken after it)
  a.bases = d_bases_;
  a.hits = out->d_hits;
  a.aux = out->d_aux;
  a.from = out->d_from;
  a.n_hits = out->n_hits;
  if (int rc = segment_records(out->n_hits)) return rc;
  a.out_hits = d_seg_hits_;
  a.out_aux = d_seg_aux_;
  a.out_seg = d_seg_of_;
  a.out_from = d_seg_from_;
  size_t tb = seg_temp_bytes_;
  uint64_t *first = const_cast<uint64_t *>(a.first);
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_TRY(hg_segments_launch(a, HgSegStep::Bases, static_cast<uint32_t>(num_cus_), stream), "segment stage launch (bases)");
  HG_TRY(hg_segments_launch(a, HgSegStep::Runs, static_cast<uint32_t>(num_cus_), stream), "segment stage launch (runs)");
  HG_TRY(rocprim::exclusive_scan(d_seg_temp_, tb, a.kept, first, uint64_t{0}, a.n_seg + 1, rocprim::plus<uint64_t>(), stream), "scan (segment stage)");
  HG_TRY(hg_segments_launch(a, HgSegStep::Write, static_cast<uint32_t>(num_cus_), stream), "segment stage launch (write)");
  uint64_t total = 0;
  HG_TRY(hipMemcpyAsync(&total, first + a.n_seg, sizeof total, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (segment stage)");
  if (total > out->n_hits) return error(HG_ERR_HIP, "the segment stage kept more records than the scan has");
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ev_[0], ev_[3]);
  seg_last_ = a;  // (what a per-file context stage behind this pass reads: the packed records stay where they are)
  seg->ms_segments = ms_check + ms;
  seg->d_record_segment = d_seg_of_;
  seg->d_first_record = a.first;
  seg->d_n_lines = a.n_lines;
  seg->d_n_selected = a.n_selected;
  out->n_hits = total;
  out->d_hits = d_seg_hits_;
  out->d_aux = d_seg_aux_;
  if (out->d_from) out->d_from = d_seg_from_;
  return HG_OK;
}

int HgScanner::scan_packed(const void *d_text, uint64_t nbytes, int buffer_size, hipStream_t stream, const HgSegParams &params, bool invert, HgScanOutput *out,
                           HgSegOutput *seg) {
  if (!out || !seg || (!d_text && nbytes) || buffer_size < 2 || (params.n_seg && (!params.d_seg_start || !params.d_seg_end)))
    return error(HG_ERR_ARG, "invalid arguments");
  if ((reinterpret_cast<uintptr_t>(d_text) & 15u) != 0) return error(HG_ERR_ARG, "text pointer must be 16-byte aligned");
  *seg = HgSegOutput{};
  HG_TRY(hipSetDevice(device_), "hipSetDevice");
  const uint64_t n_seg = params.n_seg;
  if (int rc = segment_alloc(n_seg)) return rc;
  HgSegArgs a{};
  a.text = static_cast<const uint8_t *>(d_text);
  a.nbytes = nbytes;
  a.bs1 = static_cast<uint64_t>(buffer_size) - 1;
  a.ntiles = (nbytes + HG_TILE_BYTES - 1) / HG_TILE_BYTES;
  a.seg_start = params.d_seg_start;
  a.seg_end = params.d_seg_end;
  a.n_seg = n_seg;
  a.limit = params.max_per_segment;
  a.invert = invert ? 1u : 0u;
  a.flag = d_seg_flag_;
  a.B = d_segw_;
  a.E = d_segw_ + seg_cap_;
  a.r0 = d_segw_ + 2 * seg_cap_;
  a.kept = d_segw_ + 3 * seg_cap_;
  a.first = d_segw_ + 4 * seg_cap_;
  a.n_lines = d_segw_ + 5 * seg_cap_;
  a.n_selected = d_segw_ + 6 * seg_cap_;
  // the argument check comes first: malformed segments scan nothing
  uint32_t bad = 0;
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_TRY(hipMemsetAsync(d_seg_flag_, 0, sizeof(uint32_t), stream), "memset (segment stage)");
  HG_TRY(hg_segments_launch(a, HgSegStep::Check, static_cast<uint32_t>(num_cus_), stream), "segment stage launch (check)");
  HG_TRY(hipMemcpyAsync(&bad, d_seg_flag_, sizeof bad, hipMemcpyDeviceToHost, stream), "copy flag");
  HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (segment check)");
  if (bad)
    return error(HG_ERR_ARG, bad & HG_SEG_BAD_ORDER ? "segments are not ascending or overlap"
                             : bad & HG_SEG_BAD_END ? "a segment ends past the buffer"
                                                    : "a segment does not start at a line start");
  float ms_check = 0;
  (void)hipEventElapsedTime(&ms_check, ev_[0], ev_[3]);
  // an inverted call: the plain scan, the pad filter, then the invert stage on the hits that belong to a file
  if (int rc = scan_impl(d_text, nbytes, buffer_size, 0, false, false, stream, out)) return rc;
  if (invert) {
    if (int rc = pad_filter(a, &ms_check, stream, out)) return rc;
    if (int rc = invert_pass(a.text, nbytes, a.bs1, 0, stream, out)) return rc;
  }
  return segment_pass(a, ms_check, stream, out, seg);
}

// The per-file context stage over a finished segment pass (`out`: the surviving records, file-relative; seg_last_: the packed
// records and the per-segment arrays they came from; all untouched): the surviving records' packed piece numbers and their segments'
// windows, the per-tile counts from those alone, their exclusive scan, the ordered write pass over the tiles that hold
// context, and the records made file-relative with their segments and per-segment offsets (hg_segctx.hip).  It shares the
// context stage's per-tile and record buffers: a scanner runs one of the two per call.  Two host synchronisations, as in
// context_pass: the one that sizes the output, and the one behind the write that the stage's time is read after.
int HgScanner::segctx_pass(uint32_t before, uint32_t after, hipStream_t stream, const HgScanOutput &out, HgContextOutput *ctx, HgSegCtxOutput *sc) {
  const HgSegArgs &g = seg_last_;
  const uint64_t ntiles = g.ntiles, n_seg = g.n_seg;
  if (n_seg + 1 > segctx_seg_cap_) {
    const uint64_t cap = std::max<uint64_t>(n_seg + n_seg / 4 + 1, 4096);
    segctx_seg_cap_ = 0;
    HG_TRY(realloc_dev(d_segctx_first_, cap, "d_segctx_first_"), "alloc (per-file context stage)");
    segctx_seg_cap_ = cap;
  }
  uint64_t *d_first = d_segctx_first_;
  sc->d_first_context = d_first;
  if ((!before && !after) || ntiles == 0 || out.n_hits == 0) {  // no context asked for, or no record to have any: the stage is skipped
    HG_TRY(hipMemsetAsync(d_first, 0, (n_seg + 1) * sizeof(uint64_t), stream), "memset (per-file context stage)");
    HG_TRY(hipStreamSynchronize(stream), "stream sync (per-file context stage)");
    return HG_OK;
  }
  if (ntiles + 2 > ctx_tiles_cap_) {
    const uint64_t cap = std::max<uint64_t>(ntiles + ntiles / 4 + 2, 4096);
    ctx_tiles_cap_ = 0;
    HG_TRY(realloc_dev(d_ctx_count_, cap, "d_ctx_count_"), "alloc (context stage)");
    HG_TRY(realloc_dev(d_ctx_pos_, cap, "d_ctx_pos_"), "alloc (context stage)");
    ctx_tiles_cap_ = cap;
  }
  size_t tb = 0;  // the scan's scratch, asked for the size that is scanned
  HG_TRY(rocprim::exclusive_scan(nullptr, tb, d_ctx_count_, d_ctx_pos_, uint64_t{0}, ntiles + 1, rocprim::plus<uint64_t>(), stream), "scan (per-file context stage)");
  if (tb > ctx_temp_bytes_ || !d_ctx_temp_) {
    ctx_temp_bytes_ = 0;
    HG_TRY(realloc_dev(d_ctx_temp_, tb + tb / 4, "d_ctx_temp_"), "alloc (context stage)");
    ctx_temp_bytes_ = tb + tb / 4;
  }
  if (out.n_hits > segctx_k_cap_) {
    const uint64_t cap = std::max<uint64_t>(out.n_hits + out.n_hits / 4, 4096);
    segctx_k_cap_ = 0;
    HG_TRY(realloc_dev(d_segctx_k_, cap, "d_segctx_k_"), "alloc (per-file context stage)");
    HG_TRY(realloc_dev(d_segctx_win_, cap, "d_segctx_win_"), "alloc (per-file context stage)");
    segctx_k_cap_ = cap;
  }
  HgSegCtxArgs a{};
  a.text = g.text;
  a.nbytes = g.nbytes;
  a.bs1 = g.bs1;
  a.ntiles = ntiles;
  a.end_piece = g.end_piece;
  a.before = before;
  a.after = after;
  a.sums = g.sums;
  a.bases = g.bases;
  a.hits = g.hits;
  a.aux = g.aux;
  a.n_hits = g.n_hits;
  a.seg_start = g.seg_start;
  a.seg_end = g.seg_end;
  a.n_seg = n_seg;
  a.limit = g.limit;
  a.invert = g.invert;
  a.B = g.B;
  a.E = g.E;
  a.r0 = g.r0;
  a.kept = g.kept;
  a.seg_hits = out.d_hits;
  a.seg_of = d_seg_of_;
  a.n_kept = out.n_hits;
  a.K = d_segctx_k_;
  a.W = d_segctx_win_;
  a.count = d_ctx_count_;
  a.pos = d_ctx_pos_;
  a.first_ctx = d_first;
  const uint32_t cus = static_cast<uint32_t>(num_cus_);
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_TRY(hg_segctx_launch(a, HgSegCtxStep::Prep, cus, stream), "per-file context stage launch (prepare)");
  HG_TRY(hg_segctx_launch(a, HgSegCtxStep::Count, cus, stream), "per-file context stage launch (count)");
  HG_TRY(rocprim::exclusive_scan(d_ctx_temp_, tb, d_ctx_count_, d_ctx_pos_, uint64_t{0}, ntiles + 1, rocprim::plus<uint64_t>(), stream), "scan (per-file context stage)");
  uint64_t total = 0;
  HG_TRY(hipMemcpyAsync(&total, d_ctx_pos_ + ntiles, sizeof total, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (per-file context stage)");
  if (total > g.end_piece) return error(HG_ERR_HIP, "the per-file context stage counted more pieces than the buffer has");
  if (total > ctx_cap_) {
    const uint64_t cap = std::max<uint64_t>(total + total / 4, 4096);
    ctx_cap_ = 0;
    HG_TRY(realloc_dev(d_ctx_hits_, cap, "d_ctx_hits_"), "alloc (context stage records)");
    HG_TRY(realloc_dev(d_ctx_aux_, cap, "d_ctx_aux_"), "alloc (context stage records)");
    ctx_cap_ = cap;
  }
  if (total > segctx_of_cap_) {
    const uint64_t cap = std::max<uint64_t>(total + total / 4, 4096);
    segctx_of_cap_ = 0;
    HG_TRY(realloc_dev(d_segctx_of_, cap, "d_segctx_of_"), "alloc (per-file context stage records)");
    segctx_of_cap_ = cap;
  }
  a.n_ctx = total;
  a.out_hits = d_ctx_hits_;
  a.out_aux = d_ctx_aux_;
  a.out_seg = d_segctx_of_;
  if (total) {
    HG_TRY(hg_segctx_launch(a, HgSegCtxStep::Write, cus, stream), "per-file context stage launch (write)");
    HG_TRY(hg_segctx_launch(a, HgSegCtxStep::Map, cus, stream), "per-file context stage launch (map)");
  }
  HG_TRY(hg_segctx_launch(a, HgSegCtxStep::First, cus, stream), "per-file context stage launch (offsets)");
  HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (per-file context stage)");
  (void)hipEventElapsedTime(&ctx->ms_context, ev_[0], ev_[3]);
  ctx->n_context = total;
  ctx->d_hits = d_ctx_hits_;
  ctx->d_aux = d_ctx_aux_;
  sc->d_context_segment = d_segctx_of_;
  return HG_OK;
}

int HgScanner::scan_packed_context(const void *d_text, uint64_t nbytes, int buffer_size, hipStream_t stream, const HgSegParams &params, uint32_t before,
                                   uint32_t after, bool invert, HgScanOutput *out, HgSegOutput *seg, HgContextOutput *ctx, HgSegCtxOutput *sc) {
  if (!ctx || !sc) return error(HG_ERR_ARG, "invalid arguments");
  *ctx = HgContextOutput{};
  *sc = HgSegCtxOutput{};
  if (int rc = scan_packed(d_text, nbytes, buffer_size, stream, params, invert, out, seg)) return rc;
  return segctx_pass(before, after, stream, *out, ctx, sc);
}

// The per-file parts stage over a finished segment pass (`out`: the surviving records, file-relative, untouched; d_seg_of_:
// their segments; seg_last_: the caller's segment arrays and first_record): the count pass over the surviving records where
// they lie (a wave per piece a file keeps a record of), an exclusive scan of the per-record counts, the write pass with each
// part's segment beside it, and first_part from the scan and first_record (hg_segparts.hip).  No packed copy of the records
// and no second pass over the parts.  It shares the parts stage's count, scan, bitmap and record buffers: a scanner runs one
// of the two per call.  One host synchronisation sizes the output, one behind the write is where the stage's time is read.
int HgScanner::segparts_pass(hipStream_t stream, const HgScanOutput &out, HgPartsOutput *parts, HgSegPartsOutput *sp) {
  const HgSegArgs &g = seg_last_;
  const uint64_t n = out.n_hits, n_seg = g.n_seg;
  if (n_seg + 1 > segparts_seg_cap_) {
    const uint64_t cap = std::max<uint64_t>(n_seg + n_seg / 4 + 1, 4096);
    segparts_seg_cap_ = 0;
    HG_TRY(realloc_dev(d_segparts_first_, cap, "d_segparts_first_"), "alloc (per-file parts stage)");
    segparts_seg_cap_ = cap;
  }
  sp->d_first_part = d_segparts_first_;
  if (n == 0) {  // no record, no part
    HG_TRY(hipMemsetAsync(d_segparts_first_, 0, (n_seg + 1) * sizeof(uint64_t), stream), "memset (per-file parts stage)");
    HG_TRY(hipStreamSynchronize(stream), "stream sync (per-file parts stage)");
    return HG_OK;
  }
  size_t tb = 0;
  if (int rc = parts_alloc(n, &tb, stream)) return rc;
  const HgDb &db = *db_;
  const uint32_t npatterns = static_cast<uint32_t>(db.patterns.size()), cus = static_cast<uint32_t>(num_cus_);
  HgSegPartsArgs a{};
  a.text = g.text;
  a.hits = out.d_hits;
  a.aux = out.d_aux;
  a.seg_of = d_seg_of_;
  a.n_hits = n;
  a.seg_start = g.seg_start;
  a.first_record = g.first;
  a.n_seg = n_seg;
  a.patterns = static_cast<const HgPattern *>(d_patterns_);
  a.pool = static_cast<const uint32_t *>(d_pool_);
  a.npatterns = npatterns;
  a.first = d_parts_first_;
  a.first_words = (npatterns + 31) / 32;
  a.count = d_parts_count_;
  a.pos = d_parts_pos_;
  a.first_part = d_segparts_first_;
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_TRY(hg_segparts_launch(a, HgSegPartsStep::Count, db.max_nw, cus, stream), "per-file parts stage launch (count)");
  HG_TRY(rocprim::exclusive_scan(d_parts_temp_, tb, d_parts_count_, d_parts_pos_, uint64_t{0}, n + 1, rocprim::plus<uint64_t>(), stream), "scan (per-file parts stage)");
  uint64_t total = 0;
  HG_TRY(hipMemcpyAsync(&total, d_parts_pos_ + n, sizeof total, hipMemcpyDeviceToHost, stream), "copy count");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (per-file parts stage)");
  if (int rc = parts_records(total)) return rc;
  if (total > segparts_of_cap_) {
    const uint64_t cap = std::max<uint64_t>(total + total / 4, 4096);
    segparts_of_cap_ = 0;
    HG_TRY(realloc_dev(d_segparts_of_, cap, "d_segparts_of_"), "alloc (per-file parts stage records)");
    segparts_of_cap_ = cap;
  }
  if (total) {
    a.out = d_parts_;
    a.out_pattern = d_part_pattern_;
    a.out_seg = d_segparts_of_;
    HG_TRY(hg_segparts_launch(a, HgSegPartsStep::Write, db.max_nw, cus, stream), "per-file parts stage launch (write)");
  }
  HG_TRY(hg_segparts_launch(a, HgSegPartsStep::First, db.max_nw, cus, stream), "per-file parts stage launch (offsets)");
  HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (per-file parts stage)");
  (void)hipEventElapsedTime(&parts->ms_parts, ev_[0], ev_[3]);
  parts->n_parts = total;
  parts->d_parts = d_parts_;
  parts->d_pattern = d_part_pattern_;
  sp->d_part_segment = d_segparts_of_;
  return HG_OK;
}

int HgScanner::scan_packed_parts(const void *d_text, uint64_t nbytes, int buffer_size, hipStream_t stream, const HgSegParams &params, HgScanOutput *out,
                                 HgSegOutput *seg, HgPartsOutput *parts, HgSegPartsOutput *sp) {
  if (!parts || !sp) return error(HG_ERR_ARG, "invalid arguments");
  *parts = HgPartsOutput{};
  *sp = HgSegPartsOutput{};
  if (const char *why = hg_parts_refusal(db_->nhuge, db_->ncomb, db_->nquiet, db_->n_ext != 0)) return error(HG_ERR_ARG, why);
  if (int rc = scan_packed(d_text, nbytes, buffer_size, stream, params, false, out, seg)) return rc;  // (the segment check comes before its scan)
  return segparts_pass(stream, *out, parts, sp);
}

int HgScanner::run_once(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, const PassRange &range, bool block_mode, hipStream_t stream,
                        HgScanOutput *out) {
  // (the first pass that streams asks how many stream workgroups a CU holds)
  if (range.tile_hi > range.tile_lo && stream_wgs_per_cu_ == 0) stream_wgs_per_cu_ = hg_stream_blocks_per_cu(db_->filter_log2, db_->filter_wide, db_->dense);
  PassPlan p = plan_pass(text, nbytes, bs1, line_base, range, block_mode, stream);
  HG_TRY(hipEventRecord(ev_[0], stream), "event");
  if (p.ntiles && !fin_fallback_ && p.fin_nb > fin_alloc_)
    if (int rc = alloc_fin(p.fin_nb, stream)) return rc;
  p.bucketed = p.bucketed && d_fin_fill_;
  p.ca.bucket_cap = p.bucketed ? p.fin_cap : 0u;
  p.ca.bucket_fill = d_fin_fill_;
  fin_info_ = FinInfo{p.bucketed ? 1u : 0u, p.fin_shift, p.fin_nb, p.fin_cap, p.id_bits, p.to_bits, 0, 0, 0};
  // one launch puts the device state in place (counters, cursors, finalize totals, tile-scan state, bucket fill levels, the
  // first chunk's verified-occurrence counts)
  hipLaunchKernelGGL(hg_reset_kernel, dim3(std::max<uint32_t>(1, std::min<uint32_t>((p.fin_nb + 255) / 256, 256))), dim3(256), 0, stream, d_counters_, static_cast<uint32_t>(HG_ST_ZERO_WORDS), d_final_,
                     range.cs0, range.piece0, d_fin_fill_, p.bucketed ? p.fin_nb : 0u, d_defer_count_, static_cast<uint32_t>(HG_CONFIRM_MODES * HG_DEFER_SHARDS));
  HG_TRY(hipGetLastError(), "reset launch");
  if (p.split) return HG_SPLIT;
  out->stream_launches = p.ntiles ? p.nchunks : 0;  // (run_fitting hands in a zeroed output)
  if (p.ntiles) {
    if (p.piped && !ev_side_done_[0])
      for (int i = 0; i < kMaxChunks; i++) {
        HG_TRY(hipEventCreate(&ev_k1_begin_[i]), "hipEventCreate");
        HG_TRY(hipEventCreate(&ev_k1_end_[i]), "hipEventCreate");
        HG_TRY(hipEventCreate(&ev_side_done_[i]), "hipEventCreate");  // (timed: which of stream pass / side passes ends later, below)
      }
    if (p.piped) {  // side stream starts after the counters / state are in place
      HG_TRY(hipEventRecord(ev_side_done_[kMaxChunks - 1], stream), "event");
      HG_TRY(hipStreamWaitEvent(p.side, ev_side_done_[kMaxChunks - 1], 0), "stream wait");
    }
    for (uint32_t c = 0; c < p.nchunks; c++) {
      if (p.piped && c >= 2) HG_TRY(hipStreamWaitEvent(stream, ev_side_done_[c - 2], 0), "stream wait");  // buffer set is free again
      if (int rc = launch_stream(p, c, out)) return rc;
      if (int rc = launch_side(p, c)) return rc;
      if (p.bucketed && c + 1 == p.nchunks)  // the side passes of the last chunk are queued: order what is left
        if (int rc = finalize_last(p, c)) return rc;
      if (p.piped) HG_TRY(hipEventRecord(ev_side_done_[c], p.side), "event");
    }
    if (p.piped) HG_TRY(hipStreamWaitEvent(stream, ev_side_done_[p.nchunks - 1], 0), "stream wait");
  } else {
    HG_TRY(hipEventRecord(ev_[1], stream), "event");
    HG_TRY(hipEventRecord(ev_[2], stream), "event");
  }
  HG_TRY(hipMemcpyAsync(h_counters_, d_counters_, HG_ST_WORDS * 4, hipMemcpyDeviceToHost, stream), "copy state");  // the whole state block in one copy
  if (p.bucketed) HG_TRY(hipEventRecord(ev_[3], stream), "event");
  HG_TRY(hipStreamSynchronize(stream), "stream sync (scan kernels)");
  if (p.piped) {
    // Which half of the pipeline set the pace: did the side passes of chunk c - 1 end after the stream launch of chunk c?
    // (config 5: yes — 42 M candidates per pass.)  Then the side stream has no idle window for the next pass to use.
    uint32_t late = 0;
    for (uint32_t c = 0; c < p.nchunks; c++) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, ev_k1_begin_[c], ev_k1_end_[c]);
      out->ms_stream += ms;
      if (c >= 1 && hipEventElapsedTime(&ms, ev_k1_end_[c], ev_side_done_[c - 1]) == hipSuccess && ms > 0) late++;
    }
    side_bound_ = late * 2 > p.nchunks - 1;
  }

  out->joiner_tiles = h_counters_[HG_CNT_JOIN_TILES];
  const uint64_t n_raw = p.bucketed ? h_counters_[HG_ST_FIN_TOTAL + 1] : h_counters_[HG_CNT_HITS];
  if (int rc = regrow(p, n_raw)) return rc;
  fin_expect_hits_ = n_raw;
  // (a pass that stops short of the text's end leaves no piece count: scan_segments takes it from its last pass)
  const uint64_t n_pieces = block_mode ? 1 : !range.last ? 0 : h_final_->L - line_base + (nbytes > h_final_->cs ? hg_pieces(nbytes - h_final_->cs, bs1) : 0);
  uint32_t n = static_cast<uint32_t>(n_raw);
  const HgHit *fin_hits = d_hits_raw_;
  const HgHitAux *fin_aux = d_aux_raw_;
  if (n && d_min_lengths_) {  // min_length applies before the report rules: the finalize sees the surviving raw reports only
    if (int rc = minlen_pass(text, &n, p.stream)) return rc;
    fin_hits = d_minlen_hits_;
    fin_aux = d_minlen_aux_;
  }
  const uint64_t line_bound = line_base + (range.last ? n_pieces : nbytes) + 1;
  if (!p.bucketed) fin_info_.path = compact_key_packed(line_bound, p.id_bits, p.to_bits) ? 2u : 3u;
  if (n && !p.bucketed)
    if (int rc = finalize_compact(fin_hits, fin_aux, n, p.id_bits, p.to_bits, line_bound, p.stream)) return rc;
  if (!p.bucketed) {
    HG_TRY(hipEventRecord(ev_[3], stream), "event");
    HG_TRY(hipStreamSynchronize(stream), "stream sync (finalize)");
  }
  out->n_hits = !n ? 0 : p.bucketed ? h_counters_[HG_ST_FIN_TOTAL] : h_counters_[HG_ST_SELECTED];
  out->n_pieces = n_pieces;
  out->n_cands = h_counters_[HG_CNT_CANDS];
  out->n_raw_hits = n_raw;
  out->d_hits = d_hits_out_;
  out->d_aux = d_aux_out_;
  if (out->ms_stream == 0) (void)hipEventElapsedTime(&out->ms_stream, ev_[1], ev_[2]);
  (void)hipEventElapsedTime(&out->ms_total, ev_[0], ev_[3]);
  return HG_OK;
}

uint32_t HgScanner::launch_block_small(const uint8_t *h_text, uint32_t nbytes, hipStream_t stream, HgHit *h_out, uint32_t *h_counts, uint32_t *h_flag, uint32_t seq) {
  uint32_t ppw;
  const uint32_t segs = hg_block_small_grouping(view_.npatterns, &ppw);
  if (nbytes == 0 || nbytes > HG_BLOCK_SMALL_MAX || segs == 0 || segs > 64 || db_->nhuge) return 0;  // (huge automata: the general path)
  if (hipSetDevice(device_) != hipSuccess) return 0;
  hipLaunchKernelGGL(hg_block_small_kernel, dim3(segs), dim3(256), 0, stream, view_, h_text, nbytes, h_out, static_cast<uint32_t>(HG_BLOCK_SMALL_SEG), h_counts,
                     d_counters_ + HG_ST_BLOCK_DONE, h_flag, seq, ppw);
  return hipGetLastError() == hipSuccess ? segs : 0;
}

int HgScanner::scan_block(const void *d_text, uint64_t nbytes, hipStream_t stream, HgScanOutput *out) {
  return scan_impl(d_text, nbytes, 0x7FFFFFFF, 0, true, false, stream, out);
}

int HgScanner::scan(const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, hipStream_t stream, HgScanOutput *out, bool invert) {
  return scan_impl(d_text, nbytes, buffer_size, line_base, false, invert, stream, out);
}

// One pass over `range` (run_once), repeated while the workspace grows, 16 times at most: out->reruns.
int HgScanner::run_fitting(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, const PassRange &range, bool block_mode, hipStream_t stream,
                           HgScanOutput *out) {
  for (uint32_t reruns = 0;; reruns++) {
    std::memset(out, 0, sizeof(*out));
    const int rc = run_once(text, nbytes, bs1, line_base, range, block_mode, stream, out);
    out->reruns = reruns;
    if (rc != HG_GROWN) return rc;
    if (reruns == 16) return error(HG_ERR_NOMEM, "workspace kept overflowing");
    if (knobs_.verbose) std::fprintf(stderr, "hypergrep_amd: workspace grown (cands %u, hits %u), repeating the pass\n", cand_cap_, hit_cap_);
  }
}

int HgScanner::scan_impl(const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, bool block_mode, bool invert, hipStream_t stream,
                         HgScanOutput *out) {
  if (!out || (!d_text && nbytes) || buffer_size < 2) return error(HG_ERR_ARG, "invalid arguments");
  if ((reinterpret_cast<uintptr_t>(d_text) & 15u) != 0) return error(HG_ERR_ARG, "text pointer must be 16-byte aligned");
  const uint64_t bs1 = static_cast<uint64_t>(buffer_size) - 1;
  HG_TRY(hipSetDevice(device_), "hipSetDevice");
  std::memset(out, 0, sizeof(*out));
  if (hgmem::log_file()) hgmem::note("scan  %p text %p .. %p  %llu  bs %d block %d\n", static_cast<void *>(this), d_text, static_cast<const void *>(static_cast<const char *>(d_text) + nbytes), static_cast<unsigned long long>(nbytes), buffer_size, block_mode ? 1 : 0);
  int rc = ensure(nbytes);
  if (rc) return rc;
  const uint8_t *text = static_cast<const uint8_t *>(d_text);
  const uint64_t ntiles = (nbytes + HG_TILE_BYTES - 1) / HG_TILE_BYTES;
  const PassRange whole{0, ntiles, 0, line_base, 0, ~0ull, true};
  rc = run_fitting(text, nbytes, bs1, line_base, whole, block_mode, stream, out);
  if (rc == HG_OK && db_->comb_pass()) rc = comb_pass(out, bs1, line_base + nbytes + 2, stream);
  if (rc == HG_SPLIT) {
    // More reports (or pipeline chunks) than one pass may have: the buffer is scanned in 2, 4, 8 ... segments.  (The scan
    // reports the repeats of its whole-buffer attempt.)
    const uint32_t reruns = out->reruns;
    for (uint32_t nsegments = 2; (rc = scan_segments(text, nbytes, bs1, line_base, stream, out, nsegments)) == HG_SPLIT; nsegments *= 2)
      if (nsegments >= (1u << 16)) return error(HG_ERR_NOMEM, "a single stretch of the text holds more reports than one pass may have");
    out->reruns = reruns;
  }
  if (rc) return rc;
  // the invert stage: behind the finalize, the match-length and the combination stages, on the delivered hits of the whole
  // buffer (no start-of-match pass: the selected pieces have no match)
  if (invert && !block_mode) return invert_pass(text, nbytes, bs1, line_base, stream, out);
  if (db_->nsom) {
    // start of match (behind the combination pass: only delivered hits get a start): one pass over the final ordered hits (those of all segments, one after the other)
    if (out->n_hits > from_cap_) {
      from_cap_ = 0;
      const uint64_t cap = std::max<uint64_t>(out->n_hits + out->n_hits / 4, 4096);
      HG_TRY(realloc_dev(d_from_, cap, "d_from_"), "alloc (hit starts)");
      from_cap_ = cap;
    }
    HG_TRY(hg_som_launch(text, out->d_hits, out->d_aux, out->n_hits, static_cast<const HgPattern *>(d_patterns_), static_cast<const uint32_t *>(d_pool_), som_max_nw_,
                         d_min_lengths_, d_from_, stream),
           "start-of-match launch");
    HG_TRY(hipStreamSynchronize(stream), "stream sync (start of match)");
    out->d_from = d_from_;
  }
  return HG_OK;
}

// The buffer in `nsegments` passes.  Segment s reports the pieces whose first scanned byte lies in its stretch of the text
// (whole tiles) and scans on past the stretch's end for as long as such a piece can reach (bs1 bytes);
// hits of pieces that belong to a neighbour are dropped where they are emitted (HitSink::push), so every piece is ordered
// and filtered (SINGLEMATCH / duplicate rules) in exactly one pass.  The tile-scan state (carry-in line start, piece index)
// at a segment's first tile is read from the previous pass, which has scanned past it.  The passes' ordered hits are put one
// after the other: segments are in text order, so is their concatenation.  HG_SPLIT: some segment still overflowed a pass.
// The tile summaries and prefix states (d_sums_, d_bases_) are indexed by ABSOLUTE tile, and a pass that rewrites the tiles a
// neighbour has written (the `reach` overlap) writes the same values, since it starts from that neighbour's state: after the
// last segment they describe the whole buffer.  The invert stage (invert_pass) relies on this.
int HgScanner::scan_segments(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, hipStream_t stream, HgScanOutput *out, uint32_t nsegments) {
  const uint64_t ntiles = (nbytes + HG_TILE_BYTES - 1) / HG_TILE_BYTES;
  const uint64_t reach = (bs1 >> HG_TILE_SHIFT) + 2;  // tiles a piece that starts inside a stretch can extend past its end
  constexpr uint64_t kAlign = 16;  // (tiles; real segments are gigabytes)
  const uint64_t seg_tiles = ((ntiles + nsegments - 1) / nsegments + kAlign - 1) / kAlign * kAlign;
  if (seg_tiles <= reach)  // (scan buffers of gigabytes on a text that needs many segments)
    return error(HG_ERR_NOMEM, "more reports than one pass may have, and the scan buffer size leaves no room for segments");
  fin_fallback_ = false;  // (a smaller stretch: bucketed emission gets another chance)
  fin_expect_hits_ /= nsegments;
  uint64_t acc = 0, cs0 = 0, piece0 = line_base;
  HgScanOutput sum{}, part{};
  for (uint64_t lo = 0; lo < ntiles; lo += seg_tiles) {
    const bool last = lo + seg_tiles >= ntiles;
    const PassRange range{lo, last ? ntiles : std::min<uint64_t>(ntiles, lo + seg_tiles + reach), cs0, piece0, lo << HG_TILE_SHIFT, last ? ~0ull : (lo + seg_tiles) << HG_TILE_SHIFT, last};
    if (int rc = run_fitting(text, nbytes, bs1, line_base, range, false, stream, &part)) return rc;
    if (db_->comb_pass())  // (pieces never cross segments: each pass's hits are complete pieces)
      if (int rc = comb_pass(&part, bs1, line_base + nbytes + 2, stream)) return rc;
    // this pass's ordered hits behind those of the earlier segments
    if (acc + part.n_hits > acc_cap_) {
      // sized from the hits so far, the share of the text they came from, and a quarter on top
      const uint64_t done = std::max<uint64_t>(std::min<uint64_t>(ntiles, lo + seg_tiles), 1);
      const uint64_t guess = static_cast<uint64_t>(static_cast<double>(acc + part.n_hits) * static_cast<double>(ntiles) / static_cast<double>(done) * 1.25) + 4096;
      const uint64_t cap = std::max<uint64_t>(acc + part.n_hits, guess);
      HgHit *nh = nullptr;
      HgHitAux *na = nullptr;
      if (fail(hgmem::dev_alloc(&nh, cap * sizeof(HgHit), "d_acc_hits_"), "alloc (segment hits)") || fail(hgmem::dev_alloc(&na, cap * sizeof(HgHitAux), "d_acc_aux_"), "alloc (segment hits)")) {
        hgmem::dev_free(nh, "d_acc_hits_");
        return HG_ERR_HIP;
      }
      if (acc) {
        HG_TRY(hipMemcpyAsync(nh, d_acc_hits_, acc * sizeof(HgHit), hipMemcpyDeviceToDevice, stream), "copy");
        HG_TRY(hipMemcpyAsync(na, d_acc_aux_, acc * sizeof(HgHitAux), hipMemcpyDeviceToDevice, stream), "copy");
        HG_TRY(hipStreamSynchronize(stream), "sync");
      }
      hgmem::dev_free(d_acc_hits_, "d_acc_hits_");
      hgmem::dev_free(d_acc_aux_, "d_acc_aux_");
      d_acc_hits_ = nh;
      d_acc_aux_ = na;
      acc_cap_ = cap;
    }
    if (part.n_hits) {
      HG_TRY(hipMemcpyAsync(d_acc_hits_ + acc, part.d_hits, part.n_hits * sizeof(HgHit), hipMemcpyDeviceToDevice, stream), "copy");
      HG_TRY(hipMemcpyAsync(d_acc_aux_ + acc, part.d_aux, part.n_hits * sizeof(HgHitAux), hipMemcpyDeviceToDevice, stream), "copy");
    }
    acc += part.n_hits;
    sum.n_cands += part.n_cands;
    sum.n_raw_hits += part.n_raw_hits;
    sum.ms_stream += part.ms_stream;
    sum.ms_total += part.ms_total;
    sum.stream_launches += part.stream_launches;
    sum.joiner_launches += part.joiner_launches;
    sum.joiner_tiles += part.joiner_tiles;
    if (!last) {  // the tile-scan state at the next segment's first tile (this pass has scanned past it)
      HgTileBase next{};
      HG_TRY(hipMemcpyAsync(&next, d_bases_ + (lo + seg_tiles), sizeof next, hipMemcpyDeviceToHost, stream), "copy");
      HG_TRY(hipStreamSynchronize(stream), "sync");
      cs0 = next.cs;
      piece0 = next.L;
    }
  }
  HG_TRY(hipStreamSynchronize(stream), "sync");
  sum.n_hits = acc;
  sum.n_pieces = part.n_pieces;
  sum.d_hits = d_acc_hits_;
  sum.d_aux = d_acc_aux_;
  *out = sum;
  return HG_OK;
}

// ---------------------------------------------------------------- gather stage (hg_gather_lines): buffers and launch sequence
HgGather::~HgGather() {
  (void)hipSetDevice(device_);  // (the buffers are freed behind this body)
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
}

#define HG_GATHER_TRY(expr, what)                                                                    \
  do {                                                                                               \
    const hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                          \
      *err = std::string("gather stage: ") + (what) + ": " + hipGetErrorString(e_);                 \
      return HG_ERR_HIP;                                                                             \
    }                                                                                                \
  } while (0)

int HgGather::run(const HgGatherInput &in, hipStream_t stream, HgGatherOutput *out, std::string *err) {
  *out = HgGatherOutput{};
  HG_GATHER_TRY(hipSetDevice(device_), "hipSetDevice");
  for (hipEvent_t &e : ev_)
    if (!e) HG_GATHER_TRY(hipEventCreate(&e), "event");
  const uint64_t n = in.main.n + in.ctx.n, cap = n + 1;
  size_t tb = 0;
  HG_GATHER_TRY(rocprim::exclusive_scan(nullptr, tb, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), uint64_t{0}, cap, rocprim::plus<uint64_t>(), stream),
                "scan size");
  tb = std::max<size_t>(tb, 16);
  const size_t grow = cap + cap / 4;
  const bool ok = head_.reserve(cap, grow) && F_.reserve(cap, grow) && size_.reserve(cap, grow) && off_.reserve(cap, grow) && line_.reserve(cap, grow) &&
                  kind_.reserve(cap, grow) && (!in.seg_start || (seg_.reserve(cap, grow) && first_.reserve(in.n_seg + 1, in.n_seg + 1))) && entries_.reserve(cap, grow) &&
                  temp_.reserve(tb, tb + tb / 4) && totals_.reserve(2, 2);
  if (!ok) {
    *err = "gather stage: out of memory";
    return HG_ERR_NOMEM;
  }
  HgGatherArgs a{};
  a.text = HgGatherText{in.text};
  a.main = in.main;
  a.ctx = in.ctx;
  a.seg_start = in.seg_start;
  a.first_record = in.first_record;
  a.first_context = in.first_context;
  a.n_seg = in.n_seg;
  a.flags = in.flags;
  a.head = head_.get();
  a.F = F_.get();
  a.size = size_.get();
  a.entries = entries_.get();
  a.line_number = line_.get();
  a.kind = kind_.get();
  a.segment = in.seg_start ? seg_.get() : nullptr;
  a.first_entry = in.seg_start ? first_.get() : nullptr;
  a.off = off_.get();
  HG_GATHER_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_GATHER_TRY(hg_gather_launch(a, HgGatherStep::Flag, stream), "launch (flags)");
  size_t t = temp_.cap();
  HG_GATHER_TRY(rocprim::exclusive_scan(temp_.get(), t, head_.get(), F_.get(), uint64_t{0}, cap, rocprim::plus<uint64_t>(), stream), "scan (heads)");
  HG_GATHER_TRY(hipMemsetAsync(size_.get(), 0, cap * sizeof(uint64_t), stream), "memset");
  HG_GATHER_TRY(hg_gather_launch(a, HgGatherStep::Entry, stream), "launch (entries)");
  if (in.seg_start) HG_GATHER_TRY(hg_gather_launch(a, HgGatherStep::First, stream), "launch (first_entry)");
  t = temp_.cap();
  HG_GATHER_TRY(rocprim::exclusive_scan(temp_.get(), t, size_.get(), off_.get(), uint64_t{0}, cap, rocprim::plus<uint64_t>(), stream), "scan (sizes)");
  uint64_t *totals = totals_.get();
  HG_GATHER_TRY(hipMemcpyAsync(totals, F_.get() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy count");
  HG_GATHER_TRY(hipMemcpyAsync(totals + 1, off_.get() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy count");
  HG_GATHER_TRY(hipStreamSynchronize(stream), "stream sync");
  a.n_entries = totals[0];
  a.n_bytes = totals[1];
  const uint64_t padded = (a.n_bytes + 15) & ~static_cast<uint64_t>(15);
  if (!bytes_.reserve(std::max<uint64_t>(padded, 16), std::max<uint64_t>(padded + padded / 8, 16))) {
    *err = "gather stage: out of memory for " + std::to_string(a.n_bytes) + " bytes of lines";
    return HG_ERR_NOMEM;
  }
  a.out = bytes_.get();
  const uint64_t n_spans = (a.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE;
  if (!span_.reserve(n_spans + 1, n_spans + n_spans / 8 + 1)) {
    *err = "gather stage: out of memory";
    return HG_ERR_NOMEM;
  }
  a.span = span_.get();
  HG_GATHER_TRY(hg_gather_launch(a, HgGatherStep::Span, stream), "launch (spans)");
  HG_GATHER_TRY(hg_gather_launch(a, HgGatherStep::Copy, stream), "launch (copy)");
  HG_GATHER_TRY(hipEventRecord(ev_[1], stream), "event");
  HG_GATHER_TRY(hipStreamSynchronize(stream), "stream sync");
  HG_GATHER_TRY(hipEventElapsedTime(&out->ms_gather, ev_[0], ev_[1]), "event time");
  out->n_entries = a.n_entries;
  out->n_bytes = a.n_bytes;
  out->d_bytes = bytes_.get();
  out->d_entry_off = off_.get();
  out->d_line_number = line_.get();
  out->d_kind = kind_.get();
  out->d_segment = a.segment;
  out->d_first_entry = a.first_entry;
  return HG_OK;
}

// ---------------------------------------------------------------- parts gather (hg_gather_parts): buffers and launch sequence
HgPartLines::~HgPartLines() {
  (void)hipSetDevice(device_);  // (the buffers are freed behind this body)
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
}

#define HG_PARTLINES_TRY(expr, what)                                                      \
  do {                                                                                    \
    const hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                               \
      *err = std::string("parts gather: ") + (what) + ": " + hipGetErrorString(e_);       \
      return HG_ERR_HIP;                                                                  \
    }                                                                                     \
  } while (0)

int HgPartLines::run(const HgPartLinesInput &in, hipStream_t stream, HgPartLinesOutput *out, std::string *err) {
  *out = HgPartLinesOutput{};
  HG_PARTLINES_TRY(hipSetDevice(device_), "hipSetDevice");
  for (hipEvent_t &e : ev_)
    if (!e) HG_PARTLINES_TRY(hipEventCreate(&e), "event");
  const uint64_t n = in.n_parts, cap = n + 1;
  size_t tb = 0;
  HG_PARTLINES_TRY(rocprim::exclusive_scan(nullptr, tb, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), uint64_t{0}, cap, rocprim::plus<uint64_t>(), stream),
                   "scan size");
  tb = std::max<size_t>(tb, 16);
  const size_t grow = cap + cap / 4;
  const bool ok = size_.reserve(cap, grow) && off_.reserve(cap, grow) && line_.reserve(cap, grow) && kind_.reserve(cap, grow) && pattern_.reserve(cap, grow) &&
                  (!in.seg_start || (seg_.reserve(cap, grow) && first_.reserve(in.n_seg + 1, in.n_seg + 1))) && entries_.reserve(cap, grow) && temp_.reserve(tb, tb + tb / 4) &&
                  totals_.reserve(1, 1);
  if (!ok) {
    *err = "parts gather: out of memory";
    return HG_ERR_NOMEM;
  }
  HgPartLinesArgs a{};
  a.text = HgGatherText{in.text};
  a.recs = in.recs;
  a.parts = in.parts;
  a.part_pattern = in.part_pattern;
  a.part_seg = in.seg_start ? in.part_seg : nullptr;
  a.n_parts = n;
  a.seg_start = in.seg_start;
  a.flags = in.flags;
  a.byte_base = in.byte_base;
  a.marks = in.marks;
  a.size = size_.get();
  a.entries = entries_.get();
  a.line_number = line_.get();
  a.kind = kind_.get();
  a.pattern = pattern_.get();
  a.segment = in.seg_start ? seg_.get() : nullptr;
  a.off = off_.get();
  HG_PARTLINES_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_PARTLINES_TRY(hg_partlines_launch(a, HgPartLinesStep::Entry, stream), "launch (entries)");
  // an entry per part: the segments' first entries are their first parts
  if (in.seg_start) HG_PARTLINES_TRY(hipMemcpyAsync(first_.get(), in.first_part, (in.n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream), "copy (first_entry)");
  size_t t = temp_.cap();
  HG_PARTLINES_TRY(rocprim::exclusive_scan(temp_.get(), t, size_.get(), off_.get(), uint64_t{0}, cap, rocprim::plus<uint64_t>(), stream), "scan (sizes)");
  uint64_t *totals = totals_.get();
  HG_PARTLINES_TRY(hipMemcpyAsync(totals, off_.get() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy count");
  HG_PARTLINES_TRY(hipStreamSynchronize(stream), "stream sync");
  a.n_entries = n;
  a.n_bytes = totals[0];
  const uint64_t padded = (a.n_bytes + 15) & ~static_cast<uint64_t>(15);
  if (!bytes_.reserve(std::max<uint64_t>(padded, 16), std::max<uint64_t>(padded + padded / 8, 16))) {
    *err = "parts gather: out of memory for " + std::to_string(a.n_bytes) + " bytes of parts";
    return HG_ERR_NOMEM;
  }
  a.out = bytes_.get();
  const uint64_t n_spans = (a.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE;
  if (!span_.reserve(n_spans + 1, n_spans + n_spans / 8 + 1)) {
    *err = "parts gather: out of memory";
    return HG_ERR_NOMEM;
  }
  a.span = span_.get();
  HG_PARTLINES_TRY(hg_partlines_launch(a, HgPartLinesStep::Span, stream), "launch (spans)");
  HG_PARTLINES_TRY(hg_partlines_launch(a, HgPartLinesStep::Copy, stream), "launch (copy)");
  HG_PARTLINES_TRY(hipEventRecord(ev_[1], stream), "event");
  HG_PARTLINES_TRY(hipStreamSynchronize(stream), "stream sync");
  HG_PARTLINES_TRY(hipEventElapsedTime(&out->ms_gather, ev_[0], ev_[1]), "event time");
  out->n_entries = a.n_entries;
  out->n_bytes = a.n_bytes;
  out->d_bytes = bytes_.get();
  out->d_entry_off = off_.get();
  out->d_line_number = line_.get();
  out->d_kind = kind_.get();
  out->d_pattern = pattern_.get();
  out->d_segment = a.segment;
  out->d_first_entry = in.seg_start ? first_.get() : nullptr;
  return HG_OK;
}

// ---------------------------------------------------------------- values stage (hg_count_values): buffers and launch sequence
HgValues::~HgValues() {
  (void)hipSetDevice(device_);  // (the buffers are freed behind this body)
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
}

#define HG_VALUES_TRY(expr, what)                                                   \
  do {                                                                              \
    const hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                         \
      *err = std::string("values stage: ") + (what) + ": " + hipGetErrorString(e_); \
      return HG_ERR_HIP;                                                            \
    }                                                                               \
  } while (0)

int HgValues::group(const HgValuesInput &in, hipStream_t stream, HgValuesGroups *groups, std::string *err) {
  *groups = HgValuesGroups{};
  HG_VALUES_TRY(hipSetDevice(device_), "hipSetDevice");
  for (hipEvent_t &e : ev_)
    if (!e) HG_VALUES_TRY(hipEventCreate(&e), "event");
  const uint64_t n = in.n_parts, cap = uint64_t{1} << in.table_log2, np = n + 1;
  // per part and per slot now; per value once their number is known
  size_t tb = 0;
  HG_VALUES_TRY(rocprim::exclusive_scan(nullptr, tb, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), uint64_t{0}, cap, rocprim::plus<uint64_t>(), stream),
                "scan size");
  tb = std::max<size_t>(tb, 16);
  const size_t grow = np + np / 4;
  const bool ok = src_.reserve(np, grow) && hash_.reserve(np, grow) && long_.reserve(np, grow) && len_.reserve(np, grow) && pair_first_.reserve(np, grow) &&
                  pair_count_.reserve(np, grow) && slot_.reserve(cap, cap) && slot_count_.reserve(cap, cap) && slot_first_.reserve(cap, cap) && pos_.reserve(cap, cap) &&
                  counters_.reserve(HG_VALUES_COUNTERS, HG_VALUES_COUNTERS) && temp_.reserve(tb, tb + tb / 4) && totals_.reserve(HG_VALUES_COUNTERS + 1, HG_VALUES_COUNTERS + 1);
  const bool by_seg = (in.flags & HG_VALUES_F_BY_SEGMENT) != 0;  // (the rank stage's: the segment in the key)
  if (!ok || (by_seg && !key_.reserve(np, grow))) {
    *err = "values stage: out of memory (" + std::to_string(n) + " parts, a table of 2^" + std::to_string(in.table_log2) + " slots)";
    return HG_ERR_NOMEM;
  }
  HgValuesArgs a{};
  a.text = HgGatherText{in.text};
  a.recs = in.recs;
  a.parts = in.parts;
  a.part_pattern = in.part_pattern;
  a.part_seg = in.seg_start ? in.part_seg : nullptr;
  a.n_parts = n;
  a.seg_start = in.seg_start;
  a.flags = in.flags;
  a.hash_bits = in.hash_bits;
  a.table_log2 = in.table_log2;
  a.src = src_.get();
  a.len = len_.get();
  a.hash = hash_.get();
  a.long_list = long_.get();
  a.counters = counters_.get();
  a.slot = slot_.get();
  a.count = slot_count_.get();
  a.first = slot_first_.get();
  a.pos = pos_.get();
  a.pair_first = pair_first_.get();
  a.pair_count = pair_count_.get();
  a.key = by_seg ? key_.get() : nullptr;
  uint64_t *totals = totals_.get();
  HG_VALUES_TRY(hipEventRecord(ev_[0], stream), "event");
  HG_VALUES_TRY(hipMemsetAsync(counters_.get(), 0, HG_VALUES_COUNTERS * sizeof(unsigned long long), stream), "memset");
  if (n) {
    HG_VALUES_TRY(hipMemsetAsync(slot_.get(), 0xFF, cap * sizeof(unsigned long long), stream), "memset");  // HG_VALUES_EMPTY
    HG_VALUES_TRY(hipMemsetAsync(slot_first_.get(), 0xFF, cap * sizeof(unsigned long long), stream), "memset");
    HG_VALUES_TRY(hipMemsetAsync(slot_count_.get(), 0, cap * sizeof(unsigned long long), stream), "memset");
    const auto launch = by_seg ? hg_rank_group_launch : hg_values_launch;
    HG_VALUES_TRY(launch(a, HgValuesStep::Hash, stream), "launch (hash)");
    HG_VALUES_TRY(launch(a, HgValuesStep::Long, stream), "launch (long parts)");
    HG_VALUES_TRY(launch(a, HgValuesStep::Insert, stream), "launch (insert)");
    HG_VALUES_TRY(hg_values_launch(a, HgValuesStep::Mark, stream), "launch (mark)");
    size_t t = temp_.cap();
    HG_VALUES_TRY(rocprim::exclusive_scan(temp_.get(), t, pos_.get(), pos_.get(), uint64_t{0}, cap, rocprim::plus<uint64_t>(), stream), "scan (marks)");
    HG_VALUES_TRY(hg_values_launch(a, HgValuesStep::Compact, stream), "launch (compact)");
  }
  HG_VALUES_TRY(hipMemcpyAsync(totals, counters_.get(), HG_VALUES_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy counters");
  HG_VALUES_TRY(hipStreamSynchronize(stream), "stream sync");
  if (totals[HG_VALUES_OVERFLOW] || totals[HG_VALUES_N_VALUES] > n) {
    *err = "values stage: a probe went round the whole table of 2^" + std::to_string(in.table_log2) + " slots";
    return HG_ERR_NOMEM;
  }
  a.n_values = totals[HG_VALUES_N_VALUES];
  {
    const uint64_t nv = a.n_values + 1, nv_grow = nv + nv / 4;
    size_t t_sort = 0, t_size = 0;
    HG_VALUES_TRY(rocprim::radix_sort_pairs(nullptr, t_sort, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr),
                                            static_cast<uint64_t *>(nullptr), nv, 0, 64, stream),
                  "sort size");
    HG_VALUES_TRY(rocprim::exclusive_scan(nullptr, t_size, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), uint64_t{0}, nv, rocprim::plus<uint64_t>(), stream),
                  "scan size");
    const size_t tv = std::max<size_t>(std::max(t_sort, t_size), 16);
    if (!first_.reserve(nv, nv_grow) || !count_.reserve(nv, nv_grow) || !temp_.reserve(tv, tv + tv / 4)) {
      *err = "values stage: out of memory for " + std::to_string(a.n_values) + " values";
      return HG_ERR_NOMEM;
    }
  }
  a.v_first = first_.get();
  if (a.n_values) {
    size_t t = temp_.cap();
    uint32_t bits = 1;
    while (bits < 64 && (n >> bits)) bits++;  // first < n_parts
    HG_VALUES_TRY(rocprim::radix_sort_pairs(temp_.get(), t, pair_first_.get(), first_.get(), pair_count_.get(), count_.get(), a.n_values, 0, bits, stream), "sort (first)");
  }
  groups->args = a;
  groups->n_values = a.n_values;
  groups->d_first = first_.get();
  groups->d_count = count_.get();
  return HG_OK;
}

int HgValues::run(const HgValuesInput &in, hipStream_t stream, HgValuesOutput *out, std::string *err) {
  *out = HgValuesOutput{};
  HgValuesGroups groups{};
  const int rc = group(in, stream, &groups, err);
  if (rc != HG_OK) return rc;
  HgValuesArgs a = groups.args;
  const uint64_t n = in.n_parts;
  uint64_t *totals = totals_.get();
  {
    const uint64_t nv = a.n_values + 1, nv_grow = nv + nv / 4;
    if (!size_.reserve(nv, nv_grow) || !off_.reserve(nv, nv_grow) || !line_.reserve(nv, nv_grow) || !pattern_.reserve(nv, nv_grow) || (in.seg_start && !seg_.reserve(nv, nv_grow)) ||
        !entries_.reserve(nv, nv_grow)) {
      *err = "values stage: out of memory for " + std::to_string(a.n_values) + " values";
      return HG_ERR_NOMEM;
    }
  }
  a.size = size_.get();
  a.entries = entries_.get();
  a.pattern = pattern_.get();
  a.segment = in.seg_start ? seg_.get() : nullptr;
  a.line_number = line_.get();
  HG_VALUES_TRY(hg_values_launch(a, HgValuesStep::Derive, stream), "launch (derive)");
  {
    size_t t = temp_.cap();
    HG_VALUES_TRY(rocprim::exclusive_scan(temp_.get(), t, size_.get(), off_.get(), uint64_t{0}, a.n_values + 1, rocprim::plus<uint64_t>(), stream), "scan (lengths)");
  }
  HG_VALUES_TRY(hipMemcpyAsync(totals + HG_VALUES_COUNTERS, off_.get() + a.n_values, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy count");
  HG_VALUES_TRY(hipStreamSynchronize(stream), "stream sync");
  HgGatherArgs g{};
  g.text = a.text;
  g.entries = entries_.get();
  g.off = off_.get();
  g.n_entries = a.n_values;
  g.n_bytes = totals[HG_VALUES_COUNTERS];
  const uint64_t padded = (g.n_bytes + 15) & ~static_cast<uint64_t>(15), n_spans = (g.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE;
  if (!bytes_.reserve(std::max<uint64_t>(padded, 16), std::max<uint64_t>(padded + padded / 8, 16)) || !span_.reserve(n_spans + 1, n_spans + n_spans / 8 + 1)) {
    *err = "values stage: out of memory for " + std::to_string(g.n_bytes) + " bytes of values";
    return HG_ERR_NOMEM;
  }
  g.span = span_.get();
  g.out = bytes_.get();
  HG_VALUES_TRY(hg_gather_launch(g, HgGatherStep::Span, stream), "launch (spans)");  // (nothing without bytes)
  HG_VALUES_TRY(hg_gather_launch(g, HgGatherStep::Copy, stream), "launch (copy)");
  HG_VALUES_TRY(hipEventRecord(ev_[1], stream), "event");
  HG_VALUES_TRY(hipStreamSynchronize(stream), "stream sync");
  HG_VALUES_TRY(hipEventElapsedTime(&out->ms_values, ev_[0], ev_[1]), "event time");
  out->n_values = a.n_values;
  out->n_parts = n;
  out->n_bytes = g.n_bytes;
  out->d_bytes = bytes_.get();
  out->d_off = off_.get();
  out->d_count = count_.get();
  out->d_first = first_.get();
  out->d_line_number = line_.get();
  out->d_pattern = pattern_.get();
  out->d_segment = a.segment;
  out->table_log2 = in.table_log2;
  return HG_OK;
}

// ---------------------------------------------------------------- rank stage (hg_rank_values): buffers and launch sequence
HgRank::~HgRank() {
  (void)hipSetDevice(device_);  // (the buffers are freed behind this body)
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
}

#define HG_RANK_TRY(expr, what)                                                   \
  do {                                                                            \
    const hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess) {                                                       \
      *err = std::string("rank stage: ") + (what) + ": " + hipGetErrorString(e_); \
      return HG_ERR_HIP;                                                          \
    }                                                                             \
  } while (0)

int HgRank::run(const HgRankInput &in, hipStream_t stream, HgRankOutput *out, std::string *err) {
  *out = HgRankOutput{};
  HG_RANK_TRY(hipSetDevice(device_), "hipSetDevice");
  for (hipEvent_t &e : ev_)
    if (!e) HG_RANK_TRY(hipEventCreate(&e), "event");
  HG_RANK_TRY(hipEventRecord(ev_[0], stream), "event");
  // the groups, sorted by first: the values stage's passes with the segment in the key (one host synchronisation)
  HgValuesGroups groups{};
  const int rc = groups_.group(in.values, stream, &groups, err);
  if (rc != HG_OK) return rc;
  const bool per_seg = (in.values.flags & HG_RANK_F_PER_SEGMENT) != 0;
  const uint64_t ng = groups.n_values, np = ng + 1, np_grow = np + np / 4, n_parts = in.values.n_parts;
  const uint32_t n_seg = per_seg ? in.n_seg : 1u;
  const uint64_t ns = static_cast<uint64_t>(n_seg) + 1;
  uint32_t bits = 1, seg_bits = 1;
  while (bits < 64 && (n_parts >> bits)) bits++;            // count <= n_parts
  while (seg_bits < 32 && (n_seg >> seg_bits)) seg_bits++;  // segment < n_seg
  size_t t_count = 0, t_seg = 0, t_scan = 0, t_scan_seg = 0;
  HG_RANK_TRY(rocprim::radix_sort_pairs_desc(nullptr, t_count, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr),
                                             static_cast<uint64_t *>(nullptr), std::max<uint64_t>(ng, 1), 0, bits, stream),
              "sort size");
  HG_RANK_TRY(rocprim::radix_sort_pairs(nullptr, t_seg, static_cast<uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), static_cast<uint64_t *>(nullptr),
                                        static_cast<uint64_t *>(nullptr), std::max<uint64_t>(ng, 1), 0, seg_bits, stream),
              "sort size");
  HG_RANK_TRY(rocprim::exclusive_scan(nullptr, t_scan, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), uint64_t{0}, np, rocprim::plus<uint64_t>(), stream),
              "scan size");
  HG_RANK_TRY(rocprim::exclusive_scan(nullptr, t_scan_seg, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), uint64_t{0}, ns, rocprim::plus<uint64_t>(), stream),
              "scan size");
  const size_t tb = std::max<size_t>(std::max(std::max(t_count, t_seg), std::max(t_scan, t_scan_seg)), 16);
  const bool ok = g_first_.reserve(np, np_grow) && g_count_.reserve(np, np_grow) && s_count_.reserve(np, np_grow) && cum_.reserve(np, np_grow) && first_.reserve(np, np_grow) &&
                  count_.reserve(np, np_grow) && size_.reserve(np, np_grow) && off_.reserve(np, np_grow) && line_.reserve(np, np_grow) && pattern_.reserve(np, np_grow) &&
                  entries_.reserve(np, np_grow) && (!in.values.seg_start || seg_.reserve(np, np_grow)) &&
                  (!per_seg || (key_idx_.reserve(np, np_grow) && s_idx_.reserve(np, np_grow) && key_seg_.reserve(np, np_grow) && s_seg_.reserve(np, np_grow))) &&
                  first_group_.reserve(ns, ns + ns / 4) && seg_distinct_.reserve(ns, ns + ns / 4) && seg_parts_.reserve(ns, ns + ns / 4) && kept_.reserve(ns, ns + ns / 4) &&
                  first_value_.reserve(ns, ns + ns / 4) && temp_.reserve(tb, tb + tb / 4) && totals_.reserve(2, 2);
  if (!ok) {
    *err = "rank stage: out of memory (" + std::to_string(ng) + " distinct values, " + std::to_string(n_seg) + " segments)";
    return HG_ERR_NOMEM;
  }
  HgRankArgs a{};
  a.parts = groups.args.parts;
  a.part_pattern = groups.args.part_pattern;
  a.part_seg = groups.args.part_seg;
  a.n_parts = n_parts;
  a.src = groups.args.src;
  a.len = groups.args.len;
  a.flags = in.values.flags;
  a.n_seg = n_seg;
  a.top = in.top;
  a.n_groups = ng;
  a.g_first = g_first_.get();
  a.g_count = g_count_.get();
  a.s_count = s_count_.get();
  a.cum = cum_.get();
  a.first_group = first_group_.get();
  a.seg_distinct = seg_distinct_.get();
  a.seg_parts = seg_parts_.get();
  a.kept = kept_.get();
  a.first_value = first_value_.get();
  a.out_first = first_.get();
  a.out_count = count_.get();
  a.size = size_.get();
  a.entries = entries_.get();
  a.pattern = pattern_.get();
  a.segment = in.values.seg_start ? seg_.get() : nullptr;
  a.line_number = line_.get();
  if (ng) {
    size_t t = temp_.cap();
    HG_RANK_TRY(rocprim::radix_sort_pairs_desc(temp_.get(), t, groups.d_count, g_count_.get(), groups.d_first, g_first_.get(), ng, 0, bits, stream), "sort (count)");
  }
  if (per_seg) {
    a.key_seg = key_seg_.get();
    a.key_idx = key_idx_.get();
    HG_RANK_TRY(hg_rank_launch(a, HgRankStep::Keys, stream), "launch (keys)");
    if (ng) {
      size_t t = temp_.cap();
      HG_RANK_TRY(rocprim::radix_sort_pairs(temp_.get(), t, key_seg_.get(), s_seg_.get(), key_idx_.get(), s_idx_.get(), ng, 0, seg_bits, stream), "sort (segment)");
    }
    a.s_seg = s_seg_.get();
    a.s_idx = s_idx_.get();
  }
  HG_RANK_TRY(hg_rank_launch(a, HgRankStep::Counts, stream), "launch (counts)");
  {
    size_t t = temp_.cap();
    HG_RANK_TRY(rocprim::exclusive_scan(temp_.get(), t, s_count_.get(), cum_.get(), uint64_t{0}, np, rocprim::plus<uint64_t>(), stream), "scan (counts)");
  }
  HG_RANK_TRY(hg_rank_launch(a, HgRankStep::Bounds, stream), "launch (bounds)");
  {
    size_t t = temp_.cap();
    HG_RANK_TRY(rocprim::exclusive_scan(temp_.get(), t, kept_.get(), first_value_.get(), uint64_t{0}, ns, rocprim::plus<uint64_t>(), stream), "scan (kept)");
  }
  HG_RANK_TRY(hipMemsetAsync(size_.get(), 0, np * sizeof(uint64_t), stream), "memset");
  HG_RANK_TRY(hg_rank_launch(a, HgRankStep::Place, stream), "launch (place)");
  {
    size_t t = temp_.cap();
    HG_RANK_TRY(rocprim::exclusive_scan(temp_.get(), t, size_.get(), off_.get(), uint64_t{0}, np, rocprim::plus<uint64_t>(), stream), "scan (lengths)");
  }
  uint64_t *totals = totals_.get();
  HG_RANK_TRY(hipMemcpyAsync(totals, first_value_.get() + n_seg, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy rows");
  HG_RANK_TRY(hipMemcpyAsync(totals + 1, off_.get() + ng, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy bytes");
  HG_RANK_TRY(hipStreamSynchronize(stream), "stream sync");
  if (totals[0] > ng) {
    *err = "rank stage: more rows than distinct values";
    return HG_ERR_HIP;
  }
  HgGatherArgs g{};
  g.text = groups.args.text;
  g.entries = entries_.get();
  g.off = off_.get();
  g.n_entries = totals[0];
  g.n_bytes = totals[1];
  const uint64_t padded = (g.n_bytes + 15) & ~static_cast<uint64_t>(15), n_spans = (g.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE;
  if (!bytes_.reserve(std::max<uint64_t>(padded, 16), std::max<uint64_t>(padded + padded / 8, 16)) || !span_.reserve(n_spans + 1, n_spans + n_spans / 8 + 1)) {
    *err = "rank stage: out of memory for " + std::to_string(g.n_bytes) + " bytes of values";
    return HG_ERR_NOMEM;
  }
  g.span = span_.get();
  g.out = bytes_.get();
  HG_RANK_TRY(hg_gather_launch(g, HgGatherStep::Span, stream), "launch (spans)");  // (nothing without bytes)
  HG_RANK_TRY(hg_gather_launch(g, HgGatherStep::Copy, stream), "launch (copy)");
  HG_RANK_TRY(hipEventRecord(ev_[1], stream), "event");
  HG_RANK_TRY(hipStreamSynchronize(stream), "stream sync");
  HG_RANK_TRY(hipEventElapsedTime(&out->ms_rank, ev_[0], ev_[1]), "event time");
  out->n_values = totals[0];
  out->n_distinct = ng;
  out->n_parts = n_parts;
  out->n_bytes = g.n_bytes;
  out->d_bytes = bytes_.get();
  out->d_off = off_.get();
  out->d_count = count_.get();
  out->d_first = first_.get();
  out->d_line_number = line_.get();
  out->d_pattern = pattern_.get();
  out->d_segment = a.segment;
  if (per_seg) {
    out->d_first_value = first_value_.get();
    out->d_seg_distinct = seg_distinct_.get();
    out->d_seg_parts = seg_parts_.get();
  }
  out->n_seg = per_seg ? n_seg : 0;
  out->table_log2 = in.values.table_log2;
  return HG_OK;
}

// ---------------------------------------------------------------- value store (hg_accumulate_values, hg_rank_accumulated)
HgValueStore::~HgValueStore() {
  (void)hipSetDevice(device_);  // (the buffers are freed behind this body)
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
}

#define HG_VALSTORE_TRY(expr, what)                                                \
  do {                                                                             \
    const hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) {                                                        \
      *err = std::string("value store: ") + (what) + ": " + hipGetErrorString(e_); \
      return HG_ERR_HIP;                                                           \
    }                                                                              \
  } while (0)

const char *HgValueStore::mismatch(uint32_t flags, uint32_t hash_bits, bool reset) const {
  if (!began_ || reset) return nullptr;
  if (flags != flags_) return "HG_ACC_BY_PATTERN differs from the call that began the store (HG_ACC_RESET begins another)";
  if (hash_bits != hash_bits_) return "hash_bits differs from the call that began the store (HG_ACC_RESET begins another)";
  return nullptr;
}

int HgValueStore::accumulate(const HgValStoreInput &in, hipStream_t stream, HgValStoreOutput *out, std::string *err) {
  *out = HgValStoreOutput{};
  HG_VALSTORE_TRY(hipSetDevice(device_), "hipSetDevice");
  for (hipEvent_t &e : ev_)
    if (!e) HG_VALSTORE_TRY(hipEventCreate(&e), "event");
  HG_VALSTORE_TRY(hipEventRecord(ev_[0], stream), "event");
  // the store this call joins: with reset an empty one, which replaces the old one on success only
  const bool fresh = in.reset || !began_;
  const uint64_t n_old = fresh ? 0 : n_values_, parts_before = fresh ? 0 : n_parts_, bytes_before = fresh ? 0 : n_bytes_;
  const uint64_t tail16 = fresh ? 0 : (tail_ + 15) & ~static_cast<uint64_t>(15);
  const uint32_t log2_old = fresh ? 0 : log2_;
  // 1. the call's groups, sorted by first (one host synchronisation)
  HgValuesGroups groups{};
  const int rc = groups_.group(in.values, stream, &groups, err);
  if (rc != HG_OK) return rc;
  const uint64_t ng = groups.n_values, np = ng + 1, np_grow = np + np / 4;
  size_t tb = 0;
  HG_VALSTORE_TRY(rocprim::exclusive_scan(nullptr, tb, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), uint64_t{0}, np, rocprim::plus<uint64_t>(), stream), "scan size");
  tb = std::max<size_t>(tb, 16);
  if (!match_.reserve(np, np_grow) || !long_.reserve(np, np_grow) || !new_flag_.reserve(np, np_grow) || !new_len_.reserve(np, np_grow) || !new_idx_.reserve(np, np_grow) ||
      !new_off_.reserve(np, np_grow) || !counters_.reserve(HG_VALSTORE_COUNTERS, HG_VALSTORE_COUNTERS) || !temp_.reserve(tb, tb + tb / 4) || !totals_.reserve(4, 4)) {
    *err = "value store: out of memory (" + std::to_string(ng) + " groups)";
    return HG_ERR_NOMEM;
  }
  HgValStoreArgs a{};
  a.text = groups.args.text;
  a.arena = HgGatherText{arena_.get()};
  a.parts = groups.args.parts;
  a.part_pattern = groups.args.part_pattern;
  a.n_parts = in.values.n_parts;
  a.src = groups.args.src;
  a.len = groups.args.len;
  a.hash = groups.args.hash;
  a.g_first = groups.d_first;
  a.g_count = groups.d_count;
  a.n_groups = ng;
  a.flags = in.values.flags;
  a.store_log2 = log2_old;
  a.slot = slot_.get();
  a.n_values = n_old;
  a.v_off = v_off_.get();
  a.v_count = v_count_.get();
  a.v_first = v_first_.get();
  a.v_line = v_line_.get();
  a.v_hash = v_hash_.get();
  a.v_len = v_len_.get();
  a.v_pattern = v_pattern_.get();
  a.parts_before = parts_before;
  a.arena_tail = tail16;
  a.match = match_.get();
  a.long_list = long_.get();
  a.counters = counters_.get();
  a.new_flag = new_flag_.get();
  a.new_len = new_len_.get();
  a.new_idx = new_idx_.get();
  a.new_off = new_off_.get();
  // 2. lookup (read-only) and 3. the sizes: one host synchronisation reads the two totals
  uint64_t *totals = totals_.get();
  HG_VALSTORE_TRY(hipMemsetAsync(counters_.get(), 0, HG_VALSTORE_COUNTERS * sizeof(unsigned long long), stream), "memset");
  HG_VALSTORE_TRY(hg_valstore_launch(a, HgValStoreStep::Lookup, stream), "launch (lookup)");
  HG_VALSTORE_TRY(hg_valstore_launch(a, HgValStoreStep::Long, stream), "launch (long groups)");
  HG_VALSTORE_TRY(hg_valstore_launch(a, HgValStoreStep::Size, stream), "launch (size)");
  {
    size_t t = temp_.cap();
    HG_VALSTORE_TRY(rocprim::exclusive_scan(temp_.get(), t, new_flag_.get(), new_idx_.get(), uint64_t{0}, np, rocprim::plus<uint64_t>(), stream), "scan (new values)");
    t = temp_.cap();
    HG_VALSTORE_TRY(rocprim::exclusive_scan(temp_.get(), t, new_len_.get(), new_off_.get(), uint64_t{0}, np, rocprim::plus<uint64_t>(), stream), "scan (new bytes)");
  }
  HG_VALSTORE_TRY(hipMemcpyAsync(totals, new_idx_.get() + ng, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy count");
  HG_VALSTORE_TRY(hipMemcpyAsync(totals + 1, new_off_.get() + ng, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy bytes");
  HG_VALSTORE_TRY(hipMemcpyAsync(totals + 2, counters_.get(), HG_VALSTORE_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy counters");
  HG_VALSTORE_TRY(hipStreamSynchronize(stream), "stream sync");
  const uint64_t n_new = totals[0], new_bytes = totals[1], n_after = n_old + n_new;
  if (totals[2 + HG_VALSTORE_OVERFLOW] || n_new > ng) {
    *err = "value store: a probe went round the whole table of 2^" + std::to_string(log2_old) + " slots";
    return HG_ERR_NOMEM;
  }
  // the table the store has after the call
  uint32_t log2_new = in.store_log2 ? in.store_log2 : std::max(log2_old, hg_valstore_default_log2(n_after));
  if (log2_new > HG_VALUES_MAX_TABLE_LOG2 || (uint64_t{1} << log2_new) <= n_after) {
    *err = "value store: " + std::to_string(n_after) + " distinct values do not fit a table of 2^" + std::to_string(std::min(log2_new, HG_VALUES_MAX_TABLE_LOG2)) + " slots with one to spare";
    return HG_ERR_NOMEM;
  }
  // every buffer the rest of the call writes, now: the rows and the arena keep their contents, the table is built aside
  const uint64_t cap_new = uint64_t{1} << log2_new, nv = std::max<uint64_t>(n_after, 1), nv_grow = nv + nv / 2;
  const uint64_t padded = (new_bytes + 15) & ~static_cast<uint64_t>(15), arena_need = std::max<uint64_t>(tail16 + padded, 16), arena_grow = arena_need + arena_need / 2;
  // (with reset the old store is kept too, until the call can no longer run out of memory)
  const uint64_t n_spans = (new_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE, keep_rows = began_ ? n_values_ : 0, keep_arena = began_ ? tail_ : 0;
  const uint64_t keep_slots = began_ && log2_ ? uint64_t{1} << log2_ : 0;
  const bool rebuild = !fresh && n_old && log2_new != log2_old;
  const bool ok = v_off_.grow(nv, nv_grow, keep_rows, stream) && v_count_.grow(nv, nv_grow, keep_rows, stream) && v_first_.grow(nv, nv_grow, keep_rows, stream) &&
                  v_line_.grow(nv, nv_grow, keep_rows, stream) && v_hash_.grow(nv, nv_grow, keep_rows, stream) && v_len_.grow(nv, nv_grow, keep_rows, stream) &&
                  v_pattern_.grow(nv, nv_grow, keep_rows, stream) && arena_.grow(arena_need, arena_grow, keep_arena, stream) && entries_.reserve(n_new + 1, n_new + n_new / 4 + 1) &&
                  ent_off_.reserve(n_new + 1, n_new + n_new / 4 + 1) && span_.reserve(n_spans + 1, n_spans + n_spans / 8 + 1) &&
                  (rebuild ? slot_new_.reserve(cap_new, cap_new) : slot_.grow(cap_new, cap_new, keep_slots, stream));
  if (!ok) {
    *err = "value store: out of memory (" + std::to_string(n_after) + " distinct values, " + std::to_string(tail16 + new_bytes) + " bytes, a table of 2^" + std::to_string(log2_new) + " slots)";
    return HG_ERR_NOMEM;
  }
  a.arena = HgGatherText{arena_.get()};
  a.v_off = v_off_.get();
  a.v_count = v_count_.get();
  a.v_first = v_first_.get();
  a.v_line = v_line_.get();
  a.v_hash = v_hash_.get();
  a.v_len = v_len_.get();
  a.v_pattern = v_pattern_.get();
  a.max_values = n_after;
  a.entries = entries_.get();
  a.ent_off = ent_off_.get();
  // from here on the store changes, and what is left can only fail with a HIP error: the store is emptied then
  const auto finish = [&]() -> int {
    if (rebuild) {  // the stored values into a table of the new size, which then is the store's
      a.slot_new = slot_new_.get();
      a.new_log2 = log2_new;
      HG_VALSTORE_TRY(hipMemsetAsync(slot_new_.get(), 0xFF, cap_new * sizeof(unsigned long long), stream), "memset");  // HG_VALUES_EMPTY
      HG_VALSTORE_TRY(hg_valstore_launch(a, HgValStoreStep::Rehash, stream), "launch (rehash)");
      HG_VALSTORE_TRY(hipStreamSynchronize(stream), "stream sync");  // (nothing queued reads the old table when it changes hands)
      slot_.swap(slot_new_);
    } else if (!n_old) {
      HG_VALSTORE_TRY(hipMemsetAsync(slot_.get(), 0xFF, cap_new * sizeof(unsigned long long), stream), "memset");
    }
    a.slot = slot_.get();
    a.store_log2 = log2_new;
    began_ = true, flags_ = in.values.flags, hash_bits_ = in.values.hash_bits, log2_ = log2_new;
    n_values_ = n_after, n_parts_ = parts_before + in.values.n_parts, tail_ = tail16 + new_bytes, n_bytes_ = bytes_before + new_bytes;
    // 4. apply and 5. the new values' bytes, from the text to the arena's tail
    HG_VALSTORE_TRY(hg_valstore_launch(a, HgValStoreStep::Apply, stream), "launch (apply)");
    HgGatherArgs g{};
    g.text = a.text;
    g.entries = entries_.get();
    g.off = ent_off_.get();
    g.n_entries = n_new;
    g.n_bytes = new_bytes;
    g.span = span_.get();
    g.out = arena_.get() + tail16;
    HG_VALSTORE_TRY(hg_gather_launch(g, HgGatherStep::Span, stream), "launch (spans)");  // (nothing without bytes)
    HG_VALSTORE_TRY(hg_gather_launch(g, HgGatherStep::Copy, stream), "launch (copy)");
    HG_VALSTORE_TRY(hipMemcpyAsync(totals + 2, counters_.get(), HG_VALSTORE_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy counters");
    HG_VALSTORE_TRY(hipEventRecord(ev_[1], stream), "event");
    HG_VALSTORE_TRY(hipStreamSynchronize(stream), "stream sync");
    HG_VALSTORE_TRY(hipEventElapsedTime(&out->ms_acc, ev_[0], ev_[1]), "event time");
    if (totals[2 + HG_VALSTORE_OVERFLOW]) {  // (a table with a slot to spare has room for every claim)
      *err = "value store: a claim went round the whole table of 2^" + std::to_string(log2_new) + " slots";
      return HG_ERR_HIP;
    }
    return HG_OK;
  };
  if (const int rc_finish = finish()) {
    reset();
    *err += "; the store is emptied";
    return rc_finish;
  }
  out->n_distinct = n_after;
  out->n_added = n_new;
  out->n_groups = ng;
  out->n_parts = in.values.n_parts;
  out->n_parts_total = n_parts_;
  out->n_bytes = n_bytes_;
  out->store_log2 = log2_new;
  return HG_OK;
}

int HgValueStore::rank(uint64_t top, bool order_first, hipStream_t stream, HgValRankOutput *out, std::string *err) {
  *out = HgValRankOutput{};
  HG_VALSTORE_TRY(hipSetDevice(device_), "hipSetDevice");
  for (hipEvent_t &e : ev_)
    if (!e) HG_VALSTORE_TRY(hipEventCreate(&e), "event");
  HG_VALSTORE_TRY(hipEventRecord(ev_[0], stream), "event");
  const uint64_t n = n_values_, rows = (top && top < n) ? top : n, np = rows + 1, np_grow = np + np / 4, nn = std::max<uint64_t>(n, 1);
  uint32_t bits = 1;
  while (bits < 64 && (n_parts_ >> bits)) bits++;  // count <= the accumulated parts
  size_t t_sort = 0, t_scan = 0;
  HG_VALSTORE_TRY(rocprim::radix_sort_pairs_desc(nullptr, t_sort, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), rocprim::counting_iterator<uint64_t>(0),
                                                 static_cast<uint64_t *>(nullptr), nn, 0, bits, stream),
                  "sort size");
  HG_VALSTORE_TRY(rocprim::exclusive_scan(nullptr, t_scan, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), uint64_t{0}, np, rocprim::plus<uint64_t>(), stream), "scan size");
  const size_t tb = std::max<size_t>(std::max(t_sort, t_scan), 16);
  if ((!order_first && (!r_keys_.reserve(nn, nn + nn / 4) || !r_order_.reserve(nn, nn + nn / 4))) || !r_count_.reserve(np, np_grow) || !r_first_.reserve(np, np_grow) ||
      !r_line_.reserve(np, np_grow) || !r_size_.reserve(np, np_grow) || !r_off_.reserve(np, np_grow) || !r_pattern_.reserve(np, np_grow) || !r_entries_.reserve(np, np_grow) ||
      !temp_.reserve(tb, tb + tb / 4) || !totals_.reserve(4, 4)) {
    *err = "value store: out of memory (ranking " + std::to_string(n) + " distinct values)";
    return HG_ERR_NOMEM;
  }
  if (!order_first && n) {  // stable: ties stay in index order, which is the order of first
    size_t t = temp_.cap();
    HG_VALSTORE_TRY(rocprim::radix_sort_pairs_desc(temp_.get(), t, v_count_.get(), r_keys_.get(), rocprim::counting_iterator<uint64_t>(0), r_order_.get(), n, 0, bits, stream), "sort (count)");
  }
  HgValRankArgs a{};
  a.n_values = n;
  a.n_rows = rows;
  a.order = order_first ? nullptr : r_order_.get();
  a.v_off = v_off_.get();
  a.v_count = v_count_.get();
  a.v_first = v_first_.get();
  a.v_line = v_line_.get();
  a.v_len = v_len_.get();
  a.v_pattern = v_pattern_.get();
  a.out_count = r_count_.get();
  a.out_first = r_first_.get();
  a.out_line = r_line_.get();
  a.out_pattern = r_pattern_.get();
  a.size = r_size_.get();
  a.entries = r_entries_.get();
  HG_VALSTORE_TRY(hg_valstore_place_launch(a, stream), "launch (place)");
  {
    size_t t = temp_.cap();
    HG_VALSTORE_TRY(rocprim::exclusive_scan(temp_.get(), t, r_size_.get(), r_off_.get(), uint64_t{0}, np, rocprim::plus<uint64_t>(), stream), "scan (lengths)");
  }
  uint64_t *totals = totals_.get();
  HG_VALSTORE_TRY(hipMemcpyAsync(totals, r_off_.get() + rows, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "copy bytes");
  HG_VALSTORE_TRY(hipStreamSynchronize(stream), "stream sync");
  HgGatherArgs g{};
  g.text = HgGatherText{arena_.get()};
  g.entries = r_entries_.get();
  g.off = r_off_.get();
  g.n_entries = rows;
  g.n_bytes = totals[0];
  const uint64_t padded = (g.n_bytes + 15) & ~static_cast<uint64_t>(15), n_spans = (g.n_bytes + HG_GATHER_TILE - 1) / HG_GATHER_TILE;
  if (g.n_bytes > n_bytes_) {
    *err = "value store: more bytes in the kept rows than in the store";
    return HG_ERR_HIP;
  }
  if (!r_bytes_.reserve(std::max<uint64_t>(padded, 16), std::max<uint64_t>(padded + padded / 8, 16)) || !r_span_.reserve(n_spans + 1, n_spans + n_spans / 8 + 1)) {
    *err = "value store: out of memory for " + std::to_string(g.n_bytes) + " bytes of values";
    return HG_ERR_NOMEM;
  }
  g.span = r_span_.get();
  g.out = r_bytes_.get();
  HG_VALSTORE_TRY(hg_gather_launch(g, HgGatherStep::Span, stream), "launch (spans)");  // (nothing without bytes)
  HG_VALSTORE_TRY(hg_gather_launch(g, HgGatherStep::Copy, stream), "launch (copy)");
  HG_VALSTORE_TRY(hipEventRecord(ev_[1], stream), "event");
  HG_VALSTORE_TRY(hipStreamSynchronize(stream), "stream sync");
  HG_VALSTORE_TRY(hipEventElapsedTime(&out->ms_rank, ev_[0], ev_[1]), "event time");
  out->n_values = rows;
  out->n_distinct = n;
  out->n_parts = n_parts_;
  out->n_bytes = g.n_bytes;
  out->d_bytes = r_bytes_.get();
  out->d_off = r_off_.get();
  out->d_count = r_count_.get();
  out->d_first = r_first_.get();
  out->d_line_number = r_line_.get();
  out->d_pattern = r_pattern_.get();
  out->store_log2 = log2_;
  return HG_OK;
}

// ---------------------------------------------------------------- counts stage (hg_count_records): buffers and launch sequence
HgCounts::~HgCounts() {
  (void)hipSetDevice(device_);  // (the buffers are freed behind this body)
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
}

#define HG_COUNTS_TRY(expr, what)                                                   \
  do {                                                                              \
    const hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                         \
      *err = std::string("counts stage: ") + (what) + ": " + hipGetErrorString(e_); \
      return HG_ERR_HIP;                                                            \
    }                                                                               \
  } while (0)

int HgCounts::run(const HgCountsInput &in, hipStream_t stream, HgCountsOutput *out, std::string *err) {
  *out = HgCountsOutput{};
  HG_COUNTS_TRY(hipSetDevice(device_), "hipSetDevice");
  for (hipEvent_t &e : ev_)
    if (!e) HG_COUNTS_TRY(hipEventCreate(&e), "event");
  const uint32_t n_bins = static_cast<uint32_t>(ids_host_.size());
  const bool per_seg = (in.flags & HG_COUNTS_F_PER_SEGMENT) != 0;
  const uint64_t cells = per_seg ? static_cast<uint64_t>(in.n_seg) * n_bins : 0;
  const bool fresh = !totals_.get();  // the first run: the bins go up, the totals start from zero
  if (!ids_.reserve(std::max<size_t>(n_bins, 1), std::max<size_t>(n_bins, 1)) || !totals_.reserve(std::max<size_t>(2 * n_bins, 1), std::max<size_t>(2 * n_bins, 1)) ||
      (cells && (!seg_lines_.reserve(cells, cells + cells / 4) || !seg_reports_.reserve(cells, cells + cells / 4)))) {
    *err = "counts stage: out of memory";
    return HG_ERR_NOMEM;
  }
  HG_COUNTS_TRY(hipEventRecord(ev_[0], stream), "event");
  if (fresh && n_bins) HG_COUNTS_TRY(hipMemcpyAsync(ids_.get(), ids_host_.data(), n_bins * sizeof(uint32_t), hipMemcpyHostToDevice, stream), "copy ids");
  if ((fresh || !(in.flags & HG_COUNTS_F_ACCUMULATE)) && n_bins) HG_COUNTS_TRY(hipMemsetAsync(totals_.get(), 0, 2 * n_bins * sizeof(unsigned long long), stream), "memset");
  if (cells) {
    HG_COUNTS_TRY(hipMemsetAsync(seg_lines_.get(), 0, cells * sizeof(uint32_t), stream), "memset");
    HG_COUNTS_TRY(hipMemsetAsync(seg_reports_.get(), 0, cells * sizeof(uint32_t), stream), "memset");
  }
  HgCountsArgs a{};
  a.list = in.list;
  a.ids = ids_.get();
  a.n_bins = n_bins;
  a.n_seg = per_seg ? in.n_seg : 0;
  a.n_lines = totals_.get();
  a.n_reports = totals_.get() + n_bins;
  a.seg_lines = cells ? seg_lines_.get() : nullptr;
  a.seg_reports = cells ? seg_reports_.get() : nullptr;
  HG_COUNTS_TRY(hg_counts_launch(a, stream), "launch");
  HG_COUNTS_TRY(hipEventRecord(ev_[1], stream), "event");
  HG_COUNTS_TRY(hipStreamSynchronize(stream), "stream sync");
  HG_COUNTS_TRY(hipEventElapsedTime(&out->ms_counts, ev_[0], ev_[1]), "event time");
  out->n_bins = n_bins;
  out->n_seg = per_seg ? in.n_seg : 0;
  out->n_records = in.list.n;
  out->d_ids = ids_.get();
  out->d_n_lines = reinterpret_cast<const uint64_t *>(a.n_lines);
  out->d_n_reports = reinterpret_cast<const uint64_t *>(a.n_reports);
  out->d_seg_lines = a.seg_lines;
  out->d_seg_reports = a.seg_reports;
  return HG_OK;
}

bool HgCounts::copy_totals(uint64_t *n_lines, uint64_t *n_reports) const {
  const size_t n = ids_host_.size();
  if (!totals_.get()) {
    std::fill(n_lines, n_lines + n, uint64_t{0});
    std::fill(n_reports, n_reports + n, uint64_t{0});
    return true;
  }
  return !n || (hipSetDevice(device_) == hipSuccess && hipMemcpy(n_lines, totals_.get(), n * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(n_reports, totals_.get() + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess);
}
