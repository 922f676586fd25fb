// Face A: the libhs symbols the reference shim links against (hypergrep/lib/c/hyperscanner.c:136,140,165,217,
// 301,323,324), then stream mode (hs_*_stream, hg_scan_stream_batch: hg_flows.hip) and the batched block scan
// (hg_scan_blocks: hg_batch.hip).  hs_scan copies the block to HBM and runs the same stream / filter kernels in
// block mode (the buffer is one scan unit, no line splitting), then delivers reports in ascending end offset.
// Per-call cost is a few launches and two synchronisations, so this face is for compatibility (per-line callers such
// as the reference shim); bulk scanning goes through hyperscan() / hg_scan_device().
// A scratch owns its buffers (hgmem::Buf: freed with the scratch, whatever is added to it).  The three routes that report
// through pinned memory share the wait (wait_done); stream mode and the batched block scan also share one staging set
// (HgStage) and the launch-wait-grow-repeat loop over it (launch_until_fits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hypergrep_amd.h"
#include "hg_batch.h"
#include "hg_batch_launch.h"
#include "hg_compile.h"
#include "hg_engine.h"
#include "hg_flow_rules.h"
#include "hg_flows.h"
#include "hg_mem.h"

namespace {
// What one launch takes at most (stream mode and the batched block scan cut their calls into launches by these)
constexpr uint64_t FLOW_LAUNCH_BYTES = 64u << 20;     // bytes of writes / items (a longer write: several launches)
constexpr uint32_t FLOW_LAUNCH_ITEMS = 1u << 16;      // items
constexpr uint64_t FLOW_SOM_WORK_MAX = 256ull << 20;  // bytes of the SOM lanes' start buffers
constexpr uint32_t BATCH_OUT_MAX = 1u << 24;  // records the batched block scan's pinned report array grows to at most (256 MiB); past it: item by item

template <typename T>
using HostBuf = hgmem::Buf<T, hgmem::Space::Host>;
template <typename T>
using DevBuf = hgmem::Buf<T, hgmem::Space::Dev>;
}  // namespace

// Stream-mode data of a database (none in block mode): where each expression's words sit in a stream's state, and the state
// of a freshly opened stream (header words: HG_PC_START, HG_FLOW_HOLD where the expression holds a trailing '\n').
struct HgFlowDb {
  std::vector<uint32_t> soff;  // npatterns
  std::vector<uint32_t> init;  // swords
  uint32_t swords = 0, ngroups = 0;
  // start of match (HS_MODE_SOM_HORIZON_*; empty / 0 without): the SOM expressions (hg_flow_som_kernel's lanes), bytes per
  // carried start (SMALL 2, MEDIUM 4, LARGE 8), the largest SOM automaton, and the horizon (to - from >= 2^horizon_bits:
  // HS_OFFSET_PAST_HORIZON; 0: exact)
  std::vector<uint32_t> som;
  uint32_t som_width = 0, som_total = 0, horizon_bits = 0;
  uint32_t launch_items = 0;  // items per launch at most (SOM databases: bounded by the SOM lanes' start buffers)
};
struct hs_database {
  std::shared_ptr<HgDb> db;
  unsigned int mode = HS_MODE_BLOCK;
  std::shared_ptr<const HgFlowDb> flow;  // HS_MODE_STREAM only
};
struct hs_stream {
  std::shared_ptr<HgDb> db;
  std::shared_ptr<const HgFlowDb> flow;
  std::vector<uint32_t> state;  // flow->swords words (hg_core.h, flows)
  bool terminated = false;
  HgFlowRuleState rules;        // offset, SINGLEMATCH ids reported, recent reports (hg_flow_rules.h)
};
// What a launch with pinned reports needs (launch_until_fits).  A scratch serves one database, whose mode never changes, so
// there is one set per scratch: stream mode or the batched block scan uses it, whichever the database allows.
struct HgStage {
  HostBuf<uint8_t> text{"hs st_text"};  // the launch's writes / items, packed; their copy in HBM
  DevBuf<uint8_t> dtext{"hs st_dtext"};
  HostBuf<uint32_t> flag{"hs st_flag", 0};  // 4 words: [0] reports of the launch, [1] completion word (the launch's seq)
  DevBuf<uint32_t> dctr{"hs st_dctr", 0};   // 4 words: the kernel's counters, cleared once (the last workgroup resets them)
  HostBuf<HgHit> out{"hs st_out", 0};       // the report array; out.cap() is its capacity in records
  HostBuf<int64_t> from{"hs st_from", 0};   // (with_from: stream mode with start of match) the starts beside it, as many
  bool with_from = false;
};
struct hs_scratch {
  std::shared_ptr<HgDb> db;
  HgScanner *sc = nullptr;
  // (destroyed after the buffers below: members go in reverse order, after ~hs_scratch has deleted the scanner)
  struct Stream {
    hipStream_t h = nullptr;
    ~Stream() { if (h) (void)hipStreamDestroy(h); }
    operator hipStream_t() const { return h; }
  } stream;
  DevBuf<uint8_t> d_text{"hs d_text"};
  std::vector<HgHit> hits;
  std::vector<uint32_t> from;  // (SOM databases) the start of each hit
  std::vector<uint32_t> order;
  // short blocks (HgScanner::launch_block_small): pinned copies of the block and of the raw reports
  HostBuf<uint8_t> h_text{"hs h_text"};
  HostBuf<HgHit> h_out{"hs h_out", 0};
  HostBuf<uint32_t> h_counts{"hs h_counts", 0};  // [0, 64) reports per segment, [64] completion flag
  uint32_t seq = 0;  // of the last launch that reports through a pinned completion word (next_seq)
  HgStage stage;  // allocated at the first stream call / hg_scan_blocks call, as everything below
  // stream mode (hg_flow_scan_kernel): pinned items and states, the expressions' state offsets on the device
  HostBuf<HgFlowItem> f_items{"hs f_items"};
  HostBuf<uint32_t> f_sin{"hs f_sin"}, f_sout{"hs f_sout"};
  DevBuf<uint32_t> f_dsoff{"hs f_dsoff"};
  // ... with start of match: the SOM expressions on the device, the SOM lanes' start buffers
  DevBuf<uint32_t> f_dsom{"hs f_dsom"};
  DevBuf<int64_t> f_dwork{"hs f_dwork"};
  // batched block scan (hg_block_batch_kernel): the pinned item table and its copy in HBM
  HostBuf<HgBatchItem> b_items{"hs b_items"};
  DevBuf<HgBatchItem> b_ditems{"hs b_ditems", 0};

  ~hs_scratch() {  // the scanner, the buffers, the stream: in this order, on the scanner's device
    if (sc) (void)hipSetDevice(sc->device());
    delete sc;
  }
};

namespace {
inline void cpu_relax() {  // a polite spin-wait hint, whatever the host is
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#else
  std::this_thread::yield();
#endif
}

uint32_t next_seq(hs_scratch_t *sc) { return ++sc->seq ? sc->seq : ++sc->seq; }  // (never 0)

// Waits for a kernel's completion word in pinned memory to become `seq` (a few microseconds of polling; a stream
// synchronisation sleeps until an interrupt); after ~2 ms of polling falls back to the synchronisation, which also reports
// errors.  false: the stream failed, or ended without the word.
bool wait_done(hipStream_t stream, const uint32_t *word, uint32_t seq) {
  const volatile uint32_t *flag = word;
  bool done = false;
  for (uint32_t spin = 0; spin < 400000 && !(done = *flag == seq); spin++) cpu_relax();
  if (!done && hipStreamSynchronize(stream) != hipSuccess) return false;
  std::atomic_thread_fence(std::memory_order_acquire);
  return *flag == seq;
}

constexpr int LAUNCH_TOO_MANY = 1;  // launch_until_fits: more reports than the report array may grow to (a result, not an error)

// One launch that reports into the scratch's pinned report array (after stage_setup), repeated with a larger array while its reports do not fit
// (so a launch must leave its input untouched).  launch(seq, out, from, cap) -> 0 or an error: starts the kernels on
// sc->stream with room for `cap` reports; they publish the count in stage.flag[0], then `seq` in stage.flag[1].
// grow(total, cap) -> the capacity to repeat with after `total` reports did not fit `cap`, 0 (anything below `total`) if the array may not grow so far.
// Returns HS_SUCCESS with the count in *total, LAUNCH_TOO_MANY, HS_NOMEM, HS_INVALID or launch's error.
// The stage's flag words and device counters, at a scratch's first launch.  flow_launch and batch_launch call it before they
// allocate anything else: the pinned flag words are then the scratch's first staging allocation, as they have always been (with
// them after the text and state buffers, report-heavy batches measured 2-4 % slower: profiles/hsface_refactor_bench.txt).
int stage_setup(hs_scratch_t *sc) {
  HgStage &st = sc->stage;
  if (!st.flag.get()) {
    if (!st.flag.reserve(4, 4)) return HS_NOMEM;
    st.flag.get()[0] = st.flag.get()[1] = 0;
  }
  if (!st.dctr.get()) {
    if (!st.dctr.reserve(4, 4)) return HS_NOMEM;
    // (on the scratch's stream, which does not wait for the null stream: ordered before the first launch)
    if (hipMemsetAsync(st.dctr.get(), 0, 4 * sizeof(uint32_t), sc->stream) != hipSuccess) return HS_NOMEM;
  }
  return HS_SUCCESS;
}
template <typename Grow, typename Launch>
int launch_until_fits(hs_scratch_t *sc, Grow &&grow, Launch &&launch, uint32_t *total) {
  HgStage &st = sc->stage;
  for (uint32_t cap = static_cast<uint32_t>(std::max<size_t>(st.out.cap(), 4096));;) {
    if (!st.out.reserve(cap, cap) || (st.with_from && !st.from.reserve(cap, cap))) return HS_NOMEM;
    const uint32_t seq = next_seq(sc);
    if (int rc = launch(seq, st.out.get(), st.from.get(), cap)) return rc;
    if (!wait_done(sc->stream, st.flag.get() + 1, seq)) return HS_INVALID;
    *total = st.flag.get()[0];
    if (*total <= cap) return HS_SUCCESS;
    if ((cap = grow(*total, cap)) < *total) return LAUNCH_TOO_MANY;
  }
}

// The one-launch block path (HgScanner::launch_block_small, hg_block_batch_kernel) takes this database.  Databases with
// HS_FLAG_SOM_LEFTMOST expressions take the general path: its start-of-match pass fills `from`; so do databases with
// combinations or QUIET expressions (its combination pass applies them), with offset bounds and with a min_length that can
// remove reports (its match-length pass applies it).
bool block_small_db(const HgDb &d) {
  static const bool enabled = !std::getenv("HG_NO_BLOCK_SMALL");
  return enabled && !d.nsom && !d.comb_pass() && d.bounds.empty() && d.min_lengths.empty();
}

// The general path of a block scan (hs_scan's tail; hg_scan_blocks for what its kernel does not take): the block copied to
// HBM, HgScanner::scan_block, the reports copied back into scratch->hits / from, their delivery order (to, id) in
// scratch->order.  HS_SUCCESS or an error.
int block_general(hs_scratch_t *scratch, const char *data, unsigned int length) {
  if (!scratch->d_text.reserve(length, std::max<size_t>(length, 4096) * 2)) return HS_NOMEM;
  uint8_t *d_text = scratch->d_text.get();
  if (hipMemcpyAsync(d_text, data, length, hipMemcpyHostToDevice, scratch->stream) != hipSuccess) return HS_INVALID;
  HgScanOutput out{};
  if (scratch->sc->scan_block(d_text, length, scratch->stream, &out) != HG_OK) {
    std::fprintf(stderr, "hypergrep_amd: block scan (hs_scan / hg_scan_blocks): %s\n", scratch->sc->last_error().c_str());
    return HS_INVALID;
  }
  scratch->hits.resize(out.n_hits);
  scratch->from.assign(out.n_hits, 0u);
  if (out.n_hits) {
    if (hipMemcpyAsync(scratch->hits.data(), out.d_hits, out.n_hits * sizeof(HgHit), hipMemcpyDeviceToHost, scratch->stream) != hipSuccess ||
        (out.d_from && hipMemcpyAsync(scratch->from.data(), out.d_from, out.n_hits * sizeof(uint32_t), hipMemcpyDeviceToHost, scratch->stream) != hipSuccess) ||
        hipStreamSynchronize(scratch->stream) != hipSuccess)
      return HS_INVALID;
  }
  // device order is (id, to); Hyperscan delivers by ascending end offset (ties by id here)
  auto &h = scratch->hits;
  auto &order = scratch->order;
  order.resize(h.size());
  for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return h[a].to != h[b].to ? h[a].to < h[b].to : h[a].id < h[b].id; });
  return HS_SUCCESS;
}

// block_general, then the reports to emit(id, from, to) in delivery order up to the first non-zero return.  HS_SUCCESS,
// HS_SCAN_TERMINATED (emit returned non-zero) or an error.
template <typename Emit>
int block_general_deliver(hs_scratch_t *scratch, const char *data, unsigned int length, Emit &&emit) {
  if (int rc = block_general(scratch, data, length)) return rc;
  const auto &h = scratch->hits;
  for (uint32_t i : scratch->order)
    if (emit(h[i].id, scratch->from[i], h[i].to)) return HS_SCAN_TERMINATED;
  return HS_SUCCESS;
}

// The stream-mode data of a compiled database.  Null, with the expression's index in *bad and the reason in *msg, when a flow
// cannot carry one of its expressions.
std::shared_ptr<HgFlowDb> flow_db(const HgDb &db, unsigned int horizon, int *bad, std::string *msg) {
  const uint32_t np = static_cast<uint32_t>(db.patterns.size());
  for (uint32_t i = 0; i < db.min_lengths.size(); i++) {  // (a flow carries no starts for expressions without HS_FLAG_SOM_LEFTMOST)
    if (!db.min_lengths[i]) continue;
    *bad = static_cast<int>(i);
    *msg = "expression " + std::to_string(i) + ": min_length that can remove reports is not supported in stream mode";
    return nullptr;
  }
  for (uint32_t i = 0; i < np; i++) {
    const HgPattern &p = db.patterns[i];
    const bool wide = p.nw > HG_MAX_W, som_wide = (p.flags & HG_FLAG_SOM_LEFTMOST) && p.nnodes > HG_FLOW_SOM_NODES;
    if (!wide && !som_wide) continue;
    *bad = static_cast<int>(i);
    *msg = "expression " + std::to_string(i) + ": automaton of more than " +
           (wide ? std::string("1024 positions, too large for stream mode")
                 : std::to_string(HG_FLOW_SOM_NODES) + " positions, too large for start of match in stream mode");
    return nullptr;
  }
  auto flow = std::make_shared<HgFlowDb>();
  flow->som_width = horizon == HS_MODE_SOM_HORIZON_SMALL ? 2u : horizon == HS_MODE_SOM_HORIZON_MEDIUM ? 4u : horizon ? 8u : 0u;
  flow->horizon_bits = horizon == HS_MODE_SOM_HORIZON_SMALL ? 16u : horizon == HS_MODE_SOM_HORIZON_MEDIUM ? 32u : 0u;
  HgFlowLayout l = hg_flow_layout(db.pool.data(), db.patterns.data(), np, flow->som_width);
  flow->soff = std::move(l.soff);
  flow->init = std::move(l.init);
  flow->som = std::move(l.som);
  flow->swords = l.swords;
  flow->som_total = l.som_total;
  flow->launch_items = FLOW_LAUNCH_ITEMS;
  if (l.som_total)  // 2 x 8 bytes per node of every SOM expression and item: at most FLOW_SOM_WORK_MAX bytes per launch
    flow->launch_items = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(FLOW_LAUNCH_ITEMS, FLOW_SOM_WORK_MAX / (16ull * l.som_total))));
  flow->ngroups = (np + HG_FLOW_PPW - 1) / HG_FLOW_PPW;
  return flow;
}
}  // namespace

extern "C" {

int hs_compile_multi(const char *const *expressions, const unsigned int *flags, const unsigned int *ids, unsigned int elements,
                     unsigned int mode, const hs_platform_info_t *platform, hs_database_t **db, hs_compile_error_t **error) {
  return hs_compile_ext_multi(expressions, flags, ids, nullptr, elements, mode, platform, db, error);
}

int hs_compile_ext_multi(const char *const *expressions, const unsigned int *flags, const unsigned int *ids, const hs_expr_ext_t *const *ext,
                         unsigned int elements, unsigned int mode, const hs_platform_info_t *platform, hs_database_t **db,
                         hs_compile_error_t **error) {
  (void)platform;
  if (error) *error = nullptr;
  std::string msg;
  int bad = -1;
  HgDb *raw = nullptr;
  // a horizon bit: stream mode with start of match (include/hypergrep_amd.h, stream mode rule 7)
  const unsigned int horizon = mode & (HS_MODE_SOM_HORIZON_LARGE | HS_MODE_SOM_HORIZON_MEDIUM | HS_MODE_SOM_HORIZON_SMALL);
  mode &= ~horizon;
  bool any_som = false;
  for (unsigned int i = 0; flags && expressions && i < elements; i++) any_som = any_som || (flags[i] & HS_FLAG_SOM_LEFTMOST);
  if (!db || !expressions || elements == 0 || (mode != HS_MODE_BLOCK && mode != HS_MODE_STREAM) || (horizon & (horizon - 1)) ||
      (horizon && mode != HS_MODE_STREAM)) {
    msg = "invalid arguments (block or stream mode, at most one HS_MODE_SOM_HORIZON_* bit with stream mode, at least one expression)";
  } else if (horizon && !any_som) {
    msg = "invalid mode: an HS_MODE_SOM_HORIZON_* bit needs at least one HS_FLAG_SOM_LEFTMOST expression";
  } else if (mode == HS_MODE_STREAM && flags) {  // stream mode: what a flow cannot carry (include/hypergrep_amd.h, rule 7)
    for (unsigned int i = 0; i < elements && bad < 0; i++) {
      const char *rule = (flags[i] & HS_FLAG_SOM_LEFTMOST) && !horizon
                             ? "HS_FLAG_SOM_LEFTMOST in stream mode needs an HS_MODE_SOM_HORIZON_* mode bit"
                         : (flags[i] & HS_FLAG_COMBINATION) ? "HS_FLAG_COMBINATION is not supported in stream mode"
                         : (flags[i] & HS_FLAG_QUIET)       ? "HS_FLAG_QUIET is not supported in stream mode"
                                                            : nullptr;
      if (rule) bad = static_cast<int>(i), msg = "expression " + std::to_string(i) + ": " + rule;
    }
  }
  if (msg.empty() && hgc_compile_ext(expressions, flags, ids, ext, elements, &raw, &msg, &bad) == 0) {
    std::shared_ptr<HgDb> owned(raw, [](HgDb *d) { hgc_free(d); });
    const std::shared_ptr<HgFlowDb> flow = mode == HS_MODE_STREAM ? flow_db(*owned, horizon, &bad, &msg) : nullptr;
    if (flow || mode != HS_MODE_STREAM) {
      *db = new hs_database{owned, mode, flow};
      return HS_SUCCESS;
    }
  }
  if (db) *db = nullptr;
  if (error) {
    hs_compile_error_t *e = static_cast<hs_compile_error_t *>(std::malloc(sizeof(hs_compile_error_t)));
    e->message = strdup(msg.c_str());
    e->expression = bad;
    *error = e;
  }
  return HS_COMPILER_ERROR;
}

int hs_free_compile_error(hs_compile_error_t *error) {
  if (!error) return HS_SUCCESS;
  std::free(error->message);
  std::free(error);
  return HS_SUCCESS;
}

int hs_free_database(hs_database_t *db) {
  delete db;
  return HS_SUCCESS;
}

int hs_alloc_scratch(const hs_database_t *db, hs_scratch_t **scratch) {
  if (!db || !scratch) return HS_INVALID;
  if (*scratch && (*scratch)->db == db->db) return HS_SUCCESS;
  if (*scratch) hs_free_scratch(*scratch);
  *scratch = nullptr;
  std::unique_ptr<hs_scratch_t> s(new hs_scratch_t());  // (a half-built scratch releases what it has on every failure path)
  s->db = db->db;
  std::string err;
  int device = 0;
  if (const char *env = std::getenv("HYPERGREP_DEVICE")) device = std::atoi(env);
  if (HgScanner::create(s->db, device, &s->sc, &err) != HG_OK) {
    std::fprintf(stderr, "hypergrep_amd: hs_alloc_scratch: %s\n", err.c_str());
    return HS_NOMEM;
  }
  if (hipStreamCreateWithFlags(&s->stream.h, hipStreamNonBlocking) != hipSuccess) return HS_NOMEM;
  if (!s->h_text.reserve(HG_BLOCK_SMALL_MAX, HG_BLOCK_SMALL_MAX) || !s->h_out.reserve(64 * HG_BLOCK_SMALL_SEG, 64 * HG_BLOCK_SMALL_SEG) ||
      !s->h_counts.reserve(80, 80))
    return HS_NOMEM;
  s->h_counts.get()[64] = 0;
  *scratch = s.release();
  return HS_SUCCESS;
}

int hs_free_scratch(hs_scratch_t *scratch) {
  delete scratch;  // (~hs_scratch)
  return HS_SUCCESS;
}

int hs_scan(const hs_database_t *db, const char *data, unsigned int length, unsigned int flags, hs_scratch_t *scratch,
            match_event_handler on_event, void *context) {
  (void)flags;
  if (!db || !scratch || !scratch->sc || scratch->db != db->db || (!data && length)) return HS_INVALID;
  if (db->mode != HS_MODE_BLOCK) return HS_DB_MODE_ERROR;
  if (length == 0) return HS_SUCCESS;  // no expression can match the empty buffer (such expressions are rejected at compile time)
  if (hipSetDevice(scratch->sc->device()) != hipSuccess) return HS_INVALID;
  // Short blocks (the reference shim scans line by line, hyperscanner.c:217): one launch on a pinned copy of the block,
  // raw reports straight into pinned memory, the report rules on the host.
  if (length <= HG_BLOCK_SMALL_MAX && block_small_db(*db->db)) {
    uint8_t *h_text = scratch->h_text.get();
    HgHit *h_out = scratch->h_out.get();
    uint32_t *h_counts = scratch->h_counts.get();
    std::memcpy(h_text, data, length);
    std::memset(h_text + length, 0, (16 - (length & 15)) & 15);
    const uint32_t seq = next_seq(scratch);
    const uint32_t segs = scratch->sc->launch_block_small(h_text, length, scratch->stream, h_out, h_counts, h_counts + 64, seq);
    if (segs) {
      if (!wait_done(scratch->stream, h_counts + 64, seq)) return HS_INVALID;
      bool fits = true;
      scratch->hits.clear();
      for (uint32_t g = 0; g < segs && fits; g++) {
        const uint32_t n = h_counts[g];
        fits = n <= HG_BLOCK_SMALL_SEG;
        if (fits) scratch->hits.insert(scratch->hits.end(), h_out + static_cast<size_t>(g) * HG_BLOCK_SMALL_SEG, h_out + static_cast<size_t>(g) * HG_BLOCK_SMALL_SEG + n);
      }
      if (fits) {
        hg_block_rules(scratch->hits);  // (hg_batch.h: every item of hg_scan_blocks runs the same rules)
        for (const HgHit &x : scratch->hits)
          if (on_event && on_event(x.id, 0, x.to, 0, context)) return HS_SCAN_TERMINATED;
        return HS_SUCCESS;
      }
    }
  }
  return block_general_deliver(scratch, data, length,
                               [&](uint32_t id, uint32_t from, uint32_t to) { return on_event ? on_event(id, from, to, 0, context) : 0; });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ stream mode ------
namespace {
// Writes of a launch are copied to HBM once (instead of every workgroup of an item reading them over the host link) when
// bytes x workgroups per item reach this (tools/stream_bench.py measures it; HG_FLOW_HBM_MIN overrides it)
uint64_t flow_hbm_min() {
  static const uint64_t v = [] {
    const char *e = std::getenv("HG_FLOW_HBM_MIN");
    return e ? std::strtoull(e, nullptr, 10) : static_cast<uint64_t>(HG_FLOW_HBM_MIN_DEFAULT);
  }();
  return v;
}

struct FlowReq {   // one write of one stream in one launch
  hs_stream_t *s;
  uint32_t item;   // the caller's item number (callbacks)
  const char *data;
  uint32_t len;
  bool close;
};

// The database's tables a stream-mode launch needs on the device: uploaded at the scratch's first stream call.
int flow_setup(hs_scratch_t *sc, const HgFlowDb &f) {
  if (!sc->f_dsoff.get()) {
    if (!sc->f_dsoff.reserve(f.soff.size(), f.soff.size())) return HS_NOMEM;
    if (hipMemcpy(sc->f_dsoff.get(), f.soff.data(), f.soff.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return HS_NOMEM;
  }
  if (!f.som.empty() && !sc->f_dsom.get()) {
    if (!sc->f_dsom.reserve(f.som.size(), f.som.size())) return HS_NOMEM;
    if (hipMemcpy(sc->f_dsom.get(), f.som.data(), f.som.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return HS_NOMEM;  // (and the offsets)
  }
  sc->stage.with_from = !f.som.empty();
  return HS_SUCCESS;
}

// One launch over `reqs` (distinct streams): their writes scanned, their states advanced; the reports of each request after
// the report rules go to on_event(item, id, to) in (to, id) order, request after request.  A non-zero return terminates
// that stream.  Returns HS_SUCCESS, HS_SCAN_TERMINATED (some stream was terminated) or an error.
template <typename OnEvent>
int flow_launch(hs_scratch_t *sc, const HgFlowDb &f, const std::vector<FlowReq> &reqs, OnEvent &&on_event) {
  const uint32_t n = static_cast<uint32_t>(reqs.size());
  if (int rc = stage_setup(sc)) return rc;
  if (int rc = flow_setup(sc, f)) return rc;
  uint64_t bytes = 0;
  for (const FlowReq &r : reqs) bytes += (static_cast<uint64_t>(r.len) + 15u) & ~15ull;
  const size_t sw = static_cast<size_t>(n) * f.swords;
  HgStage &st = sc->stage;
  if (!st.text.reserve(bytes + 16, std::max<size_t>(bytes + 16, 2 * st.text.cap())) || !sc->f_items.reserve(n, std::max<size_t>(n, 2 * sc->f_items.cap())) ||
      !sc->f_sin.reserve(sw, sw) || !sc->f_sout.reserve(sw, sw))
    return HS_NOMEM;
  uint8_t *h_text = st.text.get();
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; i++) {
    const FlowReq &r = reqs[i];
    sc->f_items.get()[i] = HgFlowItem{at, r.len, r.close ? HG_FLOW_ITEM_CLOSE : 0u};
    if (r.len) std::memcpy(h_text + at, r.data, r.len);
    const uint64_t end = (at + r.len + 15u) & ~15ull;
    std::memset(h_text + at + r.len, 0, end - at - r.len);
    at = end;
    std::memcpy(sc->f_sin.get() + static_cast<size_t>(i) * f.swords, r.s->state.data(), f.swords * sizeof(uint32_t));
  }
  const uint8_t *text = h_text;
  // (the SOM lanes read their write byte by byte: from HBM always, not over the host link)
  if (bytes && (bytes * f.ngroups >= flow_hbm_min() || !f.som.empty())) {
    if (!st.dtext.reserve(bytes, std::max<size_t>(bytes, 1u << 20))) return HS_NOMEM;
    if (hipMemcpyAsync(st.dtext.get(), h_text, bytes, hipMemcpyHostToDevice, sc->stream) != hipSuccess) return HS_INVALID;
    text = st.dtext.get();
  }
  const size_t work = static_cast<size_t>(n) * 2 * f.som_total;  // int64 starts of the SOM lanes (n <= f.launch_items)
  if (!sc->f_dwork.reserve(work, work)) return HS_NOMEM;
  const HgDbView &v = sc->sc->view();
  uint32_t total = 0;
  // (more reports than room: the states in f_sin are untouched, the launch is repeated with room for twice the reports)
  const int launched = launch_until_fits(
      sc, [](uint32_t reports, uint32_t) { return reports > 0x7FFFFFFFu ? 0u : reports * 2; },
      [&](uint32_t seq, HgHit *out, int64_t *from, uint32_t cap) {
        HgFlowArgs a{};
        a.patterns = v.patterns;
        a.pool = v.pool;
        a.npatterns = v.npatterns;
        a.text = text;
        a.items = sc->f_items.get();
        a.soff = sc->f_dsoff.get();
        a.state_in = sc->f_sin.get();
        a.state_out = sc->f_sout.get();
        a.out = out;
        a.cap = cap;
        a.ngroups = f.ngroups;
        a.swords = f.swords;
        a.seq = seq;
        a.d_total = st.dctr.get();
        a.d_done = st.dctr.get() + 1;
        a.h_flag = st.flag.get();
        a.som_list = sc->f_dsom.get();
        a.nsom = static_cast<uint32_t>(f.som.size() / 2);
        a.som_width = f.som_width;
        a.som_work = sc->f_dwork.get();
        a.from_out = from;
        return hg_flow_launch(a, n, sc->stream) != 0 ? HS_INVALID : HS_SUCCESS;
      },
      &total);
  if (launched != HS_SUCCESS) return launched == LAUNCH_TOO_MANY ? HS_NOMEM : launched;  // (2^31 reports and more: the doubled array has no 32-bit capacity)
  // the report rules, per request (hg_flow_rules.h)
  const HgDb &db = *sc->db;
  const bool som = f.som_total != 0;
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> per(n);
  std::vector<std::vector<int64_t>> per_from(som ? n : 0);
  const HgHit *out = st.out.get();
  const int64_t *from = st.from.get();
  for (uint32_t i = 0; i < total; i++) {
    const HgHit &h = out[i];
    per[h.line_no & 0xFFFFFFFFu].emplace_back(static_cast<uint32_t>(h.line_no >> 32), h.to);
    if (som) per_from[h.line_no & 0xFFFFFFFFu].push_back(from[i]);  // (read for SOM expressions only)
  }
  int rc = HS_SUCCESS;
  std::vector<HgFlowRep> reps;
  for (uint32_t i = 0; i < n; i++) {
    hs_stream_t *s = reqs[i].s;
    std::memcpy(s->state.data(), sc->f_sout.get() + static_cast<size_t>(i) * f.swords, f.swords * sizeof(uint32_t));
    hg_flow_rules(db.patterns.data(), db.bounds.empty() ? nullptr : db.bounds.data(), s->rules, reqs[i].len, per[i].data(), per[i].size(), reps,
                  som ? per_from[i].data() : nullptr, f.horizon_bits);
    for (const HgFlowRep &x : reps)
      if (!s->terminated && on_event(reqs[i].item, x.id, x.from, x.to) != 0) s->terminated = true;
    if (s->terminated) rc = HS_SCAN_TERMINATED;
  }
  return rc;
}

void flow_reset(hs_stream_t *s) {
  s->state = s->flow->init;
  s->terminated = false;
  s->rules = HgFlowRuleState{};
}

bool flow_usable(const hs_stream_t *s, const hs_scratch_t *sc) {
  return s && sc && sc->sc && sc->db == s->db && hipSetDevice(sc->sc->device()) == hipSuccess;
}

// hg_scan_stream_batch, after argument checks: the items in launches of at most FLOW_LAUNCH_BYTES / FLOW_LAUNCH_ITEMS, a
// longer write cut over consecutive launches (so every launch holds a stream once, and reports stay in item order)
template <typename OnEvent>
int flow_batch(hs_scratch_t *sc, hs_stream_t *const *streams, const char *const *data, const unsigned int *lengths, const unsigned int *item_flags,
               unsigned int n, OnEvent &&on_event) {
  const HgFlowDb &f = *streams[0]->flow;
  std::vector<FlowReq> reqs;
  uint64_t bytes = 0;
  int rc = HS_SUCCESS;
  // A write longer than one launch takes is cut over consecutive launches; its reports are held back until its last cut and
  // delivered in (to, id) order then, so that one call's reports stay ordered (a cut is not a write boundary for the caller)
  constexpr uint32_t NO_ITEM = 0xFFFFFFFFu;
  uint32_t cut_item = NO_ITEM;
  struct Held {
    uint64_t to;
    uint32_t id;
    uint64_t from;
  };
  std::vector<Held> held;
  auto deliver = [&](uint32_t item, uint32_t id, uint64_t from, uint64_t to) {
    if (item == cut_item) {
      held.push_back(Held{to, id, from});
      return 0;
    }
    return on_event(item, id, from, to);
  };
  auto flush = [&](bool cut_done) {
    int r = reqs.empty() ? HS_SUCCESS : flow_launch(sc, f, reqs, deliver);
    if (cut_done && cut_item != NO_ITEM) {
      hs_stream_t *s = streams[cut_item];
      std::stable_sort(held.begin(), held.end(), [](const Held &a, const Held &b) { return a.to != b.to ? a.to < b.to : a.id < b.id; });
      for (const Held &x : held)
        if (!s->terminated && on_event(cut_item, x.id, x.from, x.to) != 0) s->terminated = true;
      if (s->terminated && r == HS_SUCCESS) r = HS_SCAN_TERMINATED;
      held.clear();
      cut_item = NO_ITEM;
    }
    for (const FlowReq &q : reqs)
      if (q.close) flow_reset(q.s);  // (after the held reports: the reset follows the write's deliveries)
    reqs.clear();
    bytes = 0;
    return r;
  };
  for (unsigned int i = 0; i < n; i++) {
    hs_stream_t *s = streams[i];
    const bool last = item_flags && (item_flags[i] & HG_STREAM_ITEM_LAST);
    uint32_t done = 0;
    const uint32_t len = lengths ? lengths[i] : 0u;
    do {
      const uint32_t room = static_cast<uint32_t>(std::min<uint64_t>(FLOW_LAUNCH_BYTES - bytes, len - done));
      const bool all = done + room == len;
      const bool cut = done > 0 || !all;  // this write spans launches
      if (cut) cut_item = i;
      if (!s->terminated) {
        reqs.push_back(FlowReq{s, i, len ? data[i] + done : nullptr, room, last && all});
        bytes += room;
      } else {
        rc = HS_SCAN_TERMINATED;  // as hs_scan_stream on a terminated stream: nothing scanned or delivered
        if (last && all) flow_reset(s);  // (its LAST still resets it)
      }
      done += room;
      if (cut || bytes >= FLOW_LAUNCH_BYTES || reqs.size() >= f.launch_items) {
        const int r = flush(all);
        if (r != HS_SUCCESS && r != HS_SCAN_TERMINATED) return r;
        if (r == HS_SCAN_TERMINATED) rc = r;
      }
    } while (done < len);
  }
  const int r = flush(true);
  if (r != HS_SUCCESS && r != HS_SCAN_TERMINATED) return r;
  return r == HS_SCAN_TERMINATED ? r : rc;
}
}  // namespace

extern "C" {

int hs_stream_size(const hs_database_t *db, size_t *stream_size) {
  if (!db || !stream_size) return HS_INVALID;
  if (db->mode != HS_MODE_STREAM) return HS_DB_MODE_ERROR;
  *stream_size = sizeof(hs_stream_t) + db->flow->swords * sizeof(uint32_t);
  return HS_SUCCESS;
}

int hs_open_stream(const hs_database_t *db, unsigned int flags, hs_stream_t **stream) {
  (void)flags;
  if (!db || !stream) return HS_INVALID;
  if (db->mode != HS_MODE_STREAM) return HS_DB_MODE_ERROR;
  hs_stream_t *s = new hs_stream_t();
  s->db = db->db;
  s->flow = db->flow;
  flow_reset(s);
  *stream = s;
  return HS_SUCCESS;
}

int hs_scan_stream(hs_stream_t *id, const char *data, unsigned int length, unsigned int flags, hs_scratch_t *scratch, match_event_handler on_event,
                   void *context) {
  (void)flags;
  if (!id || !scratch || (!data && length)) return HS_INVALID;
  if (id->terminated) return HS_SCAN_TERMINATED;
  if (length == 0) return HS_SUCCESS;  // (nothing changes: the state and what is pending stay as they are)
  if (!flow_usable(id, scratch)) return HS_INVALID;
  hs_stream_t *const streams[1] = {id};
  const char *const datas[1] = {data};
  const unsigned int lengths[1] = {length};
  return flow_batch(scratch, streams, datas, lengths, nullptr, 1, [&](uint32_t, uint32_t rid, uint64_t from, uint64_t to) {
    return on_event ? on_event(rid, from, to, 0, context) : 0;
  });
}

int hs_reset_stream(hs_stream_t *id, unsigned int flags, hs_scratch_t *scratch, match_event_handler on_event, void *context) {
  (void)flags;
  if (!id) return HS_INVALID;
  if (on_event && !id->terminated) {
    if (!flow_usable(id, scratch)) return HS_INVALID;
    hs_stream_t *const streams[1] = {id};
    const char *const datas[1] = {nullptr};
    const unsigned int lengths[1] = {0};
    const unsigned int last[1] = {HG_STREAM_ITEM_LAST};
    const int rc = flow_batch(scratch, streams, datas, lengths, last, 1,
                              [&](uint32_t, uint32_t rid, uint64_t from, uint64_t to) { return on_event(rid, from, to, 0, context); });
    if (rc != HS_SUCCESS && rc != HS_SCAN_TERMINATED) return rc;
  }
  flow_reset(id);
  return HS_SUCCESS;
}

int hs_close_stream(hs_stream_t *id, hs_scratch_t *scratch, match_event_handler on_event, void *context) {
  if (!id) return HS_INVALID;
  int rc = HS_SUCCESS;
  if (on_event && !id->terminated) {
    if (!flow_usable(id, scratch)) return HS_INVALID;
    rc = hs_reset_stream(id, 0, scratch, on_event, context);
    if (rc == HS_SCAN_TERMINATED) rc = HS_SUCCESS;
  }
  delete id;
  return rc;
}

int hs_copy_stream(hs_stream_t **to_id, const hs_stream_t *from_id) {
  if (!to_id || !from_id) return HS_INVALID;
  *to_id = new hs_stream_t(*from_id);
  return HS_SUCCESS;
}

int hg_scan_stream_batch(hs_stream_t *const *streams, const char *const *data, const unsigned int *lengths, const unsigned int *item_flags, unsigned int n,
                         hs_scratch_t *scratch, hg_stream_match_handler on_event, void *context) {
  if (n == 0) return HS_SUCCESS;
  if (!streams || !lengths || !scratch || !scratch->sc) return HS_INVALID;
  std::vector<const hs_stream_t *> seen(streams, streams + n);
  for (unsigned int i = 0; i < n; i++) {
    if (!streams[i] || streams[i]->db != scratch->db || (lengths[i] && (!data || !data[i]))) return HS_INVALID;
  }
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return HS_INVALID;
  if (hipSetDevice(scratch->sc->device()) != hipSuccess) return HS_INVALID;
  return flow_batch(scratch, streams, data, lengths, item_flags, n, [&](uint32_t item, uint32_t rid, uint64_t from, uint64_t to) {
    return on_event ? on_event(item, rid, from, to, 0, context) : 0;
  });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------- batched block scan ------
namespace {
// One launch of hg_block_batch_kernel over the items `pick` (indices into data / lengths, each of 1 .. HG_BLOCK_SMALL_MAX
// bytes): per[k] receives item pick[k]'s reports after the report rules, in (to, id) order.  Returns HS_SUCCESS, an error, or
// LAUNCH_TOO_MANY when the launch's reports exceed what the report array may grow to (the caller then scans these items one by one).
int batch_launch(hs_scratch_t *sc, const char *const *data, const unsigned int *lengths, const std::vector<uint32_t> &pick, std::vector<std::vector<HgHit>> &per) {
  const uint32_t n = static_cast<uint32_t>(pick.size());
  HgStage &st = sc->stage;
  if (int rc = stage_setup(sc)) return rc;
  const uint64_t bytes = hg_batch_bytes(lengths, pick.data(), n);
  if (!st.text.reserve(bytes + 16, std::max<size_t>(bytes + 16, 2 * st.text.cap())) || !sc->b_items.reserve(n, std::max<size_t>(n, 2 * sc->b_items.cap())))
    return HS_NOMEM;
  hg_batch_pack(data, lengths, pick.data(), n, st.text.get(), sc->b_items.get());
  const HgDbView &v = sc->sc->view();
  uint32_t ppw;
  const uint32_t ngroups = hg_block_small_grouping(v.npatterns, &ppw);
  const uint8_t *text = st.text.get();
  const HgBatchItem *items = sc->b_items.get();
  // Every group's workgroups read every item once: past bytes x groups the bytes go to HBM first.  The threshold is the flow
  // path's (HG_FLOW_HBM_MIN), which is no measured optimum there and none here.
  if (bytes * ngroups >= flow_hbm_min()) {
    // ... and the item table with them (every group's workgroups read their shard's entries)
    if (!st.dtext.reserve(bytes, std::max<size_t>(bytes, 1u << 20)) || !sc->b_ditems.reserve(n, std::max<size_t>(n, 4096))) return HS_NOMEM;
    if (hipMemcpyAsync(st.dtext.get(), text, bytes, hipMemcpyHostToDevice, sc->stream) != hipSuccess ||
        hipMemcpyAsync(sc->b_ditems.get(), items, n * sizeof(HgBatchItem), hipMemcpyHostToDevice, sc->stream) != hipSuccess)
      return HS_INVALID;
    text = st.dtext.get();
    items = sc->b_ditems.get();
  }
  uint32_t total = 0;
  // (more reports than room: items keep no state, the launch is repeated with room for all, up to BATCH_OUT_MAX records)
  const int launched = launch_until_fits(
      sc,
      [](uint32_t reports, uint32_t cap) {
        return reports > BATCH_OUT_MAX ? 0u : static_cast<uint32_t>(std::min<uint64_t>(BATCH_OUT_MAX, std::max<uint64_t>(reports, 2ull * cap)));
      },
      [&](uint32_t seq, HgHit *out, int64_t *, uint32_t cap) {
        HgBatchArgs a{};
        a.patterns = v.patterns;
        a.pool = v.pool;
        a.npatterns = v.npatterns;
        a.ppw = ppw;
        a.ngroups = ngroups;
        a.nshards = std::max(1u, std::min(n, HG_BATCH_MAX_WGS / ngroups));
        a.text = text;
        a.items = items;
        a.nitems = n;
        a.out = out;
        a.cap = cap;
        a.seq = seq;
        a.d_total = st.dctr.get();
        a.d_done = st.dctr.get() + 1;
        a.h_flag = st.flag.get();
        return hg_batch_launch(a, sc->stream) != 0 ? HS_INVALID : HS_SUCCESS;
      },
      &total);
  if (launched != HS_SUCCESS) return launched;
  const HgHit *out = st.out.get();
  per.assign(n, {});
  for (uint32_t i = 0; i < total; i++)
    if (out[i].line_no < n) per[out[i].line_no].push_back(out[i]);
  for (auto &h : per) hg_block_rules(h);
  return HS_SUCCESS;
}
}  // namespace

extern "C" {

int hg_scan_blocks(const hs_database_t *db, const char *const *data, const unsigned int *lengths, unsigned int n, hs_scratch_t *scratch,
                   hg_stream_match_handler on_event, void *context) {
  if (n == 0) return HS_SUCCESS;
  if (!db || !lengths || !scratch || !scratch->sc || scratch->db != db->db) return HS_INVALID;
  for (unsigned int i = 0; i < n; i++)
    if (lengths[i] && (!data || !data[i])) return HS_INVALID;
  if (db->mode != HS_MODE_BLOCK) return HS_DB_MODE_ERROR;
  if (hipSetDevice(scratch->sc->device()) != hipSuccess) return HS_INVALID;
  // What the kernel takes is what hs_scan's one-launch path takes; everything else goes item by item through the general path.
  const HgDb &d = *db->db;
  uint32_t ppw;
  const bool kernel_db = block_small_db(d) && !d.nhuge && hg_block_small_grouping(static_cast<uint32_t>(d.patterns.size()), &ppw) <= 64;
  // a launch's reports are counted in 32 bits: at most (bytes + items) x expressions of them
  const uint64_t launch_bytes = std::max<uint64_t>(HG_BLOCK_SMALL_MAX + 16, std::min<uint64_t>(FLOW_LAUNCH_BYTES, 0xF0000000ull / d.patterns.size() / 2));
  int rc = HS_SUCCESS;
  std::vector<uint32_t> pick;
  std::vector<std::vector<HgHit>> per;
  unsigned int i = 0;
  while (i < n) {
    // the next launch: consecutive items [i, end), of them `pick` for the kernel
    pick.clear();
    uint64_t bytes = 0;
    unsigned int end = i;
    for (; end < n && pick.size() < FLOW_LAUNCH_ITEMS && end - i < 4 * FLOW_LAUNCH_ITEMS; end++) {
      const uint32_t len = lengths[end];
      if (!kernel_db || len == 0 || len > HG_BLOCK_SMALL_MAX) continue;
      if (bytes + len + 16 > launch_bytes) break;
      pick.push_back(end);
      bytes += hg_batch_pad16(len);
    }
    bool launched = false;
    if (!pick.empty()) {
      const int r = batch_launch(scratch, data, lengths, pick, per);
      if (r < 0) return r;
      launched = r == HS_SUCCESS;
    }
    // delivery in item order: the launch's items from `per`, the others scanned now
    size_t k = 0;
    for (unsigned int j = i; j < end; j++) {
      const bool picked = k < pick.size() && pick[k] == j;
      if (picked && launched) {
        for (const HgHit &x : per[k])
          if (on_event && on_event(j, x.id, 0, x.to, 0, context)) {
            rc = HS_SCAN_TERMINATED;
            break;
          }
      } else if (lengths[j]) {
        const int r = block_general_deliver(scratch, data[j], lengths[j], [&](uint32_t id, uint32_t from, uint32_t to) {
          return on_event ? on_event(j, id, from, to, 0, context) : 0;
        });
        if (r != HS_SUCCESS && r != HS_SCAN_TERMINATED) return r;
        if (r == HS_SCAN_TERMINATED) rc = r;  // (the rest of this item is dropped, the next items are still scanned)
      }
      if (picked) k++;
    }
    i = end;
  }
  return rc;
}

}  // extern "C"
