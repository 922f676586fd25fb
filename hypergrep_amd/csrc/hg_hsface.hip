// Face A: the libhs symbols the reference shim links against (hypergrep/lib/c/hyperscanner.c:136,140,165,217,
// 301,323,324), stream mode (hs_*_stream, hg_scan_stream_batch: hg_flows.hip) and the batched block scan (hg_scan_blocks: hg_batch.hip), at the end.  hs_scan copies the block to HBM and runs the same stream / filter kernels in
// block mode (the buffer is one scan unit, no line splitting), then delivers reports in ascending end offset.
// Per-call cost is a few launches and two synchronisations, so this face is for compatibility (per-line callers such
// as the reference shim); bulk scanning goes through hyperscan() / hg_scan_device().
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
constexpr uint32_t FLOW_LAUNCH_ITEMS = 1u << 16;      // items one stream-mode launch takes at most
constexpr uint64_t FLOW_SOM_WORK_MAX = 256ull << 20;  // bytes of the SOM lanes' start buffers one launch may take
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
struct hs_scratch {
  std::shared_ptr<HgDb> db;
  HgScanner *sc = nullptr;
  hipStream_t stream = nullptr;
  uint8_t *d_text = nullptr;
  size_t d_cap = 0;
  std::vector<HgHit> hits;
  std::vector<uint32_t> from;  // (SOM databases) the start of each hit
  std::vector<uint32_t> order;
  // short blocks (HgScanner::launch_block_small): pinned copies of the block and of the raw reports
  uint8_t *h_text = nullptr;
  HgHit *h_out = nullptr;
  uint32_t *h_counts = nullptr;  // [0, 64) reports per segment, [64] completion flag
  uint32_t seq = 0;
  // stream mode (hg_flow_scan_kernel), allocated at the first stream call: pinned staging of writes, items and states, the
  // pinned report array, the writes' HBM copy and the kernel's device counters
  uint8_t *f_text = nullptr, *f_dtext = nullptr;
  size_t f_text_cap = 0, f_dtext_cap = 0;
  HgFlowItem *f_items = nullptr;
  uint32_t *f_sin = nullptr, *f_sout = nullptr;
  size_t f_items_cap = 0, f_state_cap = 0;
  HgHit *f_out = nullptr;
  uint32_t f_out_cap = 0;
  uint32_t *f_flag = nullptr, *f_dctr = nullptr, *f_dsoff = nullptr;
  // start of match: the pinned starts beside f_out (f_out_cap of them), the SOM expressions on the device, the SOM lanes'
  // start buffers
  int64_t *f_from = nullptr, *f_dwork = nullptr;
  size_t f_work_cap = 0;
  uint32_t *f_dsom = nullptr;
  // batched block scan (hg_block_batch_kernel), allocated at the first hg_scan_blocks call: pinned staging of the items' bytes
  // and their table, the pinned report array, the bytes' HBM copy, the pinned flag words and the kernel's device counters
  uint8_t *b_text = nullptr, *b_dtext = nullptr;
  size_t b_text_cap = 0, b_dtext_cap = 0;
  HgBatchItem *b_items = nullptr, *b_ditems = nullptr;
  size_t b_items_cap = 0, b_ditems_cap = 0;
  HgHit *b_out = nullptr;
  uint32_t b_out_cap = 0;
  uint32_t *b_flag = nullptr, *b_dctr = nullptr;
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

// The general path of a block scan (hs_scan's tail; hg_scan_blocks for what its kernel does not take): the block copied to
// HBM, HgScanner::scan_block, the reports copied back into scratch->hits / from, their delivery order (to, id) in
// scratch->order.  HS_SUCCESS or an error.
int block_general(hs_scratch_t *scratch, const char *data, unsigned int length) {
  if (scratch->d_cap < length) {
    hgmem::dev_free(scratch->d_text, "hs d_text");
    scratch->d_text = nullptr;
    size_t cap = std::max<size_t>(length, 4096) * 2;
    if (hgmem::dev_alloc(&scratch->d_text, cap + 16, "hs d_text") != hipSuccess) return HS_NOMEM;
    scratch->d_cap = cap;
  }
  if (hipMemcpyAsync(scratch->d_text, data, length, hipMemcpyHostToDevice, scratch->stream) != hipSuccess) return HS_INVALID;
  HgScanOutput out{};
  if (scratch->sc->scan_block(scratch->d_text, length, scratch->stream, &out) != HG_OK) {
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
    std::shared_ptr<HgFlowDb> flow;
    if (mode == HS_MODE_STREAM) {
      flow = std::make_shared<HgFlowDb>();
      const uint32_t np = static_cast<uint32_t>(owned->patterns.size());
      for (uint32_t i = 0; i < np && bad < 0; i++) {
        const HgPattern &p = owned->patterns[i];
        if (p.nw > HG_MAX_W)
          bad = static_cast<int>(i), msg = "expression " + std::to_string(i) + ": automaton of more than 1024 positions, too large for stream mode";
        else if ((p.flags & HG_FLAG_SOM_LEFTMOST) && p.nnodes > HG_FLOW_SOM_NODES)
          bad = static_cast<int>(i), msg = "expression " + std::to_string(i) + ": automaton of more than " + std::to_string(HG_FLOW_SOM_NODES) +
                                           " positions, too large for start of match in stream mode";
      }
      if (bad >= 0) goto fail;
      flow->som_width = horizon == HS_MODE_SOM_HORIZON_SMALL ? 2u : horizon == HS_MODE_SOM_HORIZON_MEDIUM ? 4u : horizon ? 8u : 0u;
      flow->horizon_bits = horizon == HS_MODE_SOM_HORIZON_SMALL ? 16u : horizon == HS_MODE_SOM_HORIZON_MEDIUM ? 32u : 0u;
      HgFlowLayout l = hg_flow_layout(owned->pool.data(), owned->patterns.data(), np, flow->som_width);
      flow->soff = std::move(l.soff);
      flow->init = std::move(l.init);
      flow->som = std::move(l.som);
      flow->swords = l.swords;
      flow->som_total = l.som_total;
      flow->launch_items = FLOW_LAUNCH_ITEMS;
      if (l.som_total)  // 2 x 8 bytes per node of every SOM expression and item: at most FLOW_SOM_WORK_MAX bytes per launch
        flow->launch_items = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(FLOW_LAUNCH_ITEMS, FLOW_SOM_WORK_MAX / (16ull * l.som_total))));
      flow->ngroups = (np + HG_FLOW_PPW - 1) / HG_FLOW_PPW;
    }
    *db = new hs_database{owned, mode, flow};
    return HS_SUCCESS;
  }
fail:
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
  // (a half-built scratch is handed to hs_free_scratch on every failure path: scanner, stream and pinned buffers are released)
  struct Guard {
    hs_scratch_t *p;
    ~Guard() { if (p) hs_free_scratch(p); }
  } s{new hs_scratch()};
  s.p->db = db->db;
  std::string err;
  int device = 0;
  if (const char *env = std::getenv("HYPERGREP_DEVICE")) device = std::atoi(env);
  if (HgScanner::create(s.p->db, device, &s.p->sc, &err) != HG_OK) {
    std::fprintf(stderr, "hypergrep_amd: hs_alloc_scratch: %s\n", err.c_str());
    return HS_NOMEM;
  }
  if (hipStreamCreateWithFlags(&s.p->stream, hipStreamNonBlocking) != hipSuccess) return HS_NOMEM;
  if (hgmem::host_alloc(&s.p->h_text, HG_BLOCK_SMALL_MAX + 16, "hs h_text") != hipSuccess ||
      hgmem::host_alloc(&s.p->h_out, 64 * HG_BLOCK_SMALL_SEG * sizeof(HgHit), "hs h_out") != hipSuccess ||
      hgmem::host_alloc(&s.p->h_counts, 80 * sizeof(uint32_t), "hs h_counts") != hipSuccess)
    return HS_NOMEM;
  s.p->h_counts[64] = 0;
  *scratch = s.p;
  s.p = nullptr;
  return HS_SUCCESS;
}

int hs_free_scratch(hs_scratch_t *scratch) {
  if (!scratch) return HS_SUCCESS;
  if (scratch->sc) (void)hipSetDevice(scratch->sc->device());
  delete scratch->sc;
  hgmem::dev_free(scratch->d_text, "hs d_text");
  hgmem::host_free(scratch->h_text, "hs h_text");
  hgmem::host_free(scratch->h_out, "hs h_out");
  hgmem::host_free(scratch->h_counts, "hs h_counts");
  hgmem::host_free(scratch->f_text, "hs f_text");
  hgmem::dev_free(scratch->f_dtext, "hs f_dtext");
  hgmem::host_free(scratch->f_items, "hs f_items");
  hgmem::host_free(scratch->f_sin, "hs f_sin");
  hgmem::host_free(scratch->f_sout, "hs f_sout");
  hgmem::host_free(scratch->f_out, "hs f_out");
  hgmem::host_free(scratch->f_flag, "hs f_flag");
  hgmem::dev_free(scratch->f_dctr, "hs f_dctr");
  hgmem::dev_free(scratch->f_dsoff, "hs f_dsoff");
  hgmem::host_free(scratch->f_from, "hs f_from");
  hgmem::dev_free(scratch->f_dwork, "hs f_dwork");
  hgmem::dev_free(scratch->f_dsom, "hs f_dsom");
  hgmem::host_free(scratch->b_text, "hs b_text");
  hgmem::dev_free(scratch->b_dtext, "hs b_dtext");
  hgmem::host_free(scratch->b_items, "hs b_items");
  hgmem::dev_free(scratch->b_ditems, "hs b_ditems");
  hgmem::host_free(scratch->b_out, "hs b_out");
  hgmem::host_free(scratch->b_flag, "hs b_flag");
  hgmem::dev_free(scratch->b_dctr, "hs b_dctr");
  if (scratch->stream) (void)hipStreamDestroy(scratch->stream);
  delete scratch;
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
  static const bool small_path = !std::getenv("HG_NO_BLOCK_SMALL");
  // (databases with HS_FLAG_SOM_LEFTMOST expressions take the general path: its start-of-match pass fills `from`; so do databases
  // with combinations or QUIET expressions: its combination pass applies them)
  if (length <= HG_BLOCK_SMALL_MAX && small_path && !db->db->nsom && !db->db->comb_pass() && db->db->bounds.empty()) {
    std::memcpy(scratch->h_text, data, length);
    std::memset(scratch->h_text + length, 0, (16 - (length & 15)) & 15);
    const uint32_t seq = ++scratch->seq ? scratch->seq : ++scratch->seq;  // (never 0)
    const uint32_t segs = scratch->sc->launch_block_small(scratch->h_text, length, scratch->stream, scratch->h_out, scratch->h_counts, scratch->h_counts + 64, seq);
    if (segs) {
      // wait for the kernel's completion word in pinned memory (a few microseconds of polling; a stream synchronisation
      // sleeps until an interrupt); after ~2 ms of polling fall back to the synchronisation, which also reports errors
      volatile uint32_t *flag = scratch->h_counts + 64;
      bool done = false;
      for (uint32_t spin = 0; spin < 400000 && !(done = *flag == seq); spin++) cpu_relax();
      if (!done && hipStreamSynchronize(scratch->stream) != hipSuccess) return HS_INVALID;
      std::atomic_thread_fence(std::memory_order_acquire);
      bool fits = true;
      scratch->hits.clear();
      for (uint32_t g = 0; g < segs && fits; g++) {
        const uint32_t n = scratch->h_counts[g];
        fits = n <= HG_BLOCK_SMALL_SEG;
        if (fits) scratch->hits.insert(scratch->hits.end(), scratch->h_out + static_cast<size_t>(g) * HG_BLOCK_SMALL_SEG, scratch->h_out + static_cast<size_t>(g) * HG_BLOCK_SMALL_SEG + n);
      }
      if (fits) {
        hg_block_rules(scratch->hits);  // (hg_batch.h: every item of hg_scan_blocks runs the same rules)
        for (const HgHit &x : scratch->hits)
          if (on_event && on_event(x.id, 0, x.to, 0, context)) return HS_SCAN_TERMINATED;
        return HS_SUCCESS;
      }
    }
  }
  if (int rc = block_general(scratch, data, length)) return rc;
  const auto &h = scratch->hits;
  for (uint32_t i : scratch->order)
    if (on_event && on_event(h[i].id, scratch->from[i], h[i].to, 0, context)) return HS_SCAN_TERMINATED;
  return HS_SUCCESS;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ stream mode ------
namespace {
constexpr uint64_t FLOW_LAUNCH_BYTES = 64u << 20;  // bytes of writes one launch takes at most (a longer write: several launches)

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

template <typename T>
bool grow_host(T **p, size_t *cap, size_t need, const char *name) {
  if (*cap >= need) return true;
  const size_t n = std::max(need, *cap * 2);
  hgmem::host_free(*p, name);
  *p = nullptr;
  *cap = 0;
  if (hgmem::host_alloc(p, n * sizeof(T) + 16, name) != hipSuccess) return false;
  *cap = n;
  return true;
}

int flow_setup(hs_scratch_t *sc, const HgFlowDb &f) {
  if (!sc->f_flag) {
    if (hgmem::host_alloc(&sc->f_flag, 4 * sizeof(uint32_t), "hs f_flag") != hipSuccess) return HS_NOMEM;
    sc->f_flag[0] = sc->f_flag[1] = 0;
  }
  if (!sc->f_dctr) {
    if (hgmem::dev_alloc(&sc->f_dctr, 4 * sizeof(uint32_t), "hs f_dctr") != hipSuccess) return HS_NOMEM;
    // (on the scratch's stream, which does not wait for the null stream: ordered before the first launch)
    if (hipMemsetAsync(sc->f_dctr, 0, 4 * sizeof(uint32_t), sc->stream) != hipSuccess) return HS_NOMEM;
  }
  if (!sc->f_dsoff) {
    if (hgmem::dev_alloc(&sc->f_dsoff, f.soff.size() * sizeof(uint32_t) + 16, "hs f_dsoff") != hipSuccess) return HS_NOMEM;
    if (hipMemcpy(sc->f_dsoff, f.soff.data(), f.soff.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return HS_NOMEM;
  }
  if (!f.som.empty() && !sc->f_dsom) {
    if (hgmem::dev_alloc(&sc->f_dsom, f.som.size() * sizeof(uint32_t) + 16, "hs f_dsom") != hipSuccess) return HS_NOMEM;
    if (hipMemcpy(sc->f_dsom, f.som.data(), f.som.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return HS_NOMEM;  // (and the offsets)
  }
  return HS_SUCCESS;
}

// The pinned report array and, for SOM databases, the starts beside it: room for `cap` reports.
bool flow_out_alloc(hs_scratch_t *sc, const HgFlowDb &f, uint32_t cap) {
  hgmem::host_free(sc->f_out, "hs f_out");
  hgmem::host_free(sc->f_from, "hs f_from");
  sc->f_out = nullptr;
  sc->f_from = nullptr;
  sc->f_out_cap = 0;
  if (hgmem::host_alloc(&sc->f_out, static_cast<size_t>(cap) * sizeof(HgHit), "hs f_out") != hipSuccess) return false;
  if (!f.som.empty() && hgmem::host_alloc(&sc->f_from, static_cast<size_t>(cap) * sizeof(int64_t), "hs f_from") != hipSuccess) return false;
  sc->f_out_cap = cap;
  return true;
}

// One launch over `reqs` (distinct streams): their writes scanned, their states advanced; the reports of each request after
// the report rules go to on_event(item, id, to) in (to, id) order, request after request.  A non-zero return terminates
// that stream.  Returns HS_SUCCESS, HS_SCAN_TERMINATED (some stream was terminated) or an error.
template <typename OnEvent>
int flow_launch(hs_scratch_t *sc, const HgFlowDb &f, const std::vector<FlowReq> &reqs, OnEvent &&on_event) {
  const uint32_t n = static_cast<uint32_t>(reqs.size());
  if (int rc = flow_setup(sc, f)) return rc;
  uint64_t bytes = 0;
  for (const FlowReq &r : reqs) bytes += (static_cast<uint64_t>(r.len) + 15u) & ~15ull;
  const size_t sw = static_cast<size_t>(n) * f.swords;
  if (!grow_host(&sc->f_text, &sc->f_text_cap, bytes + 16, "hs f_text") || !grow_host(&sc->f_items, &sc->f_items_cap, n, "hs f_items"))
    return HS_NOMEM;
  if (sc->f_state_cap < sw) {  // (f_sin and f_sout have the same capacity)
    hgmem::host_free(sc->f_sin, "hs f_sin");
    hgmem::host_free(sc->f_sout, "hs f_sout");
    sc->f_sin = sc->f_sout = nullptr;
    sc->f_state_cap = 0;
    if (hgmem::host_alloc(&sc->f_sin, sw * sizeof(uint32_t) + 16, "hs f_sin") != hipSuccess ||
        hgmem::host_alloc(&sc->f_sout, sw * sizeof(uint32_t) + 16, "hs f_sout") != hipSuccess)
      return HS_NOMEM;
    sc->f_state_cap = sw;
  }
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; i++) {
    const FlowReq &r = reqs[i];
    sc->f_items[i] = HgFlowItem{at, r.len, r.close ? HG_FLOW_ITEM_CLOSE : 0u};
    if (r.len) std::memcpy(sc->f_text + at, r.data, r.len);
    const uint64_t end = (at + r.len + 15u) & ~15ull;
    std::memset(sc->f_text + at + r.len, 0, end - at - r.len);
    at = end;
    std::memcpy(sc->f_sin + static_cast<size_t>(i) * f.swords, r.s->state.data(), f.swords * sizeof(uint32_t));
  }
  const uint8_t *text = sc->f_text;
  // (the SOM lanes read their write byte by byte: from HBM always, not over the host link)
  if (bytes && (bytes * f.ngroups >= flow_hbm_min() || !f.som.empty())) {
    if (sc->f_dtext_cap < bytes) {
      hgmem::dev_free(sc->f_dtext, "hs f_dtext");
      sc->f_dtext = nullptr;
      sc->f_dtext_cap = 0;
      const size_t cap = std::max<size_t>(bytes, 1u << 20);
      if (hgmem::dev_alloc(&sc->f_dtext, cap + 16, "hs f_dtext") != hipSuccess) return HS_NOMEM;
      sc->f_dtext_cap = cap;
    }
    if (hipMemcpyAsync(sc->f_dtext, sc->f_text, bytes, hipMemcpyHostToDevice, sc->stream) != hipSuccess) return HS_INVALID;
    text = sc->f_dtext;
  }
  const size_t work = static_cast<size_t>(n) * 2 * f.som_total;  // int64 starts of the SOM lanes (n <= f.launch_items)
  if (sc->f_work_cap < work) {
    hgmem::dev_free(sc->f_dwork, "hs f_dwork");
    sc->f_dwork = nullptr;
    sc->f_work_cap = 0;
    if (hgmem::dev_alloc(&sc->f_dwork, work * sizeof(int64_t) + 16, "hs f_dwork") != hipSuccess) return HS_NOMEM;
    sc->f_work_cap = work;
  }
  const HgDbView &v = sc->sc->view();
  uint32_t total = 0;
  for (;;) {
    if (sc->f_out_cap == 0 && !flow_out_alloc(sc, f, 4096)) return HS_NOMEM;
    const uint32_t seq = ++sc->seq ? sc->seq : ++sc->seq;
    HgFlowArgs a{};
    a.patterns = v.patterns;
    a.pool = v.pool;
    a.npatterns = v.npatterns;
    a.text = text;
    a.items = sc->f_items;
    a.soff = sc->f_dsoff;
    a.state_in = sc->f_sin;
    a.state_out = sc->f_sout;
    a.out = sc->f_out;
    a.cap = sc->f_out_cap;
    a.ngroups = f.ngroups;
    a.swords = f.swords;
    a.seq = seq;
    a.d_total = sc->f_dctr;
    a.d_done = sc->f_dctr + 1;
    a.h_flag = sc->f_flag;
    a.som_list = sc->f_dsom;
    a.nsom = static_cast<uint32_t>(f.som.size() / 2);
    a.som_width = f.som_width;
    a.som_work = sc->f_dwork;
    a.from_out = sc->f_from;
    if (hg_flow_launch(a, n, sc->stream) != 0) return HS_INVALID;
    volatile uint32_t *flag = sc->f_flag + 1;
    bool done = false;
    for (uint32_t spin = 0; spin < 400000 && !(done = *flag == seq); spin++) cpu_relax();
    if (!done && hipStreamSynchronize(sc->stream) != hipSuccess) return HS_INVALID;
    std::atomic_thread_fence(std::memory_order_acquire);
    if (*flag != seq) return HS_INVALID;
    total = sc->f_flag[0];
    if (total <= sc->f_out_cap) break;
    // more reports than room: the states in f_sin are untouched, the launch is repeated with room for all
    if (!flow_out_alloc(sc, f, total * 2)) return HS_NOMEM;
  }
  // the report rules, per request (hg_flow_rules.h)
  const HgDb &db = *sc->db;
  const bool som = f.som_total != 0;
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> per(n);
  std::vector<std::vector<int64_t>> per_from(som ? n : 0);
  for (uint32_t i = 0; i < total; i++) {
    const HgHit &h = sc->f_out[i];
    per[h.line_no & 0xFFFFFFFFu].emplace_back(static_cast<uint32_t>(h.line_no >> 32), h.to);
    if (som) per_from[h.line_no & 0xFFFFFFFFu].push_back(sc->f_from[i]);  // (read for SOM expressions only)
  }
  int rc = HS_SUCCESS;
  std::vector<HgFlowRep> reps;
  for (uint32_t i = 0; i < n; i++) {
    hs_stream_t *s = reqs[i].s;
    std::memcpy(s->state.data(), sc->f_sout + static_cast<size_t>(i) * f.swords, f.swords * sizeof(uint32_t));
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
constexpr uint32_t BATCH_OUT_MAX = 1u << 24;  // records the pinned report array grows to at most (256 MiB); past it: item by item

int batch_setup(hs_scratch_t *sc) {
  if (!sc->b_flag) {
    if (hgmem::host_alloc(&sc->b_flag, 4 * sizeof(uint32_t), "hs b_flag") != hipSuccess) return HS_NOMEM;
    sc->b_flag[0] = sc->b_flag[1] = 0;
  }
  if (!sc->b_dctr) {
    if (hgmem::dev_alloc(&sc->b_dctr, 4 * sizeof(uint32_t), "hs b_dctr") != hipSuccess) return HS_NOMEM;
    // (on the scratch's stream, which does not wait for the null stream: ordered before the first launch)
    if (hipMemsetAsync(sc->b_dctr, 0, 4 * sizeof(uint32_t), sc->stream) != hipSuccess) return HS_NOMEM;
  }
  return HS_SUCCESS;
}

bool batch_out_alloc(hs_scratch_t *sc, uint32_t cap) {
  hgmem::host_free(sc->b_out, "hs b_out");
  sc->b_out = nullptr;
  sc->b_out_cap = 0;
  if (hgmem::host_alloc(&sc->b_out, static_cast<size_t>(cap) * sizeof(HgHit), "hs b_out") != hipSuccess) return false;
  sc->b_out_cap = cap;
  return true;
}

// One launch of hg_block_batch_kernel over the items `pick` (indices into data / lengths, each of 1 .. HG_BLOCK_SMALL_MAX
// bytes): per[k] receives item pick[k]'s reports after the report rules, in (to, id) order.  Returns HS_SUCCESS, an error, or
// 1 when the launch's reports exceed what the report array may grow to (the caller then scans these items one by one).
int batch_launch(hs_scratch_t *sc, const char *const *data, const unsigned int *lengths, const std::vector<uint32_t> &pick, std::vector<std::vector<HgHit>> &per) {
  const uint32_t n = static_cast<uint32_t>(pick.size());
  if (int rc = batch_setup(sc)) return rc;
  const uint64_t bytes = hg_batch_bytes(lengths, pick.data(), n);
  if (!grow_host(&sc->b_text, &sc->b_text_cap, bytes + 16, "hs b_text") || !grow_host(&sc->b_items, &sc->b_items_cap, n, "hs b_items")) return HS_NOMEM;
  hg_batch_pack(data, lengths, pick.data(), n, sc->b_text, sc->b_items);
  const HgDbView &v = sc->sc->view();
  uint32_t ppw;
  const uint32_t ngroups = hg_block_small_grouping(v.npatterns, &ppw);
  const uint8_t *text = sc->b_text;
  const HgBatchItem *items = sc->b_items;
  // Every group's workgroups read every item once: past bytes x groups the bytes go to HBM first.  The threshold is the flow
  // path's (HG_FLOW_HBM_MIN), which is no measured optimum there and none here.
  if (bytes * ngroups >= flow_hbm_min()) {
    if (sc->b_dtext_cap < bytes) {
      hgmem::dev_free(sc->b_dtext, "hs b_dtext");
      sc->b_dtext = nullptr;
      sc->b_dtext_cap = 0;
      const size_t cap = std::max<size_t>(bytes, 1u << 20);
      if (hgmem::dev_alloc(&sc->b_dtext, cap + 16, "hs b_dtext") != hipSuccess) return HS_NOMEM;
      sc->b_dtext_cap = cap;
    }
    if (hipMemcpyAsync(sc->b_dtext, sc->b_text, bytes, hipMemcpyHostToDevice, sc->stream) != hipSuccess) return HS_INVALID;
    text = sc->b_dtext;
    // ... and the item table with them (every group's workgroups read their shard's entries)
    if (sc->b_ditems_cap < n) {
      hgmem::dev_free(sc->b_ditems, "hs b_ditems");
      sc->b_ditems = nullptr;
      sc->b_ditems_cap = 0;
      const size_t cap = std::max<size_t>(n, 4096);
      if (hgmem::dev_alloc(&sc->b_ditems, cap * sizeof(HgBatchItem), "hs b_ditems") != hipSuccess) return HS_NOMEM;
      sc->b_ditems_cap = cap;
    }
    if (hipMemcpyAsync(sc->b_ditems, sc->b_items, n * sizeof(HgBatchItem), hipMemcpyHostToDevice, sc->stream) != hipSuccess) return HS_INVALID;
    items = sc->b_ditems;
  }
  uint32_t total = 0;
  for (;;) {
    if (sc->b_out_cap == 0 && !batch_out_alloc(sc, 4096)) return HS_NOMEM;
    const uint32_t seq = ++sc->seq ? sc->seq : ++sc->seq;
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
    a.out = sc->b_out;
    a.cap = sc->b_out_cap;
    a.seq = seq;
    a.d_total = sc->b_dctr;
    a.d_done = sc->b_dctr + 1;
    a.h_flag = sc->b_flag;
    if (hg_batch_launch(a, sc->stream) != 0) return HS_INVALID;
    volatile uint32_t *flag = sc->b_flag + 1;
    bool done = false;
    for (uint32_t spin = 0; spin < 400000 && !(done = *flag == seq); spin++) cpu_relax();
    if (!done && hipStreamSynchronize(sc->stream) != hipSuccess) return HS_INVALID;
    std::atomic_thread_fence(std::memory_order_acquire);
    if (*flag != seq) return HS_INVALID;
    total = sc->b_flag[0];
    if (total <= sc->b_out_cap) break;
    // more reports than room: items keep no state, the launch is repeated with room for all
    if (total > BATCH_OUT_MAX) return 1;
    if (!batch_out_alloc(sc, static_cast<uint32_t>(std::min<uint64_t>(BATCH_OUT_MAX, std::max<uint64_t>(total, 2ull * sc->b_out_cap))))) return HS_NOMEM;
  }
  per.assign(n, {});
  for (uint32_t i = 0; i < total; i++)
    if (sc->b_out[i].line_no < n) per[sc->b_out[i].line_no].push_back(sc->b_out[i]);
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
  static const bool small_path = !std::getenv("HG_NO_BLOCK_SMALL");
  const HgDb &d = *db->db;
  uint32_t ppw;
  const bool kernel_db = small_path && !d.nsom && !d.comb_pass() && d.bounds.empty() && !d.nhuge &&
                         hg_block_small_grouping(static_cast<uint32_t>(d.patterns.size()), &ppw) <= 64;
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
        if (int r = block_general(scratch, data[j], lengths[j])) return r;
        const auto &h = scratch->hits;
        for (uint32_t o : scratch->order)
          if (on_event && on_event(j, h[o].id, scratch->from[o], h[o].to, 0, context)) {
            rc = HS_SCAN_TERMINATED;
            break;
          }
      }
      if (picked) k++;
    }
    i = end;
  }
  return rc;
}

}  // extern "C"
