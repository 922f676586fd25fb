// Face B: hyperscan() and check_patterns() with the reference shim's exact C ABI
// (hypergrep/lib/c/hyperscanner.c:154-159, :248-258), so hypergrep/utils.py:116-121 and :339-349 can call
// this library unchanged.  The file is streamed through pinned memory into HBM in large chunks, each
// chunk is scanned by the device pipeline (HgScanner), and hit records come back to fill the same
// batched result ring the reference fills in hs_callback() (hyperscanner.c:83-102).
//
// Ingest is a three-stage pipeline: a reader thread fills pinned slots (plain files: several pread stripes in
// parallel; gzip / zstd: the decoder) and cuts them at line-piece boundaries, the calling thread copies slot k+1 to
// HBM on a copy stream while slot k is scanned, and delivers slot k's hits from the pinned bytes while the reader is
// already filling the next slot.
//
// What stays on the host: file IO, gzip/zstd decoding (the reference does that on the CPU too, through
// zlibWrapper), cutting chunks at line boundaries, copying matched line bytes into the result ring and
// calling back.  No byte of the text is matched on the CPU.
#include <hip/hip_runtime.h>

#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hypergrep_amd.h"
#include "hg_compile.h"
#include "hg_deliver.h"
#include "hg_engine.h"
#include "hg_mem.h"
#include "hg_reader.h"

namespace {

// ---------------------------------------------------------------- compiled-database cache
// The reference recompiles the database for every file (hyperscanner.c:296); here identical pattern sets share one
// compiled database for the life of the process (at most kDbCacheMax sets, least recently used evicted; scanners keep
// their own reference).  An entry is re-tuned once, on the first large file scanned with it (maybe_tune below).
struct DbEntry {
  std::shared_ptr<const HgDb> db;
  bool tune_tried = false;
  uint64_t stamp = 0;  // last use
};
constexpr size_t kDbCacheMax = 16;
std::mutex g_mu;
std::map<std::string, DbEntry> g_dbs;
uint64_t g_stamp = 0;
std::atomic<uint64_t> g_cache_hits{0}, g_cache_misses{0}, g_tunes{0};

// Extended parameters (hs_expr_ext_t) follow the expressions, one record per expression, only when some expression has any:
// a set without them keeps the key it always had, and no key of a set with them can equal one without (it is longer).
std::string db_key(const char *const *patterns, const unsigned *flags, const unsigned *ids, const hs_expr_ext_t *const *ext, unsigned n) {
  std::string k;
  bool any_ext = false;
  for (unsigned i = 0; i < n; i++) {
    const char *p = patterns[i] ? patterns[i] : "";
    uint32_t len = static_cast<uint32_t>(std::strlen(p)), f = flags ? flags[i] : 0, id = ids ? ids[i] : 0;
    k.append(reinterpret_cast<const char *>(&len), 4);
    k.append(reinterpret_cast<const char *>(&f), 4);
    k.append(reinterpret_cast<const char *>(&id), 4);
    k.append(p, len);
    any_ext = any_ext || (ext && ext[i] && ext[i]->flags);
  }
  if (any_ext)
    for (unsigned i = 0; i < n; i++) {
      hs_expr_ext_t x{};
      if (ext[i] && ext[i]->flags) x = *ext[i];
      const uint64_t words[6] = {x.flags, x.min_offset, x.max_offset, x.min_length, x.edit_distance, x.hamming_distance};
      k.append(reinterpret_cast<const char *>(words), sizeof words);
    }
  return k;
}

std::shared_ptr<const HgDb> get_db(const char *const *patterns, const unsigned *flags, const unsigned *ids, const hs_expr_ext_t *const *ext, unsigned n,
                                   std::string *err, std::string *key_out = nullptr) {
  if (!patterns || n == 0) {
    if (err) *err = "no patterns";
    return nullptr;
  }
  for (unsigned i = 0; i < n; i++)
    if (!patterns[i]) return nullptr;
  std::string key = db_key(patterns, flags, ids, ext, n);
  if (key_out) *key_out = key;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_dbs.find(key);
    if (it != g_dbs.end()) {
      it->second.stamp = ++g_stamp;
      g_cache_hits++;
      return it->second.db;
    }
  }
  g_cache_misses++;
  HgDb *raw = nullptr;
  int bad = -1;
  if (hgc_compile_ext(patterns, flags, ids, ext, n, &raw, err, &bad) != 0) return nullptr;
  std::shared_ptr<const HgDb> db(raw, [](const HgDb *d) { hgc_free(const_cast<HgDb *>(d)); });
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_dbs.find(key);
  if (it != g_dbs.end()) {  // another thread compiled the same set meanwhile: keep one
    it->second.stamp = ++g_stamp;
    return it->second.db;
  }
  while (g_dbs.size() >= kDbCacheMax) {
    auto oldest = g_dbs.begin();
    for (auto j = g_dbs.begin(); j != g_dbs.end(); ++j)
      if (j->second.stamp < oldest->second.stamp) oldest = j;
    g_dbs.erase(oldest);
  }
  DbEntry e;
  e.db = db;
  e.stamp = ++g_stamp;
  g_dbs.emplace(std::move(key), std::move(e));
  return db;
}

// The window prefilter picks, per required literal, WHICH four bytes of it the stream pass looks for.  Statically that is
// a guess from byte frequencies of English-like logs; with a sample of the actual text it is the window that is rarest in
// that text (bench.py's workload: first-level matches 4 % -> 1.2 % of dwords).  The file API does this by itself: the
// first time a pattern set meets a file of at least HYPERGREP_TUNE_MIN_MB (default 32; 0 = never), 1 MiB of the first
// ingest chunk (four spread pieces) is sampled on the host (~20 ms), the tuned copy replaces the cache entry, and this
// and every later call of the pattern set scan with it.  Results never depend on it.
size_t tune_min_bytes() {
  static const size_t v = [] {
    if (const char *env = std::getenv("HYPERGREP_TUNE_MIN_MB")) {
      const long mb = std::atol(env);
      if (mb >= 0 && mb <= (1 << 20)) return static_cast<size_t>(mb) << 20;
    }
    return static_cast<size_t>(32) << 20;
  }();
  return v;
}
std::shared_ptr<const HgDb> maybe_tune(const std::string &key, const std::shared_ptr<const HgDb> &db, const uint8_t *chunk, size_t nbytes) {
  const size_t min_bytes = tune_min_bytes();
  if (db->tuned || !db->nreal_factors || !min_bytes || nbytes < min_bytes) return db;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_dbs.find(key);
    if (it == g_dbs.end() || it->second.tune_tried) return it != g_dbs.end() && it->second.db->tuned ? it->second.db : db;
    it->second.tune_tried = true;  // concurrent calls with the same set scan untuned this once
  }
  constexpr size_t kPiece = 256u << 10, kPieces = 4;
  std::vector<uint8_t> sample;
  sample.reserve(kPiece * kPieces);
  for (size_t i = 0; i < kPieces; i++) {
    const size_t at = (nbytes / kPieces * i) & ~static_cast<size_t>(15);
    const size_t len = std::min(kPiece, nbytes - at);
    sample.insert(sample.end(), chunk + at, chunk + at + len);
  }
  HgDb *raw = nullptr;
  std::string err;
  if (hgc_tune(db.get(), sample.data(), sample.size(), &raw, &err) != 0) return db;
  std::shared_ptr<const HgDb> tuned(raw, [](const HgDb *d) { hgc_free(const_cast<HgDb *>(d)); });
  g_tunes++;
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_dbs.find(key);
  if (it != g_dbs.end()) it->second.db = tuned;
  return tuned;
}

// ---------------------------------------------------------------- per-call device context, pooled
// A context = streams + staging buffers (pinned slots, device text buffers) + the scanner of ONE pattern set.  At most
// HYPERGREP_POOL contexts exist at a time (default 16: the reference's thread pool runs up to ncpu-1 scans, each of them
// link-bound here); a call beyond that waits for one to come back.  Idle contexts are kept, most recently used last: a
// call takes one that already holds its pattern set's scanner if there is one (the reference's use: one pattern set, many
// files), else creates a new context while the bound allows, else re-binds the least recently used idle one (buffers and
// streams stay, the scanner is replaced).
struct Ctx {
  std::shared_ptr<const HgDb> db;  // pattern set of `sc`
  HgScanner *sc = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  static constexpr int kSlots = 3, kDevBufs = 2;
  uint8_t *h_slot[kSlots] = {nullptr, nullptr, nullptr};  // pinned staging buffers
  size_t h_cap = 0;
  uint8_t *d_text[kDevBufs] = {nullptr, nullptr};
  size_t d_cap = 0;
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_h2d[kDevBufs] = {nullptr, nullptr};
  std::vector<HgHit> hits;
  std::vector<HgHitAux> aux;
  ~Ctx() {
    (void)hipSetDevice(device);
    delete sc;
    for (uint8_t *p : h_slot) hgmem::host_free(p, "h_slot");
    for (uint8_t *p : d_text) hgmem::dev_free(p, "d_text");
    for (hipEvent_t e : ev_h2d)
      if (e) (void)hipEventDestroy(e);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
struct Pool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Ctx *> idle;  // least recently used first; intentionally never destroyed at exit (no HIP calls in static dtors)
  size_t live = 0;          // contexts in existence (idle + checked out)
  size_t cap = 16;
  std::atomic<uint64_t> created{0}, reused{0}, rebound{0};
  Pool() {
    if (const char *env = std::getenv("HYPERGREP_POOL")) cap = static_cast<size_t>(std::max(1l, std::min(1024l, std::atol(env))));  // read once
  }
};
Pool &pool() {
  static Pool *p = new Pool();
  return *p;
}
std::atomic<unsigned> g_next_device{0};

}  // namespace
// Device of the next Face B context when the node has `ndev` GPUs: HYPERGREP_DEVICE pins one, else files round-robin.
extern "C" int hg_faceb_next_device(int ndev) {
  if (ndev <= 0) return -1;
  if (const char *env = std::getenv("HYPERGREP_DEVICE")) return std::abs(std::atoi(env)) % ndev;
  return static_cast<int>(g_next_device.fetch_add(1) % static_cast<unsigned>(ndev));
}
// Counters of the caches above (tests, HYPERGREP_TRACE): database cache hits / misses / size, tunes, contexts created /
// reused with their scanner / re-bound to another pattern set / alive.
extern "C" void hg_faceb_stats(uint64_t out[8]) {
  Pool &p = pool();
  out[0] = g_cache_hits;
  out[1] = g_cache_misses;
  out[3] = g_tunes;
  out[4] = p.created;
  out[5] = p.reused;
  out[6] = p.rebound;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    out[2] = g_dbs.size();
  }
  std::lock_guard<std::mutex> lock(p.mu);
  out[7] = p.live;
}
namespace {

Ctx *checkout(const std::shared_ptr<const HgDb> &db, std::string *err) {
  Pool &p = pool();
  Ctx *c = nullptr;
  {
    std::unique_lock<std::mutex> lock(p.mu);
    for (;;) {
      for (size_t i = p.idle.size(); i-- > 0;)
        if (p.idle[i]->db == db) {
          c = p.idle[i];
          p.idle.erase(p.idle.begin() + static_cast<long>(i));
          p.reused++;
          return c;
        }
      if (p.live < p.cap) {
        p.live++;
        break;  // create one (outside the lock)
      }
      if (!p.idle.empty()) {
        c = p.idle.front();
        p.idle.erase(p.idle.begin());
        p.rebound++;
        return c;  // the caller replaces its scanner (ensure_scanner)
      }
      p.cv.wait(lock);
    }
  }
  auto fail = [&](const char *what) {
    *err = what;
    {
      std::lock_guard<std::mutex> lock(p.mu);
      p.live--;
    }
    p.cv.notify_one();
    return static_cast<Ctx *>(nullptr);
  };
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device available; hypergrep_amd has no CPU scan path");
  auto fresh = std::make_unique<Ctx>();
  fresh->device = hg_faceb_next_device(ndev);  // files shard over the node's GPUs
  if (hipSetDevice(fresh->device) != hipSuccess || hipStreamCreateWithFlags(&fresh->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&fresh->copy_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&fresh->ev_h2d[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&fresh->ev_h2d[1], hipEventDisableTiming) != hipSuccess)
    return fail("hipStreamCreate failed");
  p.created++;
  return fresh.release();
}
// healthy = the call ended without a device error: the context goes back for reuse.  After a HIP error the scanner's
// streams and workspace are in an unknown state: everything is synchronised and destroyed instead.
void checkin(Ctx *c, bool healthy) {
  Pool &p = pool();
  if (!healthy) {
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;
    c = nullptr;
  }
  {
    std::lock_guard<std::mutex> lock(p.mu);
    if (c) p.idle.push_back(c);
    else p.live--;
  }
  p.cv.notify_one();
}
// The context's scanner must be the one of `db` (created on first use; replaced when the context is re-bound).
bool ensure_scanner(Ctx *c, const std::shared_ptr<const HgDb> &db, std::string *err) {
  if (c->sc && c->db == db) return true;
  if (hipSetDevice(c->device) != hipSuccess) return false;
  delete c->sc;  // (hipFree synchronises the device: nothing of the old scanner is in flight afterwards)
  c->sc = nullptr;
  c->db = db;
  return HgScanner::create(db, c->device, &c->sc, err) == HG_OK;
}
// slots: pinned buffers needed (1 for a file that fits one chunk, else all)
bool ensure_buffers(Ctx *c, size_t cap, int slots) {
  if (c->h_cap < cap) {
    for (uint8_t *&p : c->h_slot) {
      hgmem::host_free(p, "h_slot");
      p = nullptr;
    }
    c->h_cap = cap;
  }
  for (int i = 0; i < slots; i++)
    if (!c->h_slot[i] && hgmem::host_alloc(&c->h_slot[i], c->h_cap, "h_slot") != hipSuccess) return false;
  if (c->d_cap < cap) {
    for (uint8_t *&p : c->d_text) {
      hgmem::dev_free(p, "d_text");
      p = nullptr;
    }
    c->d_cap = cap;
  }
  // + 32: slack.  The kernels read the text up to its size rounded up to 16 bytes and no further (include/hypergrep_amd.h,
  // hg_scan_device): the verify pass's aligned discriminator dword ends before the size rounded up to 4, its byte-aligned
  // windows are read byte by byte inside the text (verify_body).  What lies behind a batch is the previous, longer batch;
  // no result depends on it (tests/test_text_bounds_gpu.py).
  for (int i = 0; i < (slots > 1 ? Ctx::kDevBufs : 1); i++)
    if (!c->d_text[i] && hgmem::dev_alloc(&c->d_text[i], c->d_cap + 32, "d_text") != hipSuccess) return false;
  return true;
}
// A call's context goes back to the pool when the call ends, however it ends.
struct CheckinGuard {
  Ctx *&c;
  const bool &healthy;
  ~CheckinGuard() {
    if (c) checkin(c, healthy);
  }
};

size_t chunk_bytes() {
  if (const char *env = std::getenv("HYPERGREP_CHUNK_MB")) {
    long mb = std::atol(env);
    if (mb >= 1 && mb <= 16384) return static_cast<size_t>(mb) << 20;
  }
  return static_cast<size_t>(256) << 20;
}

// ---------------------------------------------------------------- steps the single-file and the packed route share
// How a call (or a pack) stands.  This is the one place that turns a failed step into the message, the rc and the context's
// fate: after a device error the context is destroyed, not pooled (checkin); a refusal leaves it healthy.
struct CallStatus {
  int rc = 0;
  bool healthy = true;
  enum Kind { DeviceError, Refusal };
  // why == nullptr: the step has no message of its own (a copy).  Returns false, for `return ok || st.scan_failed(..)`.
  bool scan_failed(const char *why, Kind kind = DeviceError) {
    if (why) std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (%s)\n", why);
    rc = HYPERSCANNER_SCAN;
    if (kind == DeviceError) healthy = false;
    return false;
  }
  bool scratch_failed(const char *why) {
    std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (%s)\n", why);
    rc = HYPERSCANNER_SCRATCH;
    healthy = false;
    return false;
  }
};

// Queue the download of n elements of a device array into a host vector on `stream`; the caller synchronises.
template <typename T>
bool queue_download(std::vector<T> &dst, const T *d_src, size_t n, hipStream_t stream) {
  dst.resize(n);
  return !n || hipMemcpyAsync(dst.data(), d_src, n * sizeof(T), hipMemcpyDeviceToHost, stream) == hipSuccess;
}

// Distinct values with their counts and expressions, as the values stage, the value store's ranking and the per-file ranking
// leave them: value j is bytes[off[j], off[j + 1]).
struct ValueRows {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off, count;
  std::vector<uint32_t> pattern;
};
template <typename StageOutput>
bool queue_value_rows(const StageOutput &o, ValueRows *rows, hipStream_t stream) {
  return queue_download(rows->bytes, o.d_bytes, o.n_bytes, stream) && queue_download(rows->off, o.d_off, o.n_values + 1, stream) &&
         queue_download(rows->count, o.d_count, o.n_values, stream) && queue_download(rows->pattern, o.d_pattern, o.n_values, stream);
}

// The hash table of a values, store or rank stage over the n_parts parts of a `unit` (chunk, pack): the caller's table_log2,
// or the default for that many parts.  False, with the reason, when it cannot hold them.
bool values_table_log2(uint32_t asked, uint64_t n_parts, const char *unit, uint32_t *log2, std::string *why) {
  *log2 = asked ? asked : hg_values_default_log2(n_parts);
  if (*log2 <= HG_VALUES_MAX_TABLE_LOG2 && (uint64_t{1} << *log2) > n_parts) return true;
  *why = std::string("a ") + unit + " has " + std::to_string(n_parts) + " parts: more than a table of 2^" + std::to_string(*log2) + " slots serves";
  return false;
}
// What those stages read of a scan with the parts stage behind it (without segments; the packed route adds its own).
HgValuesInput values_input(const uint8_t *d_text, const HgScanOutput &out, const HgPartsOutput &pout, uint32_t flags, uint32_t hash_bits, uint32_t log2) {
  return HgValuesInput{d_text, HgGatherList{out.d_hits, out.d_aux, nullptr, out.n_hits}, pout.d_parts, pout.d_pattern, nullptr, pout.n_parts, nullptr, flags, hash_bits ? hash_bits : 64u, log2};
}

// ---------------------------------------------------------------- one file
// Face B's file scan: the reports of the file's pieces, or (invert) one HG_ID_INVERT result per piece without a report.
// With context lines (before / after, hg_hyperscan_context) each chunk is scanned with the context stage behind it and the
// two ordered lists are merged; between chunks the call carries what the device API's chaining identity needs: the
// after-context still owed (owed_after -> carry_after) and the bytes of the previous chunks' tail pieces, `before` at most
// (HgDelivery, hg_deliver.h).
//
// With `counts` (hg_hyperscan_counts) nothing is delivered: the counts stage runs behind every chunk's scan, adding to its totals
// (chunks are cut at piece boundaries, so they share no line), no record is downloaded, and the bins and totals come back once
// at the end.  counts->ids is filled as soon as the database exists, the totals stay zero when the call fails.
using FileEvent = std::function<void(hyperscanner_result_t *, int)>;
struct FileCounts {
  std::vector<uint32_t> ids;
  std::vector<uint64_t> n_lines, n_reports;
};
// With `values` (hg_hyperscan_values) nothing is delivered either: every chunk is scanned with the parts stage, the values stage runs
// behind it, and only the chunk's distinct values come back (bytes, offsets, counts, expressions), to be merged here by key.  No
// part record and no line is downloaded.  The rows keep the order in which their keys first occurred in the file.
// With values->on_device (hg_hyperscan_values_top) not even those: a value store accumulates every chunk's parts on the device, one
// ranking at the end cuts it to `top` rows, and only those come back (`ranked`), in the ranking's order, with the totals before the cut.
struct FileValues {
  hg_values_params_t params;
  bool on_device = false;
  uint64_t top = 0, n_distinct = 0, n_parts = 0;
  ValueRows ranked;
  std::map<std::string, size_t> index;  // key ([expression index, 4 bytes] value bytes) -> row
  std::vector<std::string> value;
  std::vector<uint32_t> pattern;
  std::vector<uint64_t> count;
  void add(const uint8_t *bytes, uint64_t len, uint32_t pat, uint64_t n) {
    std::string key;
    if (params.flags & HG_VALUES_BY_PATTERN) key.assign(reinterpret_cast<const char *>(&pat), 4);
    key.append(reinterpret_cast<const char *>(bytes), len);
    const auto it = index.find(key);
    if (it != index.end()) {
      count[it->second] += n;
      return;
    }
    index.emplace(std::move(key), value.size());
    value.emplace_back(reinterpret_cast<const char *>(bytes), len);
    pattern.push_back(pat);
    count.push_back(n);
  }
  // The merged rows order[0 .. kept) as one ValueRows.
  ValueRows rows(const std::vector<size_t> &order, size_t kept) const {
    ValueRows r;
    r.off.assign(1, 0);
    for (size_t j = 0; j < kept; j++) {
      r.bytes.insert(r.bytes.end(), value[order[j]].begin(), value[order[j]].end());
      r.off.push_back(r.bytes.size());
      r.count.push_back(count[order[j]]);
      r.pattern.push_back(pattern[order[j]]);
    }
    return r;
  }
};
struct PatternSet {
  const char *const *patterns;
  const unsigned int *flags, *ids;
  const hs_expr_ext_t *const *ext;
  unsigned int n;
};
// What a call asks of a file's scan.  The entry points fill it by name.
struct FileScan {
  FileEvent on_event;
  int buffer_size = 0, buffer_count = 1;
  unsigned long long max_match_count = 0;
  bool invert = false;
  uint32_t before = 0, after = 0;
  bool parts = false;
  uint64_t *pieces_scanned = nullptr;
  FileCounts *counts = nullptr;
  FileValues *values = nullptr;
};
// Which of the combinations that exist a call is, decided once.  It says what scans a chunk (the parts scan for Parts, Values
// and Store, the context scan for Context, else the plain one, inverted or not), which stage runs behind the scan (Counts,
// Values, Store), and what comes back: hit records unless one of those three stages consumes them on the device, part records
// for Parts (and for Store, which reads none of them), context records for Context.
enum class ScanMode { Plain, Invert, Context, Parts, Counts, Values, Store };
ScanMode mode_of(const FileScan &o) {
  if (o.counts) return ScanMode::Counts;
  if (o.values) return o.values->on_device ? ScanMode::Store : ScanMode::Values;
  if (o.parts) return ScanMode::Parts;
  if (o.before || o.after) return ScanMode::Context;
  return o.invert ? ScanMode::Invert : ScanMode::Plain;
}
bool scans_parts(ScanMode m) { return m == ScanMode::Parts || m == ScanMode::Values || m == ScanMode::Store; }
bool downloads_hits(ScanMode m) { return m != ScanMode::Counts && m != ScanMode::Values && m != ScanMode::Store; }

std::shared_ptr<const HgDb> get_db(const PatternSet &set, std::string *err, std::string *key_out = nullptr) {
  return get_db(set.patterns, set.flags, set.ids, set.ext, set.n, err, key_out);
}
// The database of a Face B call, with the refusal of the parts stage for the kinds it is not offered for.
std::shared_ptr<const HgDb> call_db(const PatternSet &set, bool parts, std::string *key_out = nullptr) {
  std::string err;
  std::shared_ptr<const HgDb> db = get_db(set, &err, key_out);
  if (!db) {
    std::fprintf(stderr, "ERROR: Unable to create database. Exiting.\n");
    return nullptr;
  }
  if (parts)
    if (const char *why = hg_parts_refusal(db->nhuge, db->ncomb, db->nquiet, db->n_ext != 0)) {
      std::fprintf(stderr, "ERROR: Unable to create database. Exiting. (%s)\n", why);
      return nullptr;
    }
  return db;
}

// What a chunk goes through between the reader and the delivery, on the call's context: the steps of scan_file's loop.
struct ChunkSteps {
  Ctx *const ctx;
  const FileScan &opt;
  const ScanMode mode;
  const int nslots;
  CallStatus &st;
  std::shared_ptr<const HgDb> db;
  std::string err;
  std::unique_ptr<HgCounts> counts;     // the mode's stage (made with the scanner; its buffers are its own)
  std::unique_ptr<HgValues> values;
  std::unique_ptr<HgValueStore> store;  // (the file's value store)
  ValueRows rows;                       // a chunk's distinct values
  HgScanOutput out{};                   // the chunk's results on the device ...
  HgContextOutput cout{};
  HgPartsOutput pout{};
  std::vector<HgHit> ctx_hits;  // ... and what of them came back, beside the hit records in ctx->hits / ctx->aux
  std::vector<HgHitAux> ctx_aux;
  std::vector<HgPart> part_recs;
  std::vector<uint32_t> part_pattern;
  bool copied[Ctx::kSlots] = {false, false, false};
  double t_setup = 0;

  // The pattern set's first large file picks the prefilter windows from this text (maybe_tune); then the scanner and the stage.
  bool first_chunk(const std::string &db_key, const uint8_t *host, size_t cut) {
    const double t0 = hg_now();
    if (cut) db = maybe_tune(db_key, db, host, cut);
    if (!ensure_scanner(ctx, db, &err)) return st.scratch_failed(err.c_str());
    if (mode == ScanMode::Counts) counts = std::make_unique<HgCounts>(ctx->device, *db);
    if (mode == ScanMode::Store) store = std::make_unique<HgValueStore>(ctx->device);
    if (mode == ScanMode::Values) values = std::make_unique<HgValues>(ctx->device);
    t_setup = hg_now() - t0;
    return true;
  }
  uint8_t *d_text(unsigned k) const { return ctx->d_text[nslots > 1 ? k % Ctx::kDevBufs : 0]; }
  // Slot k % nslots -> device buffer k % 2 on the copy stream, once per fill of the slot; one event per device buffer.
  bool issue_copy(unsigned k, size_t cut) {
    const int sl = static_cast<int>(k % nslots), db_i = static_cast<int>(k % Ctx::kDevBufs);
    if (copied[sl]) return true;
    copied[sl] = true;
    if (!cut) return true;
    return hipMemcpyAsync(d_text(k), ctx->h_slot[sl], cut, hipMemcpyHostToDevice, ctx->copy_stream) == hipSuccess &&
           hipEventRecord(ctx->ev_h2d[db_i], ctx->copy_stream) == hipSuccess;
  }
  // Chunk k's copy; chunk k + 1's too when its slot is already filled (it travels while this one is scanned); the scan waits for k's.
  bool copy(unsigned k, const SlotReader::Chunk &c, const SlotReader &reader) {
    return (issue_copy(k, c.cut) && (!c.next_filled || issue_copy(k + 1, reader.cut_of(k + 1))) &&
            hipStreamWaitEvent(ctx->stream, ctx->ev_h2d[k % Ctx::kDevBufs], 0) == hipSuccess) ||
           st.scan_failed(nullptr);
  }
  bool scan(unsigned k, size_t cut, const HgDelivery &delivery) {
    out = HgScanOutput{};
    cout = HgContextOutput{};
    pout = HgPartsOutput{};
    int src;
    if (scans_parts(mode)) src = ctx->sc->scan_parts(d_text(k), cut, opt.buffer_size, delivery.line_base(), ctx->stream, &out, &pout);
    else if (mode == ScanMode::Context) src = ctx->sc->scan_context(d_text(k), cut, opt.buffer_size, delivery.line_base(), ctx->stream, delivery.context_params(), opt.invert, &out, &cout);
    else src = ctx->sc->scan(d_text(k), cut, opt.buffer_size, delivery.line_base(), ctx->stream, &out, opt.invert);
    return src == HG_OK || st.scan_failed(ctx->sc->last_error().c_str());
  }
  // The stage behind the scan: it works on the chunk's records where they lie.
  bool stage(unsigned k) {
    if (mode == ScanMode::Counts) {  // none is downloaded, nothing is delivered
      HgCountsOutput co{};
      return counts->run(HgCountsInput{HgCountsList{out.d_hits, nullptr, out.n_hits}, 0, HG_COUNTS_F_ACCUMULATE}, ctx->stream, &co, &err) == HG_OK || st.scan_failed(err.c_str());
    }
    if (mode != ScanMode::Values && mode != ScanMode::Store) return true;
    const hg_values_params_t &p = opt.values->params;
    uint32_t log2;
    if (!values_table_log2(p.table_log2, pout.n_parts, "chunk", &log2, &err)) return st.scan_failed(err.c_str(), CallStatus::Refusal);
    const HgValuesInput vin = values_input(d_text(k), out, pout, p.flags, p.hash_bits, log2);
    if (mode == ScanMode::Store) {  // the chunk's parts join the file's store: nothing comes back
      HgValStoreInput sin{};
      sin.values = vin;
      HgValStoreOutput so{};
      return store->accumulate(sin, ctx->stream, &so, &err) == HG_OK || st.scan_failed(err.c_str());
    }
    HgValuesOutput vo{};  // the chunk's parts are grouped: only the distinct values come back
    if (values->run(vin, ctx->stream, &vo, &err) != HG_OK) return st.scan_failed(err.c_str());
    if (!queue_value_rows(vo, &rows, ctx->stream) || hipStreamSynchronize(ctx->stream) != hipSuccess) return st.scan_failed("copying the values");
    for (uint64_t j = 0; j < vo.n_values; j++) opt.values->add(rows.bytes.data() + rows.off[j], rows.off[j + 1] - rows.off[j], rows.pattern[j], rows.count[j]);
    return true;
  }
  // The records the delivery reads, by mode.
  bool download() {
    const uint64_t n_rows = downloads_hits(mode) ? out.n_hits : 0, n_part_rows = mode == ScanMode::Values ? 0 : pout.n_parts;
    hipStream_t s = ctx->stream;
    return (queue_download(ctx->hits, out.d_hits, n_rows, s) && queue_download(ctx->aux, out.d_aux, n_rows, s) && queue_download(ctx_hits, cout.d_hits, cout.n_context, s) &&
            queue_download(ctx_aux, cout.d_aux, cout.n_context, s) && queue_download(part_recs, pout.d_parts, n_part_rows, s) &&
            queue_download(part_pattern, pout.d_pattern, n_part_rows, s) && (!(n_rows || cout.n_context || n_part_rows) || hipStreamSynchronize(s) == hipSuccess)) ||
           st.scan_failed(nullptr);
  }
  HgChunkRecords records(const uint8_t *host) const {
    HgChunkRecords r;
    r.base = host;
    r.hits = ctx->hits.data(), r.aux = ctx->aux.data(), r.n_hits = ctx->hits.size();
    r.ctx_hits = ctx_hits.data(), r.ctx_aux = ctx_aux.data(), r.n_ctx = ctx_hits.size();
    r.parts = part_recs.data(), r.part_pattern = part_pattern.data(), r.n_parts = part_recs.size();
    r.patterns = db->patterns.data();
    r.n_pieces = out.n_pieces;
    r.owed_after = cout.owed_after;
    return r;
  }
  // What the mode brings back once, at the end of a call that went well.
  bool finish() {
    if (mode == ScanMode::Counts && counts) return counts->copy_totals(opt.counts->n_lines.data(), opt.counts->n_reports.data()) || st.scan_failed(nullptr);  // n_bins x 16 bytes
    if (mode != ScanMode::Store || !store || !store->began()) return true;
    FileValues &fv = *opt.values;  // one ranking, and the kept rows
    HgValRankOutput ro{};
    if (store->rank(fv.top, false, ctx->stream, &ro, &err) != HG_OK) return st.scan_failed(err.c_str());
    fv.n_distinct = ro.n_distinct;
    fv.n_parts = ro.n_parts;
    return (queue_value_rows(ro, &fv.ranked, ctx->stream) && hipStreamSynchronize(ctx->stream) == hipSuccess) || st.scan_failed("copying the values");
  }
};

int scan_file(const char *file_name, const PatternSet &set, FileScan opt) {
  // ---- validate
  if (opt.max_match_count > 0 && opt.max_match_count < static_cast<unsigned long long>(opt.buffer_count)) opt.buffer_count = static_cast<int>(opt.max_match_count);
  if (opt.buffer_count < 1 || opt.buffer_size < 1 || !opt.on_event) return HYPERSCANNER_STATE_MEM;
  Ring ring;
  if (!ring.init(opt.buffer_count, opt.buffer_size, opt.on_event)) return HYPERSCANNER_COMPILE_MEM;
  const ScanMode mode = mode_of(opt);

  // ---- database
  std::string err, db_key_str;
  std::shared_ptr<const HgDb> db = call_db(set, scans_parts(mode), &db_key_str);
  if (!db) return HYPERSCANNER_DB;
  if (opt.counts) {
    opt.counts->ids = db->report_ids;
    opt.counts->n_lines.assign(db->report_ids.size(), 0);
    opt.counts->n_reports.assign(db->report_ids.size(), 0);
  }

  // ---- open: before any device resource is taken, so a missing file is HYPERSCANNER_GZ_OPEN with or without a GPU
  // (the reference's scratch allocation cannot fail for want of a device; its order is database, scratch, file)
  Reader in;
  if (!file_name || !in.open(file_name)) return HYPERSCANNER_GZ_OPEN;
  if (opt.buffer_size < 2) return 0;  // gzgets(len <= 1) returns NULL at once: nothing is scanned (hyperscanner.c:199)

  // ---- context and its buffers
  Ctx *ctx = checkout(db, &err);
  if (!ctx) {
    std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (%s)\n", err.c_str());
    return HYPERSCANNER_SCRATCH;
  }
  CallStatus st;
  CheckinGuard guard{ctx, st.healthy};
  const uint64_t bs1 = static_cast<uint64_t>(opt.buffer_size) - 1;
  size_t cap = chunk_bytes();
  const bool one_chunk = !in.compressed() && in.size_hint() && in.size_hint() < cap;
  if (one_chunk) cap = std::max<size_t>(in.size_hint() + 16, 1 << 16);
  // a chunk must hold a whole piece plus the carry of the previous one — unless the whole file is one chunk anyway
  if (!one_chunk) cap = std::max<size_t>(cap, static_cast<size_t>(std::min<uint64_t>(2 * bs1 + 16, static_cast<uint64_t>(1) << 32)));
  const int nslots = one_chunk ? 1 : Ctx::kSlots;
  if (hipSetDevice(ctx->device) != hipSuccess || !ensure_buffers(ctx, cap, nslots)) {
    st.scratch_failed("device buffers");
    return st.rc;
  }

  // ---- stage 1: the reader thread fills slots and cuts them at piece boundaries
  // HYPERGREP_TRACE=1: where the call's wall time went (seconds), printed to stderr at the end
  const bool trace = std::getenv("HYPERGREP_TRACE") != nullptr;
  const double t_call = hg_now();
  double t_scan = 0, t_deliver = 0;  // consumer: copy + scan + hit copy, ring + callbacks
  uint64_t bytes_in = 0;
  SlotReader reader(in, ctx->h_slot, nslots, cap, bs1);

  // ---- stages 2 and 3 per chunk: copy to HBM (one chunk ahead when the reader is), scan, the mode's stage, download, deliver
  ChunkSteps steps{ctx, opt, mode, nslots, st, db};
  HgDelivery delivery(ring, mode == ScanMode::Parts, opt.before, opt.after, opt.max_match_count);
  for (unsigned k = 0;; k++) {
    const SlotReader::Chunk c = reader.wait(k);
    if (k == 0 && !steps.first_chunk(db_key_str, c.bytes, c.cut)) break;
    bool stop = false;
    if (c.cut) {
      const double t_begin = hg_now();
      bytes_in += c.cut;
      if (!steps.copy(k, c, reader) || !steps.scan(k, c.cut, delivery) || !steps.stage(k) || !steps.download()) break;
      const double t_scanned = hg_now();
      t_scan += t_scanned - t_begin;
      stop = delivery.chunk(steps.records(c.bytes));  // (the held pieces' bytes are copied out of the slot here)
      t_deliver += hg_now() - t_scanned;
    }
    steps.copied[k % nslots] = false;
    reader.release(k);  // the slot goes back to the reader only now, after delivery
    if (c.last || stop) break;
  }

  // ---- finish
  reader.stop();
  (void)hipStreamSynchronize(ctx->copy_stream);  // a copy issued ahead may still be in flight
  ring.flush();
  if (opt.pieces_scanned) *opt.pieces_scanned = delivery.line_base();
  if (st.rc == 0) steps.finish();
  if (trace)
    std::fprintf(stderr, "[hypergrep_amd] %s: %.1f MiB in %.4f s; reader filling slots %.4f s; consumer: waiting for data %.4f s, window tuning + scanner %.4f s (%s), copy + scan %.4f s, delivering %llu hits %.4f s\n",
                 file_name, bytes_in / 1048576.0, hg_now() - t_call, reader.t_read, reader.t_wait, steps.t_setup, steps.db->tuned ? "tuned windows" : "static windows", t_scan,
                 static_cast<unsigned long long>(ring.delivered), t_deliver);
  return st.rc;
}


// ---------------------------------------------------------------- many files
// Many files in one call (grep -r): the files are packed, in the given order, into buffers of at most the file path's chunk
// size by the packing rule of hg_scan_device_segments (an unterminated file is followed by "\0\n"), and each pack is ONE scan
// with the segment stage behind it.  A file that does not fit a pack, a compressed one (the decoder of the per-file route reads
// it), a pipe or the like, and everything when buffer_size < 2, takes scan_file inside the call; the call never holds a
// context of the pool while scan_file takes one.  An empty regular file is an empty segment.  Batches go out in file
// order and no batch mixes files; a file's results and rc are those of hg_hyperscan_ext / hg_hyperscan_invert for that file.
// The line bytes of a result come from the pack's host copy: only the 32-byte records and the per-file arrays leave the GPU.
//
// With before / after (hg_hyperscan_files_context) each pack is one scan_packed_context: the per-file context stage runs behind
// the segment stage, and a file's own results and its context records (file-relative both) are merged by line on the way into
// the ring, as scan_file merges a chunk's.  The limit needs no trailing state here: the stage has already ended the last kept
// line's after-context before the next matching piece.  Files of the per-file route take scan_file with the same before / after.
//
// With parts (hg_hyperscan_files_parts) each pack is one scan_packed_parts: the per-file parts stage runs behind the segment
// stage, and a file's batches hold one Result per part of each line it keeps (the bytes from the pack's host copy), as
// scan_file delivers a chunk's.  Files of the per-file route take scan_file with parts.
//
// With `counts` (hg_hyperscan_files_counts; on_event is NULL then) the counts stage runs behind every pack's segment stage with
// per-segment matrices, which are all that leaves the GPU beside the per-file arrays; a pack is closed early where one more
// file would take the matrices past the stage's limit of cells.  Files of the per-file route take scan_file with counts.
//
// With `values` (hg_hyperscan_files_values; on_event is NULL then) every pack is scanned with parts and the rank stage runs behind
// it with HG_RANK_PER_SEGMENT and the caller's cut: only the kept rows (bytes, offsets, counts, expressions) and three numbers
// per file leave the GPU, no part record and no line.  on_file is called once per file, in file order, so a file that cannot be
// opened closes the pack before it.  Files of the per-file route take scan_file with values (hg_hyperscan_values' chunk merge)
// and are ordered and cut here by the same rule: count descending, then first occurrence in the file.
struct FilesCounts {
  uint32_t *ids;
  unsigned int max_ids, *n_ids;
  uint64_t *file_lines, *file_reports;  // n_files rows of max_ids values
};
struct FilesValues {
  hg_rank_params_t params;
  hg_file_values_event on_file;
  void *context;
  void none(unsigned int f) const { on_file(context, f, nullptr, nullptr, nullptr, nullptr, 0, 0, 0); }
};
// Where a many-file call's results go.  (What it asks of each file's scan is a FileScan, whose per-file fields stay empty.)
struct FilesOut {
  hg_files_event on_event = nullptr;
  void *context = nullptr;
  hg_file_summary_t *summaries = nullptr;
  const FilesCounts *counts = nullptr;
  const FilesValues *values = nullptr;
};
// The files packed so far, in the context's first pinned slot, with the device copy of their bounds.
struct Pack {
  std::vector<uint64_t> seg_start, seg_end;
  std::vector<unsigned int> seg_file;
  size_t fill = 0;             // bytes of the pack so far
  uint64_t *d_segs = nullptr;  // seg_start and seg_end, one after the other
  size_t d_segs_cap = 0;
  ~Pack() { hgmem::dev_free(d_segs, "d_segs"); }
  size_t n_seg() const { return seg_file.size(); }
  void clear() {
    seg_start.clear();
    seg_end.clear();
    seg_file.clear();
    fill = 0;
  }
  bool ensure_d_segs() {
    if (2 * n_seg() <= d_segs_cap) return true;
    hgmem::dev_free(d_segs, "d_segs");
    d_segs = nullptr;
    d_segs_cap = std::max<size_t>(2 * n_seg() + n_seg() / 2, 4096);
    if (hgmem::dev_alloc(&d_segs, d_segs_cap * sizeof(uint64_t), "d_segs") == hipSuccess) return true;
    d_segs_cap = 0;
    return false;
  }
};

// One many-file call: the per-file route (single) and the packed route (flush: scan, the mode's stage, per-file delivery).
struct FilesRun {
  const char *const *file_names;
  const PatternSet &set;
  const FileScan &opt;  // (before / after / parts already cleared where only summaries are asked for)
  const FilesOut &to;
  std::shared_ptr<const HgDb> db;
  const size_t n_bins, n_cols;  // the database's report ids; those of them the caller's count rows hold
  Ring ring;
  unsigned int cur_file = 0;  // the file whose results the ring holds
  Ctx *ctx = nullptr;
  CallStatus st;
  CheckinGuard guard{ctx, st.healthy};
  std::string err;
  // a pack's results on the device ...
  HgScanOutput out{};
  HgSegOutput seg{};
  HgContextOutput cout{};
  HgSegCtxOutput sx{};
  HgPartsOutput pout{};
  HgSegPartsOutput spo{};
  // ... and what of them came back: per-file arrays, records (the hit records in ctx->hits / ctx->aux), matrices, ranked rows
  std::vector<uint64_t> first, n_lines, n_selected, first_ctx, first_part;
  std::vector<HgHit> ctx_hits;  // file-relative, file after file
  std::vector<HgHitAux> ctx_aux;
  std::vector<HgPart> part_recs;  // likewise
  std::vector<uint32_t> part_pattern;
  std::vector<uint32_t> seg_lines, seg_reports;
  std::unique_ptr<HgRank> rank;  // (made with the first pack, on its device; its buffers are its own)
  int rank_device = -1;
  ValueRows ranked;
  std::vector<uint64_t> r_first_value, r_distinct, r_parts;

  bool with_context() const { return opt.before || opt.after; }
  // A file that is not scanned: its rc, and its callback in its place in the order.
  void skip(unsigned int f, int rc) {
    to.summaries[f].rc = rc;
    if (to.values) to.values->none(f);
  }
  void fail_pack(const Pack &p, int rc) {
    for (unsigned int f : p.seg_file) skip(f, rc);
    st.healthy = false;
  }

  // One file through the per-file route: its events carry its index, its distinct lines are counted on the way.
  void single(unsigned int f) {
    uint64_t selected = 0, last = ~0ull, pieces = 0;
    FileCounts fc;
    FileValues fv;
    if (to.values) fv.params = hg_values_params_t{to.values->params.flags & HG_VALUES_BY_PATTERN, to.values->params.hash_bits, to.values->params.table_log2, 0};
    FileScan one = opt;
    one.on_event = [&](hyperscanner_result_t *r, int n) {
      for (int i = 0; i < n; i++)
        if (r[i].line_number != last && !(with_context() && r[i].id == HG_CTX_ID_CONTEXT)) {  // (a context line is no result of the file's)
          last = r[i].line_number;
          selected++;
        }
      if (to.on_event) to.on_event(f, r, n, to.context);
    };
    one.pieces_scanned = &pieces;
    one.counts = to.counts ? &fc : nullptr;
    one.values = to.values ? &fv : nullptr;
    const int rc = scan_file(file_names[f], set, one);
    if (to.values && rc) to.values->none(f);
    if (to.values && !rc) ranked_single(f, fv);
    if (to.counts && fc.n_lines.size() >= n_cols) {  // (nothing was delivered, so `selected` stays 0: the row says what was selected)
      std::copy(fc.n_lines.begin(), fc.n_lines.begin() + n_cols, to.counts->file_lines + static_cast<size_t>(f) * to.counts->max_ids);
      std::copy(fc.n_reports.begin(), fc.n_reports.begin() + n_cols, to.counts->file_reports + static_cast<size_t>(f) * to.counts->max_ids);
    }
    to.summaries[f] = hg_file_summary_t{rc, pieces, selected};
  }
  // The merged rows of a file of the per-file route come in the order of their first occurrence: a stable sort by count, then the cut.
  void ranked_single(unsigned int f, const FileValues &fv) {
    std::vector<size_t> order(fv.value.size());
    for (size_t j = 0; j < order.size(); j++) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return fv.count[x] > fv.count[y]; });
    uint64_t n_parts = 0;
    for (uint64_t c : fv.count) n_parts += c;
    const uint64_t top = to.values->params.top;
    const size_t kept = top && top < order.size() ? static_cast<size_t>(top) : order.size();
    const ValueRows r = fv.rows(order, kept);
    to.values->on_file(to.values->context, f, r.bytes.data(), r.off.data(), r.count.data(), r.pattern.data(), kept, order.size(), n_parts);
  }

  // The pack's bytes and bounds to the device, one scan by mode, and the per-file arrays and the records the delivery reads.
  int scan_pack(Pack &p) {
    const size_t n_seg = p.n_seg();
    const HgSegParams params{p.d_segs, p.d_segs + n_seg, static_cast<uint32_t>(n_seg), opt.max_match_count};
    uint8_t *d_text = ctx->d_text[0];
    hipStream_t s = ctx->stream;
    if ((p.fill && hipMemcpyAsync(d_text, ctx->h_slot[0], p.fill, hipMemcpyHostToDevice, s) != hipSuccess) ||
        hipMemcpyAsync(p.d_segs, p.seg_start.data(), n_seg * sizeof(uint64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(p.d_segs + n_seg, p.seg_end.data(), n_seg * sizeof(uint64_t), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return HG_ERR_HIP;
    out = HgScanOutput{}, seg = HgSegOutput{}, cout = HgContextOutput{}, sx = HgSegCtxOutput{}, pout = HgPartsOutput{}, spo = HgSegPartsOutput{};
    const int src = opt.parts        ? ctx->sc->scan_packed_parts(d_text, p.fill, opt.buffer_size, s, params, &out, &seg, &pout, &spo)
                    : with_context() ? ctx->sc->scan_packed_context(d_text, p.fill, opt.buffer_size, s, params, opt.before, opt.after, opt.invert, &out, &seg, &cout, &sx)
                                     : ctx->sc->scan_packed(d_text, p.fill, opt.buffer_size, s, params, opt.invert, &out, &seg);
    if (src != HG_OK) return src;
    const bool part_rows = opt.parts && !to.values;  // (with values no part record comes back)
    const uint64_t n_rows = to.on_event ? out.n_hits : 0;  // (summaries or counts only: no record leaves the GPU)
    first_ctx.assign(n_seg + 1, 0);
    first_part.assign(n_seg + 1, 0);
    const bool ok = queue_download(ctx_hits, cout.d_hits, cout.n_context, s) && queue_download(ctx_aux, cout.d_aux, cout.n_context, s) &&
                    (!with_context() || queue_download(first_ctx, sx.d_first_context, n_seg + 1, s)) &&
                    queue_download(part_recs, pout.d_parts, part_rows ? pout.n_parts : 0, s) && queue_download(part_pattern, pout.d_pattern, part_rows ? pout.n_parts : 0, s) &&
                    (!part_rows || queue_download(first_part, spo.d_first_part, n_seg + 1, s)) &&
                    queue_download(ctx->hits, out.d_hits, n_rows, s) && queue_download(ctx->aux, out.d_aux, n_rows, s) && queue_download(first, seg.d_first_record, n_seg + 1, s) &&
                    queue_download(n_lines, seg.d_n_lines, n_seg, s) && queue_download(n_selected, seg.d_n_selected, n_seg, s) && hipStreamSynchronize(s) == hipSuccess;
    return ok ? HG_OK : HG_ERR_HIP;
  }
  // The counts stage behind the segment stage; the two matrices come back.
  int count_pack(const Pack &p) {
    HgCounts counts(ctx->device, *db);
    HgCountsOutput co{};
    const size_t cells = p.n_seg() * n_bins;
    seg_lines.resize(cells);
    seg_reports.resize(cells);
    const int src = counts.run(HgCountsInput{HgCountsList{out.d_hits, seg.d_record_segment, out.n_hits}, static_cast<uint32_t>(p.n_seg()), HG_COUNTS_F_PER_SEGMENT}, ctx->stream, &co, &err);
    if (src != HG_OK) return src;
    return hipMemcpy(seg_lines.data(), co.d_seg_lines, cells * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
                   hipMemcpy(seg_reports.data(), co.d_seg_reports, cells * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess
               ? HG_OK
               : HG_ERR_HIP;
  }
  // The rank stage behind the parts stage, per file; the kept rows and the per-file arrays come back.
  int rank_pack(const Pack &p) {
    const hg_rank_params_t &rp = to.values->params;
    const size_t n_seg = p.n_seg();
    uint32_t log2;
    int src = values_table_log2(rp.table_log2, pout.n_parts, "pack", &log2, &err) ? HG_OK : HG_ERR_ARG;
    HgRankOutput ro{};
    if (src == HG_OK) {
      if (!rank || rank_device != ctx->device) {
        rank = std::make_unique<HgRank>(ctx->device);
        rank_device = ctx->device;
      }
      HgRankInput rin{};
      rin.values = values_input(ctx->d_text[0], out, pout, (rp.flags & HG_RANK_F_BY_PATTERN) | HG_RANK_F_PER_SEGMENT, rp.hash_bits, log2);
      rin.values.recs.seg_of = seg.d_record_segment;
      rin.values.part_seg = spo.d_part_segment;
      rin.values.seg_start = p.d_segs;
      rin.n_seg = static_cast<uint32_t>(n_seg);
      rin.top = rp.top;
      src = rank->run(rin, ctx->stream, &ro, &err);
    }
    if (src == HG_OK && !(queue_value_rows(ro, &ranked, ctx->stream) && queue_download(r_first_value, ro.d_first_value, n_seg + 1, ctx->stream) &&
                          queue_download(r_distinct, ro.d_seg_distinct, n_seg, ctx->stream) && queue_download(r_parts, ro.d_seg_parts, n_seg, ctx->stream) &&
                          hipStreamSynchronize(ctx->stream) == hipSuccess)) {
      err = "copying the ranked values";
      src = HG_ERR_HIP;
    }
    if (src != HG_OK) ctx->sc->set_error(src, err);
    return src;
  }
  // File after file of a scanned pack: the summary, the count row, the ranked rows, the batches.
  void deliver_pack(const Pack &p) {
    if (std::getenv("HYPERGREP_TRACE"))  // the packed route: one line per pack
      std::fprintf(stderr, "[hypergrep_amd] pack: %zu files, %.1f MiB in one scan; segment stage %.0f us, %llu records; context stage %.0f us, %llu context records\n", p.n_seg(),
                   p.fill / 1048576.0, seg.ms_segments * 1e3, static_cast<unsigned long long>(out.n_hits), cout.ms_context * 1e3, static_cast<unsigned long long>(cout.n_context));
    for (size_t s = 0; s < p.n_seg(); s++) {
      cur_file = p.seg_file[s];
      to.summaries[cur_file] = hg_file_summary_t{0, n_lines[s], n_selected[s]};
      if (to.counts)
        for (size_t b = 0; b < n_cols; b++) {
          to.counts->file_lines[static_cast<size_t>(cur_file) * to.counts->max_ids + b] = seg_lines[s * n_bins + b];
          to.counts->file_reports[static_cast<size_t>(cur_file) * to.counts->max_ids + b] = seg_reports[s * n_bins + b];
        }
      if (to.values) {  // the file's rows of the pack's ranking (off[0] is where its first value lies among the pack's bytes)
        const uint64_t lo = r_first_value[s], n = r_first_value[s + 1] - lo;
        to.values->on_file(to.values->context, cur_file, ranked.bytes.data(), ranked.off.data() + lo, ranked.count.data() + lo, ranked.pattern.data() + lo, n, r_distinct[s], r_parts[s]);
      }
      if (!to.on_event) continue;
      HgChunkRecords r;  // the file's records are file-relative; the limit and the context's end were settled by the stages
      r.base = ctx->h_slot[0] + p.seg_start[s];
      r.hits = ctx->hits.data() + first[s], r.aux = ctx->aux.data() + first[s], r.n_hits = first[s + 1] - first[s];
      r.ctx_hits = ctx_hits.data() + first_ctx[s], r.ctx_aux = ctx_aux.data() + first_ctx[s], r.n_ctx = first_ctx[s + 1] - first_ctx[s];
      r.parts = part_recs.data() + first_part[s], r.part_pattern = part_pattern.data() + first_part[s], r.n_parts = first_part[s + 1] - first_part[s];
      r.patterns = db->patterns.data();
      hg_deliver_file(ring, r, opt.parts);
      ring.flush();  // no batch mixes files
    }
  }
  // Scan the pack and deliver its files.
  void flush(Pack &p) {
    if (p.seg_file.empty()) return;
    if (!(hipSetDevice(ctx->device) == hipSuccess && ensure_scanner(ctx, db, &err) && p.ensure_d_segs())) {
      std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (%s)\n", err.c_str());
      fail_pack(p, HYPERSCANNER_SCRATCH);
    } else {
      int src = scan_pack(p);
      if (src == HG_OK && to.counts && n_bins) src = count_pack(p);
      if (src == HG_OK && to.values) src = rank_pack(p);
      if (src != HG_OK) {
        st.scan_failed(ctx->sc ? ctx->sc->last_error().c_str() : "copy");
        fail_pack(p, HYPERSCANNER_SCAN);
      } else {
        deliver_pack(p);
      }
    }
    p.clear();
  }
  // The call's own context goes back to the pool: scan_file takes one of its own from the bounded pool, and a call that held
  // one while it waited for a second could wait for ever (HYPERGREP_POOL=1, or as many concurrent calls as the pool holds).
  void give_back_context() {
    if (ctx) checkin(ctx, st.healthy);
    ctx = nullptr;
  }
  bool take_context(size_t cap) {
    if (ctx) return true;
    ctx = checkout(db, &err);
    if (ctx && hipSetDevice(ctx->device) == hipSuccess && ensure_buffers(ctx, cap, 1)) return true;
    std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (%s)\n", err.c_str());
    if (ctx) st.healthy = false;
    return false;
  }
};

int files_impl(const char *const *file_names, unsigned int n_files, const PatternSet &set, FileScan opt, const FilesOut &to) {
  // ---- validate
  if (!to.on_event) opt.before = opt.after = 0;  // summaries only: they are those of the call without context
  if (!to.summaries || (!file_names && n_files) || opt.buffer_count < 1 || opt.buffer_size < 1) return HYPERSCANNER_STATE_MEM;
  if (to.counts && to.counts->n_ids) *to.counts->n_ids = 0;
  if (opt.max_match_count > 0 && opt.max_match_count < static_cast<unsigned long long>(opt.buffer_count)) opt.buffer_count = static_cast<int>(opt.max_match_count);
  for (unsigned int i = 0; i < n_files; i++) to.summaries[i] = hg_file_summary_t{0, 0, 0};

  // ---- database; the parts stage is refused for the whole call, before anything is read (as hg_hyperscan_parts)
  std::shared_ptr<const HgDb> db = call_db(set, opt.parts);
  if (!db) return HYPERSCANNER_DB;
  if (!to.on_event && !to.values) opt.parts = false;  // summaries only: they are those of the call without parts
  const size_t n_bins = db->report_ids.size(), n_cols = to.counts ? std::min<size_t>(n_bins, to.counts->max_ids) : 0;
  if (const FilesCounts *fcs = to.counts) {
    *fcs->n_ids = static_cast<unsigned int>(n_bins);
    std::copy(db->report_ids.begin(), db->report_ids.begin() + n_cols, fcs->ids);
    std::fill(fcs->file_lines, fcs->file_lines + static_cast<size_t>(n_files) * fcs->max_ids, uint64_t{0});
    std::fill(fcs->file_reports, fcs->file_reports + static_cast<size_t>(n_files) * fcs->max_ids, uint64_t{0});
  }
  FilesRun run{file_names, set, opt, to, db, n_bins, n_cols};
  if (to.on_event && !run.ring.init(opt.buffer_count, std::max(opt.buffer_size, 2), [&](hyperscanner_result_t *r, int n) { to.on_event(run.cur_file, r, n, to.context); }))
    return HYPERSCANNER_COMPILE_MEM;

  // ---- file after file: into the pack, or through the per-file route in its place in the order
  const size_t cap = chunk_bytes();
  Pack pack;
  for (unsigned int f = 0; f < n_files; f++) {
    if (!run.st.healthy) {  // a device error ended the packs: the rest is not scanned
      run.skip(f, HYPERSCANNER_SCAN);
      continue;
    }
    Reader in;
    if (!file_names[f] || !in.open(file_names[f])) {
      if (to.values) run.flush(pack);  // (its callback comes in its place in the order)
      run.skip(f, HYPERSCANNER_GZ_OPEN);
      continue;
    }
    const size_t size = in.size_hint();
    struct stat st;
    const bool empty_regular = !in.compressed() && !size && ::stat(file_names[f], &st) == 0 && S_ISREG(st.st_mode) && st.st_size == 0;
    if (opt.buffer_size < 2 || in.compressed() || (!size && !empty_regular) || size + 2 > cap) {  // the per-file route
      run.flush(pack);
      run.give_back_context();
      if (run.st.healthy) run.single(f);
      else run.skip(f, HYPERSCANNER_SCAN);
      continue;
    }
    if (pack.fill + size + 2 > cap || (to.counts && (pack.n_seg() + 1) * n_bins > HG_COUNTS_MAX_CELLS)) run.flush(pack);
    if (!run.st.healthy) {
      run.skip(f, HYPERSCANNER_SCAN);
      continue;
    }
    if (!run.take_context(cap)) {
      for (unsigned int g = f; g < n_files; g++) run.skip(g, HYPERSCANNER_SCRATCH);
      return 0;
    }
    uint8_t *buf = run.ctx->h_slot[0];
    size_t got = 0;
    while (got < size) {  // (the size seen at open: a file that grows meanwhile is read up to it)
      const long r = in.read(buf + pack.fill + got, size - got);
      if (r <= 0) break;
      got += static_cast<size_t>(r);
    }
    pack.seg_start.push_back(pack.fill);
    pack.seg_end.push_back(pack.fill + got);
    pack.seg_file.push_back(f);
    pack.fill += got;
    if (got && buf[pack.fill - 1] != '\n') {  // the pad behind an unterminated file
      buf[pack.fill++] = 0;
      buf[pack.fill++] = '\n';
    }
  }
  if (run.st.healthy) run.flush(pack);
  return 0;
}

// The entry points' argument checks that several share.
bool context_ids_clash(const unsigned int *pattern_ids, unsigned int elements) {  // an expression with one of the context ids could not be told from a context line by the callback
  for (unsigned int i = 0; pattern_ids && i < elements; i++)
    if (pattern_ids[i] >= HG_CTX_ID_TAIL) return true;
  return false;
}
bool bad_values_params(const hg_values_params_t &p) { return (p.flags & ~HG_VALUES_BY_PATTERN) || p.hash_bits > 64 || p.table_log2 > HG_VALUES_MAX_TABLE_LOG2; }
// (the modes that deliver nothing still pass scan_file's check for an event)
void no_event(hyperscanner_result_t *, int) {}
// The result ring every entry point describes with the same three arguments; the other fields are set by name.
FileScan ring_of(int buffer_size, int buffer_count, unsigned long long max_match_count) {
  FileScan opt;
  opt.buffer_size = buffer_size;
  opt.buffer_count = buffer_count;
  opt.max_match_count = max_match_count;
  return opt;
}

}  // namespace

extern "C" int hg_check_patterns_ext(const char *const *patterns, const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                                  const hs_expr_ext_t *const *ext, const unsigned int elements) {
  std::string err;
  return get_db(patterns, pattern_flags, pattern_ids, ext, elements, &err) ? 0 : HYPERSCANNER_DB;
}

extern "C" int check_patterns(const char *const *patterns, const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                              const unsigned int elements) {
  return hg_check_patterns_ext(patterns, pattern_flags, pattern_ids, nullptr, elements);
}

extern "C" int hyperscan(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                         const unsigned int *pattern_ids, const unsigned int elements, hs_event on_event, const int buffer_size,
                         int buffer_count, unsigned long long max_match_count) {
  return hg_hyperscan_ext(file_name, patterns, pattern_flags, pattern_ids, nullptr, elements, on_event, buffer_size, buffer_count, max_match_count);
}

extern "C" int hg_hyperscan_ext(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                             const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hs_event on_event,
                             const int buffer_size, int buffer_count, unsigned long long max_match_count) {
  FileScan opt = ring_of(buffer_size, buffer_count, max_match_count);
  opt.on_event = on_event;
  return scan_file(file_name, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt);
}

extern "C" int hg_hyperscan_invert(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                                   const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hs_event on_event,
                                   const int buffer_size, int buffer_count, unsigned long long max_match_count) {
  FileScan opt = ring_of(buffer_size, buffer_count, max_match_count);
  opt.on_event = on_event;
  opt.invert = true;
  return scan_file(file_name, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt);
}

extern "C" int hg_hyperscan_parts(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                                  const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hs_event on_event,
                                  const int buffer_size, int buffer_count, unsigned long long max_match_count) {
  FileScan opt = ring_of(buffer_size, buffer_count, max_match_count);
  opt.on_event = on_event;
  opt.parts = true;
  return scan_file(file_name, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt);
}

extern "C" int hg_hyperscan_context(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                                    const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hs_event on_event,
                                    const int buffer_size, int buffer_count, unsigned long long max_match_count, unsigned int before, unsigned int after,
                                    int invert) {
  if (context_ids_clash(pattern_ids, elements)) return HYPERSCANNER_DB;
  FileScan opt = ring_of(buffer_size, buffer_count, max_match_count);
  opt.on_event = on_event;
  opt.invert = invert != 0;
  opt.before = before;
  opt.after = after;
  return scan_file(file_name, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt);
}

extern "C" int hg_hyperscan_counts(char *file_name, const char *const *patterns, const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                                   const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size, hg_id_count_t *counts,
                                   unsigned int max_counts, unsigned int *n_counts, uint64_t *n_lines) {
  if (!n_counts || (max_counts && !counts)) return HYPERSCANNER_STATE_MEM;
  *n_counts = 0;
  if (n_lines) *n_lines = 0;
  FileCounts fc;
  uint64_t pieces = 0;
  FileScan opt = ring_of(buffer_size, 1, 0);
  opt.on_event = no_event;
  opt.pieces_scanned = &pieces;
  opt.counts = &fc;
  const int rc = scan_file(file_name, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt);
  *n_counts = static_cast<unsigned int>(fc.ids.size());
  for (size_t b = 0; b < fc.ids.size() && b < max_counts; b++) counts[b] = hg_id_count_t{fc.ids[b], 0, fc.n_lines[b], fc.n_reports[b]};
  if (n_lines) *n_lines = pieces;
  return rc;
}

extern "C" int hg_hyperscan_values(char *file_name, const char *const *patterns, const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                                   const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size, const hg_values_params_t *params,
                                   hg_values_event on_values, void *context) {
  if (!on_values) return HYPERSCANNER_STATE_MEM;
  FileValues fv;
  fv.params = params ? *params : hg_values_params_t{0, 0, 0, 0};
  if (bad_values_params(fv.params)) return HYPERSCANNER_STATE_MEM;
  FileScan opt = ring_of(buffer_size, 1, 0);
  opt.on_event = no_event;
  opt.values = &fv;
  const int rc = scan_file(file_name, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt);
  if (rc) return rc;
  std::vector<size_t> order(fv.value.size());
  for (size_t j = 0; j < order.size(); j++) order[j] = j;
  const ValueRows r = fv.rows(order, order.size());
  on_values(context, r.bytes.data(), r.off.data(), r.count.data(), r.pattern.data(), order.size());
  return 0;
}

extern "C" int hg_hyperscan_values_top(char *file_name, const char *const *patterns, const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                                       const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size, const hg_values_params_t *params, uint64_t top,
                                       hg_values_event on_values, void *context, uint64_t *n_distinct, uint64_t *n_parts) {
  if (n_distinct) *n_distinct = 0;
  if (n_parts) *n_parts = 0;
  if (!on_values) return HYPERSCANNER_STATE_MEM;
  FileValues fv;
  fv.params = params ? *params : hg_values_params_t{0, 0, 0, 0};
  fv.on_device = true;
  fv.top = top;
  if (bad_values_params(fv.params)) return HYPERSCANNER_STATE_MEM;
  FileScan opt = ring_of(buffer_size, 1, 0);
  opt.on_event = no_event;
  opt.values = &fv;
  const int rc = scan_file(file_name, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt);
  if (rc) return rc;
  if (fv.ranked.off.empty()) fv.ranked.off.assign(1, 0);
  if (n_distinct) *n_distinct = fv.n_distinct;
  if (n_parts) *n_parts = fv.n_parts;
  on_values(context, fv.ranked.bytes.data(), fv.ranked.off.data(), fv.ranked.count.data(), fv.ranked.pattern.data(), fv.ranked.count.size());
  return 0;
}

extern "C" int hg_hyperscan_files(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                  const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event,
                                  void *context, const int buffer_size, int buffer_count, unsigned long long max_match_count, int invert,
                                  hg_file_summary_t *summaries) {
  FileScan opt = ring_of(buffer_size, buffer_count, max_match_count);
  opt.invert = invert != 0;
  const FilesOut to{on_event, context, summaries};
  return files_impl(file_names, n_files, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt, to);
}

extern "C" int hg_hyperscan_files_context(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                          const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event,
                                          void *context, const int buffer_size, int buffer_count, unsigned long long max_match_count, int invert,
                                          hg_file_summary_t *summaries, unsigned int before, unsigned int after) {
  if (on_event && context_ids_clash(pattern_ids, elements)) return HYPERSCANNER_DB;
  FileScan opt = ring_of(buffer_size, buffer_count, max_match_count);
  opt.invert = invert != 0;
  opt.before = before;
  opt.after = after;
  const FilesOut to{on_event, context, summaries};
  return files_impl(file_names, n_files, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt, to);
}

extern "C" int hg_hyperscan_files_parts(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                        const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event,
                                        void *context, const int buffer_size, int buffer_count, unsigned long long max_match_count,
                                        hg_file_summary_t *summaries) {
  FileScan opt = ring_of(buffer_size, buffer_count, max_match_count);
  opt.parts = true;
  const FilesOut to{on_event, context, summaries};
  return files_impl(file_names, n_files, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt, to);
}

extern "C" int hg_hyperscan_files_counts(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                         const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size,
                                         hg_file_summary_t *summaries, uint32_t *ids, unsigned int max_ids, unsigned int *n_ids, uint64_t *file_lines,
                                         uint64_t *file_reports) {
  if (!n_ids || (max_ids && (!ids || (n_files && (!file_lines || !file_reports))))) return HYPERSCANNER_STATE_MEM;
  const FilesCounts fcs{ids, max_ids, n_ids, file_lines, file_reports};
  FileScan opt = ring_of(buffer_size, 1, 0);
  FilesOut to;
  to.summaries = summaries;
  to.counts = &fcs;
  return files_impl(file_names, n_files, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt, to);
}

extern "C" int hg_hyperscan_files_values(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                         const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size,
                                         const hg_rank_params_t *params, hg_file_values_event on_file, void *context, hg_file_summary_t *summaries) {
  if (!on_file) return HYPERSCANNER_STATE_MEM;
  FilesValues fvs{params ? *params : hg_rank_params_t{0, 0, 0, 0, 0}, on_file, context};
  if ((fvs.params.flags & ~HG_RANK_BY_PATTERN) || fvs.params.hash_bits > 64 || fvs.params.table_log2 > HG_VALUES_MAX_TABLE_LOG2) return HYPERSCANNER_STATE_MEM;
  FileScan opt = ring_of(buffer_size, 1, 0);
  opt.parts = true;
  FilesOut to;
  to.summaries = summaries;
  to.values = &fvs;
  return files_impl(file_names, n_files, PatternSet{patterns, pattern_flags, pattern_ids, ext, elements}, opt, to);
}
