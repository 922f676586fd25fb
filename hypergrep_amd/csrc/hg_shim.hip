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

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hypergrep_amd.h"
#include "hg_compile.h"
#include "hg_engine.h"
#include "hg_mem.h"

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

// ---------------------------------------------------------------- input: plain / gzip / zstd
// gzopen("rb") in the reference (through zstd's zlibWrapper, hyperscanner.c:22,191) auto-detects gzip and
// zstd by magic and reads anything else verbatim; this reader does the same.
struct ZIn { const void *src; size_t size, pos; };
struct ZOut { void *dst; size_t size, pos; };
struct Zstd {
  void *lib = nullptr;
  void *(*create)() = nullptr;
  size_t (*destroy)(void *) = nullptr;
  size_t (*step)(void *, ZOut *, ZIn *) = nullptr;
  unsigned (*is_error)(size_t) = nullptr;
  bool load() {
    if (lib) return true;
    for (const char *name : {"libzstd.so.1", "libzstd.so"}) {
      lib = dlopen(name, RTLD_NOW);
      if (lib) break;
    }
    if (!lib) return false;
    create = reinterpret_cast<void *(*)()>(dlsym(lib, "ZSTD_createDStream"));
    destroy = reinterpret_cast<size_t (*)(void *)>(dlsym(lib, "ZSTD_freeDStream"));
    step = reinterpret_cast<size_t (*)(void *, ZOut *, ZIn *)>(dlsym(lib, "ZSTD_decompressStream"));
    is_error = reinterpret_cast<unsigned (*)(size_t)>(dlsym(lib, "ZSTD_isError"));
    return create && destroy && step && is_error;
  }
};
Zstd g_zstd;

class Reader {
 public:
  ~Reader() { close(); }
  bool open(const char *path) {
    fd_ = ::open(path, O_RDONLY);
    if (fd_ < 0) return false;
    struct stat st;
    if (fstat(fd_, &st) != 0 || S_ISDIR(st.st_mode)) return false;
    size_hint_ = S_ISREG(st.st_mode) ? static_cast<size_t>(st.st_size) : 0;
    unsigned char magic[4] = {0, 0, 0, 0};
    ssize_t got = ::pread(fd_, magic, 4, 0);
    if (got >= 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
      gz_ = gzdopen(fd_, "rb");
      if (!gz_) return false;
      fd_ = -1;  // owned by zlib now
      gzbuffer(gz_, 1 << 20);
      kind_ = 1;
    } else if (got == 4 && magic[0] == 0x28 && magic[1] == 0xB5 && magic[2] == 0x2F && magic[3] == 0xFD) {
      std::lock_guard<std::mutex> lock(g_mu);
      if (!g_zstd.load()) return false;
      zds_ = g_zstd.create();
      if (!zds_) return false;
      zin_.resize(1 << 20);
      kind_ = 2;
    }
    return true;
  }
  bool compressed() const { return kind_ != 0; }
  size_t size_hint() const { return size_hint_; }
  // Fill dst with up to n bytes; returns bytes produced, 0 at EOF, -1 on error.
  long read(uint8_t *dst, size_t n) {
    if (kind_ == 0) {
      // regular files: the request is cut into stripes read by parallel preads (one thread copies ~5 GB/s out of the page
      // cache, the host link takes ten times that); pipes and the like: plain read()
      auto pread_all = [this](uint8_t *p, size_t len, off_t at) -> long {
        size_t total = 0;
        while (total < len) {
          ssize_t r = ::pread(fd_, p + total, len - total, at + static_cast<off_t>(total));
          if (r < 0) return -1;
          if (r == 0) break;
          total += static_cast<size_t>(r);
        }
        return static_cast<long>(total);
      };
      if (size_hint_) {
        const size_t left = static_cast<size_t>(off_) < size_hint_ ? size_hint_ - static_cast<size_t>(off_) : 0;
        const size_t want = std::min(n, left);
        if (want == 0) {  // at the size seen at open: the file may have grown meanwhile
          const long g = pread_all(dst, n, off_);
          if (g > 0) off_ += g;
          return g;
        }
        const size_t kStripe = static_cast<size_t>(8) << 20;
        const unsigned workers = static_cast<unsigned>(std::min<size_t>(read_threads(), want / kStripe));
        long got;
        if (workers <= 1) {
          got = pread_all(dst, want, off_);
        } else {
          std::vector<long> part(workers, 0);
          std::vector<std::thread> pool;
          const size_t per = (want / workers + 4095) & ~static_cast<size_t>(4095);
          for (unsigned w = 0; w < workers; w++) {
            const size_t b = std::min(want, per * w), e = w + 1 == workers ? want : std::min(want, per * (w + 1));
            pool.emplace_back([&, w, b, e] { part[w] = pread_all(dst + b, e - b, off_ + static_cast<off_t>(b)); });
          }
          for (auto &t : pool) t.join();
          got = 0;
          for (unsigned w = 0; w < workers; w++) {
            const size_t b = std::min(want, per * w), e = w + 1 == workers ? want : std::min(want, per * (w + 1));
            if (part[w] < 0) return -1;
            got += part[w];
            if (static_cast<size_t>(part[w]) < e - b) break;  // the file shrank: stop at the first short stripe
          }
        }
        if (got > 0) off_ += got;
        return got;
      }
      size_t total = 0;
      while (total < n) {
        ssize_t r = ::read(fd_, dst + total, n - total);
        if (r < 0) return -1;
        if (r == 0) break;
        total += static_cast<size_t>(r);
      }
      return static_cast<long>(total);
    }
    if (kind_ == 1) {
      size_t total = 0;
      while (total < n) {
        unsigned want = static_cast<unsigned>(std::min<size_t>(n - total, 1u << 30));
        int r = gzread(gz_, dst + total, want);
        if (r < 0) return -1;
        if (r == 0) break;
        total += static_cast<size_t>(r);
      }
      return static_cast<long>(total);
    }
    size_t total = 0;
    while (total < n) {
      if (zpos_ == zlen_ && !zeof_) {
        ssize_t r = ::read(fd_, zin_.data(), zin_.size());
        if (r < 0) return -1;
        if (r == 0) zeof_ = true;
        zlen_ = static_cast<size_t>(r > 0 ? r : 0);
        zpos_ = 0;
      }
      if (zpos_ == zlen_ && zeof_) break;
      ZIn in{zin_.data(), zlen_, zpos_};
      ZOut out{dst + total, n - total, 0};
      size_t rc = g_zstd.step(zds_, &out, &in);
      if (g_zstd.is_error(rc)) return -1;
      zpos_ = in.pos;
      total += out.pos;
    }
    return static_cast<long>(total);
  }
  void close() {
    if (gz_) gzclose(gz_);
    gz_ = nullptr;
    if (fd_ >= 0) ::close(fd_);
    fd_ = -1;
    if (zds_) g_zstd.destroy(zds_);
    zds_ = nullptr;
  }

 private:
  static unsigned read_threads() {
    if (const char *env = std::getenv("HYPERGREP_READ_THREADS")) {
      long v = std::atol(env);
      if (v >= 1 && v <= 64) return static_cast<unsigned>(v);
    }
    const unsigned hw = std::thread::hardware_concurrency();
    return hw >= 16 ? 8u : (hw >= 4 ? hw / 2 : 1u);
  }
  int fd_ = -1, kind_ = 0;
  off_t off_ = 0;  // plain regular files are read with pread from here
  gzFile gz_ = nullptr;
  void *zds_ = nullptr;
  std::vector<uint8_t> zin_;
  size_t zpos_ = 0, zlen_ = 0, size_hint_ = 0;
  bool zeof_ = false;
};

// ---------------------------------------------------------------- result ring (hyperscanner.c:64-72, :83-102)
struct Ring {
  std::vector<hyperscanner_result_t> slots;
  char *storage = nullptr;  // buffer_count line buffers of buffer_size bytes (hyperscanner.c:277-291); malloc, not a zero-filled
                            // vector: with a large buffer_count most of it is never touched (1 GiB for 4096 x 262140)
  int fill = 0;
  std::function<void(hyperscanner_result_t *, int)> cb;  // (hs_event, or hg_hyperscan_files' event with its file index)
  unsigned long long delivered = 0;
  Ring() = default;
  Ring(const Ring &) = delete;
  Ring &operator=(const Ring &) = delete;
  ~Ring() { std::free(storage); }
  bool init(int count, int buffer_size, std::function<void(hyperscanner_result_t *, int)> on_event) {
    cb = std::move(on_event);
    try {
      slots.resize(static_cast<size_t>(count));
    } catch (const std::bad_alloc &) {
      return false;
    }
    storage = static_cast<char *>(std::malloc(static_cast<size_t>(count) * static_cast<size_t>(buffer_size)));
    if (!storage) return false;
    for (int i = 0; i < count; i++) slots[i].line = storage + static_cast<size_t>(i) * static_cast<size_t>(buffer_size);
    return true;
  }
  void push(unsigned id, unsigned long long line_number, const uint8_t *line, uint32_t len) {
    hyperscanner_result_t &r = slots[static_cast<size_t>(fill++)];
    r.id = id;
    r.line_number = line_number;
    std::memcpy(r.line, line, len);
    r.line[len] = 0;
    delivered++;
    if (fill == static_cast<int>(slots.size())) flush();
  }
  void flush() {
    if (fill) cb(slots.data(), fill);
    fill = 0;
  }
};

size_t chunk_bytes() {
  if (const char *env = std::getenv("HYPERGREP_CHUNK_MB")) {
    long mb = std::atol(env);
    if (mb >= 1 && mb <= 16384) return static_cast<size_t>(mb) << 20;
  }
  return static_cast<size_t>(256) << 20;
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

// Face B's file scan: the reports of the file's pieces, or (invert) one HG_ID_INVERT result per piece without a report.
// With context lines (before / after, hg_hyperscan_context) each chunk is scanned with the context stage behind it and the
// two ordered lists are merged; between chunks the call carries what the device API's chaining identity needs: the
// after-context still owed (owed_after -> carry_after) and the bytes of the previous chunks' tail pieces, `before` at most.
//
// With `fc` (hg_hyperscan_counts) nothing is delivered: the counts stage runs behind every chunk's scan, adding to its totals
// (chunks are cut at piece boundaries, so they share no line), no record is downloaded, and the bins and totals come back once
// at the end.  fc->ids is filled as soon as the database exists, the totals stay zero when the call fails.
using FileEvent = std::function<void(hyperscanner_result_t *, int)>;
struct FileCounts {
  std::vector<uint32_t> ids;
  std::vector<uint64_t> n_lines, n_reports;
};
// With `fv` (hg_hyperscan_values) nothing is delivered either: every chunk is scanned with the parts stage, the values stage runs
// behind it, and only the chunk's distinct values come back (bytes, offsets, counts, expressions), to be merged here by key.  No
// part record and no line is downloaded.  The rows keep the order in which their keys first occurred in the file.
// With fv->on_device (hg_hyperscan_values_top) not even those: a value store accumulates every chunk's parts on the device, one
// ranking at the end cuts it to `top` rows, and only those come back, in the ranking's order, with the totals before the cut.
struct FileValues {
  hg_values_params_t params;
  bool on_device = false;
  uint64_t top = 0, n_distinct = 0, n_parts = 0;
  std::vector<uint8_t> top_bytes;
  std::vector<uint64_t> top_off;
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
};
static int scan_file(const char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                     const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, FileEvent on_event,
                     const int buffer_size, int buffer_count, unsigned long long max_match_count, const bool invert, const uint32_t before = 0,
                     const uint32_t after = 0, uint64_t *pieces_scanned = nullptr, const bool parts = false, FileCounts *fc = nullptr, FileValues *fv = nullptr) {
  if (max_match_count > 0 && max_match_count < static_cast<unsigned long long>(buffer_count)) buffer_count = static_cast<int>(max_match_count);
  if (buffer_count < 1 || buffer_size < 1 || !on_event) return HYPERSCANNER_STATE_MEM;
  Ring ring;
  if (!ring.init(buffer_count, buffer_size, on_event)) return HYPERSCANNER_COMPILE_MEM;

  std::string err, db_key_str;
  std::shared_ptr<const HgDb> db = get_db(patterns, pattern_flags, pattern_ids, ext, elements, &err, &db_key_str);
  if (!db) {
    std::fprintf(stderr, "ERROR: Unable to create database. Exiting.\n");
    return HYPERSCANNER_DB;
  }
  if (parts) {
    if (const char *why = hg_parts_refusal(db->nhuge, db->ncomb, db->nquiet, db->n_ext != 0)) {
      std::fprintf(stderr, "ERROR: Unable to create database. Exiting. (%s)\n", why);
      return HYPERSCANNER_DB;
    }
  }
  std::unique_ptr<HgCounts> counts;  // (made with the scanner; its buffers are its own)
  std::unique_ptr<HgValues> values;  // (likewise)
  std::unique_ptr<HgValueStore> store;  // (likewise: the file's value store, hg_hyperscan_values_top)
  std::vector<uint8_t> v_bytes;      // a chunk's distinct values
  std::vector<uint64_t> v_off, v_count;
  std::vector<uint32_t> v_pattern;
  if (fc) {
    fc->ids = db->report_ids;
    fc->n_lines.assign(fc->ids.size(), 0);
    fc->n_reports.assign(fc->ids.size(), 0);
  }
  // the file is opened before any device resource is taken: a missing file is HYPERSCANNER_GZ_OPEN with or without a GPU
  // (the reference's scratch allocation cannot fail for want of a device; its order is database, scratch, file)
  Reader in;
  if (!file_name || !in.open(file_name)) return HYPERSCANNER_GZ_OPEN;
  if (buffer_size < 2) return 0;  // gzgets(len <= 1) returns NULL at once: nothing is scanned (hyperscanner.c:199)

  Ctx *ctx = checkout(db, &err);
  if (!ctx) {
    std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (%s)\n", err.c_str());
    return HYPERSCANNER_SCRATCH;
  }
  bool healthy = true;  // false after a device error: the context is destroyed, not pooled
  struct Return {
    Ctx *c;
    bool *healthy;
    ~Return() { checkin(c, *healthy); }
  } ret_guard{ctx, &healthy};

  const uint64_t bs1 = static_cast<uint64_t>(buffer_size) - 1;
  size_t cap = chunk_bytes();
  const bool one_chunk = !in.compressed() && in.size_hint() && in.size_hint() < cap;
  if (one_chunk) cap = std::max<size_t>(in.size_hint() + 16, 1 << 16);
  // a chunk must hold a whole piece plus the carry of the previous one — unless the whole file is one chunk anyway
  if (!one_chunk) cap = std::max<size_t>(cap, static_cast<size_t>(std::min<uint64_t>(2 * bs1 + 16, static_cast<uint64_t>(1) << 32)));
  const int nslots = one_chunk ? 1 : Ctx::kSlots;
  if (hipSetDevice(ctx->device) != hipSuccess || !ensure_buffers(ctx, cap, nslots)) {
    std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (device buffers)\n");
    healthy = false;
    return HYPERSCANNER_SCRATCH;
  }

  // ---- stage 1: the reader thread fills slots and cuts them at piece boundaries
  struct Slot {
    size_t cut = 0;     // bytes to scan (whole pieces)
    bool last = false;  // nothing follows
    int state = 0;      // 0 free (reader's), 1 ready (consumer's)
  };
  Slot slots[Ctx::kSlots];
  // HYPERGREP_TRACE=1: where the call's wall time went (seconds), printed to stderr at the end
  const bool trace = std::getenv("HYPERGREP_TRACE") != nullptr;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_call = now();
  double t_read = 0, t_wait_slot = 0, t_scan = 0, t_deliver = 0, t_setup = 0;  // reader: filling slots; consumer: waiting for a slot, copy + scan + hit copy, ring + callbacks
  uint64_t bytes_in = 0;
  std::mutex mu;
  std::condition_variable cv;
  bool abandon = false;  // the consumer stopped early (match limit, error)
  std::thread reader([&] {
    std::vector<uint8_t> carry;  // bytes after the cut, they open the next slot
    bool eof = false;
    for (unsigned k = 0;; k++) {
      Slot &s = slots[k % nslots];
      uint8_t *buf = ctx->h_slot[k % nslots];
      {
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return s.state == 0 || abandon; });
        if (abandon) return;
      }
      size_t have = carry.size();
      if (have) std::memcpy(buf, carry.data(), have);
      carry.clear();
      const double t_fill = now();
      while (!eof && have < cap) {
        const long got = in.read(buf + have, cap - have);
        if (got <= 0) {  // end of the stream; a read error ends it like gzgets returning NULL
          eof = true;
          break;
        }
        have += static_cast<size_t>(got);
      }
      t_read += now() - t_fill;
      size_t cut = have;
      if (!eof && have) {  // cut at a piece boundary so that every piece is scanned whole
        const void *nl = memrchr(buf, '\n', have);
        if (nl) cut = static_cast<size_t>(static_cast<const uint8_t *>(nl) - buf) + 1;
        else cut = static_cast<size_t>((have / bs1) * bs1);  // one unterminated line: stop at a forced break
        if (!cut) cut = have;
        carry.assign(buf + cut, buf + have);
      }
      {
        std::lock_guard<std::mutex> lock(mu);
        s.cut = cut;
        s.last = eof && carry.empty();
        s.state = 1;
      }
      cv.notify_all();
      if (eof && carry.empty()) return;
    }
  });
  auto stop_reader = [&] {
    {
      std::lock_guard<std::mutex> lock(mu);
      abandon = true;
    }
    cv.notify_all();
    reader.join();
  };

  // ---- stages 2 and 3: copy to HBM (one chunk ahead when the reader is), scan, deliver
  uint64_t line_base = 0;  // pieces delivered to the scanner so far == reference line_number of the chunk's first piece
  bool stop = false;
  // context lines
  const bool with_context = before || after;
  uint64_t carry_after = 0;  // after-context the chunks so far still owe
  struct HeldPiece {
    uint64_t line_no;
    std::string bytes;
  };
  std::deque<HeldPiece> held;  // tail pieces of the chunks so far: the next match's before-context, maybe (`before` at most)
  std::vector<HgHit> ctx_hits;
  std::vector<HgHitAux> ctx_aux;
  std::vector<HgPart> part_recs;  // matched parts (hg_hyperscan_parts): the chunk's parts and their expressions
  std::vector<uint32_t> part_pattern;
  unsigned long long matches = 0;  // match results delivered (max_match_count counts those, not the context lines)
  bool trailing = false;           // the limit is reached: only the last delivered line's after-context still goes out
  uint64_t trailing_next = 0, trailing_end = 0;  // ... the pieces [trailing_next, trailing_end), up to the next matching piece
  int rc = 0;
  bool copied[Ctx::kSlots] = {false, false, false};
  auto issue_copy = [&](unsigned k) -> bool {  // slot k -> device buffer k % 2, asynchronously
    const int sl = static_cast<int>(k % nslots), db_i = static_cast<int>(k % Ctx::kDevBufs);
    if (copied[sl]) return true;
    copied[sl] = true;
    if (!slots[sl].cut) return true;
    return hipMemcpyAsync(ctx->d_text[nslots > 1 ? db_i : 0], ctx->h_slot[sl], slots[sl].cut, hipMemcpyHostToDevice, ctx->copy_stream) == hipSuccess &&
           hipEventRecord(ctx->ev_h2d[db_i], ctx->copy_stream) == hipSuccess;
  };
  for (unsigned k = 0; !stop; k++) {
    const int sl = static_cast<int>(k % nslots);
    Slot &s = slots[sl];
    bool next_ready = false;
    {
      const double t0 = now();
      std::unique_lock<std::mutex> lock(mu);
      cv.wait(lock, [&] { return s.state == 1; });
      t_wait_slot += now() - t0;
      next_ready = nslots > 1 && !s.last && slots[(k + 1) % nslots].state == 1;
    }
    const uint8_t *host = ctx->h_slot[sl];
    const size_t cut = s.cut;
    const bool last = s.last;
    if (k == 0) {  // the pattern set's first large file picks the prefilter windows from this text (maybe_tune); then the scanner
      const double t0 = now();
      if (cut) db = maybe_tune(db_key_str, db, host, cut);
      if (!ensure_scanner(ctx, db, &err)) {
        std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (%s)\n", err.c_str());
        rc = HYPERSCANNER_SCRATCH;
        healthy = false;
        break;
      }
      if (fc) counts = std::make_unique<HgCounts>(ctx->device, *db);
      if (fv && fv->on_device) store = std::make_unique<HgValueStore>(ctx->device);
      else if (fv) values = std::make_unique<HgValues>(ctx->device);
      t_setup = now() - t0;
    }
    if (cut) {
      const double t_begin = now();
      bytes_in += cut;
      uint8_t *d_text = ctx->d_text[nslots > 1 ? k % Ctx::kDevBufs : 0];
      if (!issue_copy(k) || (next_ready && !issue_copy(k + 1)) ||  // the next chunk travels while this one is scanned
          hipStreamWaitEvent(ctx->stream, ctx->ev_h2d[k % Ctx::kDevBufs], 0) != hipSuccess) {
        rc = HYPERSCANNER_SCAN;
        healthy = false;
        break;
      }
      HgScanOutput out{};
      HgContextOutput cout{};
      HgPartsOutput pout{};
      int src;
      if (parts) {
        src = ctx->sc->scan_parts(d_text, cut, buffer_size, line_base, ctx->stream, &out, &pout);
      } else if (with_context) {
        // (after the limit: the owed pieces only, as carry; no new windows, no tail)
        const HgContextParams cp{trailing ? 0u : before, trailing ? 0u : after, trailing ? trailing_end - trailing_next : carry_after, !trailing && before != 0};
        src = ctx->sc->scan_context(d_text, cut, buffer_size, line_base, ctx->stream, cp, invert, &out, &cout);
      } else {
        src = ctx->sc->scan(d_text, cut, buffer_size, line_base, ctx->stream, &out, invert);
      }
      if (src != HG_OK) {
        std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (%s)\n", ctx->sc->last_error().c_str());
        rc = HYPERSCANNER_SCAN;
        healthy = false;
        break;
      }
      if (counts) {  // the chunk's records are counted where they lie: none is downloaded, nothing is delivered below
        HgCountsOutput co{};
        if (counts->run(HgCountsInput{HgCountsList{out.d_hits, nullptr, out.n_hits}, 0, HG_COUNTS_F_ACCUMULATE}, ctx->stream, &co, &err) != HG_OK) {
          std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (%s)\n", err.c_str());
          rc = HYPERSCANNER_SCAN;
          healthy = false;
          break;
        }
      }
      if (store) {  // the chunk's parts join the file's store where they lie: nothing comes back
        const uint32_t log2 = fv->params.table_log2 ? fv->params.table_log2 : hg_values_default_log2(pout.n_parts);
        if (log2 > HG_VALUES_MAX_TABLE_LOG2 || (uint64_t{1} << log2) <= pout.n_parts) {
          std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (a chunk has %llu parts: more than a table of 2^%u slots serves)\n",
                       static_cast<unsigned long long>(pout.n_parts), log2);
          rc = HYPERSCANNER_SCAN;
          break;
        }
        HgValStoreInput vin{};
        vin.values = HgValuesInput{d_text, HgGatherList{out.d_hits, out.d_aux, nullptr, out.n_hits}, pout.d_parts, pout.d_pattern, nullptr, pout.n_parts, nullptr, fv->params.flags,
                                   fv->params.hash_bits ? fv->params.hash_bits : 64u, log2};
        HgValStoreOutput so{};
        if (store->accumulate(vin, ctx->stream, &so, &err) != HG_OK) {
          std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (%s)\n", err.c_str());
          rc = HYPERSCANNER_SCAN;
          healthy = false;
          break;
        }
      }
      if (values) {  // the chunk's parts are grouped where they lie: only the distinct values come back
        const uint32_t log2 = fv->params.table_log2 ? fv->params.table_log2 : hg_values_default_log2(pout.n_parts);
        HgValuesOutput vo{};
        if (log2 > HG_VALUES_MAX_TABLE_LOG2 || (uint64_t{1} << log2) <= pout.n_parts) {
          std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (a chunk has %llu parts: more than a table of 2^%u slots serves)\n",
                       static_cast<unsigned long long>(pout.n_parts), log2);
          rc = HYPERSCANNER_SCAN;
          break;
        }
        const HgValuesInput vin{d_text, HgGatherList{out.d_hits, out.d_aux, nullptr, out.n_hits}, pout.d_parts, pout.d_pattern, nullptr, pout.n_parts, nullptr, fv->params.flags,
                                fv->params.hash_bits ? fv->params.hash_bits : 64u, log2};
        bool ok = values->run(vin, ctx->stream, &vo, &err) == HG_OK;
        if (ok) {
          v_bytes.resize(vo.n_bytes);
          v_off.resize(vo.n_values + 1);
          v_count.resize(vo.n_values);
          v_pattern.resize(vo.n_values);
          ok = (!vo.n_bytes || hipMemcpyAsync(v_bytes.data(), vo.d_bytes, vo.n_bytes, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess) &&
               hipMemcpyAsync(v_off.data(), vo.d_off, (vo.n_values + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
               (!vo.n_values || (hipMemcpyAsync(v_count.data(), vo.d_count, vo.n_values * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                                 hipMemcpyAsync(v_pattern.data(), vo.d_pattern, vo.n_values * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess)) &&
               hipStreamSynchronize(ctx->stream) == hipSuccess;
          if (!ok) err = "copying the values";
        }
        if (!ok) {
          std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (%s)\n", err.c_str());
          rc = HYPERSCANNER_SCAN;
          healthy = false;
          break;
        }
        for (uint64_t j = 0; j < vo.n_values; j++) fv->add(v_bytes.data() + v_off[j], v_off[j + 1] - v_off[j], v_pattern[j], v_count[j]);
      }
      const uint64_t n_rows = counts || values || store ? 0 : out.n_hits;
      ctx->hits.resize(n_rows);
      ctx->aux.resize(n_rows);
      if (n_rows) {
        if (hipMemcpyAsync(ctx->hits.data(), out.d_hits, out.n_hits * sizeof(HgHit), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(ctx->aux.data(), out.d_aux, out.n_hits * sizeof(HgHitAux), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
          rc = HYPERSCANNER_SCAN;
          healthy = false;
          break;
        }
      }
      ctx_hits.resize(cout.n_context);
      ctx_aux.resize(cout.n_context);
      if (cout.n_context) {
        if (hipMemcpyAsync(ctx_hits.data(), cout.d_hits, cout.n_context * sizeof(HgHit), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(ctx_aux.data(), cout.d_aux, cout.n_context * sizeof(HgHitAux), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
          rc = HYPERSCANNER_SCAN;
          healthy = false;
          break;
        }
      }
      const uint64_t n_part_rows = values ? 0 : pout.n_parts;
      part_recs.resize(n_part_rows);
      part_pattern.resize(n_part_rows);
      if (n_part_rows) {
        if (hipMemcpyAsync(part_recs.data(), pout.d_parts, pout.n_parts * sizeof(HgPart), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(part_pattern.data(), pout.d_pattern, pout.n_parts * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
          rc = HYPERSCANNER_SCAN;
          healthy = false;
          break;
        }
      }
      size_t pi = 0;  // cursor into the parts
      const double t_scanned = now();
      t_scan += t_scanned - t_begin;
      size_t ci = 0;  // cursor into the context records
      // the owed after-context of the last delivered line: consecutive pieces, ending before the next matching piece (which is
      // no context record) or when all are out
      auto deliver_trailing = [&] {
        while (ci < ctx_hits.size() && ctx_hits[ci].line_no < trailing_next) ci++;
        while (trailing_next < trailing_end && ci < ctx_hits.size() && ctx_hits[ci].line_no == trailing_next && ctx_hits[ci].id == HG_CTX_ID_CONTEXT) {
          ring.push(HG_CTX_ID_CONTEXT, trailing_next, host + ctx_aux[ci].start, ctx_aux[ci].len);
          ci++;
          trailing_next++;
        }
        if (trailing_next < line_base + out.n_pieces) trailing_end = trailing_next;  // stopped inside the chunk: nothing is owed any more
      };
      std::vector<size_t> tails;  // this chunk's tail records
      // context records below `upto`, in order; tail records are set aside
      auto deliver_context = [&](uint64_t upto) {
        for (; ci < ctx_hits.size() && ctx_hits[ci].line_no < upto; ci++) {
          if (ctx_hits[ci].id == HG_CTX_ID_TAIL) tails.push_back(ci);
          else ring.push(HG_CTX_ID_CONTEXT, ctx_hits[ci].line_no, host + ctx_aux[ci].start, ctx_aux[ci].len);
        }
      };
      const bool was_trailing = trailing;
      if (trailing) {
        deliver_trailing();
        stop = trailing_next >= trailing_end;
      } else if (with_context && !ctx->hits.empty()) {  // the held tail pieces within `before` of the chunk's first match
        for (const HeldPiece &hp : held)
          if (hp.line_no + before >= ctx->hits[0].line_no) ring.push(HG_CTX_ID_CONTEXT, hp.line_no, reinterpret_cast<const uint8_t *>(hp.bytes.data()), static_cast<uint32_t>(hp.bytes.size()));
        held.clear();
      }
      // deliver line by line; inside a line reports go out by ascending end offset, then id (hs_scan order)
      size_t i = 0;
      while (i < ctx->hits.size() && !stop && !was_trailing) {
        if (with_context) deliver_context(ctx->hits[i].line_no);
        size_t j = i;
        while (j < ctx->hits.size() && ctx->hits[j].line_no == ctx->hits[i].line_no) j++;
        if (parts) {  // every part of the line, in order, in place of its reports (which still count for the limit)
          while (pi < part_recs.size() && part_recs[pi].line_no < ctx->hits[i].line_no) pi++;
          for (; pi < part_recs.size() && part_recs[pi].line_no == ctx->hits[i].line_no; pi++)
            ring.push(db->patterns[part_pattern[pi]].id, part_recs[pi].line_no, host + ctx->aux[i].start + part_recs[pi].from, part_recs[pi].to - part_recs[pi].from);
        } else if (j - i > 1) {
          std::vector<size_t> order(j - i);
          for (size_t q = 0; q < order.size(); q++) order[q] = i + q;
          std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
            if (ctx->hits[x].to != ctx->hits[y].to) return ctx->hits[x].to < ctx->hits[y].to;
            return ctx->hits[x].id < ctx->hits[y].id;
          });
          for (size_t q : order) ring.push(ctx->hits[q].id, ctx->hits[q].line_no, host + ctx->aux[q].start, ctx->aux[q].len);
        } else {
          ring.push(ctx->hits[i].id, ctx->hits[i].line_no, host + ctx->aux[i].start, ctx->aux[i].len);
        }
        // the reference checks the limit after each line's hs_scan returns (hyperscanner.c:222-224)
        matches += j - i;
        if (max_match_count > 0 && matches >= max_match_count) {
          stop = true;
          if (after) {  // GNU grep's -m with -A: the trailing context of the last delivered line still goes out
            trailing = true;
            trailing_next = ctx->hits[i].line_no + 1;
            trailing_end = hg_sat_add(trailing_next, after);
            deliver_trailing();
            stop = trailing_next >= trailing_end;  // else the chunk ended first: the next one is read for what is still owed
            break;
          }
        }
        i = j;
      }
      if (with_context && !trailing && !stop) {  // (a call that ends at the limit delivers nothing behind its last line but that line's after-context)
        deliver_context(~0ull);
        // the tail pieces' bytes leave the pinned slot before it goes back to the reader
        for (size_t t : tails) held.push_back(HeldPiece{ctx_hits[t].line_no, std::string(reinterpret_cast<const char *>(host) + ctx_aux[t].start, ctx_aux[t].len)});
        while (held.size() > before) held.pop_front();
        carry_after = cout.owed_after;
      }
      line_base += out.n_pieces;
      t_deliver += now() - t_scanned;
    }
    copied[sl] = false;
    {
      std::lock_guard<std::mutex> lock(mu);
      s.state = 0;  // the slot goes back to the reader
    }
    cv.notify_all();
    if (last) break;
  }
  stop_reader();
  (void)hipStreamSynchronize(ctx->copy_stream);  // a copy issued ahead may still be in flight
  ring.flush();
  if (pieces_scanned) *pieces_scanned = line_base;
  if (counts && rc == 0 && !counts->copy_totals(fc->n_lines.data(), fc->n_reports.data())) {  // n_bins x 16 bytes, once
    rc = HYPERSCANNER_SCAN;
    healthy = false;
  }
  if (store && rc == 0 && store->began()) {  // one ranking, and the kept rows once
    HgValRankOutput ro{};
    bool ok = store->rank(fv->top, false, ctx->stream, &ro, &err) == HG_OK;
    if (ok) {
      fv->n_distinct = ro.n_distinct;
      fv->n_parts = ro.n_parts;
      fv->top_bytes.resize(ro.n_bytes);
      fv->top_off.resize(ro.n_values + 1);
      fv->count.resize(ro.n_values);
      fv->pattern.resize(ro.n_values);
      ok = (!ro.n_bytes || hipMemcpyAsync(fv->top_bytes.data(), ro.d_bytes, ro.n_bytes, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess) &&
           hipMemcpyAsync(fv->top_off.data(), ro.d_off, (ro.n_values + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
           (!ro.n_values || (hipMemcpyAsync(fv->count.data(), ro.d_count, ro.n_values * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                             hipMemcpyAsync(fv->pattern.data(), ro.d_pattern, ro.n_values * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess)) &&
           hipStreamSynchronize(ctx->stream) == hipSuccess;
      if (!ok) err = "copying the values";
    }
    if (!ok) {
      std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (%s)\n", err.c_str());
      rc = HYPERSCANNER_SCAN;
      healthy = false;
    }
  }
  if (trace)
    std::fprintf(stderr, "[hypergrep_amd] %s: %.1f MiB in %.4f s; reader filling slots %.4f s; consumer: waiting for data %.4f s, window tuning + scanner %.4f s (%s), copy + scan %.4f s, delivering %llu hits %.4f s\n",
                 file_name, bytes_in / 1048576.0, now() - t_call, t_read, t_wait_slot, t_setup, db->tuned ? "tuned windows" : "static windows", t_scan,
                 static_cast<unsigned long long>(ring.delivered), t_deliver);
  return rc;
}

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
// With `fcs` (hg_hyperscan_files_counts; on_event is NULL then) the counts stage runs behind every pack's segment stage with
// per-segment matrices, which are all that leaves the GPU beside the per-file arrays; a pack is closed early where one more
// file would take the matrices past the stage's limit of cells.  Files of the per-file route take scan_file with counts.
//
// With `fvs` (hg_hyperscan_files_values; on_event is NULL then) every pack is scanned with parts and the rank stage runs behind
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
static int files_impl(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                      const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event, void *context,
                      const int buffer_size, int buffer_count, unsigned long long max_match_count, int invert, hg_file_summary_t *summaries, uint32_t before,
                      uint32_t after, bool parts = false, const FilesCounts *fcs = nullptr, const FilesValues *fvs = nullptr) {
  if (!on_event) before = after = 0;  // summaries only: they are those of the call without context
  const bool with_context = before || after;
  if (!summaries || (!file_names && n_files) || buffer_count < 1 || buffer_size < 1) return HYPERSCANNER_STATE_MEM;
  if (fcs && fcs->n_ids) *fcs->n_ids = 0;
  if (max_match_count > 0 && max_match_count < static_cast<unsigned long long>(buffer_count)) buffer_count = static_cast<int>(max_match_count);
  for (unsigned int i = 0; i < n_files; i++) summaries[i] = hg_file_summary_t{0, 0, 0};
  std::string err;
  std::shared_ptr<const HgDb> db = get_db(patterns, pattern_flags, pattern_ids, ext, elements, &err);
  if (!db) {
    std::fprintf(stderr, "ERROR: Unable to create database. Exiting.\n");
    return HYPERSCANNER_DB;
  }
  if (parts) {  // refused for the whole call, before anything is read (as hg_hyperscan_parts)
    if (const char *why = hg_parts_refusal(db->nhuge, db->ncomb, db->nquiet, db->n_ext != 0)) {
      std::fprintf(stderr, "ERROR: Unable to create database. Exiting. (%s)\n", why);
      return HYPERSCANNER_DB;
    }
    if (!on_event && !fvs) parts = false;  // summaries only: they are those of the call without parts
  }
  const size_t n_bins = db->report_ids.size(), n_cols = fcs ? std::min<size_t>(n_bins, fcs->max_ids) : 0;
  if (fcs) {
    *fcs->n_ids = static_cast<unsigned int>(n_bins);
    std::copy(db->report_ids.begin(), db->report_ids.begin() + n_cols, fcs->ids);
    std::fill(fcs->file_lines, fcs->file_lines + static_cast<size_t>(n_files) * fcs->max_ids, uint64_t{0});
    std::fill(fcs->file_reports, fcs->file_reports + static_cast<size_t>(n_files) * fcs->max_ids, uint64_t{0});
  }
  std::vector<uint32_t> seg_lines, seg_reports;  // the pack's matrices
  std::unique_ptr<HgRank> rank;  // (hg_hyperscan_files_values: made with the first pack, on its device; its buffers are its own)
  int rank_device = -1;
  std::vector<uint8_t> r_bytes;  // a pack's kept rows and per-file arrays
  std::vector<uint64_t> r_off, r_count, r_first_value, r_distinct, r_parts;
  std::vector<uint32_t> r_pattern;
  // one file through the per-file route: its events carry its index, its distinct lines are counted on the way
  auto single = [&](unsigned int f) {
    uint64_t selected = 0, last = ~0ull, pieces = 0;
    FileEvent ev = [&](hyperscanner_result_t *r, int n) {
      for (int i = 0; i < n; i++)
        if (r[i].line_number != last && !(with_context && r[i].id == HG_CTX_ID_CONTEXT)) {  // (a context line is no result of the file's)
          last = r[i].line_number;
          selected++;
        }
      if (on_event) on_event(f, r, n, context);
    };
    FileCounts fc;
    FileValues fv;
    if (fvs) fv.params = hg_values_params_t{fvs->params.flags & HG_VALUES_BY_PATTERN, fvs->params.hash_bits, fvs->params.table_log2, 0};
    const int rc = scan_file(file_names[f], patterns, pattern_flags, pattern_ids, ext, elements, ev, buffer_size, buffer_count, max_match_count, invert != 0, before, after, &pieces, parts,
                             fcs ? &fc : nullptr, fvs ? &fv : nullptr);
    if (fvs && rc) fvs->none(f);
    if (fvs && !rc) {  // the merged rows come in the order of their first occurrence: a stable sort by count, then the cut
      std::vector<size_t> order(fv.value.size());
      for (size_t j = 0; j < order.size(); j++) order[j] = j;
      std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return fv.count[x] > fv.count[y]; });
      uint64_t n_parts = 0;
      for (uint64_t c : fv.count) n_parts += c;
      const size_t kept = fvs->params.top && fvs->params.top < order.size() ? static_cast<size_t>(fvs->params.top) : order.size();
      std::vector<uint8_t> bytes;
      std::vector<uint64_t> off(1, 0), count(kept);
      std::vector<uint32_t> pattern(kept);
      for (size_t j = 0; j < kept; j++) {
        const std::string &v = fv.value[order[j]];
        bytes.insert(bytes.end(), v.begin(), v.end());
        off.push_back(bytes.size());
        count[j] = fv.count[order[j]];
        pattern[j] = fv.pattern[order[j]];
      }
      fvs->on_file(fvs->context, f, bytes.data(), off.data(), count.data(), pattern.data(), kept, order.size(), n_parts);
    }
    if (fcs && fc.n_lines.size() >= n_cols) {  // (nothing was delivered, so `selected` stays 0: the row says what was selected)
      std::copy(fc.n_lines.begin(), fc.n_lines.begin() + n_cols, fcs->file_lines + static_cast<size_t>(f) * fcs->max_ids);
      std::copy(fc.n_reports.begin(), fc.n_reports.begin() + n_cols, fcs->file_reports + static_cast<size_t>(f) * fcs->max_ids);
    }
    summaries[f] = hg_file_summary_t{rc, pieces, selected};
  };
  const size_t cap = chunk_bytes();
  Ctx *ctx = nullptr;
  bool healthy = true;
  struct Return {
    Ctx **c;
    bool *healthy;
    ~Return() {
      if (*c) checkin(*c, *healthy);
    }
  } ret_guard{&ctx, &healthy};
  uint64_t *d_segs = nullptr;  // seg_start and seg_end of the pack, one after the other
  size_t d_segs_cap = 0;
  struct FreeSegs {
    uint64_t **p;
    ~FreeSegs() { hgmem::dev_free(*p, "d_segs"); }
  } free_segs{&d_segs};
  std::vector<uint64_t> seg_start, seg_end, first, n_lines, n_selected, first_ctx;
  std::vector<HgHit> ctx_hits;  // the pack's context records, file-relative, file after file
  std::vector<HgHitAux> ctx_aux;
  std::vector<HgPart> part_recs;  // matched parts (hg_hyperscan_files_parts): the pack's parts, file-relative, file after file
  std::vector<uint32_t> part_pattern;
  std::vector<uint64_t> first_part;
  std::vector<unsigned int> seg_file;
  size_t fill = 0;  // bytes of the pack so far (in ctx->h_slot[0])
  Ring ring;
  unsigned int cur_file = 0;
  if (on_event && !ring.init(buffer_count, std::max(buffer_size, 2), [&](hyperscanner_result_t *r, int n) { on_event(cur_file, r, n, context); }))
    return HYPERSCANNER_COMPILE_MEM;
  auto fail_pack = [&](int rc) {
    for (unsigned int f : seg_file) {
      summaries[f].rc = rc;
      if (fvs) fvs->none(f);
    }
    healthy = false;
  };
  // scan the pack and deliver its files
  auto flush_pack = [&]() {
    if (seg_file.empty()) return;
    const size_t n_seg = seg_file.size();
    bool ok = hipSetDevice(ctx->device) == hipSuccess && ensure_scanner(ctx, db, &err);
    if (ok && 2 * n_seg > d_segs_cap) {
      hgmem::dev_free(d_segs, "d_segs");
      d_segs = nullptr;
      d_segs_cap = std::max<size_t>(2 * n_seg + n_seg / 2, 4096);
      ok = hgmem::dev_alloc(&d_segs, d_segs_cap * sizeof(uint64_t), "d_segs") == hipSuccess;
      if (!ok) d_segs_cap = 0;
    }
    if (!ok) {
      std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (%s)\n", err.c_str());
      fail_pack(HYPERSCANNER_SCRATCH);
    } else {
      const uint8_t *host = ctx->h_slot[0];
      HgScanOutput out{};
      HgSegOutput seg{};
      const HgSegParams params{d_segs, d_segs + n_seg, static_cast<uint32_t>(n_seg), max_match_count};
      first.resize(n_seg + 1);
      n_lines.resize(n_seg);
      n_selected.resize(n_seg);
      bool copied = (!fill || hipMemcpyAsync(ctx->d_text[0], host, fill, hipMemcpyHostToDevice, ctx->stream) == hipSuccess) &&
                    hipMemcpyAsync(d_segs, seg_start.data(), n_seg * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                    hipMemcpyAsync(d_segs + n_seg, seg_end.data(), n_seg * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                    hipStreamSynchronize(ctx->stream) == hipSuccess;
      HgContextOutput cout{};
      HgSegCtxOutput sx{};
      HgPartsOutput pout{};
      HgSegPartsOutput spo{};
      int src = !copied        ? HG_ERR_HIP
                : parts        ? ctx->sc->scan_packed_parts(ctx->d_text[0], fill, buffer_size, ctx->stream, params, &out, &seg, &pout, &spo)
                : with_context ? ctx->sc->scan_packed_context(ctx->d_text[0], fill, buffer_size, ctx->stream, params, before, after, invert != 0, &out, &seg, &cout, &sx)
                               : ctx->sc->scan_packed(ctx->d_text[0], fill, buffer_size, ctx->stream, params, invert != 0, &out, &seg);
      first_ctx.assign(n_seg + 1, 0);
      ctx_hits.resize(src == HG_OK ? cout.n_context : 0);
      ctx_aux.resize(ctx_hits.size());
      if (src == HG_OK && with_context &&
          ((cout.n_context && (hipMemcpyAsync(ctx_hits.data(), cout.d_hits, cout.n_context * sizeof(HgHit), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                               hipMemcpyAsync(ctx_aux.data(), cout.d_aux, cout.n_context * sizeof(HgHitAux), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)) ||
           hipMemcpyAsync(first_ctx.data(), sx.d_first_context, (n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
        src = HG_ERR_HIP;  // (the synchronisation below waits for these copies too)
      first_part.assign(n_seg + 1, 0);
      part_recs.resize(src == HG_OK && !fvs ? pout.n_parts : 0);  // (with fvs no part record comes back)
      part_pattern.resize(part_recs.size());
      if (src == HG_OK && parts && !fvs &&
          ((pout.n_parts && (hipMemcpyAsync(part_recs.data(), pout.d_parts, pout.n_parts * sizeof(HgPart), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                             hipMemcpyAsync(part_pattern.data(), pout.d_pattern, pout.n_parts * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)) ||
           hipMemcpyAsync(first_part.data(), spo.d_first_part, (n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
        src = HG_ERR_HIP;
      if (src == HG_OK) {
        const bool rows = on_event != nullptr && out.n_hits;  // counts only: no record leaves the GPU
        ctx->hits.resize(rows ? out.n_hits : 0);
        ctx->aux.resize(rows ? out.n_hits : 0);
        if ((rows && (hipMemcpyAsync(ctx->hits.data(), out.d_hits, out.n_hits * sizeof(HgHit), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                      hipMemcpyAsync(ctx->aux.data(), out.d_aux, out.n_hits * sizeof(HgHitAux), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)) ||
            hipMemcpyAsync(first.data(), seg.d_first_record, (n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(n_lines.data(), seg.d_n_lines, n_seg * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(n_selected.data(), seg.d_n_selected, n_seg * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
          src = HG_ERR_HIP;
      }
      if (src == HG_OK && fcs && n_bins) {  // the counts stage behind the segment stage; the two matrices come back
        HgCounts counts(ctx->device, *db);
        HgCountsOutput co{};
        const size_t cells = n_seg * n_bins;
        seg_lines.resize(cells);
        seg_reports.resize(cells);
        src = counts.run(HgCountsInput{HgCountsList{out.d_hits, seg.d_record_segment, out.n_hits}, static_cast<uint32_t>(n_seg), HG_COUNTS_F_PER_SEGMENT}, ctx->stream, &co, &err);
        if (src == HG_OK && (hipMemcpy(seg_lines.data(), co.d_seg_lines, cells * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
                             hipMemcpy(seg_reports.data(), co.d_seg_reports, cells * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess))
          src = HG_ERR_HIP;
      }
      HgRankOutput ro{};
      if (src == HG_OK && fvs) {  // the rank stage behind the parts stage, per file; the kept rows and the per-file arrays come back
        const uint32_t log2 = fvs->params.table_log2 ? fvs->params.table_log2 : hg_values_default_log2(pout.n_parts);
        if (log2 > HG_VALUES_MAX_TABLE_LOG2 || (uint64_t{1} << log2) <= pout.n_parts) {
          err = "a pack has " + std::to_string(pout.n_parts) + " parts: more than a table of 2^" + std::to_string(log2) + " slots serves";
          src = HG_ERR_ARG;
        } else {
          if (!rank || rank_device != ctx->device) {
            rank = std::make_unique<HgRank>(ctx->device);
            rank_device = ctx->device;
          }
          HgRankInput rin{};
          rin.values = HgValuesInput{ctx->d_text[0], HgGatherList{out.d_hits, out.d_aux, seg.d_record_segment, out.n_hits}, pout.d_parts, pout.d_pattern, spo.d_part_segment, pout.n_parts,
                                     d_segs, (fvs->params.flags & HG_RANK_F_BY_PATTERN) | HG_RANK_F_PER_SEGMENT, fvs->params.hash_bits ? fvs->params.hash_bits : 64u, log2};
          rin.n_seg = static_cast<uint32_t>(n_seg);
          rin.top = fvs->params.top;
          src = rank->run(rin, ctx->stream, &ro, &err);
        }
        if (src == HG_OK) {
          r_bytes.resize(ro.n_bytes);
          r_off.resize(ro.n_values + 1);
          r_count.resize(ro.n_values);
          r_pattern.resize(ro.n_values);
          r_first_value.resize(n_seg + 1);
          r_distinct.resize(n_seg);
          r_parts.resize(n_seg);
          if ((ro.n_bytes && hipMemcpyAsync(r_bytes.data(), ro.d_bytes, ro.n_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
              hipMemcpyAsync(r_off.data(), ro.d_off, (ro.n_values + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
              (ro.n_values && (hipMemcpyAsync(r_count.data(), ro.d_count, ro.n_values * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                               hipMemcpyAsync(r_pattern.data(), ro.d_pattern, ro.n_values * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)) ||
              hipMemcpyAsync(r_first_value.data(), ro.d_first_value, (n_seg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
              hipMemcpyAsync(r_distinct.data(), ro.d_seg_distinct, n_seg * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
              hipMemcpyAsync(r_parts.data(), ro.d_seg_parts, n_seg * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
              hipStreamSynchronize(ctx->stream) != hipSuccess) {
            err = "copying the ranked values";
            src = HG_ERR_HIP;
          }
        }
        if (src != HG_OK) ctx->sc->set_error(src, err);
      }
      if (src != HG_OK) {
        std::fprintf(stderr, "ERROR: Unable to scan buffer. Exiting. (%s)\n", ctx->sc ? ctx->sc->last_error().c_str() : "copy");
        fail_pack(HYPERSCANNER_SCAN);
      } else {
        if (std::getenv("HYPERGREP_TRACE"))  // the packed route: one line per pack
          std::fprintf(stderr, "[hypergrep_amd] pack: %zu files, %.1f MiB in one scan; segment stage %.0f us, %llu records; context stage %.0f us, %llu context records\n", n_seg,
                       fill / 1048576.0, seg.ms_segments * 1e3, static_cast<unsigned long long>(out.n_hits), cout.ms_context * 1e3,
                       static_cast<unsigned long long>(cout.n_context));
        for (size_t s = 0; s < n_seg; s++) {
          cur_file = seg_file[s];
          summaries[cur_file] = hg_file_summary_t{0, n_lines[s], n_selected[s]};
          if (fcs)
            for (size_t b = 0; b < n_cols; b++) {
              fcs->file_lines[static_cast<size_t>(cur_file) * fcs->max_ids + b] = seg_lines[s * n_bins + b];
              fcs->file_reports[static_cast<size_t>(cur_file) * fcs->max_ids + b] = seg_reports[s * n_bins + b];
            }
          if (fvs) {  // the file's rows of the pack's ranking (off[0] is where its first value lies among the pack's bytes)
            const uint64_t lo = r_first_value[s], n = r_first_value[s + 1] - lo;
            fvs->on_file(fvs->context, cur_file, r_bytes.data(), r_off.data() + lo, r_count.data() + lo, r_pattern.data() + lo, n, r_distinct[s], r_parts[s]);
          }
          if (!on_event) continue;
          const uint8_t *base = host + seg_start[s];  // the records are file-relative
          if (parts) {  // every part of each kept line, in order, in place of its reports (as scan_file)
            size_t pi = first_part[s];
            for (size_t i = first[s], j; i < first[s + 1]; i = j) {
              for (j = i; j < first[s + 1] && ctx->hits[j].line_no == ctx->hits[i].line_no; j++) {}
              for (; pi < first_part[s + 1] && part_recs[pi].line_no == ctx->hits[i].line_no; pi++)
                ring.push(db->patterns[part_pattern[pi]].id, part_recs[pi].line_no, base + ctx->aux[i].start + part_recs[pi].from, part_recs[pi].to - part_recs[pi].from);
            }
            ring.flush();  // no batch mixes files
            continue;
          }
          // line by line; inside a line reports go out by ascending end offset, then id (as scan_file)
          size_t ci = first_ctx[s];  // the file's context records below a line go out in front of it, the rest behind the last
          const auto deliver_context = [&](uint64_t upto) {
            for (; ci < first_ctx[s + 1] && ctx_hits[ci].line_no < upto; ci++) ring.push(HG_CTX_ID_CONTEXT, ctx_hits[ci].line_no, base + ctx_aux[ci].start, ctx_aux[ci].len);
          };
          for (size_t i = first[s], j; i < first[s + 1]; i = j) {
            deliver_context(ctx->hits[i].line_no);
            for (j = i; j < first[s + 1] && ctx->hits[j].line_no == ctx->hits[i].line_no; j++) {}
            std::vector<size_t> order(j - i);
            for (size_t q = 0; q < order.size(); q++) order[q] = i + q;
            std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
              if (ctx->hits[x].to != ctx->hits[y].to) return ctx->hits[x].to < ctx->hits[y].to;
              return ctx->hits[x].id < ctx->hits[y].id;
            });
            for (size_t q : order) ring.push(ctx->hits[q].id, ctx->hits[q].line_no, base + ctx->aux[q].start, ctx->aux[q].len);
          }
          deliver_context(~0ull);
          ring.flush();  // no batch mixes files
        }
      }
    }
    seg_start.clear();
    seg_end.clear();
    seg_file.clear();
    fill = 0;
  };
  for (unsigned int f = 0; f < n_files; f++) {
    if (!healthy) {  // a device error ended the packs: the rest is not scanned
      summaries[f].rc = HYPERSCANNER_SCAN;
      if (fvs) fvs->none(f);
      continue;
    }
    Reader in;
    if (!file_names[f] || !in.open(file_names[f])) {
      if (fvs) flush_pack();  // (its callback comes in its place in the order)
      summaries[f].rc = HYPERSCANNER_GZ_OPEN;
      if (fvs) fvs->none(f);
      continue;
    }
    const size_t size = in.size_hint();
    struct stat st;
    const bool empty_regular = !in.compressed() && !size && ::stat(file_names[f], &st) == 0 && S_ISREG(st.st_mode) && st.st_size == 0;
    if (buffer_size < 2 || in.compressed() || (!size && !empty_regular) || size + 2 > cap) {  // the per-file route, in its place in the order
      flush_pack();
      // scan_file takes a context of its own from the bounded pool: this call's goes back first (a call that held one while
      // it waited for a second could wait for ever: HYPERGREP_POOL=1, or as many concurrent calls as the pool holds)
      if (ctx) {
        checkin(ctx, healthy);
        ctx = nullptr;
      }
      if (healthy) single(f);
      else {
        summaries[f].rc = HYPERSCANNER_SCAN;
        if (fvs) fvs->none(f);
      }
      continue;
    }
    if (fill + size + 2 > cap || (fcs && (seg_file.size() + 1) * n_bins > HG_COUNTS_MAX_CELLS)) flush_pack();
    if (!healthy) {
      summaries[f].rc = HYPERSCANNER_SCAN;
      if (fvs) fvs->none(f);
      continue;
    }
    if (!ctx) {
      ctx = checkout(db, &err);
      if (!ctx || hipSetDevice(ctx->device) != hipSuccess || !ensure_buffers(ctx, cap, 1)) {
        std::fprintf(stderr, "ERROR: Unable to allocate scratch space. Exiting. (%s)\n", err.c_str());
        if (ctx) healthy = false;
        for (unsigned int g = f; g < n_files; g++) {
          summaries[g].rc = HYPERSCANNER_SCRATCH;
          if (fvs) fvs->none(g);
        }
        return 0;
      }
    }
    uint8_t *buf = ctx->h_slot[0];
    size_t got = 0;
    while (got < size) {  // (the size seen at open: a file that grows meanwhile is read up to it)
      const long r = in.read(buf + fill + got, size - got);
      if (r <= 0) break;
      got += static_cast<size_t>(r);
    }
    seg_start.push_back(fill);
    seg_end.push_back(fill + got);
    seg_file.push_back(f);
    fill += got;
    if (got && buf[fill - 1] != '\n') {  // the pad behind an unterminated file
      buf[fill++] = 0;
      buf[fill++] = '\n';
    }
  }
  if (healthy) flush_pack();
  return 0;
}

extern "C" int hg_hyperscan_files(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                  const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event,
                                  void *context, const int buffer_size, int buffer_count, unsigned long long max_match_count, int invert,
                                  hg_file_summary_t *summaries) {
  return files_impl(file_names, n_files, patterns, pattern_flags, pattern_ids, ext, elements, on_event, context, buffer_size, buffer_count, max_match_count, invert, summaries, 0, 0);
}

extern "C" int hg_hyperscan_files_context(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                          const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event,
                                          void *context, const int buffer_size, int buffer_count, unsigned long long max_match_count, int invert,
                                          hg_file_summary_t *summaries, unsigned int before, unsigned int after) {
  // an expression with one of the context ids could not be told from a context line by the callback
  for (unsigned int i = 0; on_event && pattern_ids && i < elements; i++)
    if (pattern_ids[i] >= HG_CTX_ID_TAIL) return HYPERSCANNER_DB;
  return files_impl(file_names, n_files, patterns, pattern_flags, pattern_ids, ext, elements, on_event, context, buffer_size, buffer_count, max_match_count, invert, summaries, before,
                    after);
}

extern "C" int hg_hyperscan_files_parts(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                        const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event,
                                        void *context, const int buffer_size, int buffer_count, unsigned long long max_match_count,
                                        hg_file_summary_t *summaries) {
  return files_impl(file_names, n_files, patterns, pattern_flags, pattern_ids, ext, elements, on_event, context, buffer_size, buffer_count, max_match_count, 0, summaries, 0, 0, true);
}

extern "C" int hg_hyperscan_files_counts(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                         const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size,
                                         hg_file_summary_t *summaries, uint32_t *ids, unsigned int max_ids, unsigned int *n_ids, uint64_t *file_lines,
                                         uint64_t *file_reports) {
  if (!n_ids || (max_ids && (!ids || (n_files && (!file_lines || !file_reports))))) return HYPERSCANNER_STATE_MEM;
  const FilesCounts fcs{ids, max_ids, n_ids, file_lines, file_reports};
  return files_impl(file_names, n_files, patterns, pattern_flags, pattern_ids, ext, elements, nullptr, nullptr, buffer_size, 1, 0, 0, summaries, 0, 0, false, &fcs);
}

extern "C" int hg_hyperscan_files_values(const char *const *file_names, unsigned int n_files, const char *const *patterns, const unsigned int *pattern_flags,
                                         const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size,
                                         const hg_rank_params_t *params, hg_file_values_event on_file, void *context, hg_file_summary_t *summaries) {
  if (!on_file) return HYPERSCANNER_STATE_MEM;
  FilesValues fvs{params ? *params : hg_rank_params_t{0, 0, 0, 0, 0}, on_file, context};
  if ((fvs.params.flags & ~HG_RANK_BY_PATTERN) || fvs.params.hash_bits > 64 || fvs.params.table_log2 > HG_VALUES_MAX_TABLE_LOG2) return HYPERSCANNER_STATE_MEM;
  return files_impl(file_names, n_files, patterns, pattern_flags, pattern_ids, ext, elements, nullptr, nullptr, buffer_size, 1, 0, 0, summaries, 0, 0, true, nullptr, &fvs);
}

extern "C" int hg_hyperscan_counts(char *file_name, const char *const *patterns, const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                                   const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size, hg_id_count_t *counts,
                                   unsigned int max_counts, unsigned int *n_counts, uint64_t *n_lines) {
  if (!n_counts || (max_counts && !counts)) return HYPERSCANNER_STATE_MEM;
  *n_counts = 0;
  if (n_lines) *n_lines = 0;
  FileCounts fc;
  uint64_t pieces = 0;
  const int rc = scan_file(file_name, patterns, pattern_flags, pattern_ids, ext, elements, [](hyperscanner_result_t *, int) {}, buffer_size, 1, 0, false, 0, 0, &pieces, false, &fc);
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
  if ((fv.params.flags & ~HG_VALUES_BY_PATTERN) || fv.params.hash_bits > 64 || fv.params.table_log2 > HG_VALUES_MAX_TABLE_LOG2) return HYPERSCANNER_STATE_MEM;
  const int rc = scan_file(file_name, patterns, pattern_flags, pattern_ids, ext, elements, [](hyperscanner_result_t *, int) {}, buffer_size, 1, 0, false, 0, 0, nullptr, true, nullptr, &fv);
  if (rc) return rc;
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off(1, 0);
  for (const std::string &v : fv.value) {
    bytes.insert(bytes.end(), v.begin(), v.end());
    off.push_back(bytes.size());
  }
  on_values(context, bytes.data(), off.data(), fv.count.data(), fv.pattern.data(), fv.value.size());
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
  if ((fv.params.flags & ~HG_VALUES_BY_PATTERN) || fv.params.hash_bits > 64 || fv.params.table_log2 > HG_VALUES_MAX_TABLE_LOG2) return HYPERSCANNER_STATE_MEM;
  const int rc = scan_file(file_name, patterns, pattern_flags, pattern_ids, ext, elements, [](hyperscanner_result_t *, int) {}, buffer_size, 1, 0, false, 0, 0, nullptr, true, nullptr, &fv);
  if (rc) return rc;
  if (fv.top_off.empty()) fv.top_off.assign(1, 0);
  if (n_distinct) *n_distinct = fv.n_distinct;
  if (n_parts) *n_parts = fv.n_parts;
  on_values(context, fv.top_bytes.data(), fv.top_off.data(), fv.count.data(), fv.pattern.data(), fv.count.size());
  return 0;
}

extern "C" int hg_hyperscan_ext(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                             const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hs_event on_event,
                             const int buffer_size, int buffer_count, unsigned long long max_match_count) {
  return scan_file(file_name, patterns, pattern_flags, pattern_ids, ext, elements, on_event, buffer_size, buffer_count, max_match_count, false);
}

extern "C" int hg_hyperscan_invert(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                                   const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hs_event on_event,
                                   const int buffer_size, int buffer_count, unsigned long long max_match_count) {
  return scan_file(file_name, patterns, pattern_flags, pattern_ids, ext, elements, on_event, buffer_size, buffer_count, max_match_count, true);
}

extern "C" int hg_hyperscan_parts(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                                  const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hs_event on_event,
                                  const int buffer_size, int buffer_count, unsigned long long max_match_count) {
  return scan_file(file_name, patterns, pattern_flags, pattern_ids, ext, elements, on_event, buffer_size, buffer_count, max_match_count, false, 0, 0, nullptr, true);
}

extern "C" int hg_hyperscan_context(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                                    const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements, hs_event on_event,
                                    const int buffer_size, int buffer_count, unsigned long long max_match_count, unsigned int before, unsigned int after,
                                    int invert) {
  // an expression with one of the context ids could not be told from a context line by the callback
  for (unsigned int i = 0; pattern_ids && i < elements; i++)
    if (pattern_ids[i] >= HG_CTX_ID_TAIL) return HYPERSCANNER_DB;
  return scan_file(file_name, patterns, pattern_flags, pattern_ids, ext, elements, on_event, buffer_size, buffer_count, max_match_count, invert != 0, before, after);
}
