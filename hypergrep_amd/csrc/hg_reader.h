// Face B's input (hg_shim.hip): a file read as plain, gzip or zstd bytes, and the reader thread that fills the caller's slots
// with it, cut at line-piece boundaries.  Host only, no HIP: the slots are whatever memory the caller hands in (pinned, in
// the product).
#pragma once
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

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
  std::mutex mu;  // (of load)
  bool load() {
    std::lock_guard<std::mutex> lock(mu);
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
inline Zstd g_zstd;

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

// ---------------------------------------------------------------- the reader thread
// Where a filled slot that is not the stream's end is cut, so that every piece is scanned whole: behind the last newline;
// without one (one unterminated line) at a forced break, the largest multiple of bs1 = buffer_size - 1; else everything.
inline size_t hg_chunk_cut(const uint8_t *buf, size_t have, uint64_t bs1) {
  size_t cut;
  if (const void *nl = memrchr(buf, '\n', have)) cut = static_cast<size_t>(static_cast<const uint8_t *>(nl) - buf) + 1;
  else cut = static_cast<size_t>((have / bs1) * bs1);
  return cut ? cut : have;
}

inline double hg_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// A thread that fills the caller's `nslots` buffers of `cap` bytes in turn, chunk k into slot k % nslots, each cut by
// hg_chunk_cut; the bytes behind the cut open the next slot.  The consumer waits for chunk k, works on it, and gives the slot
// back; the thread ends at the end of the stream (a read error ends it like gzgets returning NULL) or at stop().
class SlotReader {
 public:
  static constexpr int kMaxSlots = 3;
  struct Chunk {
    const uint8_t *bytes;
    size_t cut;        // bytes to scan (whole pieces)
    bool last;         // nothing follows
    bool next_filled;  // chunk k + 1 already waits in its slot
  };
  SlotReader(Reader &in, uint8_t *const *bufs, int nslots, size_t cap, uint64_t bs1) : in_(in), nslots_(nslots), cap_(cap), bs1_(bs1) {
    for (int i = 0; i < nslots; i++) bufs_[i] = bufs[i];
    thread_ = std::thread([this] { run(); });
  }
  ~SlotReader() { stop(); }
  // Wait for chunk k.
  Chunk wait(unsigned k) {
    const Slot &s = slots_[k % nslots_];
    const double t0 = hg_now();
    std::unique_lock<std::mutex> lock(mu_);
    cv_.wait(lock, [&] { return s.state == 1; });
    t_wait += hg_now() - t0;
    return Chunk{bufs_[k % nslots_], s.cut, s.last, nslots_ > 1 && !s.last && slots_[(k + 1) % nslots_].state == 1};
  }
  size_t cut_of(unsigned k) const { return slots_[k % nslots_].cut; }  // (of a chunk the consumer holds or was told is filled)
  // Chunk k's slot goes back to the reader.
  void release(unsigned k) {
    {
      std::lock_guard<std::mutex> lock(mu_);
      slots_[k % nslots_].state = 0;
    }
    cv_.notify_all();
  }
  // The consumer stopped early (match limit, error), or is done: the thread ends and is joined.
  void stop() {
    if (!thread_.joinable()) return;
    {
      std::lock_guard<std::mutex> lock(mu_);
      abandon_ = true;
    }
    cv_.notify_all();
    thread_.join();
  }
  double t_read = 0;  // seconds the thread spent filling slots (read after stop())
  double t_wait = 0;  // seconds the consumer waited for data

 private:
  struct Slot {
    size_t cut = 0;
    bool last = false;
    int state = 0;  // 0 free (reader's), 1 ready (consumer's)
  };
  void run() {
    std::vector<uint8_t> carry;  // bytes after the cut, they open the next slot
    bool eof = false;
    for (unsigned k = 0;; k++) {
      Slot &s = slots_[k % nslots_];
      uint8_t *buf = bufs_[k % nslots_];
      {
        std::unique_lock<std::mutex> lock(mu_);
        cv_.wait(lock, [&] { return s.state == 0 || abandon_; });
        if (abandon_) return;
      }
      size_t have = carry.size();
      if (have) std::memcpy(buf, carry.data(), have);
      carry.clear();
      const double t_fill = hg_now();
      while (!eof && have < cap_) {
        const long got = in_.read(buf + have, cap_ - have);
        if (got <= 0) {
          eof = true;
          break;
        }
        have += static_cast<size_t>(got);
      }
      t_read += hg_now() - t_fill;
      size_t cut = have;
      if (!eof && have) {
        cut = hg_chunk_cut(buf, have, bs1_);
        carry.assign(buf + cut, buf + have);
      }
      {
        std::lock_guard<std::mutex> lock(mu_);
        s.cut = cut;
        s.last = eof && carry.empty();
        s.state = 1;
      }
      cv_.notify_all();
      if (eof && carry.empty()) return;
    }
  }
  Reader &in_;
  uint8_t *bufs_[kMaxSlots] = {nullptr, nullptr, nullptr};
  const int nslots_;
  const size_t cap_;
  const uint64_t bs1_;
  Slot slots_[kMaxSlots];
  std::mutex mu_;
  std::condition_variable cv_;
  bool abandon_ = false;
  std::thread thread_;
};
