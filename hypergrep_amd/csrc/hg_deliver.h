// Face B's delivery: how the records of a scanned chunk (hg_shim.hip's scan_file) or of one file of a pack (FilesRun::deliver_pack) become
// the batches of the result ring.  Host only, no HIP: the product calls it with the arrays it downloaded, the host tests
// (tests/native/deliversim.cpp) with arrays made in Python.
//
// The rules, once:
//   - results go out line by line; inside a line the reports go out by ascending end offset, then id (hs_scan order);
//   - with parts (grep -o) every part of the line goes out, in order, in place of its reports, with its expression's id;
//   - context records below a line go out in front of it, the rest behind the last line; tail records (the next chunk's
//     before-context, maybe) are set aside;
//   - the match limit counts reports, not parts and not context lines, and is checked after each line, as the reference checks
//     it after each line's hs_scan returns (hyperscanner.c:222-224).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../include/hypergrep_amd.h"
#include "hg_context.h"
#include "hg_parts.h"

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

// The records of one chunk, or of one file of a pack, on the host.  Every list is ordered by line; `base` is what the
// records' byte offsets count from (the chunk's pinned slot, the file's first byte in the pack's host copy).
struct HgChunkRecords {
  const uint8_t *base = nullptr;
  const HgHit *hits = nullptr;  // the reports, or the selected pieces of an inverted scan
  const HgHitAux *aux = nullptr;
  size_t n_hits = 0;
  const HgHit *ctx_hits = nullptr;  // context (and tail) records
  const HgHitAux *ctx_aux = nullptr;
  size_t n_ctx = 0;
  const HgPart *parts = nullptr;  // matched parts of the lines that have a report, with their expressions
  const uint32_t *part_pattern = nullptr;
  size_t n_parts = 0;
  const HgPattern *patterns = nullptr;  // (parts: the expressions, for their ids)
  uint64_t n_pieces = 0;                // the chunk's line pieces
  uint64_t owed_after = 0;              // HgContextOutput::owed_after
};
struct HgDeliverCursor {
  size_t i = 0, ci = 0, pi = 0;  // into the reports, the context records, the parts
};

// The reports [i, j) of one line.
inline void hg_deliver_reports(Ring &ring, const HgChunkRecords &r, size_t i, size_t j) {
  std::vector<size_t> order(j - i);
  for (size_t q = 0; q < order.size(); q++) order[q] = i + q;
  if (order.size() > 1)
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return r.hits[x].to != r.hits[y].to ? r.hits[x].to < r.hits[y].to : r.hits[x].id < r.hits[y].id; });
  for (size_t q : order) ring.push(r.hits[q].id, r.hits[q].line_no, r.base + r.aux[q].start, r.aux[q].len);
}
// The parts of the line of report i, in place of its reports.
inline void hg_deliver_parts(Ring &ring, const HgChunkRecords &r, size_t i, size_t *pi) {
  const uint64_t line = r.hits[i].line_no;
  while (*pi < r.n_parts && r.parts[*pi].line_no < line) ++*pi;
  for (; *pi < r.n_parts && r.parts[*pi].line_no == line; ++*pi) {
    const HgPart &p = r.parts[*pi];
    ring.push(r.patterns[r.part_pattern[*pi]].id, p.line_no, r.base + r.aux[i].start + p.from, p.to - p.from);
  }
}
// The context records below `upto`, in order; tail records are set aside in `tails` (nullptr: the list holds none).
inline void hg_deliver_context(Ring &ring, const HgChunkRecords &r, size_t *ci, uint64_t upto, std::vector<size_t> *tails) {
  for (; *ci < r.n_ctx && r.ctx_hits[*ci].line_no < upto; ++*ci) {
    if (tails && r.ctx_hits[*ci].id == HG_CTX_ID_TAIL) tails->push_back(*ci);
    else ring.push(HG_CTX_ID_CONTEXT, r.ctx_hits[*ci].line_no, r.base + r.ctx_aux[*ci].start, r.ctx_aux[*ci].len);
  }
}
// The line at the cursor with the context records in front of it; the cursor moves behind it.  Returns the line's reports.
inline size_t hg_deliver_line(Ring &ring, const HgChunkRecords &r, bool parts, HgDeliverCursor *c, std::vector<size_t> *tails) {
  const size_t i = c->i;
  hg_deliver_context(ring, r, &c->ci, r.hits[i].line_no, tails);
  size_t j = i;
  while (j < r.n_hits && r.hits[j].line_no == r.hits[i].line_no) j++;
  if (parts) hg_deliver_parts(ring, r, i, &c->pi);
  else hg_deliver_reports(ring, r, i, j);
  c->i = j;
  return j - i;
}
// A whole file whose limit and context were settled on the device (the packed route): every line, then the rest of the context.
inline void hg_deliver_file(Ring &ring, const HgChunkRecords &r, bool parts) {
  HgDeliverCursor c;
  while (c.i < r.n_hits) hg_deliver_line(ring, r, parts, &c, nullptr);
  hg_deliver_context(ring, r, &c.ci, ~0ull, nullptr);
}

// A file delivered chunk by chunk (scan_file).  Between chunks it carries what the device API's chaining identity needs: the
// after-context still owed (owed_after -> carry_after) and the bytes of the previous chunks' tail pieces, `before` at most.
// At the limit with after-context (GNU grep's -m with -A) the trailing context of the last delivered line still goes out: the
// pieces [trailing_next, trailing_end), up to the next matching piece, read from as many further chunks as they take.
class HgDelivery {
 public:
  HgDelivery(Ring &ring, bool parts, uint32_t before, uint32_t after, unsigned long long max_match_count)
      : ring_(ring), parts_(parts), before_(before), after_(after), max_match_count_(max_match_count) {}
  uint64_t line_base() const { return line_base_; }  // pieces scanned so far == reference line_number of the next chunk's first piece
  // What the next chunk's context stage is asked (after the limit: the owed pieces only, as carry; no new windows, no tail).
  HgContextParams context_params() const {
    if (trailing_) return HgContextParams{0u, 0u, trailing_end_ - trailing_next_, false};
    return HgContextParams{before_, after_, carry_after_, before_ != 0};
  }
  // Deliver the chunk's records.  True: the call stops here (the limit is reached and nothing is owed any more).
  bool chunk(const HgChunkRecords &r) {
    const bool with_context = before_ || after_;
    bool stop = false;
    HgDeliverCursor c;
    if (trailing_) {
      stop = deliver_trailing(r, &c.ci);
    } else {
      std::vector<size_t> tails;  // this chunk's tail records
      if (with_context && r.n_hits) {  // the held tail pieces within `before` of the chunk's first match
        for (const HeldPiece &hp : held_)
          if (hp.line_no + before_ >= r.hits[0].line_no) ring_.push(HG_CTX_ID_CONTEXT, hp.line_no, reinterpret_cast<const uint8_t *>(hp.bytes.data()), static_cast<uint32_t>(hp.bytes.size()));
        held_.clear();
      }
      while (c.i < r.n_hits && !stop && !trailing_) {
        const uint64_t line = r.hits[c.i].line_no;
        matches_ += hg_deliver_line(ring_, r, parts_, &c, &tails);
        if (max_match_count_ > 0 && matches_ >= max_match_count_) {
          stop = true;
          if (after_) {
            trailing_ = true;
            trailing_next_ = line + 1;
            trailing_end_ = hg_sat_add(trailing_next_, after_);
            stop = deliver_trailing(r, &c.ci);  // false: the chunk ended first, the next one is read for what is still owed
          }
        }
      }
      if (with_context && !trailing_ && !stop) {  // (a call that ends at the limit delivers nothing behind its last line but that line's after-context)
        hg_deliver_context(ring_, r, &c.ci, ~0ull, &tails);
        // the tail pieces' bytes are copied: the chunk's bytes are gone when the next chunk needs them
        for (size_t t : tails) held_.push_back(HeldPiece{r.ctx_hits[t].line_no, std::string(reinterpret_cast<const char *>(r.base) + r.ctx_aux[t].start, r.ctx_aux[t].len)});
        while (held_.size() > before_) held_.pop_front();
        carry_after_ = r.owed_after;
      }
    }
    line_base_ += r.n_pieces;
    return stop;
  }

 private:
  // The owed after-context of the last delivered line: consecutive pieces, ending before the next matching piece (which is no
  // context record) or when all are out.  True when nothing is owed any more.
  bool deliver_trailing(const HgChunkRecords &r, size_t *ci) {
    while (*ci < r.n_ctx && r.ctx_hits[*ci].line_no < trailing_next_) ++*ci;
    while (trailing_next_ < trailing_end_ && *ci < r.n_ctx && r.ctx_hits[*ci].line_no == trailing_next_ && r.ctx_hits[*ci].id == HG_CTX_ID_CONTEXT) {
      ring_.push(HG_CTX_ID_CONTEXT, trailing_next_, r.base + r.ctx_aux[*ci].start, r.ctx_aux[*ci].len);
      ++*ci;
      trailing_next_++;
    }
    if (trailing_next_ < line_base_ + r.n_pieces) trailing_end_ = trailing_next_;  // stopped inside the chunk: nothing is owed any more
    return trailing_next_ >= trailing_end_;
  }
  struct HeldPiece {
    uint64_t line_no;
    std::string bytes;
  };
  Ring &ring_;
  const bool parts_;
  const uint32_t before_, after_;
  const unsigned long long max_match_count_;
  uint64_t line_base_ = 0;
  unsigned long long matches_ = 0;  // match results delivered (max_match_count counts those, not the context lines)
  bool trailing_ = false;           // the limit is reached: only the last delivered line's after-context still goes out
  uint64_t trailing_next_ = 0, trailing_end_ = 0;
  uint64_t carry_after_ = 0;     // after-context the chunks so far still owe
  std::deque<HeldPiece> held_;  // tail pieces of the chunks so far: the next match's before-context, maybe (`before` at most)
};
