// Device-side scanner object: uploaded database + workspace + the launch sequence of the scan path.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/hypergrep_amd.h"
#include "hg_compile.h"
#include "hg_core.h"
#include "hg_invert.h"
#include "hg_context.h"
#include "hg_segments.h"
#include "hg_segctx.h"
#include "hg_parts.h"
#include "hg_segparts.h"
#include "hg_gather.h"
#include "hg_partlines.h"
#include "hg_rank.h"
#include "hg_values.h"
#include "hg_valstore.h"
#include "hg_counts.h"
#include "hg_mem.h"
#include "hg_post.h"

// Waves per stream workgroup (one 16 KiB tile per wave at a time); shared by the kernel and the grid sizing.
#ifndef HG_STREAM_WG_WAVES
#define HG_STREAM_WG_WAVES 8
#endif
constexpr uint32_t HG_STREAM_WG_WAVES_DEFAULT = HG_STREAM_WG_WAVES;

// device counters: totals, and the largest per-segment demand seen when a private segment overflowed
constexpr uint32_t HG_CONFIRM_SPLIT = 4;   // verify blocks per candidate segment
constexpr uint32_t HG_DEFER_SHARDS = 64;   // append-only lists of verified candidates that need an automaton run

// A verified literal occurrence whose expression still needs its automaton: pattern may match in the line holding pos.
struct HgDeferred {
  uint64_t pos;       // the window's text offset (locates the tile and the line)
  uint32_t pattern;   // pattern index | offset of the window inside the literal << 24
  uint32_t rank;      // newlines between the tile start and pos
};
// The scanner's small device state is ONE block of words (reset by one launch, read back by one copy):
//   [0, 8) counters, [16] reports the match-length pass kept, [24, 28) finalize totals {kept, raw, large buckets, -}, [28, 30) {count, overflow flag}
//   of the finalize, [32, 36) tile-scan state (HgTileBase), [64, 128) tile cursors: one per pipeline chunk (a cursor of its own
//   for each of the 64 chunks a pass may have, all zeroed by hg_reset_kernel: no chunk ever waits for, or races with, the
//   reset of a cursor an earlier chunk has used)
enum { HG_ST_MINLEN_KEPT = 16, HG_ST_FIN_TOTAL = 24, HG_ST_SELECTED = 28, HG_ST_FINAL = 32, HG_ST_WORDS = 36, HG_ST_ZERO_WORDS = 32,
       HG_ST_BLOCK_DONE = 40 };  // (outside the words a pass resets: workgroups of hg_block_small_kernel that have finished)
enum { HG_CNT_CANDS = 0, HG_CNT_HITS = 1, HG_CNT_CAND_NEED = 2, HG_CNT_HIT_NEED = 3, HG_CNT_DEFER_NEED = 4,
       HG_CNT_HITS_WRAPPED = 5,  // the 32-bit hit counter went round (direct appends): the buffer is scanned in segments instead
       HG_CNT_JOIN_TILES = 6,  // tiles taken by the joiner launches of the pass (hg_stream_join_kernel)
       HG_CNT_WORDS = 8,
       HG_CNT_CURSOR0 = 64,     // one tile cursor per pipeline chunk (HgScanner::kMaxChunks = 64 of them)
       HG_CNT_CURSORS = 64,
       HG_ST_ALLOC_WORDS = 128 };
constexpr uint32_t HG_STREAM_GRAB = 2 * HG_STREAM_WG_WAVES_DEFAULT;  // tiles per draw of a stream workgroup: two per wave

// Bucketed finalize (hg_fin_*): buckets of the final ordering and the largest bucket one wave sorts in LDS.
constexpr uint32_t HG_FIN_MAX_BUCKETS = 1u << 22;  // (a pass holds at most 2^28 reports: 64 per bucket then, what one wave orders)
constexpr uint32_t HG_FIN_BUCKET_CAP = 4096;
constexpr uint32_t HG_FIN_MEDIUM_CAP = 512;  // size class of hg_fin_sort_big_kernel that needs little LDS

// Threads of a confirm block: its LDS (the per-lane follow tables of the one-word automata, 128 B per lane) decides how many
// fit on a CU next to the stream pass.
#ifndef HG_CONFIRM_THREADS
#define HG_CONFIRM_THREADS 128
#endif



struct HgStreamArgs {
  const uint8_t *text;
  uint64_t nbytes, tile_begin, tile_end;  // the launch covers tiles [tile_begin, tile_end) of the text
  HgDbView db;
  const uint32_t *filter;  // 1 << filter_log2 window-hash slots (single probe, dword-aligned windows: HgDb::filter_ctx)
  const HgSlotInfo *ext;   // per slot: window values + neighbour-dword conditions (with filter_ctx: HgDb::filter's words behind them)
  HgTileSum *sums;
  HgCand *cands;         // nsegs x cand_seg_cap: one private segment per stream workgroup
  uint32_t *seg_count;   // candidates in each segment
  uint32_t cand_seg_cap, filter_log2;
  uint32_t weights_a, weights_b;
  uint32_t filter_wide;
  uint32_t dense;  // byte-aligned probing (HgDb::dense)
  uint32_t ctx;    // the filter holds HgDb::filter_ctx and `ext` has HgDb::filter's 1 << filter_log2 words behind its 1 << filter_log2
                   // conditions (HgDb::filter_use_ctx): the kernels that test the byte after a window
  uint32_t weights_c;  // hash C weights (HgDb::weights_c)
  uint32_t alone;  // no other kernel runs next to this launch (every workgroup slot is its own)
  uint32_t cursor_slot;  // counters[cursor_slot] = tiles of the chunk handed out so far (hg_stream_kernel draws runs of HG_STREAM_GRAB tiles)
  uint32_t *counters;
};

struct HgConfirmArgs {
  const uint8_t *text;
  uint64_t nbytes, tile_begin, tile_end, bs1;
  HgDbView db;
  const HgTileSum *sums;
  const HgTileBase *bases;
  const HgCand *cands;
  const uint32_t *seg_count;
  HgHit *hits;  // compact outputs
  HgHitAux *aux;
  HgHit *tmp_hits;  // gridDim x hit_seg_cap block-private staging
  HgHitAux *tmp_aux;
  HgDeferred *deferred;   // one list per (confirm mode present in the database, shard): list_of_mode[m] * HG_DEFER_SHARDS + shard, each defer_shard_cap entries
  uint32_t *defer_count;  // entries appended to each list, indexed mode * HG_DEFER_SHARDS + shard
  uint32_t list_of_mode[HG_CONFIRM_MODES];
  uint32_t mode_present[HG_CONFIRM_MODES];
  uint32_t *always_count;                 // matches noted per block (reuses the chunk's candidate segment counts)
  uint32_t always_list_cap;               // entries per block of the always-on match list (it reuses `deferred`)
  uint32_t list_spread[HG_CONFIRM_MODES];  // automaton modes: lists per pattern (few patterns: each is spread over several lists)
  uint32_t cand_seg_cap, hit_cap, hit_seg_cap, defer_shard_cap;
  // Candidate segments [0, join_seg0) belong to the chunk's stream launch and hold cand_seg_cap records each; the segments from
  // join_seg0 on belong to the joiner launch and hold join_seg_cap (a quarter: the joiner streams a few per cent of a chunk)
  uint32_t join_seg0, join_seg_cap;
  uint32_t hit_direct;  // 1: a block whose staging segment is full appends to the compact array itself (HitSink)
  // Bucketed emission (the default, bucket_cap != 0): a hit goes straight into the region of the bucket its line starts in
  // (bucket = aux.start >> bucket_shift, bucket_cap records each, bucket_fill = records so far); the finalize kernels
  // (hg_fin_*) then sort every bucket on its own.  bucket_cap == 0: the compact array + library sort (HitSink, flush_hits).
  uint32_t bucket_shift, bucket_cap;
  uint32_t *bucket_fill;
  uint32_t *counters;
  // A pass reports the pieces whose first scanned byte lies in [own_lo, own_hi): the whole buffer normally; one segment of it
  // when the buffer is scanned in several passes (HgScanner::scan_segments).  Buckets count from own_lo.
  uint64_t own_lo, own_hi;
};
constexpr uint32_t HG_BLOCK_SMALL_POOL = 10240;  // ... words of automaton tables a workgroup of that path stages in LDS (40 KiB)
constexpr uint32_t HG_BLOCK_SLICED_MAX = 2047;   // ... blocks up to this many bytes are split over the lanes by start position
constexpr uint32_t HG_BLOCK_SLICED_WORDS = 64;   // ... (bitmap of emitted ends per expression: ends 0 .. HG_BLOCK_SLICED_MAX)
constexpr uint32_t HG_BLOCK_SMALL_MAX = 8192;   // Face A: blocks up to this many bytes take the one-launch path (hg_block_small_kernel)
constexpr uint32_t HG_BLOCK_SMALL_SEG = 1024;   // ... reports per workgroup (32 or 256 expressions) it can hold
// The grouping of the short-block paths (hg_block_small_kernel, hg_block_batch_kernel): 32 expressions per workgroup while 64
// groups hold the set (their tables then usually fit in LDS), else 256; returns the number of groups.
inline uint32_t hg_block_small_grouping(uint32_t npatterns, uint32_t *ppw) {
  *ppw = npatterns <= 32u * 64u ? 32u : 256u;
  return (npatterns + *ppw - 1) / *ppw;
}
constexpr uint32_t HG_HIT_REL_SHIFT = 40;  // raw bucketed records: line_no (< 2^40) | line start inside the bucket (< 2^24) << 40
constexpr uint32_t HG_HIT_SINGLE_BIT = 0x80000000u;  // raw bucketed records: bit 31 of `to` = the expression has HS_FLAG_SINGLEMATCH (`to` < 2^31)

struct HgScanOutput {
  uint64_t n_hits;       // final (ordered, de-duplicated) hits
  uint64_t n_pieces;     // line pieces in the buffer (the reference's final line_number)
  uint64_t n_cands;      // verified required-literal occurrences
  uint64_t n_raw_hits;   // reports before de-duplication (and before the min_length filter)
  const HgHit *d_hits;   // device arrays, valid until the next scan on this scanner
  const HgHitAux *d_aux;
  float ms_stream;       // hg_stream_kernel alone (HIP events on the launch stream)
  float ms_total;        // whole launch sequence
  uint32_t reruns;       // workspace grew and the pass was repeated this many times
  uint32_t stream_launches;  // hg_stream_kernel launches of the (last) pass: one per pipeline chunk
  uint32_t joiner_launches;  // ... and hg_stream_join_kernel launches
  uint64_t joiner_tiles;     // tiles (of 16 KiB) the joiner launches took: bytes the hg_stream_kernel launches did NOT stream
  const uint32_t *d_from;    // databases with HS_FLAG_SOM_LEFTMOST expressions: the start of each hit (hg_som.hip), else nullptr
  float ms_invert;           // inverted scans: the invert stage (count, scan, the host sync that sizes the output, write); the fields above stay the underlying scan's
};

// The start-of-match pass (hg_som.hip): from[i] for the n final hits, on `stream`.  max_nw: the most state words of any SOM
// expression (its multi-word walks keep their state in LDS).
// min_lengths: HgDb::min_lengths on the device or nullptr (expressions sharing a SOM id count only where their own report survives).
hipError_t hg_som_launch(const uint8_t *text, const HgHit *hits, const HgHitAux *aux, uint64_t n, const HgPattern *patterns, const uint32_t *pool, uint32_t max_nw,
                         const uint32_t *min_lengths, uint32_t *from, hipStream_t stream);
// The match-length pass (hg_som.hip, hs_expr_ext_t min_length): of the n raw reports of a pass, those whose expression has no
// filtering min_length or a match of at least that length ending at `to` are appended to out_* (room for n), *count (zero
// before the launch) receives their number.  max_nw: the most state words of any filtering expression.
hipError_t hg_minlen_launch(const uint8_t *text, const HgHit *hits, const HgHitAux *aux, uint32_t n, const HgPattern *patterns, const uint32_t *pool, uint32_t max_nw,
                            const uint32_t *min_lengths, HgHit *out_hits, HgHitAux *out_aux, uint32_t *count, hipStream_t stream);

// The combination pass (hg_comb.hip) over the n final hits of a pass: count (emit == false: count[i] = records of hit i,
// count[n] = 0), or write the records of hit i to out_*[pos[i] ..] (emit == true), on `stream`.
struct HgCombArgs {
  const HgHit *hits;
  const HgHitAux *aux;
  uint64_t n;
  const HgPattern *patterns;
  const HgComb *combs;
  const uint32_t *words;
  const uint32_t *feed;
  uint32_t nfeed;
  uint32_t *count;
  const uint64_t *pos;
  HgHit *out_hits;
  HgHitAux *out_aux;
};
hipError_t hg_comb_launch(const HgCombArgs &a, bool emit, hipStream_t stream);

// The invert stage (hg_invert.hip) over the ntiles tiles of a scanned buffer: the count pass (write == false) or the write
// pass, on `stream`, in a grid sized for num_cus compute units.
hipError_t hg_invert_launch(const HgInvertArgs &a, bool write, uint32_t num_cus, hipStream_t stream);

// The context stage (hg_context.hip), launched like the invert stage.
hipError_t hg_context_launch(const HgContextArgs &a, bool write, uint32_t num_cus, hipStream_t stream);
// What a call asks of it is HgContextParams (hg_context.h); what it leaves (hg_context_result_t of the C ABI):
struct HgContextOutput {
  uint64_t n_context;  // context and tail records, ordered by line
  uint64_t n_tail;     // the tail records among them
  uint64_t owed_after; // after-context owed past the buffer's end (hg_context_owed)
  const HgHit *d_hits; // device arrays, valid until the next scan on this scanner
  const HgHitAux *d_aux;
  float ms_context;    // the stage: count, scan, the host sync that sizes the output, write
};

// The segment stage (hg_segments.hip), one step per launch on `stream`: the argument check (before the scan), the segments'
// line bases (a wave per tile), the segments' runs of surviving records, and the ordered write of those runs.
enum class HgSegStep { Check, PadFlag, PadWrite, Bases, Runs, Write };
hipError_t hg_segments_launch(const HgSegArgs &a, HgSegStep step, uint32_t num_cus, hipStream_t stream);
// What a call asks of it (hg_segments_t of the C ABI) and what it leaves (hg_segment_result_t).
struct HgSegParams {
  const uint64_t *d_seg_start, *d_seg_end;
  uint32_t n_seg;
  uint64_t max_per_segment;
};
struct HgSegOutput {
  const uint32_t *d_record_segment;  // device arrays, valid until the next scan on this scanner
  const uint64_t *d_first_record, *d_n_lines, *d_n_selected;
  float ms_segments;  // the stage: check, bases, runs, scan, the host syncs, write
};

// The per-file context stage (hg_segctx.hip) behind the segment stage, one step per launch on `stream`: the surviving records
// in packed piece numbers with their segments' windows, the per-tile counts, the ordered write, the file-relative form of the
// records, and the per-segment offsets.
enum class HgSegCtxStep { Prep, Count, Write, Map, First };
hipError_t hg_segctx_launch(const HgSegCtxArgs &a, HgSegCtxStep step, uint32_t num_cus, hipStream_t stream);
// What it leaves beside HgContextOutput (hg_copy_segment_context of the C ABI).
struct HgSegCtxOutput {
  const uint32_t *d_context_segment;  // device arrays, valid until the next scan on this scanner: the segment of each context record
  const uint64_t *d_first_context;    // n_seg + 1: segment s owns the context records [first_context[s], first_context[s + 1])
};

// The parts stage (hg_parts.hip) over the n_hits final hits of a scan, on `stream`: count (write == false: count[i] = parts of
// the piece whose first hit is hit i, 0 for its other hits, count[n_hits] = 0), or write the parts of that piece to
// out / out_pattern [pos[i] ..].  max_nw: the most state words of any expression (multi-word walks keep their state in LDS).
struct HgPartsArgs {
  const uint8_t *text;
  const HgHit *hits;
  const HgHitAux *aux;
  uint64_t n_hits;
  const HgPattern *patterns;
  const uint32_t *pool;
  uint32_t npatterns;
  const uint32_t *first;  // first[c * first_words + (j >> 5)] bit (j & 31): expression j has a node that init enters on byte c
  uint32_t first_words;   // ceil(npatterns / 32)
  uint64_t *count;
  const uint64_t *pos;
  HgPart *out;
  uint32_t *out_pattern;
};
hipError_t hg_parts_launch(const HgPartsArgs &a, bool write, uint32_t max_nw, uint32_t num_cus, hipStream_t stream);
// What the stage leaves (hg_parts_result_t of the C ABI).
struct HgPartsOutput {
  uint64_t n_parts;           // ordered by (line, from)
  const HgPart *d_parts;      // device arrays, valid until the next scan on this scanner
  const uint32_t *d_pattern;  // the expression index of each part
  float ms_parts;             // the stage: count, scan, the host sync that sizes the output, write
};

// The per-file parts stage (hg_segparts.hip) behind the segment stage, one step per launch on `stream`: the count pass over the
// surviving records, the write pass, and the per-segment offsets.  max_nw as for hg_parts_launch.
enum class HgSegPartsStep { Count, Write, First };
hipError_t hg_segparts_launch(const HgSegPartsArgs &a, HgSegPartsStep step, uint32_t max_nw, uint32_t num_cus, hipStream_t stream);
// What it leaves beside HgPartsOutput (hg_copy_segment_parts of the C ABI).
struct HgSegPartsOutput {
  const uint32_t *d_part_segment;  // device arrays, valid until the next scan on this scanner: the segment of each part
  const uint64_t *d_first_part;    // n_seg + 1: segment s owns the parts [first_part[s], first_part[s + 1])
};

// The gather stage (hg_gather.hip) over the records a scan left, one step per launch on `stream`: the head flags, the entries
// (index, fields, size), the per-segment offsets, the first entry of every output span of HG_GATHER_TILE bytes, and the copy pass
// over those spans.
enum class HgGatherStep { Flag, Entry, First, Span, Copy };
hipError_t hg_gather_launch(const HgGatherArgs &a, HgGatherStep step, hipStream_t stream);
// What a gather works on (the last scan's lists, as hg_capi.hip remembers them) and what it leaves (hg_lines_result_t).
struct HgGatherInput {
  const uint8_t *text;
  HgGatherList main, ctx;  // ctx.n == 0: no context list, or not asked for
  const uint64_t *seg_start, *first_record, *first_context;  // nullptr without segments (first_context: without a per-file context list)
  uint64_t n_seg;
  uint32_t flags;
};
struct HgGatherOutput {
  uint64_t n_entries, n_bytes;
  const uint8_t *d_bytes;  // device arrays, valid until the next gather on this object
  const uint64_t *d_entry_off, *d_line_number;
  const uint32_t *d_kind, *d_segment;
  const uint64_t *d_first_entry;
  float ms_gather;  // the stage: flags, scan, entries, scan, the host sync that sizes the output, spans, copy
};
// The stage's buffers and launch sequence.  It owns its scratch (hgmem::Buf: freed with the object, every allocation logged)
// and touches nothing of the scanner's.
class HgGather {
 public:
  explicit HgGather(int device) : device_(device) {}
  ~HgGather();
  int run(const HgGatherInput &in, hipStream_t stream, HgGatherOutput *out, std::string *err);

 private:
  template <typename T>
  using DevBuf = hgmem::Buf<T, hgmem::Space::Dev>;
  int device_;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  DevBuf<uint64_t> head_{"gather head", 0}, F_{"gather F", 0}, size_{"gather size", 0}, off_{"gather off", 0}, line_{"gather line", 0}, first_{"gather first", 0},
      span_{"gather span", 0};
  DevBuf<uint32_t> kind_{"gather kind", 0}, seg_{"gather seg", 0};
  DevBuf<HgGatherEntry> entries_{"gather entries", 0};
  DevBuf<uint8_t> temp_{"gather temp", 0}, bytes_{"gather bytes", 16};
  hgmem::Buf<uint64_t, hgmem::Space::Host> totals_{"gather totals", 0};  // pinned: {entries, bytes}
};

// The parts gather (hg_partlines.hip) over the parts a scan left, one step per launch on `stream`: the entries (fields, size,
// per-entry arrays), the first entry of every output span of HG_GATHER_TILE bytes, and the copy pass over those spans.
enum class HgPartLinesStep { Entry, Span, Copy };
hipError_t hg_partlines_launch(const HgPartLinesArgs &a, HgPartLinesStep step, hipStream_t stream);
// What a parts gather works on (the last scan's records and parts, as hg_capi.hip remembers them) and what it leaves
// (hg_part_lines_result_t).
struct HgPartLinesInput {
  const uint8_t *text;
  HgGatherList recs;
  const HgPart *parts;
  const uint32_t *part_pattern, *part_seg;  // part_seg nullptr without segments
  uint64_t n_parts;
  const uint64_t *seg_start, *first_part;   // nullptr without segments
  uint64_t n_seg;
  uint32_t flags;
  uint64_t byte_base;
  HgPartLinesMarks marks;
};
struct HgPartLinesOutput {
  uint64_t n_entries, n_bytes;
  const uint8_t *d_bytes;  // device arrays, valid until the next parts gather on this object
  const uint64_t *d_entry_off, *d_line_number;
  const uint32_t *d_kind, *d_pattern, *d_segment;
  const uint64_t *d_first_entry;
  float ms_gather;  // the stage: entries, scan, the host sync that sizes the output, spans, copy
};
// The stage's buffers and launch sequence.  It owns its scratch (hgmem::Buf: freed with the object, every allocation logged)
// and touches nothing of the scanner's, of HgGather's or of HgCounts'.
class HgPartLines {
 public:
  explicit HgPartLines(int device) : device_(device) {}
  ~HgPartLines();
  int run(const HgPartLinesInput &in, hipStream_t stream, HgPartLinesOutput *out, std::string *err);

 private:
  template <typename T>
  using DevBuf = hgmem::Buf<T, hgmem::Space::Dev>;
  int device_;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  DevBuf<uint64_t> size_{"partlines size", 0}, off_{"partlines off", 0}, line_{"partlines line", 0}, first_{"partlines first", 0}, span_{"partlines span", 0};
  DevBuf<uint32_t> kind_{"partlines kind", 0}, pattern_{"partlines pattern", 0}, seg_{"partlines seg", 0};
  DevBuf<HgPartLinesEntry> entries_{"partlines entries", 0};
  DevBuf<uint8_t> temp_{"partlines temp", 0}, bytes_{"partlines bytes", 16};
  hgmem::Buf<uint64_t, hgmem::Space::Host> totals_{"partlines totals", 0};  // pinned: {bytes}
};

// The values stage (hg_values.hip) over the parts a scan left, one step per launch on `stream`: value and hash per part, the
// long parts (a wave each), the table probes, the occupied marks, the (first, count) pairs, and the per-value arrays.  The values'
// bytes are then copied by the gather stage's span and copy pass (hg_gather_launch) over entries that are nothing but a body.
enum class HgValuesStep { Hash, Long, Insert, Mark, Compact, Derive };
hipError_t hg_values_launch(const HgValuesArgs &a, HgValuesStep step, hipStream_t stream);
// What a value count works on (the last scan's records and parts, as hg_capi.hip remembers them) and what it leaves
// (hg_values_result_t).
struct HgValuesInput {
  const uint8_t *text;
  HgGatherList recs;
  const HgPart *parts;
  const uint32_t *part_pattern, *part_seg;  // part_seg nullptr without segments
  uint64_t n_parts;
  const uint64_t *seg_start;                // nullptr without segments
  uint32_t flags, hash_bits, table_log2;    // hash_bits 1 .. 64, 2^table_log2 > n_parts (the caller has checked both)
};
// What HgValues::group leaves: the groups as (first, count) pairs sorted by first, and the kernels' arguments they were made with
// (the hash pass's src and len per part among them).
struct HgValuesGroups {
  HgValuesArgs args;
  uint64_t n_values;
  const uint64_t *d_first, *d_count;
};
struct HgValuesOutput {
  uint64_t n_values, n_parts, n_bytes;
  const uint8_t *d_bytes;  // device arrays, valid until the next value count on this object
  const uint64_t *d_off, *d_count, *d_first, *d_line_number;
  const uint32_t *d_pattern, *d_segment;
  uint32_t table_log2;
  float ms_values;  // the stage: everything between the first memset and the copy pass, its two host synchronisations included
};
// The stage's buffers and launch sequence.  It owns its scratch (hgmem::Buf: freed with the object, every allocation logged)
// and touches nothing of the scanner's, of HgGather's, of HgPartLines' or of HgCounts'.
class HgValues {
 public:
  explicit HgValues(int device) : device_(device) {}
  ~HgValues();
  int run(const HgValuesInput &in, hipStream_t stream, HgValuesOutput *out, std::string *err);
  // The first half of run, for the rank stage: everything through the sort by first (one host synchronisation); in.flags may
  // carry HG_VALUES_F_BY_SEGMENT.  The arrays are valid until the next group or run on this object.
  int group(const HgValuesInput &in, hipStream_t stream, HgValuesGroups *groups, std::string *err);

 private:
  template <typename T>
  using DevBuf = hgmem::Buf<T, hgmem::Space::Dev>;
  int device_;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  DevBuf<uint64_t> key_{"values key", 0};  // (HG_VALUES_F_BY_SEGMENT only)
  DevBuf<uint64_t> src_{"values src", 0}, hash_{"values hash", 0}, long_{"values long", 0}, pos_{"values pos", 0}, pair_first_{"values pair first", 0},
      pair_count_{"values pair count", 0}, first_{"values first", 0}, count_{"values count", 0}, size_{"values size", 0}, off_{"values off", 0}, line_{"values line", 0},
      span_{"values span", 0};
  DevBuf<unsigned long long> slot_{"values slot", 0}, slot_count_{"values slot count", 0}, slot_first_{"values slot first", 0}, counters_{"values counters", 0};
  DevBuf<uint32_t> len_{"values len", 0}, pattern_{"values pattern", 0}, seg_{"values seg", 0};
  DevBuf<HgGatherEntry> entries_{"values entries", 0};
  DevBuf<uint8_t> temp_{"values temp", 0}, bytes_{"values bytes", 16};
  hgmem::Buf<uint64_t, hgmem::Space::Host> totals_{"values totals", 0};  // pinned: the counters, then {bytes}
};

// The rank stage (hg_rank.hip) behind the values stage's groups, one step per launch on `stream`: the groups' segments as sort keys,
// their counts in the final order, the segments' bounds and cuts, and the kept rows.
enum class HgRankStep { Keys, Counts, Bounds, Place };
hipError_t hg_rank_launch(const HgRankArgs &a, HgRankStep step, hipStream_t stream);
// HgValuesStep::Hash, Long and Insert with the segment in the key (a.key != nullptr): hg_rank.hip's instantiations.
hipError_t hg_rank_group_launch(const HgValuesArgs &a, HgValuesStep step, hipStream_t stream);
// What a ranking works on (HgValuesInput with HG_RANK_F_* as flags, the scan's segments and the cut) and what it leaves
// (hg_rank_result_t).
struct HgRankInput {
  HgValuesInput values;
  uint32_t n_seg;  // the scan's segments (0 without)
  uint64_t top;
};
struct HgRankOutput {
  uint64_t n_values, n_distinct, n_parts, n_bytes;
  const uint8_t *d_bytes;  // device arrays, valid until the next ranking on this object
  const uint64_t *d_off, *d_count, *d_first, *d_line_number;
  const uint32_t *d_pattern, *d_segment;
  const uint64_t *d_first_value, *d_seg_distinct, *d_seg_parts;  // nullptr without HG_RANK_F_PER_SEGMENT
  uint32_t n_seg, table_log2;
  float ms_rank;  // the stage: from the first memset to the copy pass, its host synchronisations included
};
// The stage's buffers and launch sequence.  It owns its scratch and a values stage of its own (hgmem::Buf: freed with the
// object, every allocation logged) and touches nothing of the scanner's or of any other stage, hg_count_values' HgValues included.
class HgRank {
 public:
  explicit HgRank(int device) : device_(device), groups_(device) {}
  ~HgRank();
  int run(const HgRankInput &in, hipStream_t stream, HgRankOutput *out, std::string *err);

 private:
  template <typename T>
  using DevBuf = hgmem::Buf<T, hgmem::Space::Dev>;
  int device_;
  HgValues groups_;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  DevBuf<uint64_t> g_first_{"rank group first", 0}, g_count_{"rank group count", 0}, key_idx_{"rank key idx", 0}, s_idx_{"rank sorted idx", 0}, s_count_{"rank sorted count", 0},
      cum_{"rank cum", 0}, first_group_{"rank first group", 0}, seg_distinct_{"rank seg distinct", 0}, seg_parts_{"rank seg parts", 0}, kept_{"rank kept", 0},
      first_value_{"rank first value", 0}, first_{"rank first", 0}, count_{"rank count", 0}, size_{"rank size", 0}, off_{"rank off", 0}, line_{"rank line", 0}, span_{"rank span", 0};
  DevBuf<uint32_t> key_seg_{"rank key seg", 0}, s_seg_{"rank sorted seg", 0}, pattern_{"rank pattern", 0}, seg_{"rank seg", 0};
  DevBuf<HgGatherEntry> entries_{"rank entries", 0};
  DevBuf<uint8_t> temp_{"rank temp", 0}, bytes_{"rank bytes", 16};
  hgmem::Buf<uint64_t, hgmem::Space::Host> totals_{"rank totals", 0};  // pinned: {rows, bytes}
};

// The value store (hg_valstore.hip) behind the values stage's groups, one step per launch on `stream`: the groups' lookup (a lane
// each, a wave for the long ones), the new groups' sizes, the table's rehash when it changes size, and the apply pass; a
// ranking's place pass.
enum class HgValStoreStep { Lookup, Long, Size, Rehash, Apply };
hipError_t hg_valstore_launch(const HgValStoreArgs &a, HgValStoreStep step, hipStream_t stream);
hipError_t hg_valstore_place_launch(const HgValRankArgs &a, hipStream_t stream);
// What an accumulation works on (HgValuesInput with HG_VALSTORE_F_* as flags: the call's parts; hash_bits and table_log2 govern
// the per-call grouping) and what it and a ranking leave (hg_acc_result_t, hg_acc_rank_result_t).
struct HgValStoreInput {
  HgValuesInput values;
  uint32_t store_log2;  // 0: the table grows on its own
  bool reset;           // empty the store first
};
struct HgValStoreOutput {
  uint64_t n_distinct, n_added, n_groups, n_parts, n_parts_total, n_bytes;
  uint32_t store_log2;
  float ms_acc;  // the call: from the grouping's first memset to the copy pass, its host synchronisations included
};
struct HgValRankOutput {
  uint64_t n_values, n_distinct, n_parts, n_bytes;
  const uint8_t *d_bytes;  // device arrays, valid until the next accumulate, rank or reset on this object
  const uint64_t *d_off, *d_count, *d_first, *d_line_number;
  const uint32_t *d_pattern;
  uint32_t store_log2;
  float ms_rank;
};
// The store's buffers and launch sequences.  It owns the table, the per-value rows, the byte arena, its scratch and a values
// stage of its own (hgmem::Buf: freed with the object, every allocation logged), survives scans and touches nothing of the
// scanner's or of any other stage.  A call that is refused or runs out of memory leaves the store as it was: the rows and the
// arena grow into fresh buffers that keep their contents (hgmem::Buf::grow), a table of another size is built aside and
// swapped in, and the host's view of the store changes on success only.
class HgValueStore {
 public:
  explicit HgValueStore(int device) : device_(device), groups_(device) {}
  ~HgValueStore();
  // Why a call with these flags and hash_bits cannot join the store as it is (nullptr: it can).
  const char *mismatch(uint32_t flags, uint32_t hash_bits, bool reset) const;
  int accumulate(const HgValStoreInput &in, hipStream_t stream, HgValStoreOutput *out, std::string *err);
  int rank(uint64_t top, bool order_first, hipStream_t stream, HgValRankOutput *out, std::string *err);
  void reset() { began_ = false, n_values_ = n_parts_ = tail_ = n_bytes_ = 0, log2_ = 0; }
  bool began() const { return began_; }
  int device() const { return device_; }

 private:
  template <typename T>
  using DevBuf = hgmem::Buf<T, hgmem::Space::Dev>;
  int device_;
  HgValues groups_;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  // the store: what the host knows of it, the table, the rows, the arena
  bool began_ = false;
  uint32_t flags_ = 0, hash_bits_ = 0, log2_ = 0;
  uint64_t n_values_ = 0, n_parts_ = 0, tail_ = 0, n_bytes_ = 0;  // (tail_: arena bytes in use; n_bytes_: the values' own)
  DevBuf<unsigned long long> slot_{"valstore slot", 0}, slot_new_{"valstore slot new", 0}, counters_{"valstore counters", 0};
  DevBuf<uint64_t> v_off_{"valstore off", 0}, v_count_{"valstore count", 0}, v_first_{"valstore first", 0}, v_line_{"valstore line", 0}, v_hash_{"valstore hash", 0};
  DevBuf<uint32_t> v_len_{"valstore len", 0}, v_pattern_{"valstore pattern", 0};
  DevBuf<uint8_t> arena_{"valstore arena", 16};
  // a call's scratch
  DevBuf<uint64_t> match_{"valstore match", 0}, long_{"valstore long", 0}, new_flag_{"valstore new flag", 0}, new_len_{"valstore new len", 0}, new_idx_{"valstore new idx", 0},
      new_off_{"valstore new off", 0}, ent_off_{"valstore entry off", 0}, span_{"valstore span", 0};
  DevBuf<HgGatherEntry> entries_{"valstore entries", 0};
  DevBuf<uint8_t> temp_{"valstore temp", 0};
  hgmem::Buf<uint64_t, hgmem::Space::Host> totals_{"valstore totals", 0};  // pinned: {new values, new bytes, counters}; a ranking's {bytes}
  // a ranking's
  DevBuf<uint64_t> r_keys_{"valstore rank keys", 0}, r_order_{"valstore rank order", 0}, r_count_{"valstore rank count", 0}, r_first_{"valstore rank first", 0},
      r_line_{"valstore rank line", 0}, r_size_{"valstore rank size", 0}, r_off_{"valstore rank off", 0}, r_span_{"valstore rank span", 0};
  DevBuf<uint32_t> r_pattern_{"valstore rank pattern", 0};
  DevBuf<HgGatherEntry> r_entries_{"valstore rank entries", 0};
  DevBuf<uint8_t> r_bytes_{"valstore rank bytes", 16};
};

// The counts stage (hg_counts.hip) over the record list a scan left: one launch on `stream` (nothing for an empty list).
hipError_t hg_counts_launch(const HgCountsArgs &a, hipStream_t stream);
// What a count works on (the last scan's list, as hg_capi.hip remembers it) and what it leaves (hg_counts_result_t).
struct HgCountsInput {
  HgCountsList list;  // seg_of == nullptr: the scan had no segments
  uint32_t n_seg;     // with HG_COUNTS_F_PER_SEGMENT: the segments of the scan
  uint32_t flags;     // HG_COUNTS_F_*
};
struct HgCountsOutput {
  uint32_t n_bins, n_seg;
  uint64_t n_records;
  const uint32_t *d_ids;  // device arrays of the object: the totals live as long as it does, the matrices until its next run
  const uint64_t *d_n_lines, *d_n_reports;
  const uint32_t *d_seg_lines, *d_seg_reports;
  float ms_counts;  // the stage: zeroing, the launch
};
// The stage's buffers and launch sequence.  It owns the bins of its database on the device and the running totals (zero when
// made), and touches nothing of the scanner's.  Every size is known before the launch; run() blocks once, at the end.
class HgCounts {
 public:
  HgCounts(int device, const HgDb &db) : device_(device), ids_host_(db.report_ids) {}
  ~HgCounts();
  int run(const HgCountsInput &in, hipStream_t stream, HgCountsOutput *out, std::string *err);
  const std::vector<uint32_t> &ids() const { return ids_host_; }
  // The running totals to host memory, ids().size() values each (zeroes before the first run); false on a HIP error.
  bool copy_totals(uint64_t *n_lines, uint64_t *n_reports) const;

 private:
  template <typename T>
  using DevBuf = hgmem::Buf<T, hgmem::Space::Dev>;
  int device_;
  std::vector<uint32_t> ids_host_;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  DevBuf<uint32_t> ids_{"counts ids", 0}, seg_lines_{"counts seg lines", 0}, seg_reports_{"counts seg reports", 0};
  DevBuf<unsigned long long> totals_{"counts totals", 0};  // n_lines[n_bins] then n_reports[n_bins]
};

// Test / experiment knobs of the engine, read from the environment ONCE, when a scanner is created (never during a scan:
// getenv is not safe against a concurrent setenv, and a scan must not change behaviour half-way).  None is needed in normal
// use.  The limit-lowering ones exist so that tests reach segmented scans / chunk halving on small texts.
struct HgEngineKnobs {
  uint64_t fin_target = 48;        // HG_FIN_TARGET: reports per finalize bucket
  bool no_bucket_finalize = false; // HG_NO_BUCKET_FINALIZE
  uint64_t chunk_tiles = 0;        // HG_CHUNK_TILES: pipeline chunk size (0: default)
  uint32_t max_chunks = 0;         // HG_MAX_CHUNKS (0: default)
  std::vector<double> chunk_weights;  // HG_CHUNK_WEIGHTS: relative chunk sizes
  long stream_wgs_per_cu = 0;      // HG_STREAM_WGS_PER_CU (0: default)
  long joiner = -1;                // HG_JOINER (-1: default)
  bool joiner_ahead = false;       // HG_JOINER_AHEAD: the joiner goes in front of its chunk's stream launch (it takes tiles for sure)
  bool no_early_finalize = false;  // HG_NO_EARLY_FINALIZE
  uint32_t confirm_mode_mask = 0x1F;  // HG_DEBUG_CONFIRM_MODES (profiling builds only: results are incomplete)
  long confirm_blocks_per_cu = 0;  // HG_CONFIRM_BLOCKS_PER_CU (0: default)
  uint64_t hit_limit = 0;          // HG_HIT_LIMIT (0: default 2^28)
  uint64_t cand_limit = 0;         // HG_CAND_LIMIT (0: default 2^30)
  bool verbose = false;            // HG_VERBOSE
  static HgEngineKnobs from_env();
};

class HgScanner {
 public:
  // The scanner shares ownership of the (immutable) database: launch parameters are read from it on every scan.
  static int create(std::shared_ptr<const HgDb> db, int device, HgScanner **out, std::string *err);
  const std::shared_ptr<const HgDb> &database() const { return db_; }
  ~HgScanner();
  // d_text: device pointer, 16-byte aligned, readable up to nbytes rounded up to 16.
  // invert: the result is the pieces WITHOUT a delivered report (hg_scan_device_invert), one record each.
  int scan(const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, hipStream_t stream, HgScanOutput *out, bool invert = false);
  // The same scan (inverted or not) with the context stage behind it: *out is exactly scan()'s, *ctx the pieces around its records.
  int scan_context(const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, hipStream_t stream, const HgContextParams &params, bool invert,
                   HgScanOutput *out, HgContextOutput *ctx);
  // The same scan (inverted or not) of a buffer of many files with the segment stage behind it: *out's records are the
  // segments' surviving records, file-relative; its counters stay the packed scan's.  HG_ERR_ARG (nothing scanned) for
  // malformed segments.
  int scan_packed(const void *d_text, uint64_t nbytes, int buffer_size, hipStream_t stream, const HgSegParams &params, bool invert, HgScanOutput *out,
                  HgSegOutput *seg);
  // The same with the per-file context stage behind it: *out and *seg are exactly scan_packed's, *ctx the pieces around each
  // segment's surviving records inside that segment (file-relative, segment after segment), *sc says which are whose.
  int scan_packed_context(const void *d_text, uint64_t nbytes, int buffer_size, hipStream_t stream, const HgSegParams &params, uint32_t before, uint32_t after,
                          bool invert, HgScanOutput *out, HgSegOutput *seg, HgContextOutput *ctx, HgSegCtxOutput *sc);
  // scan_packed (not inverted) with the per-file parts stage behind it: *out and *seg are exactly scan_packed's, *parts the matched
  // parts of the pieces each segment keeps a record of (file-relative, segment after segment), *sp says which are whose.
  // HG_ERR_ARG (nothing scanned) for a database the parts stage is not offered for, and for malformed segments.
  int scan_packed_parts(const void *d_text, uint64_t nbytes, int buffer_size, hipStream_t stream, const HgSegParams &params, HgScanOutput *out, HgSegOutput *seg,
                        HgPartsOutput *parts, HgSegPartsOutput *sp);
  // The plain scan with the parts stage behind it: *out is exactly scan()'s, *parts the matched parts of the pieces that have a
  // hit.  HG_ERR_ARG (nothing scanned, the reason in last_error()) for a database the stage is not offered for (hg_parts_refusal).
  int scan_parts(const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, hipStream_t stream, HgScanOutput *out, HgPartsOutput *parts);
  // Block mode (hs_scan): the whole buffer is one scan unit; hits carry line_no 0 and `to` relative to the buffer start.
  int scan_block(const void *d_text, uint64_t nbytes, hipStream_t stream, HgScanOutput *out);
  // Block mode for short blocks held in PINNED host memory (readable up to nbytes rounded up to 16): one launch, raw
  // reports {0, id, to | HG_HIT_SINGLE_BIT} in h_out (a segment of HG_BLOCK_SMALL_SEG records per workgroup), their
  // number per segment in h_counts; the caller synchronises the stream and applies the report rules.  Returns the number
  // of segments, 0 if the block or the pattern set is too large for this path.
  // *h_flag (pinned) receives `seq` when every segment is written: the caller may poll it instead of synchronising.
  uint32_t launch_block_small(const uint8_t *h_text, uint32_t nbytes, hipStream_t stream, HgHit *h_out, uint32_t *h_counts, uint32_t *h_flag, uint32_t seq);
  const std::string &last_error() const { return err_; }
  int set_error(int rc, const std::string &what) { return error(rc, what); }  // (stages that live outside the scanner report through it)
  int device() const { return device_; }
  const HgDbView &view() const { return view_; }  // the database's device tables (stream mode: hg_flows.hip)
  // What the finalize of the last pass did (hg_debug_finalize_info): noted by the host while it plans and queues the pass,
  // nothing is launched or copied for it during a scan.  path: 0 no pass yet, 1 bucketed, 2 compact with one packed key,
  // 3 compact with two sorts.
  struct FinInfo {
    uint32_t path, fin_shift, fin_nb, fin_cap, id_bits, to_bits;
    uint32_t early_buckets;  // buckets finalized before the last chunk's side passes were through (the early range) ...
    uint32_t early_beside_stream;  // ... those of them finalized beside the last stream launch, in front of the joiner
    uint32_t scan_blocks;    // blocks of hg_fin_scan_kernel, the largest bucket range of the pass
  };
  const FinInfo &finalize_info() const { return fin_info_; }
  bool left_bucketed() const { return fin_fallback_; }
  // the first `max` bucket fill levels of the last pass, read from the device now (none unless that pass was bucketed)
  int copy_fin_fill(uint32_t *dst, uint32_t max, uint32_t *n);

 private:
  HgScanner() = default;
  int init();
  int ensure(uint64_t nbytes);
  int alloc_cands(uint64_t n);
  int alloc_hits(uint64_t n);
  int scan_impl(const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base, bool block_mode, bool invert, hipStream_t stream, HgScanOutput *out);
  // One pass over the tiles [tile_lo, tile_hi) of the text: the whole buffer, or a segment of it (scan_segments).  The tile
  // scan starts from (cs0, piece0): the start of the line that contains the range's first byte and that line's piece index;
  // only pieces whose first scanned byte lies in [own_lo, own_hi) are reported.
  struct PassRange {
    uint64_t tile_lo, tile_hi, cs0, piece0, own_lo, own_hi;
    bool last;  // the range ends with the text: the pass leaves the final piece count
  };
  int scan_segments(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, hipStream_t stream, HgScanOutput *out, uint32_t nsegments);
  int run_fitting(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, const PassRange &range, bool block_mode, hipStream_t stream, HgScanOutput *out);
  int run_once(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, const PassRange &range, bool block_mode, hipStream_t stream, HgScanOutput *out);
  // the stages of a pass (hg_engine.hip)
  struct PassPlan;
  PassPlan plan_pass(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, const PassRange &range, bool block_mode, hipStream_t stream) const;
  int alloc_fin(uint32_t nb, hipStream_t stream);
  int launch_stream(PassPlan &p, uint32_t c, HgScanOutput *out);
  int launch_side(PassPlan &p, uint32_t c);
  int finalize_last(PassPlan &p, uint32_t c);
  int launch_fin(const PassPlan &p, hipStream_t s, uint32_t lo, uint32_t hi, bool beside_stream = false);
  int regrow(const PassPlan &p, uint64_t n_raw);
  int finalize_compact(const HgHit *hits, const HgHitAux *aux, uint32_t n, uint32_t id_bits, uint32_t to_bits, uint64_t line_bound, hipStream_t stream);
  int comb_pass(HgScanOutput *out, uint64_t bs1, uint64_t line_bound, hipStream_t stream);
  int minlen_pass(const uint8_t *text, uint32_t *n, hipStream_t stream);
  int invert_pass(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, hipStream_t stream, HgScanOutput *out);
  int context_pass(const uint8_t *text, uint64_t nbytes, uint64_t bs1, uint64_t line_base, const HgContextParams &params, hipStream_t stream, const HgScanOutput &out,
                   HgContextOutput *ctx);
  int parts_pass(const uint8_t *text, hipStream_t stream, const HgScanOutput &out, HgPartsOutput *parts);
  int parts_alloc(uint64_t n, size_t *tb, hipStream_t stream);
  int parts_records(uint64_t total);
  int segparts_pass(hipStream_t stream, const HgScanOutput &out, HgPartsOutput *parts, HgSegPartsOutput *sp);
  int segment_alloc(uint64_t n_seg);
  int segment_records(uint64_t n);
  int pad_filter(const HgSegArgs &checked, float *ms, hipStream_t stream, HgScanOutput *out);
  int segment_pass(const HgSegArgs &checked, float ms_check, hipStream_t stream, HgScanOutput *out, HgSegOutput *seg);
  int segctx_pass(uint32_t before, uint32_t after, hipStream_t stream, const HgScanOutput &out, HgContextOutput *ctx, HgSegCtxOutput *sc);
  int huge_lds_error() { return error(HG_ERR_HIP, "the huge-automaton kernel cannot have its LDS"); }
  bool fail(hipError_t e, const char *what);
  int error(int rc, const std::string &what) { err_ = what; return rc; }

  HgEngineKnobs knobs_;
  int device_ = 0;
  int num_cus_ = 256;
  int stream_wgs_per_cu_ = 0;
  std::string err_;
  // database on device
  HgDbView view_{};
  std::shared_ptr<const HgDb> db_;
  void *d_disc_ = nullptr, *d_bucket2_ = nullptr, *d_windows2_ = nullptr, *d_groups_ = nullptr, *d_wtab_ = nullptr, *d_bounds_ = nullptr;
  void *d_patterns_ = nullptr, *d_pool_ = nullptr, *d_factors_ = nullptr, *d_windows_ = nullptr, *d_bucket_ = nullptr,
       *d_filter_ = nullptr, *d_ext_ = nullptr, *d_slow_ = nullptr;
  // workspace
  uint64_t cap_tiles_ = 0;
  uint32_t cand_cap_ = 0, hit_cap_ = 0;
  uint64_t chunk_limit_tiles_ = 0;   // pipeline chunks no larger than this (0: the default 8 GiB): halved when a chunk's candidates would not fit
  uint32_t defer_spread_boost_ = 1;  // automaton confirm modes: lists per expression, raised when one expression's occurrences overflow its list
  bool hit_direct_ = false;  // the hits are too unevenly spread for equal per-block segments (HitSink::direct)
  HgTileSum *d_sums_ = nullptr;
  HgTileBase *d_bases_ = nullptr, *d_block_base_ = nullptr, *d_final_ = nullptr;
  HgTileElem *d_agg_ = nullptr;
  HgCand *d_cands_ = nullptr;
  HgDeferred *d_deferred_ = nullptr;
  uint32_t *d_defer_count_ = nullptr;
  HgHit *d_hits_raw_ = nullptr, *d_hits_out_ = nullptr;
  HgHitAux *d_aux_raw_ = nullptr, *d_aux_out_ = nullptr;
  HgHit *d_acc_hits_ = nullptr;  // segmented scans: the segments' ordered hits, one after the other
  HgHitAux *d_acc_aux_ = nullptr;
  uint64_t acc_cap_ = 0;
  bool side_bound_ = false;  // the last piped pass: the side passes, not the stream launches, set the pace (no joiner, no finalize on the side stream)
  uint64_t *d_key_a_ = nullptr, *d_key_b_ = nullptr;
  uint32_t *d_perm_a_ = nullptr, *d_perm_b_ = nullptr;
  uint8_t *d_keep_ = nullptr;
  uint32_t *d_counters_ = nullptr, *d_selected_ = nullptr, *d_seg_count_ = nullptr;
  uint32_t max_segs_ = 0;
  uint32_t *d_pflags_ = nullptr;
  void *d_temp_ = nullptr;
  size_t temp_bytes_ = 0;
  uint32_t *h_counters_ = nullptr;  // pinned
  HgTileBase *h_final_ = nullptr;   // pinned
  hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
  // chunked pipeline: the stream pass of chunk c+1 overlaps the verify / confirm passes of chunk c
  static constexpr int kMaxChunks = 64;
  hipStream_t side_stream_ = nullptr;
  hipEvent_t ev_tile_done_ = nullptr;  // the last chunk's tile scan is done (the early finalize starts behind it)
  hipEvent_t ev_fin_early_ = nullptr;  // the finalize of the earlier chunks' buckets (beside the last chunk's side passes) is done
  hipEvent_t ev_k1_begin_[kMaxChunks] = {}, ev_k1_end_[kMaxChunks] = {}, ev_side_done_[kMaxChunks] = {};
  // bucketed emission + finalize (hg_fin_*): records per bucket / kept counts -> output positions / {kept, raw} totals;
  // fin_fallback_: a bucket outgrew what one block sorts, the compact array + library sort is used from then on
  uint32_t *d_fin_fill_ = nullptr, *d_fin_kept_ = nullptr, *d_fin_total_ = nullptr, *d_fin_big_ = nullptr;
  bool fin_fallback_ = false;
  uint32_t fin_alloc_ = 0;  // buckets the arrays above hold (they grow with the bucket count a pass asks for)
  uint32_t fin_epoch_ = 0;  // hg_fin_scan_kernel: a fresh value per launch marks the blocks' partial sums as this launch's
  FinInfo fin_info_{};
  uint64_t fin_expect_hits_ = 0;  // raw hits of the last pass: the next one picks its bucket count for ~24 records a bucket
  void *d_huge_claim_ = nullptr;      // huge automata: (piece start, expression) pairs already run (hg_confirm_huge_kernel), 8-byte slots
  uint64_t huge_claim_slots_ = 0;
  uint32_t *d_from_ = nullptr;  // starts of the last scan's hits (SOM databases only, allocated by the first scan that needs them)
  uint64_t from_cap_ = 0;
  uint32_t som_max_nw_ = 0;
  // match-length pass (databases with a filtering min_length only): the per-expression lengths, and the second raw array the
  // survivors of a pass's raw reports go to (allocated by the first pass that needs it)
  uint32_t *d_min_lengths_ = nullptr;
  HgHit *d_minlen_hits_ = nullptr;
  HgHitAux *d_minlen_aux_ = nullptr;
  uint64_t minlen_cap_ = 0;
  uint32_t minlen_max_nw_ = 0;
  // combination pass (databases with combinations or QUIET expressions only): the tables, the per-hit counts / positions and
  // the union of delivered and combination records it hands to the finalize
  HgComb *d_combs_ = nullptr;
  uint32_t *d_comb_words_ = nullptr, *d_comb_feed_ = nullptr;
  uint32_t *d_comb_count_ = nullptr;
  uint64_t *d_comb_pos_ = nullptr;
  uint64_t comb_in_cap_ = 0;
  HgHit *d_comb_hits_ = nullptr;
  HgHitAux *d_comb_aux_ = nullptr;
  uint64_t comb_out_cap_ = 0;
  uint8_t *d_comb_temp_ = nullptr;
  size_t comb_temp_bytes_ = 0;
  // invert stage (inverted scans only, allocated by the first one): selected pieces per tile and their exclusive scan, the
  // scan's scratch, and the records of the selected pieces (they grow with the text and with the count the stage computes
  // before it writes: nothing is repeated to grow them)
  uint64_t *d_inv_count_ = nullptr, *d_inv_pos_ = nullptr;
  uint64_t inv_tiles_cap_ = 0;
  uint8_t *d_inv_temp_ = nullptr;
  size_t inv_temp_bytes_ = 0;
  HgHit *d_inv_hits_ = nullptr;
  HgHitAux *d_inv_aux_ = nullptr;
  uint64_t inv_cap_ = 0;
  // context stage (calls with context only, allocated by the first one): as the invert stage's; d_ctx_count_ has one word more,
  // the number of tail records
  uint64_t *d_ctx_count_ = nullptr, *d_ctx_pos_ = nullptr;
  uint64_t ctx_tiles_cap_ = 0;
  uint8_t *d_ctx_temp_ = nullptr;
  size_t ctx_temp_bytes_ = 0;
  HgHit *d_ctx_hits_ = nullptr;
  HgHitAux *d_ctx_aux_ = nullptr;
  uint64_t ctx_cap_ = 0;
  // parts stage (calls with parts only, allocated by the first one): the first-byte bitmap over the expressions, parts per hit
  // and their exclusive scan, the scan's scratch, and the parts with their expressions (sized from the count before the write)
  uint32_t *d_parts_first_ = nullptr;  // HgPartsArgs::first, built from the database by the first call
  uint64_t *d_parts_count_ = nullptr, *d_parts_pos_ = nullptr;
  uint64_t parts_hits_cap_ = 0;
  uint8_t *d_parts_temp_ = nullptr;
  size_t parts_temp_bytes_ = 0;
  HgPart *d_parts_ = nullptr;
  uint32_t *d_part_pattern_ = nullptr;
  uint64_t parts_cap_ = 0;
  // segment stage (calls with segments only, allocated by the first one): per segment the line base / end, the first record
  // and the length of its run, the exclusive scan of the lengths, n_lines and n_selected (seven arrays of seg_cap_ words in one
  // block), the flag word of the argument check, the scan's scratch, and the compacted records with their segments and starts
  uint64_t *d_segw_ = nullptr;
  uint64_t seg_cap_ = 0;
  uint32_t *d_seg_flag_ = nullptr;
  uint8_t *d_seg_temp_ = nullptr;
  size_t seg_temp_bytes_ = 0;
  HgHit *d_seg_hits_ = nullptr;
  HgHitAux *d_seg_aux_ = nullptr;
  uint32_t *d_seg_of_ = nullptr, *d_seg_from_ = nullptr;
  uint64_t seg_rec_cap_ = 0;
  uint64_t *d_pad_keep_ = nullptr, *d_pad_pos_ = nullptr;  // pad filter of inverted calls: a flag per hit and their exclusive scan
  uint64_t pad_cap_ = 0;
  // per-file context stage (calls with segments and context only): what the last segment pass worked on (its packed records
  // and per-segment arrays stay valid behind it), first_context, the surviving records in packed numbers with their segments'
  // windows, and the segment of each context record.  The per-tile counts,
  // their scan and the context records are the context stage's own buffers.
  HgSegArgs seg_last_{};
  uint64_t *d_segctx_first_ = nullptr;
  uint64_t segctx_seg_cap_ = 0;
  HgHit *d_segctx_k_ = nullptr;
  HgSegCtxWin *d_segctx_win_ = nullptr;
  uint64_t segctx_k_cap_ = 0;
  uint32_t *d_segctx_of_ = nullptr;
  uint64_t segctx_of_cap_ = 0;
  // per-file parts stage (calls with segments and parts only): first_part and the segment of each part.  The per-record
  // counts, their scan, the first-byte bitmap and the part records are the parts stage's own buffers.
  uint64_t *d_segparts_first_ = nullptr;
  uint64_t segparts_seg_cap_ = 0;
  uint32_t *d_segparts_of_ = nullptr;
  uint64_t segparts_of_cap_ = 0;
  uint32_t *d_seg_count2_ = nullptr;  // second set for double buffering
  HgCand *d_cands2_ = nullptr;
};
