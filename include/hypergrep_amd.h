/*
 * hypergrep_amd — C ABI of the MI355X (gfx950) multi-pattern line-scan engine.
 *
 * This one shared object replaces the native bundle the reference builds with
 * utils/build_hyperscanner.sh (libhs + libhyperscanner): every entry point is plain C, no torch or
 * C++ types cross the boundary.  Three faces:
 *
 *   Face B  hyperscan(), check_patterns()    what the reference's Python calls through ctypes
 *                                            (hypergrep/utils.py:116-121, :339-349) — same names,
 *                                            argument order, return codes and callback contract as
 *                                            hypergrep/lib/c/hyperscanner.c:154-159 and :248-258.
 *   Face A  hs_compile_multi() ... hs_scan()  the six libhs symbols the reference shim links against
 *                                            (hyperscanner.c:136,140,165,217,301,323,324), block mode.
 *   hg_*    buffer-level API for text that is already resident in HBM (bench, multi-GPU shards,
 *           framework integrations): compile once, scan device buffers, read hit records.
 *
 * The scan itself always runs on the GPU.  Without a usable HIP device the entry points fail
 * (hyperscan() returns 3 and prints the reason; hg_* return HG_ERR_HIP): there is no CPU fallback.
 */
#ifndef HYPERGREP_AMD_H
#define HYPERGREP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ Face B: shim ABI ---------- */

/* hyperscanner_result_t, hypergrep/lib/c/hyperscanner.c:42-46 == hypergrep/utils.py:25-40 (Result).
 * Offsets 0 / 8 / 16, sizeof 24.  `line` is NUL terminated and includes the trailing '\n' if the
 * line had one.  The array and every `line` buffer are owned by the library and reused for the next
 * batch: valid only during the callback. */
typedef struct hyperscanner_result {
    unsigned int id;
    unsigned long long line_number;
    char *line;
} hyperscanner_result_t;

/* hs_event, hyperscanner.c:54 == utils.CALLBACK_TYPE (utils.py:45-51). */
typedef void (*hs_event)(hyperscanner_result_t *results, int result_count);

/* Return codes, hyperscanner.c:25-33. */
enum {
    HYPERSCANNER_COMPILE_MEM = 1,
    HYPERSCANNER_COMPILE = 2,
    HYPERSCANNER_SCRATCH = 3, /* also: no usable GPU / HIP failure while setting up the scanner */
    HYPERSCANNER_DB = 4,
    HYPERSCANNER_STATE_MEM = 5,
    HYPERSCANNER_GZ_OPEN = 6,
    HYPERSCANNER_SCAN = 7
};

/* Replaces hyperscan(), hyperscanner.c:248-326.  Reads `file_name` (plain, gzip or zstd), scans it line
 * piece by line piece on the GPU and calls `on_event` with batches of `buffer_count` results in ascending
 * line order (last batch may be short).  buffer_size: a line longer than buffer_size-1 bytes is split
 * into pieces that are scanned and numbered separately (gzgets contract).  max_match_count: stop after
 * the line on which the running number of reports reaches it (0 = no limit). */
int hyperscan(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
              const unsigned int *pattern_ids, const unsigned int elements, hs_event on_event,
              const int buffer_size, int buffer_count, unsigned long long max_match_count);

/* Replaces check_patterns(), hyperscanner.c:154-167: compile only; 0 or HYPERSCANNER_DB (4). Needs no GPU. */
int check_patterns(const char *const *patterns, const unsigned int *pattern_flags,
                   const unsigned int *pattern_ids, const unsigned int elements);

/* ------------------------------------------------------------------ Face A: libhs subset ------ */

typedef struct hs_database hs_database_t;
typedef struct hs_scratch hs_scratch_t;
typedef struct hs_compile_error {
    char *message;
    int expression;
} hs_compile_error_t;
typedef struct hs_platform_info hs_platform_info_t;
typedef int (*match_event_handler)(unsigned int id, unsigned long long from, unsigned long long to,
                                   unsigned int flags, void *context);

#define HS_SUCCESS 0
#define HS_INVALID (-1)
#define HS_NOMEM (-2)
#define HS_SCAN_TERMINATED (-3)
#define HS_COMPILER_ERROR (-4)
#define HS_MODE_BLOCK 1
#define HS_MODE_STREAM 2
/* Start of match in stream mode (with HS_MODE_STREAM, exactly one; stream mode rules 1, 3 and 7): the precision of `from`.
 * LARGE is exact; MEDIUM gives HS_OFFSET_PAST_HORIZON when to - from >= 2^32, SMALL when to - from >= 2^16. */
#define HS_MODE_SOM_HORIZON_LARGE (1U << 24)
#define HS_MODE_SOM_HORIZON_MEDIUM (1U << 25)
#define HS_MODE_SOM_HORIZON_SMALL (1U << 26)
#define HS_OFFSET_PAST_HORIZON (~0ULL)
#define HS_DB_MODE_ERROR (-7)
#define HS_FLAG_CASELESS 1
#define HS_FLAG_DOTALL 2
#define HS_FLAG_MULTILINE 4
#define HS_FLAG_SINGLEMATCH 8
/* Report where each match starts.  For a report (id, to) of an expression with this flag, `from` is the SMALLEST s such
 * that the expression has a match spanning [s, to) of the scanned bytes; assertions at s (^ \b \B) see the byte before s,
 * or the start of the scanned bytes, exactly as in the forward scan.  The flag adds `from` and nothing else: the reports
 * (lines, ids, `to`, order) are those of the same database without it; expressions without it report from = 0.
 * Rejected with HS_FLAG_SINGLEMATCH, on automata of more than 1024 nodes (e.g. foo.{0,3000}bar), and unless all or none of
 * the expressions that share a report id carry it (several SOM expressions of one id that end at the same `to` give one
 * report with the smallest of their starts). */
#define HS_FLAG_SOM_LEFTMOST 256
/* Logical combinations.  An expression with HS_FLAG_COMBINATION is not a regex but a formula over the REPORT IDS of other
 * expressions of the set: decimal ids, `!` (not) > `&` (and) > `|` (or), parentheses, whitespace ignored.  Of its flags only
 * HS_FLAG_SINGLEMATCH and HS_FLAG_QUIET count (its `from` is 0).  The rules are per line piece (per block for hs_scan), on
 * the piece's reports after the report rules:
 *  - operand id X is true at offset t iff X has a report in the piece with to <= t;
 *  - combination C reports (C.id, t) at every distinct t where one of its operands reports, if C is true with the statuses
 *    at t.  All reports at offsets <= t count (this project's tie rule): `101 & !102` with both ending at 10 gives nothing;
 *  - its reports join the others under the usual rules: order by (line, id, to), an identical (id, to) once, SINGLEMATCH:
 *    the smallest `to` only.
 * HS_FLAG_QUIET on any expression: its reports still count for combinations but are never delivered (Results, hg_copy_hits,
 * hs_scan callbacks); a line whose only reports are quiet is not a matching line (max_match_count).  A QUIET combination
 * reports nothing.
 * Rejected (HS_COMPILER_ERROR / HG_ERR_COMPILE, with the rule in the message): syntax errors (empty formula, unbalanced
 * parentheses, dangling operator, a token that is not an operator or a decimal id, an id above 4294967295); an operand id no
 * expression of the set has; an operand that is itself a combination (no nesting); a combination id shared with any other
 * expression, or used as its own operand; more than 64 distinct operands, or more than 64 values on the evaluation stack; a
 * report id shared by QUIET and non-QUIET expressions; any combination that is true when none of its operands has matched
 * (e.g. `!101`, `101 | !102`): Hyperscan reports those at the end of the data, which this project does not.
 * The semantics follow Hyperscan's documentation of logical combinations; they are not checked against a Hyperscan binary. */
#define HS_FLAG_COMBINATION 512
#define HS_FLAG_QUIET 1024

/* Extended parameters of one expression (Hyperscan's hs_expr_ext_t: the same layout and flag values).  `flags` says which
 * fields are set; an expression without parameters is a NULL entry (or a NULL array, or flags 0).  Offsets have the origin
 * of `to`: the scanned bytes of the line piece (after the leading-NUL skip) for hyperscan() and hg_scan_device, the block
 * for hs_scan.
 *  - edit_distance = k: an end t is reported iff data[s:t] is within Levenshtein distance k of some string the expression
 *    matches, for some s <= t.  Edits are one-byte insertions, deletions and substitutions.  hamming_distance = k: the
 *    same with substitutions only.  An inserted or substituting byte is any byte `.` matches under the expression's flags
 *    (every byte with HS_FLAG_DOTALL, every byte but '\n' without it); under HS_FLAG_CASELESS a case change is no edit.
 *    A leading ^ / \A holds at s and a trailing $ / \z / \Z at t, with the usual multiline rules.  With
 *    HS_FLAG_SOM_LEFTMOST `from` is the smallest such s (automata of at most 1024 nodes after the expansion).
 *  - min_offset / max_offset: a report (id, to) exists only if min_offset <= to <= max_offset.  The bounds apply before
 *    the report rules: under HS_FLAG_SINGLEMATCH the delivered report is the smallest `to` in bounds.
 *  - min_length = L: a report (id, to) of the expression exists iff it has a match spanning [s, to) of the scanned bytes
 *    with to - s >= L; equivalently, the leftmost start at `to` (what HS_FLAG_SOM_LEFTMOST reports) is at most to - L.
 *    The scanned bytes are the piece after the leading-NUL skip, or the block for hs_scan (the origin of `to`);
 *    assertions are evaluated in the real context, as for start of match.  The filter applies before the report rules,
 *    as the offset bounds do: under HS_FLAG_SINGLEMATCH the delivered report is the smallest `to` that passes all of the
 *    expression's parameters; an identical (id, to) of several expressions sharing an id is delivered once if at least
 *    one of them produces it and passes its own min_length; combination operands see only surviving reports; a line
 *    whose reports are all removed is not a matching line (Face B rows, max_match_count).  HS_FLAG_SOM_LEFTMOST is not
 *    required.  With the flag `from` is unchanged, except for several SOM expressions sharing an id: there it is the
 *    smallest start over those expressions whose own report at `to` survives.  A value that can remove nothing (at most
 *    the shortest match length: the minimum match width, minus k with an edit distance) is accepted in every mode and
 *    dropped: the database is the one compiled without it.  A value that can remove a report is rejected with
 *    edit_distance or hamming_distance; when it is above the expression's longest match, or at least 2^31 on an unbounded
 *    expression (no report could survive); on automata of more than 1024 positions (they have no reverse tables: the rule
 *    of HS_FLAG_SOM_LEFTMOST); and in stream mode ("min_length that can remove reports is not supported in stream mode").
 * Rejected (HS_COMPILER_ERROR / HG_ERR_COMPILE, with the expression's index and the rule in the message): unknown
 * HS_EXT_FLAG bits; edit and Hamming distance together; min_offset > max_offset; min_length > max_offset; any parameter on
 * an HS_FLAG_COMBINATION expression; a distance above 16; a distance k >= the expression's minimum match width (the
 * expression would match anything); approximate expressions with \b, \B or an anchor anywhere but the ends above, where
 * they constrain the automaton (an assertion that only an empty alternative carries, as in (?:\b|)foo, changes nothing
 * and is accepted);
 * expansions over the node and edge limits ("pattern too large").
 * These rules are this project's reading of Hyperscan's documentation; they are not checked against a Hyperscan binary. */
typedef struct hs_expr_ext {
    unsigned long long flags; /* HS_EXT_FLAG_*: which fields are set */
    unsigned long long min_offset;
    unsigned long long max_offset;
    unsigned long long min_length;
    unsigned edit_distance;
    unsigned hamming_distance;
} hs_expr_ext_t;
#define HS_EXT_FLAG_MIN_OFFSET 1ULL
#define HS_EXT_FLAG_MAX_OFFSET 2ULL
#define HS_EXT_FLAG_MIN_LENGTH 4ULL
#define HS_EXT_FLAG_EDIT_DISTANCE 8ULL
#define HS_EXT_FLAG_HAMMING_DISTANCE 16ULL

/* Face B with extended parameters: hyperscan() and check_patterns() with `ext` (one pointer or NULL per pattern, or NULL)
 * after pattern_ids; hg_-prefixed, as every export beyond the reference's own names is.  The compiled-database cache tells
 * sets with parameters from the same patterns without them. */
int hg_hyperscan_ext(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                  const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements,
                  hs_event on_event, const int buffer_size, int buffer_count, unsigned long long max_match_count);
int hg_check_patterns_ext(const char *const *patterns, const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                       const hs_expr_ext_t *const *ext, const unsigned int elements);
/* Inverted match (grep -v) for files: hg_hyperscan_ext's arguments, reader, chunking and database cache, but `on_event`
 * receives one Result{id = HG_ID_INVERT, line_number, line} per SELECTED line piece, in ascending line order: the pieces
 * for which hg_hyperscan_ext would deliver nothing (hg_scan_device_invert below has the rules; `line` is the piece's scanned
 * bytes, empty for a piece of NULs only).  max_match_count: stop after that many selected pieces (0 = no limit). */
int hg_hyperscan_invert(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                        const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements,
                        hs_event on_event, const int buffer_size, int buffer_count, unsigned long long max_match_count);

/* Many files in one call (grep -r).  The files are packed in the given order into buffers of at most the chunk size of the
 * file path (256 MiB) by the packing rule of hg_scan_device_segments below, and each pack is ONE GPU scan with the segment
 * stage behind it.  on_event receives the results of file `file_index` in batches of at most buffer_count, in file order;
 * no batch mixes files.  Each file's results, and summaries[i].rc, are those hg_hyperscan_ext (invert == 0) or
 * hg_hyperscan_invert gives for that file alone with the same max_match_count.  A file that does not fit a pack, a gzip /
 * zstd file, and every file when buffer_size < 2 is scanned by that per-file route inside the call (the call holds no
 * context of the HYPERGREP_POOL pool meanwhile); an empty file is an empty segment; a file that cannot be
 * opened sets only its own rc (HYPERSCANNER_GZ_OPEN).  summaries[i].n_selected: the distinct line numbers among the
 * file's results; n_lines: the file's line pieces (for a file of the per-file route: those scanned before
 * max_match_count stopped it).  With on_event == NULL only the summaries are produced and no record leaves the GPU for
 * packed files (what -c, -l, -L, -q need).  Context lines: hg_hyperscan_files_context below.  Returns 0, or the code of a
 * failure that concerns the whole call (HYPERSCANNER_DB: the expressions do not compile). */
typedef void (*hg_files_event)(unsigned int file_index, hyperscanner_result_t *results, int result_count, void *context);
typedef struct hg_file_summary {
    int rc;
    uint64_t n_lines, n_selected;
} hg_file_summary_t;
int hg_hyperscan_files(const char *const *file_names, unsigned int n_files, const char *const *patterns,
                       const unsigned int *pattern_flags, const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext,
                       const unsigned int elements, hg_files_event on_event, void *context, const int buffer_size,
                       int buffer_count, unsigned long long max_match_count, int invert, hg_file_summary_t *summaries);

/* hg_hyperscan_files with context lines (grep -r -A / -B / -C): each pack is one GPU scan with the segment stage and the
 * per-file context stage behind it (hg_scan_device_segments_context below).  Each file's results go out in merged line order:
 * its own results, and one Result{id = HG_ID_CONTEXT, line_number, line} per context piece; this is exactly what
 * hg_hyperscan_context (declared below) delivers for that file alone with the same arguments, the max_match_count rule
 * included (it counts own results only).  Files of the per-file route (gzip, zstd, larger than a pack, pipes, every file when
 * buffer_size < 2) go through hg_hyperscan_context's code inside the call, in their place in the order; the call gives its
 * pooled context back first.  The summaries are those of hg_hyperscan_files: context lines are not counted.  A pattern id of
 * 0xFFFFFFFD or above is refused (HYPERSCANNER_DB), as in hg_hyperscan_context.  With on_event == NULL the call is
 * hg_hyperscan_files. */
int hg_hyperscan_files_context(const char *const *file_names, unsigned int n_files, const char *const *patterns,
                               const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                               const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event,
                               void *context, const int buffer_size, int buffer_count, unsigned long long max_match_count,
                               int invert, hg_file_summary_t *summaries, unsigned int before, unsigned int after);

/* Context lines (grep -A / -B / -C) for files: hg_hyperscan_ext's (invert == 0) or hg_hyperscan_invert's (invert != 0) call
 * with `before` and `after` line pieces of context around every line it delivers (hg_scan_device_context below has the
 * classes).  `on_event` receives the merged order: the call's own results, and one Result{id = HG_ID_CONTEXT, line_number,
 * line} per context line; a gap in the line numbers is where grep prints "--".  Context does not stop at the cuts between the
 * chunks a file is scanned in: the after-context still owed and the last `before` pieces of a chunk are carried into the next.
 * max_match_count counts the call's own results only; once it is reached the after-context of the last delivered line still
 * goes out, up to `after` pieces and ending before the next matching piece (GNU grep's -m with -A up to 3.4; grep() in
 * hypergrep_amd/utils.py builds the rule of 3.5 and later on top: all `after` lines, matching ones as context).  A pattern id of
 * 0xFFFFFFFD or above is refused (HYPERSCANNER_DB): the callback could not tell it from a context line. */
int hg_hyperscan_context(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                         const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements,
                         hs_event on_event, const int buffer_size, int buffer_count, unsigned long long max_match_count,
                         unsigned int before, unsigned int after, int invert);

/* Matched parts (grep -o) for files: hg_hyperscan_ext's arguments, reader, chunking (parts are per line piece, so the cuts
 * between a file's chunks carry nothing), decompression and database cache, with the parts stage behind each scan
 * (hg_scan_device_parts below has the definition).  `on_event` receives one Result{id = the report id of the part's
 * expression, line_number, line = the part's bytes, NUL-terminated} per part, in (line_number, from) order.  max_match_count
 * keeps hyperscan()'s rule on reports, which decides the delivered lines; every part of a delivered line goes out.  A
 * database the stage is not offered for is refused with HYPERSCANNER_DB before anything is read. */
int hg_hyperscan_parts(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                       const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements,
                       hs_event on_event, const int buffer_size, int buffer_count, unsigned long long max_match_count);

/* hg_hyperscan_files with matched parts (grep -r -o): the parameters of hg_hyperscan_files without `invert` (a line without a
 * match has no part).  Each pack is one GPU scan with the segment stage and the per-file parts stage behind it
 * (hg_scan_device_segments_parts below).  A file's batches hold one Result{id = the report id of the part's expression,
 * line_number, line = the part's bytes} per part, in (line_number, from) order: exactly what hg_hyperscan_parts delivers for
 * that file alone with the same arguments; max_match_count goes by the reports, and every part of a delivered line goes
 * out.  The summaries are those of hg_hyperscan_files.  Files of the per-file route (gzip, zstd, larger than a pack, pipes,
 * every file when buffer_size < 2) go through hg_hyperscan_parts' code inside the call.  A database the parts stage is not
 * offered for fails the whole call with HYPERSCANNER_DB before anything is read.  With on_event == NULL the call is
 * hg_hyperscan_files. */
int hg_hyperscan_files_parts(const char *const *file_names, unsigned int n_files, const char *const *patterns,
                             const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                             const hs_expr_ext_t *const *ext, const unsigned int elements, hg_files_event on_event,
                             void *context, const int buffer_size, int buffer_count, unsigned long long max_match_count,
                             hg_file_summary_t *summaries);

/* Counts per report id for files: which expressions fired, on how many lines and how often, without one callback row per
 * report.  hg_hyperscan_counts takes hg_hyperscan_ext's arguments, reader, chunking, decompression and database cache, and
 * runs the counts stage (hg_count_records below, with HG_COUNTS_ACCUMULATE) behind every chunk; no record is downloaded, and
 * n_bins x 24 bytes come back once at the end.  There is no max_match_count: counts describe the whole file.  counts[b]: the
 * b-th distinct report id of the expressions, ascending, with the file's matching lines and reports of that id; *n_counts:
 * the number of distinct ids, whatever max_counts is (a smaller max_counts fills what fits); *n_lines: the file's line
 * pieces.  Return codes are hg_hyperscan_ext's.
 * hg_hyperscan_files_counts takes hg_hyperscan_files' packing and runs the stage with HG_COUNTS_PER_SEGMENT behind every pack.
 * ids receives the distinct report ids (min(max_ids, *n_ids) of them); file_lines and file_reports are n_files rows of max_ids
 * values each, row f holding file f's counts in its first min(max_ids, *n_ids) places.  Files of the per-file route (gzip,
 * zstd, larger than a pack, every file when buffer_size < 2) go through hg_hyperscan_counts' code inside the call; a file
 * that cannot be opened sets its own rc and has a zero row.  The summaries are those of hg_hyperscan_files, but for n_selected
 * of a file of the per-file route, which is 0: nothing is delivered to count it from. */
typedef struct hg_id_count {
    uint32_t id, reserved;
    uint64_t n_lines, n_reports;
} hg_id_count_t; /* sizeof 24 */
int hg_hyperscan_counts(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                        const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements,
                        const int buffer_size, hg_id_count_t *counts, unsigned int max_counts, unsigned int *n_counts,
                        uint64_t *n_lines);
int hg_hyperscan_files_counts(const char *const *file_names, unsigned int n_files, const char *const *patterns,
                              const unsigned int *pattern_flags, const unsigned int *pattern_ids,
                              const hs_expr_ext_t *const *ext, const unsigned int elements, const int buffer_size,
                              hg_file_summary_t *summaries, uint32_t *ids, unsigned int max_ids, unsigned int *n_ids,
                              uint64_t *file_lines, uint64_t *file_reports);

/* call site hyperscanner.c:136 */
int hs_compile_multi(const char *const *expressions, const unsigned int *flags, const unsigned int *ids,
                     unsigned int elements, unsigned int mode, const hs_platform_info_t *platform,
                     hs_database_t **db, hs_compile_error_t **error);
/* hs_compile_multi with one hs_expr_ext_t pointer (or NULL) per expression, Hyperscan's argument order.  Without
 * parameters it compiles exactly the database hs_compile_multi compiles. */
int hs_compile_ext_multi(const char *const *expressions, const unsigned int *flags, const unsigned int *ids,
                         const hs_expr_ext_t *const *ext, unsigned int elements, unsigned int mode,
                         const hs_platform_info_t *platform, hs_database_t **db, hs_compile_error_t **error);
/* call site hyperscanner.c:140 (called with NULL when compilation succeeded) */
int hs_free_compile_error(hs_compile_error_t *error);
/* call site hyperscanner.c:301 */
int hs_alloc_scratch(const hs_database_t *db, hs_scratch_t **scratch);
/* call site hyperscanner.c:217: block-mode scan of data[0,length) as ONE unit (no line splitting).
 * The block is copied to HBM and scanned by the same kernels; `from` is the start of the match for expressions compiled
 * with HS_FLAG_SOM_LEFTMOST (the GPU start-of-match pass), 0 for the others. */
int hs_scan(const hs_database_t *db, const char *data, unsigned int length, unsigned int flags,
            hs_scratch_t *scratch, match_event_handler on_event, void *context);
/* call sites hyperscanner.c:323, :165/:324 (both may receive NULL) */
int hs_free_scratch(hs_scratch_t *scratch);
int hs_free_database(hs_database_t *db);

/* ---- stream mode (HS_MODE_STREAM) ----
 * A database compiled with HS_MODE_STREAM scans streams: data that arrives in writes, where a match may span writes.  Let D
 * be the concatenation of a stream's writes.
 *  1. Equivalence.  For any split of D into writes (empty and 1-byte writes, splits next to a '\n' included), the reports
 *     of all the stream's hs_scan_stream calls plus its close are exactly those hs_scan(D) delivers on a block-mode database
 *     of the same expressions, flags, ids and ext.  `to` is a stream offset (64-bit).  `from` is 0, except for expressions
 *     with HS_FLAG_SOM_LEFTMOST in a database compiled with an HS_MODE_SOM_HORIZON_* bit: their `from` is the block-mode
 *     start of match (a stream offset), or HS_OFFSET_PAST_HORIZON when to - from reaches the horizon (MEDIUM 2^32, SMALL
 *     2^16; LARGE is exact).  SINGLEMATCH: one report per id for the whole stream, the smallest `to` (in bounds).
 *     min_offset / max_offset bound stream offsets (of `to` only).  An identical (id, to) is delivered once; of several SOM
 *     expressions sharing the id, with the smallest of their starts.
 *  2. Order.  Within one call reports come in ascending (to, id).  Across a stream's calls `to` never decreases, with one
 *     exception: a write ending in a '\n' at stream offset end - 1 whose step was held (rule 4) may deliver, in the next
 *     call, a report with to = end - 1 after reports with to = end came in the call before.
 *  3. Latency.  A report (id, t) is delivered at the latest by the call whose write holds stream byte t + 1, else by the
 *     close / reset.  Expressions without assertions (^ $ \A \z \Z \b \B, after ext expansion) deliver (id, t) by the
 *     call whose write holds byte t - 1: `foo` at the very end of a write is reported by that call.  A SOM expression
 *     delivers a write-end test early only when every possible next context gives the same start; a SOM expression that
 *     shares its report id with another never delivers early (its reports wait for the next byte or the close, by the
 *     first rule of this item), and holds a trailing '\n' whenever one expression of the id does, so that every report of
 *     an (id, to) arrives in one call with the smallest `from`.
 *  4. Write boundaries.  The accept test at byte i reads the context of byte i (the next byte of the match).  At the end of
 *     a write, what holds for every possible next context (END included) is delivered at once; the rest is pending, decided
 *     by the next write's first byte or by the end of data at the close, and never delivered twice.  A '\n' is the final
 *     newline ($ and \Z before the end of data) only when it is the last byte of D, which is known only at the close: a
 *     write's trailing '\n' is held (not stepped) by the expressions that tell a final '\n' from another (non-multiline $,
 *     \Z; decided at compile time), until the next write or the close.  An expression that shares a SINGLEMATCH id with
 *     one that holds holds too (so the smallest `to` of that id is never preceded by a larger one).
 *  5. Termination.  A non-zero return from the callback ends the call with HS_SCAN_TERMINATED; the stream is terminated:
 *     later hs_scan_stream calls deliver nothing and return HS_SCAN_TERMINATED, hs_close_stream delivers nothing and frees
 *     it, hs_reset_stream clears the state.
 *  6. Streams of one database may be interleaved in any order and scanned with any scratch of the database.  A copy
 *     (hs_copy_stream) evolves independently of its original.  A stream lives in host memory; each call copies the pending
 *     writes and states of its streams to the GPU and back in one launch.
 *  7. Compile rules (HS_COMPILER_ERROR, the message names the expression's index and the rule): HS_FLAG_SOM_LEFTMOST
 *     without an HS_MODE_SOM_HORIZON_* bit, HS_FLAG_COMBINATION, HS_FLAG_QUIET, automata of more than 1024 positions after
 *     ext expansion ("too large for stream mode"), and SOM expressions of more than 256 positions after ext expansion
 *     ("too large for start of match in stream mode").  Block mode's SOM rules apply (no SOM with SINGLEMATCH; the
 *     expressions sharing a report id are all SOM or none).  Every other expression block mode accepts is accepted.  Modes:
 *     HS_MODE_BLOCK, HS_MODE_STREAM, and HS_MODE_STREAM with exactly one horizon bit when at least one expression has
 *     HS_FLAG_SOM_LEFTMOST; everything else (HS_MODE_VECTORED, a horizon bit with block mode or on a set without SOM
 *     expressions, two horizon bits) is rejected.  Block-mode databases are unchanged by stream mode.
 *  8. State.  hs_stream_size grows with the horizon: a SOM expression carries one start per automaton position, 2 (SMALL),
 *     4 (MEDIUM) or 8 (LARGE) bytes each, a saturating distance from the carried position.  A database without SOM
 *     expressions has the layout and size of one compiled without a horizon.  hs_copy_stream and hs_reset_stream carry and
 *     restore the starts.
 * The horizon and shared-id rules are this project's reading of Hyperscan's documentation, not checked against a Hyperscan
 * binary.
 * hs_open_stream on a block-mode database and hs_scan on a stream-mode one return HS_DB_MODE_ERROR; hs_alloc_scratch
 * works for both. */
typedef struct hs_stream hs_stream_t;
int hs_open_stream(const hs_database_t *db, unsigned int flags, hs_stream_t **stream);
int hs_scan_stream(hs_stream_t *id, const char *data, unsigned int length, unsigned int flags, hs_scratch_t *scratch,
                   match_event_handler on_event, void *context);
/* Delivers the end-of-data reports and frees the stream.  With on_event == NULL, scratch may be NULL and nothing is
 * delivered. */
int hs_close_stream(hs_stream_t *id, hs_scratch_t *scratch, match_event_handler on_event, void *context);
/* Delivers what hs_close_stream would (nothing with on_event == NULL), then returns the stream to its freshly opened state. */
int hs_reset_stream(hs_stream_t *id, unsigned int flags, hs_scratch_t *scratch, match_event_handler on_event,
                    void *context);
int hs_copy_stream(hs_stream_t **to_id, const hs_stream_t *from_id);
int hs_stream_size(const hs_database_t *db, size_t *stream_size);

/* Batched stream scan (one launch for the pending writes of many streams).  Equivalent to hs_scan_stream on items 0..n-1
 * in order, then hs_reset_stream for the items flagged HG_STREAM_ITEM_LAST (their end-of-data reports are delivered).
 * Reports come grouped by item, in item order, each item's in (to, id) order.  HS_INVALID before scanning anything if a
 * stream appears twice, a stream belongs to another database than the scratch, or an argument is NULL where data is
 * needed (data may be NULL when every length is 0; item_flags NULL: all 0).  A non-zero return from the callback
 * terminates that item's stream only; the other items go on, and the call returns HS_SCAN_TERMINATED. */
typedef int (*hg_stream_match_handler)(unsigned int item, unsigned int id, unsigned long long from,
                                       unsigned long long to, unsigned int flags, void *context);
#define HG_STREAM_ITEM_LAST 1u /* after this write: deliver the end-of-data reports, then reset the stream */
int hg_scan_stream_batch(hs_stream_t *const *streams, const char *const *data, const unsigned int *lengths,
                         const unsigned int *item_flags, unsigned int n, hs_scratch_t *scratch,
                         hg_stream_match_handler on_event, void *context);

/* Batched block scan: many independent buffers scanned as blocks in one call (a few launches instead of one hs_scan per
 * buffer, measured at 16.5-19 us each on a short buffer: launch and host-link latency).  `db` is a BLOCK-mode database; item i is data[i][0, lengths[i]).
 *  1. Equivalence.  For every item i the reports delivered with item == i are exactly those of
 *     hs_scan(db, data[i], lengths[i], 0, scratch, ...): the same (id, from, to) in the same (to, id) order, for every
 *     block-mode database hs_compile_ext_multi accepts.  `from` is the start of match for HS_FLAG_SOM_LEFTMOST expressions
 *     and 0 otherwise, as in hs_scan.  An item is a block, not a line: '\n' and NUL are ordinary bytes, and `$`, `\Z`, `.`
 *     see the item's real bytes and its real end.
 *  2. Order.  Reports come grouped by item, in item order (the shape of hg_scan_stream_batch).  The call collects a
 *     launch's reports before it delivers them.
 *  3. Empty items (lengths[i] == 0; data[i] may be NULL) deliver nothing.  n == 0 returns HS_SUCCESS without touching the
 *     GPU.
 *  4. Termination.  A non-zero return from the callback ends that item's delivery; the other items are still delivered,
 *     and the call returns HS_SCAN_TERMINATED.  Items keep no state, so nothing else changes.
 *  5. Errors.  HS_INVALID before anything is scanned for NULL arguments, a scratch of another database, or a NULL data[i]
 *     with lengths[i] > 0; HS_DB_MODE_ERROR for a stream-mode database.  on_event == NULL scans and delivers nothing (as
 *     hs_scan does).  An error met later in the call (HS_NOMEM, or HS_INVALID for a failed GPU operation) ends the call
 *     there: the items before the failing launch have been delivered, the others are not.
 *  6. Speed.  One kernel takes what hs_scan's one-launch path takes: databases without HS_FLAG_SOM_LEFTMOST expressions,
 *     without combinations or QUIET expressions, without offset bounds or a min_length that can remove reports, without
 *     automata over 1024 positions, of at most
 *     2048 expressions in groups of 32 (or 16384 in groups of 256), and items of at most 8192 bytes.  Everything else (a whole
 *     batch on another database, single longer items, a launch with more than 2^24 reports) is scanned item by item as
 *     hs_scan's general path scans it, inside the same call: correct by rule 1, with no speed-up. */
int hg_scan_blocks(const hs_database_t *db, const char *const *data, const unsigned int *lengths, unsigned int n,
                   hs_scratch_t *scratch, hg_stream_match_handler on_event, void *context);

/* ------------------------------------------------------------------ hg_*: device buffers ------ */

enum {
    HG_OK = 0,
    HG_ERR_ARG = -1,
    HG_ERR_NOMEM = -2,
    HG_ERR_COMPILE = -4,
    HG_ERR_HIP = -10,
    HG_ERR_SMALL_BUFFER = -11
};

typedef struct hg_database hg_database_t; /* compiled expressions (host memory) */
typedef struct hg_scanner hg_scanner_t;   /* database + workspace resident on one GPU; one scan at a time */

/* One report: (line piece, id).  16 bytes — the algorithmic write traffic per hit. */
typedef struct hg_hit {
    uint64_t line_number; /* 0-based piece index == hyperscanner_result_t.line_number */
    uint32_t id;          /* == hyperscanner_result_t.id */
    uint32_t to;          /* match end offset inside the scanned bytes (Hyperscan's `to`); its start: hg_copy_hit_starts */
} hg_hit_t;

/* Where Result.line lives in the scanned buffer. */
typedef struct hg_hit_aux {
    uint64_t start; /* byte offset of the first scanned byte of the piece */
    uint32_t len;   /* scanned length (what strlen(Result.line) would be) */
    uint32_t pattern; /* index of the expression that produced the report */
} hg_hit_aux_t;

typedef struct hg_scan_result {
    uint64_t n_hits;       /* ordered by (line_number, id, to), SINGLEMATCH / duplicate rules applied */
    uint64_t n_lines;      /* line pieces in the buffer */
    uint64_t n_candidates; /* required-literal occurrences that went to the confirm stage */
    uint64_t n_raw_hits;   /* reports before de-duplication */
    const hg_hit_t *d_hits;    /* DEVICE pointers, valid until the next scan on this scanner */
    const hg_hit_aux_t *d_aux;
    float ms_stream; /* duration of the streaming kernel (summed over its launches), HIP events on the launch stream */
    float ms_total;  /* whole launch sequence */
    uint32_t reruns; /* passes repeated because the workspace had to grow */
    uint32_t stream_launches; /* launches of the streaming kernel in this scan (one per pipeline chunk) */
    uint64_t joiner_tiles;    /* 16 KiB tiles streamed by the joiner launches (hg_stream_join_kernel), not by those */
    uint32_t joiner_launches; /* launches of the joiner kernel in this scan */
    uint32_t invert_us;       /* hg_scan_device_invert: the added stage in microseconds (HIP events around its count launch, scan and write
                                 launch, the host synchronisation that sizes the output included: more than its kernels' time); else 0 */
} hg_scan_result_t;

typedef struct hg_db_info {
    uint32_t n_patterns;
    uint32_t n_literal_anchored; /* patterns filtered by the streaming window prefilter */
    uint32_t n_always_on;        /* patterns run on every line */
    uint32_t n_factors;
    uint32_t n_windows;
    uint32_t fold_mask;
    uint32_t max_state_words;
    uint32_t table_bytes;
    uint32_t byte_windows;       /* 1: the prefilter probes a window at every byte offset (sets with 3..6-byte required literals) */
} hg_db_info_t;

/* Compile `n` expressions (same inputs as hs_compile_multi).  On failure returns HG_ERR_COMPILE and
 * writes "<expression index>: <reason>" to err. */
int hg_db_compile(const char *const *expressions, const unsigned int *flags, const unsigned int *ids,
                  unsigned int n, hg_database_t **db, char *err, size_t errlen);
/* The same with extended parameters (hs_expr_ext_t above): one pointer or NULL per expression, `ext` itself may be NULL. */
int hg_db_compile_ext(const char *const *expressions, const unsigned int *flags, const unsigned int *ids,
                      const hs_expr_ext_t *const *ext, unsigned int n, hg_database_t **db, char *err, size_t errlen);
/* Optional: re-select the literal windows of the prefilter using byte statistics of a host-side text sample (any
 * part of what will be scanned) and rebuild the filter tables.  Never changes results, only how often the slower
 * stages run.  The tuned tables are built aside and swapped in on success: scanners created BEFORE the call keep the
 * tables they were created with (still valid), scanners created after it use the tuned ones; on failure nothing changes. */
int hg_db_tune(hg_database_t *db, const void *sample, size_t nbytes);
void hg_db_release(hg_database_t *db);
int hg_db_info(const hg_database_t *db, hg_db_info_t *info);

int hg_scanner_create(const hg_database_t *db, int device, hg_scanner_t **scanner, char *err, size_t errlen);
void hg_scanner_destroy(hg_scanner_t *scanner);
const char *hg_scanner_error(const hg_scanner_t *scanner);

/* Scan `nbytes` of text resident in HBM at d_text (16-byte aligned; must be readable up to nbytes
 * rounded up to 16).  Lines are numbered from line_base.  `stream` is a hipStream_t (NULL = default).
 * The text is the bytes [d_text, d_text + nbytes) and nothing else.  The CONTENT of any byte outside them never influences a
 * result of this call or of a call built on it (invert, context, parts, segments, gather, counts): the up to 15 bytes of the
 * round-up may hold anything, a continuation of the text included, and d_text may point into the middle of a larger
 * allocation.  Only the stated round-up must be readable, and nothing before d_text is read.  (tests/test_text_bounds_gpu.py
 * scans windows of a larger text whose neighbouring bytes would complete a match, add a line or change a `\b` / `$`.)
 * Blocks until the results are ready.  No size limit besides HBM: a buffer with more than 2^28 reports (or more
 * pipeline chunks than one pass has) is scanned in segments whose ordered hits are put one after the other. */
int hg_scan_device(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size,
                   uint64_t line_base, void *stream, hg_scan_result_t *result);

/* Inverted match (grep -v): the contract of hg_scan_device, but the result holds the line pieces NO expression matches.
 * A line piece is what hg_scan_device numbers: lines end at '\n'; a line longer than buffer_size - 1 bytes is cut into pieces
 * of buffer_size - 1 bytes, each numbered on its own; a piece's scanned bytes are those after its leading NULs up to its
 * first NUL, the '\n' included; a zero-length tail after the buffer's last '\n' is not a piece.  A piece is SELECTED iff
 * hg_scan_device delivers no report for it: the SINGLEMATCH, duplicate, offset-bound, min_length, combination and QUIET
 * rules apply first, so a piece whose only reports are QUIET or were all removed is selected, and so is a piece whose
 * scanned length is 0 (nothing but NULs up to its end), with len == 0.
 * The result has one record per selected piece, in ascending line_number: hg_hit_t{line_number, id = HG_ID_INVERT, to = 0}
 * and hg_hit_aux_t{start, len, pattern = 0xFFFFFFFF}, `start` and `len` as for hits.  n_hits is the number of selected
 * pieces; n_lines, n_candidates, n_raw_hits, the timings and the counters are those of the underlying scan (invert_us: the
 * added stage).  hg_copy_hits and hg_copy_hits_device work unchanged; hg_copy_hit_starts yields zeros.
 * Complement identity, for every database and buffer: (the distinct line_number values among hg_scan_device's hits) +
 * (hg_scan_device_invert's n_hits) == n_lines.
 * The stage runs on the GPU behind the scan (hypergrep_amd/csrc/hg_invert.hip): per-tile counts from the scan's line geometry
 * and hits, their exclusive scan, one pass over the text that writes the records in order.  A piece of gigabytes (a buffer
 * without newlines under a huge buffer_size) is trimmed by a single wavefront. */
#define HG_ID_INVERT 0xFFFFFFFFu /* the id of an inverted result's records: no expression */
int hg_scan_device_invert(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base,
                          void *stream, hg_scan_result_t *result);

/* Context lines (grep -A / -B / -C): hg_scan_device (invert == 0) or hg_scan_device_invert (invert != 0) with a second
 * ordered list, the line pieces AROUND the pieces the call delivers a record for.  `result` is filled exactly as that call
 * fills it (same records, same order; hg_copy_hits* unchanged).
 * Units and classes.  Context is counted in line pieces, the unit hg_scan_device numbers (see hg_scan_device_invert above).
 * Let M be the piece numbers for which the call delivers a record: the hits after every report rule, or the selected pieces
 * of an inverted call.  With B = before and A = after, a piece q of the buffer falls in exactly one class:
 *   match    q is in M: its records are those in `result`, untouched;
 *   context  q is not in M, and some m in M has q - A <= m <= q + B, or q < line_base + carry_after (after-context the
 *            previous buffer still owes);
 *   tail     (only with HG_CONTEXT_TAIL) q is neither and lies among the buffer's last B pieces: a candidate for the next
 *            buffer's before-context, which the caller keeps or drops;
 *   otherwise nothing.
 * The context records: d_ctx_hits / d_ctx_aux hold n_context entries in ascending line_number, one hg_hit_t{line_number, id,
 * to = 0} + hg_hit_aux_t{start, len, pattern = 0xFFFFFFFF} per context or tail piece, id = HG_ID_CONTEXT or
 * HG_ID_CONTEXT_TAIL, `start` and `len` as for hits.  Both lists are ordered by line and share no line number: a consumer
 * merges them with two cursors, and a gap in the merged line numbers is where grep prints "--".
 * owed_after: the after-context pieces still owed past the buffer's end; with a record in M max(0, last m + A - last piece),
 * without one max(0, carry_after - n_lines).  n_tail: the tail records among the n_context.  context_us: the added stage in
 * microseconds (HIP events, as invert_us).  With A = B = 0, no carry and no tail flag the stage is skipped: n_context = 0.
 * before and after may be any uint32_t: the arithmetic saturates at piece 0 and at the buffer's end.
 * Chaining identity.  Cut a text at any piece boundary into buffers and scan them in order with line_base advanced by
 * n_lines, carry_after = the previous owed_after, and HG_CONTEXT_TAIL.  Of each buffer's tail records keep those with
 * line_number >= (first m of the next buffer with a record) - B, none if no later buffer has a record.  The merged output
 * equals that of the whole text scanned at once.
 * The stage runs on the GPU behind the scan (hypergrep_amd/csrc/hg_context.hip): per-tile counts from the scan's line geometry
 * and the records' lines (no text read), their exclusive scan, one pass over the tiles that hold context, written in order. */
#define HG_ID_CONTEXT 0xFFFFFFFEu      /* the id of a context record */
#define HG_ID_CONTEXT_TAIL 0xFFFFFFFDu /* the id of a tail record */
#define HG_CONTEXT_TAIL 1u             /* hg_context_t.flags: deliver tail records */
typedef struct hg_context {
    uint32_t before, after; /* B and A, in line pieces */
    uint64_t carry_after;   /* after-context owed by the previous buffer (its owed_after), 0 for the first */
    uint32_t flags;         /* 0 or HG_CONTEXT_TAIL */
} hg_context_t;
typedef struct hg_context_result {
    uint64_t n_context;  /* context and tail records */
    uint64_t n_tail;     /* the tail records among them */
    uint64_t owed_after; /* after-context still owed past the buffer's end */
    const hg_hit_t *d_ctx_hits; /* DEVICE pointers, valid until the next scan on this scanner */
    const hg_hit_aux_t *d_ctx_aux;
    uint32_t context_us; /* the context stage alone (count launch, scan, the host synchronisation that sizes the output, write launch) */
    uint32_t reserved;
} hg_context_result_t;
int hg_scan_device_context(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base,
                           void *stream, const hg_context_t *context, int invert, hg_scan_result_t *result,
                           hg_context_result_t *context_result);
/* Copy the last scan's first `max` context records (and aux records, if aux != NULL) to host memory; none after a scan
 * without context. */
int hg_copy_context(hg_scanner_t *scanner, hg_hit_t *hits, hg_hit_aux_t *aux, uint64_t max);
/* The same (16-byte records only) into a DEVICE buffer, asynchronously on `stream`. */
int hg_copy_context_device(hg_scanner_t *scanner, void *d_dst, uint64_t max, void *stream);

/* Matched parts (grep -o): hg_scan_device with a second ordered list, WHAT matched WHERE in every line piece the call
 * delivers a record for, over all expressions of the database at once.  `result` is filled exactly as hg_scan_device fills it
 * (same hits, same order; hg_copy_hits* and hg_copy_hit_starts* unchanged).
 * Definition.  Let L[0, len) be the scanned bytes of a line piece, the unit hg_scan_device numbers (after leading NULs, up to
 * the first NUL, the '\n' included: see hg_scan_device_invert above), and let the expressions be those of the database with
 * the flags they were compiled with.
 *   Expression p MATCHES EXACTLY [s, e), 0 <= s < e <= len, if it has a match spanning those bytes with every assertion
 *   (^ $ \b \B \A \z \Z, multiline or not) evaluated in the piece's real context: the byte before s, the byte at e, and the
 *   piece's ends.
 *   The PARTS of a piece follow GNU grep's -o rule over all expressions at once.  Start with a cursor at 0 and repeat:
 *   `from` is the smallest s >= cursor at which any expression matches exactly some [s, e); `to` is the largest such e over
 *   all expressions; `pattern` is the lowest expression index that matches exactly [from, to); emit the part and set the
 *   cursor to `to`; stop when there is no such s.
 * Parts of a piece never overlap and never are empty (the compiler rejects expressions that match the empty string).
 * HS_FLAG_SINGLEMATCH and HS_FLAG_SOM_LEFTMOST do not change the parts: they only govern reports.  A part may include the
 * piece's '\n' when an expression consumes it (DOTALL `.`); it is reported as it is.
 * Parts are computed for exactly the pieces for which hg_scan_device delivers at least one record: the distinct line_number
 * values of the final hits, after every report rule.
 * Identity, for every accepted database and buffer: the distinct line_number values among the parts equal the distinct
 * line_number values among the hits.  Every part's `to` is an end the same expression would report on that piece without
 * HS_FLAG_SINGLEMATCH.
 * The records: d_parts holds n_parts entries ordered by (line_number, from), hg_part_t{line_number, from, to} with the
 * offsets inside the scanned bytes (the origin of hg_hit_t.to); d_part_pattern holds the expression INDEX of each part (its
 * report id is the one the expression was compiled with).  Both are DEVICE pointers, valid until the next scan on this
 * scanner.  parts_us: the added stage in microseconds (HIP events, as invert_us).
 * Not offered: the call returns HG_ERR_ARG, scans nothing, and hg_scanner_error names the reason, for a database with an
 * automaton above 1024 nodes (HG_MAX_NODES: no dense tables to walk), with HS_FLAG_COMBINATION or HS_FLAG_QUIET expressions,
 * or with any extended parameter (hs_expr_ext_t: distances, offset bounds, min_length): none of these has a part in the above
 * sense without further rules.  Not combined with invert or context; with segments the call is
 * hg_scan_device_segments_parts below.
 * The stage runs on the GPU behind the scan (hypergrep_amd/csrc/hg_parts.hip): a wavefront per piece that has a hit, its
 * lanes 64 consecutive candidate starts, each running an anchored forward walk per expression; per-hit counts, their
 * exclusive scan, and a second walk that writes the records in order.  The text is read only inside pieces that have a hit.
 * Cost: the walks of one start are bounded by the longest match from it, so an expression such as a.*b|a on a long line of
 * `a` makes a piece quadratic in its length. */
typedef struct hg_part {
    uint64_t line_number; /* as hg_hit_t.line_number */
    uint32_t from;        /* the part is the bytes [from, to) of the piece's scanned bytes */
    uint32_t to;
} hg_part_t;
typedef struct hg_parts_result {
    uint64_t n_parts;
    const hg_part_t *d_parts;       /* DEVICE pointers, valid until the next scan on this scanner */
    const uint32_t *d_part_pattern; /* expression index of each part */
    uint32_t parts_us;              /* the parts stage alone (count launch, scan, the host synchronisation that sizes the output, write launch) */
    uint32_t reserved;
} hg_parts_result_t;
int hg_scan_device_parts(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, uint64_t line_base,
                         void *stream, hg_scan_result_t *result, hg_parts_result_t *parts);
/* Copy the last scan's first `max` parts (and their expression indices, if pattern != NULL) to host memory; none after a
 * scan without parts. */
int hg_copy_parts(hg_scanner_t *scanner, hg_part_t *parts, uint32_t *pattern, uint64_t max);
/* The same (16-byte records only) into a DEVICE buffer, asynchronously on `stream`. */
int hg_copy_parts_device(hg_scanner_t *scanner, void *d_dst, uint64_t max, void *stream);

/* Many files in one scan (grep -r): hg_scan_device (invert == 0) or hg_scan_device_invert (invert != 0) of a buffer that
 * holds many files one after the other, with per-file results.
 * Packing rule.  Segment s is the bytes [seg_start[s], seg_end[s]) of the buffer: seg_start[s] is the offset of the file's
 * first byte, seg_end[s] the offset just past its own content, seg_end[s] <= seg_start[s + 1]; equal neighbours are empty
 * files.  A file whose content is empty or ends in '\n' is packed as it is.  A file whose last line is unterminated is
 * followed by the two pad bytes "\0\n", which are not content: a piece's scanned bytes run from after its leading NULs to its
 * first NUL (hg_scan_device_invert above), so the last line's scanned bytes, and what $, \z and \Z see, are those of the file
 * scanned alone; the '\n' ends the line, so no piece spans two files.  Every seg_start[s] > 0 therefore follows a '\n'.
 * Phantom rule.  The pad can make a piece of its own (a last line of k * (buffer_size - 1) bytes leaves "\0\n", one of
 * k * (buffer_size - 1) - 1 bytes leaves "\n" one byte past the content, which may even match).  A piece that starts at or
 * after seg_end[s], and a hit whose hg_hit_aux_t.start is at or after seg_end[s], belongs to no file: it is dropped, it is
 * not counted in the segment's n_lines and it does not count against the limit.
 * Equivalence.  For every segment s, the records with segment s are those of a scan of the bytes [seg_start[s], seg_end[s])
 * alone with line_base = 0 (hg_scan_device, or hg_scan_device_invert when invert != 0), as hg_copy_hits and
 * hg_copy_hit_starts give them: line_number counts from the file's first piece, hg_hit_aux_t.start from its first byte.
 * n_lines[s] is that scan's n_lines, n_selected[s] the distinct line_number values among the segment's records.
 * With max_per_segment = m > 0 a segment keeps its records up to and including the line on which its running record count
 * reaches m (hyperscan()'s max_match_count rule, per file; an inverted record is one piece), and first_record / n_selected
 * describe what is kept.  An inverted call removes the hits that lie in a pad before it
 * selects: a last piece of NULs only, whose scanned bytes are the pad's "\n", is selected with len == 0 as the file alone
 * has it, whatever the expressions match.
 * `result` is filled as by the underlying call, except that n_hits, d_hits and d_aux describe the surviving records, in
 * segment order; n_lines, n_candidates and n_raw_hits stay those of the packed scan.  hg_copy_hits, hg_copy_hits_device and
 * hg_copy_hit_starts follow the surviving records.
 * HG_ERR_ARG, with nothing scanned: segments that are not ascending or overlap, a seg_end[s] past nbytes, a seg_start[s] > 0
 * whose preceding byte is not '\n'.  The arrays are checked on the device; they are never copied to the host.
 * The stage runs on the GPU around the scan (hypergrep_amd/csrc/hg_segments.hip): the check, then behind the scan the
 * segments' line bases from the scan's line geometry (one wavefront per 16 KiB tile that holds a boundary, however many),
 * each segment's run of surviving records, an exclusive scan, and one ordered write. */
typedef struct hg_segments {
    const uint64_t *d_seg_start, *d_seg_end; /* DEVICE arrays, n_seg ascending entries each */
    uint32_t n_seg;
    uint64_t max_per_segment; /* 0 = no limit */
} hg_segments_t;
typedef struct hg_segment_result {
    const uint32_t *d_record_segment; /* DEVICE pointers, valid until the next scan: the segment of each record of `result` */
    const uint64_t *d_first_record;   /* n_seg + 1: segment s owns the records [first_record[s], first_record[s + 1]) */
    const uint64_t *d_n_lines, *d_n_selected; /* n_seg each */
    uint32_t segments_us; /* the added stage (its launches, scan and host synchronisations) */
    uint32_t reserved;
} hg_segment_result_t;
int hg_scan_device_segments(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, void *stream,
                            const hg_segments_t *segments, int invert, hg_scan_result_t *result,
                            hg_segment_result_t *segment_result);
/* Copy the last scan's per-segment arrays to host memory (any pointer may be NULL): record_segment holds result.n_hits
 * entries, first_record n_seg + 1, n_lines and n_selected n_seg.  HG_ERR_ARG after a scan without segments. */
int hg_copy_segments(hg_scanner_t *scanner, uint32_t *record_segment, uint64_t *first_record, uint64_t *n_lines,
                     uint64_t *n_selected);

/* Context lines of many files in one scan (grep -r -A / -B / -C): hg_scan_device_segments with `before` and `after` line
 * pieces of context around every record a segment keeps, per file.  `result` and `segment_result` are filled exactly as
 * hg_scan_device_segments fills them: the same records, order, first_record, n_lines and n_selected.  In `context_result`,
 * n_context, d_ctx_hits and d_ctx_aux describe the context records of all segments, in segment order and then line order;
 * n_tail = 0 and owed_after = 0: a pack has no carry and no tail, because nothing chains across files (a single file scanned
 * in chunks stays on hg_scan_device_context).  hg_copy_context and hg_copy_context_device work unchanged on these records;
 * hg_copy_segment_context gives each context record's segment and the per-segment offsets.
 * Contract.  For every segment s, the context records with segment s are those that hg_scan_device_context gives for the
 * bytes [seg_start[s], seg_end[s]) scanned alone with line_base = 0, carry_after = 0, no tail flag, and the same before, after
 * and invert: line_number counts from the file's first piece, hg_hit_aux_t.start from its first byte.  In particular:
 *  - Context never crosses a file boundary.  A match in the last line of file s gives no after-context in file s + 1; a match
 *    in the first line of file s + 1 gives no before-context in file s.
 *  - A phantom piece (one that starts at or after seg_end[s]) is never a context record.
 *  - A file's last piece of NULs only is the file's own piece: its scanned bytes begin in the pad, and a hit there has been
 *    dropped, so it may be context.  Its record has start = seg_end[s] - seg_start[s] and len = 0, as the inverted records of
 *    hg_scan_device_segments have.
 *  - With max_per_segment = m > 0 the matching lines are the KEPT records.  The after-context of the last kept line goes out
 *    up to `after` pieces and ends before the next matching piece of that file, which is the first record the limit removed
 *    (hg_hyperscan_context's rule, GNU grep up to 3.4, per file).  Nothing behind that piece is context, and the removed
 *    records give no before-context.
 *  - before == after == 0 makes the call equal to hg_scan_device_segments: n_context = 0, context_us = 0, the stage skipped.
 *  - Malformed segments give HG_ERR_ARG with nothing scanned, as for hg_scan_device_segments.
 * The stage runs on the GPU behind the segment stage (hypergrep_amd/csrc/hg_segctx.hip): one window of piece numbers per
 * segment, per-tile counts from the kept records' lines and the windows alone (no text read), their exclusive scan, one
 * ordered write pass over the tiles that hold context, and the records made file-relative.  No sort, no per-record atomic. */
int hg_scan_device_segments_context(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, void *stream,
                                    const hg_segments_t *segments, uint32_t before, uint32_t after, int invert,
                                    hg_scan_result_t *result, hg_segment_result_t *segment_result,
                                    hg_context_result_t *context_result);
/* Copy the last scan's per-segment context arrays to host memory (either pointer may be NULL): context_segment holds
 * context_result.n_context entries, first_context n_seg + 1 (segment s owns the context records [first_context[s],
 * first_context[s + 1])).  HG_ERR_ARG after a scan of any other kind. */
int hg_copy_segment_context(hg_scanner_t *scanner, uint32_t *context_segment, uint64_t *first_context);

/* Matched parts of many files in one scan (grep -r -o): hg_scan_device_segments (invert == 0) with the matched parts of every
 * line piece a segment keeps a record of, per file.  `result` and `segment_result` are filled exactly as
 * hg_scan_device_segments(..., invert = 0, ...) fills them: the same records, order, first_record, n_lines, n_selected and
 * starts of match.  `parts` is hg_scan_device_parts' struct over the parts of all segments, in (segment, line_number, from)
 * order; hg_copy_parts and hg_copy_parts_device work unchanged on them.  `segment_parts` and hg_copy_segment_parts give each
 * part's segment and the per-segment offsets.  parts_us is this stage alone.
 * Equivalence.  For every segment s, the parts with segment s are those hg_scan_device_parts gives for the bytes
 * [seg_start[s], seg_end[s]) scanned alone with line_base = 0, restricted to the lines of the records the segment keeps:
 * line_number counts from the file's first piece, from / to lie inside the piece's scanned bytes, `pattern` is the
 * expression index.  With max_per_segment = 0 the restriction removes nothing.  In particular:
 *  - A hit that the phantom rule or the pad rule dropped heads no piece: the pad's "\n" under an expression that matches a
 *    bare newline, and a last piece of NULs only, have no part.
 *  - With max_per_segment = m > 0 the lines behind the limit have no parts; the line on which the count reaches m has all of
 *    its parts.
 *  - An unterminated last line has the parts the file alone has: $, \z and \Z see the file's end, not the pad.
 *  - A piece is named by (segment, line_number): two files whose matching lines have the same file-relative number stay two
 *    pieces (every one-line file's line is line 0).
 * HG_ERR_ARG, with nothing scanned and the reason in hg_scanner_error: a database hg_scan_device_parts refuses, and malformed
 * segments as for hg_scan_device_segments.  There is no invert argument (a line without a match has no part), and context
 * stays uncombined: parts with invert and parts with context remain refused.
 * The stage runs on the GPU behind the segment stage (hypergrep_amd/csrc/hg_segparts.hip) directly on the surviving,
 * file-relative records: a wavefront per record that is the first of its (segment, line) walks the piece at
 * seg_start[segment] + start (64-bit offsets) with the parts stage's walk; per-record counts, their exclusive scan, a write
 * pass that stores each part with its segment, and first_part[s] = pos[first_record[s]].  No packed copy of the records, no
 * renumbering pass. */
typedef struct hg_segment_parts_result {
    const uint32_t *d_part_segment; /* DEVICE, valid until the next scan: the segment of each part */
    const uint64_t *d_first_part;   /* n_seg + 1: segment s owns the parts [first_part[s], first_part[s + 1]) */
} hg_segment_parts_result_t;
int hg_scan_device_segments_parts(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, int buffer_size, void *stream,
                                  const hg_segments_t *segments, hg_scan_result_t *result,
                                  hg_segment_result_t *segment_result, hg_parts_result_t *parts,
                                  hg_segment_parts_result_t *segment_parts);
/* Copy the last scan's per-segment parts arrays to host memory (either pointer may be NULL): part_segment holds
 * parts.n_parts entries, first_part n_seg + 1.  HG_ERR_ARG after a scan of any other kind. */
int hg_copy_segment_parts(hg_scanner_t *scanner, uint32_t *part_segment, uint64_t *first_part);

/* The lines themselves: the bytes of every line piece the last scan on this scanner left a record for, gathered on the GPU into
 * one compact, ordered, optionally print-ready DEVICE buffer that goes to the host or to another GPU in a single transfer.  The
 * stage runs after a scan, on that scan's records; it scans nothing and changes nothing about scanning.
 * Entries.  An entry is a distinct (segment, line_number) among the last scan's final records: the hits (several reports on
 * one line give one entry), the selected pieces of an inverted scan, or the surviving records of a scan with segments.  Every
 * hg_scan_device* call is accepted as the last scan; after a scan with parts the hits are used, parts are not gathered (hg_gather_parts below gathers them).
 * Entries come in the records' order.
 * Entry j is the bytes d_bytes[d_entry_off[j], d_entry_off[j + 1]) = [separator][number prefix] body [terminator]:
 *   body        exactly the piece's scanned bytes text[start, start + len) (hg_hit_aux_t); after a scan with segments `start`
 *               counts from seg_start[segment], and the sum is taken in 64 bits.  The segments' d_seg_start array must still
 *               be valid when the gather runs;
 *   terminator  with HG_LINES_TERMINATE, a '\n' where the body does not end in one (len == 0 included);
 *   number      with HG_LINES_NUMBER, the decimal line_number + 1 followed by ':' for a match and '-' for a context or tail
 *               piece (grep -n);
 *   separator   with HG_LINES_SEPARATOR, "--\n" in front of entry j > 0 when its segment differs from that of entry j - 1 or
 *               its line_number is not that entry's + 1 (what grep prints between groups).
 * Context.  With HG_LINES_CONTEXT the last scan's context list (hg_scan_device_context, hg_scan_device_segments_context) is
 * merged in by (segment, line_number); the two lists share no line.  Context records give entries of kind HG_LINE_CONTEXT, tail
 * records (HG_CONTEXT_TAIL) of kind HG_LINE_TAIL, the scan's own records HG_LINE_MATCH.  Without the flag the context list is
 * ignored.
 * The per-entry arrays: d_line_number as in the records (file-relative after a scan with segments), d_kind, and after a scan
 * with segments d_segment and d_first_entry (n_seg + 1: file s owns the entries [first_entry[s], first_entry[s + 1])); both are
 * NULL otherwise.  Zero entries give n_entries = n_bytes = 0 and entry_off[0] = 0.
 * Identity, for flags = 0: n_bytes is the sum of `len` over the distinct pieces and n_entries the distinct (segment,
 * line_number) of the records; after hg_scan_device_invert n_entries = n_hits, the complement identity's second term.
 * HG_ERR_ARG, with nothing launched and the reason in hg_scanner_error: no successful scan on this scanner yet (or the last
 * one failed); d_text or nbytes differ from the last scan's (the scanner remembers them); unknown flag bits; result == NULL.
 * Lifetime.  The result stays valid until the next scan or gather on this scanner.  A gather leaves the scan's own results
 * untouched: hg_copy_hits*, hg_copy_context*, hg_copy_segments, hg_copy_segment_context, hg_copy_parts* and
 * hg_copy_segment_parts work after it as before.  gather_us: the stage in microseconds (HIP events, as invert_us: the host
 * synchronisation that sizes the output included).
 * The stage runs on the GPU (hypergrep_amd/csrc/hg_gather.hip): head flags of the records and their exclusive scan; a pass
 * that gives every head its entry index (a lower bound in the other list: no sort), fields and size; a 64-bit exclusive scan
 * of the sizes; and a copy pass divided by OUTPUT bytes, HG_GATHER_TILE per workgroup, which finds its entries by binary
 * search and writes whole aligned 16-byte words.  One piece of a gigabyte and ten million short lines spread over the chip
 * alike.  The text is read inside the gathered pieces only (whole aligned dwords: never past nbytes rounded up to 4). */
#define HG_LINES_CONTEXT 1u   /* merge the last scan's context list into the output, in line order */
#define HG_LINES_TERMINATE 2u /* every entry ends in '\n': one is appended where the piece's scanned bytes do not end in one */
#define HG_LINES_NUMBER 4u    /* every entry begins with the decimal line_number + 1 and ':' (match) or '-' (context, tail) */
#define HG_LINES_SEPARATOR 8u /* "--\n" in front of entry j > 0 when its segment differs from entry j-1's or its line_number != that one's + 1 */
#define HG_LINE_MATCH 0u
#define HG_LINE_CONTEXT 1u
#define HG_LINE_TAIL 2u
#define HG_GATHER_TILE 16384u /* output bytes per workgroup of the copy pass */
typedef struct hg_lines_result {
    uint64_t n_entries, n_bytes;
    const uint8_t *d_bytes;        /* DEVICE, valid until the next scan or gather on this scanner */
    const uint64_t *d_entry_off;   /* n_entries + 1 */
    const uint64_t *d_line_number; /* as in the records (file-relative after a scan with segments) */
    const uint32_t *d_kind;        /* HG_LINE_* */
    const uint32_t *d_segment;     /* NULL unless the last scan had segments */
    const uint64_t *d_first_entry; /* n_seg + 1, NULL unless segments */
    uint32_t gather_us, reserved;
} hg_lines_result_t;
int hg_gather_lines(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, uint32_t flags, void *stream, hg_lines_result_t *result);
/* Copy the last gather's first max_bytes bytes and the per-entry arrays of its first max_entries entries to host memory (any
 * pointer may be NULL; entry_off receives min(n_entries, max_entries) + 1 values).  HG_ERR_ARG without a gather since the last
 * scan, and for `segment` after a scan without segments. */
int hg_copy_lines(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *entry_off, uint64_t *line_number, uint32_t *kind,
                  uint32_t *segment, uint64_t max_entries);
/* first_entry (n_seg + 1 values) of the last gather; HG_ERR_ARG unless it followed a scan with segments. */
int hg_copy_lines_first(hg_scanner_t *scanner, uint64_t *first_entry);
/* The bytes (the first max_bytes of them) into a DEVICE buffer, asynchronously on `stream`. */
int hg_copy_lines_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream);

/* The matched parts themselves (grep -o -n -b, grep --color): the bytes of every part the last scan with parts on this scanner
 * left a record for, gathered on the GPU into one compact, ordered, optionally print-ready DEVICE buffer that goes to the host
 * or to another GPU in a single transfer.  The stage runs after hg_scan_device_parts or hg_scan_device_segments_parts, on that
 * scan's records; it scans nothing and changes nothing about scanning or about any other stage.
 * Entries.  One entry per part, in the parts' order.  Part q belongs to the piece (segment, line_number); S is the offset of
 * the piece's first scanned byte: hg_hit_aux_t.start of the piece's record, plus seg_start[segment] after a scan with segments
 * (the sum in 64 bits; the segments' d_seg_start array must still be valid when the stage runs); len is that record's len.
 * prev_to is the `to` of the previous part of the same piece, 0 if there is none.
 * Entry q is the bytes d_bytes[d_entry_off[q], d_entry_off[q + 1]):
 *   parts mode (default)       [number][offset] [mark_on] text[S+from, S+to) [mark_off] [terminator]
 *   line mode (HG_PARTS_LINE)  [number][offset] text[S+prev_to, S+from) [mark_on] text[S+from, S+to) [mark_off]
 *                              [ text[S+to, S+len) [terminator] ]
 *                              number and offset on the first part of a piece only, the trailing text and the terminator on
 *                              the last part of a piece only: the entries of a piece, joined, are the whole line with its
 *                              parts marked.
 *   number      with HG_PARTS_NUMBER, the decimal line_number + 1 followed by ':' (grep -n);
 *   offset      with HG_PARTS_BYTE_OFFSET, a 64-bit decimal followed by ':' (grep -b): in parts mode byte_base +
 *               hg_hit_aux_t.start + from, in line mode byte_base + hg_hit_aux_t.start.  After a scan with segments `start` is
 *               file-relative already and byte_base must be 0;
 *   terminator  with HG_PARTS_TERMINATE, one '\n' where the last text byte the entry emitted is not '\n': text[S+to-1] in
 *               parts mode, text[S+len-1] (on the last part only) in line mode;
 *   mark_on, mark_off   0 to HG_PARTS_MARK_MAX bytes each, copied by value when the call is made (grep --color's escapes).
 * The per-entry arrays: d_line_number as in the parts; d_kind, bit 0 HG_PART_FIRST and bit 1 HG_PART_LAST of its piece (both
 * modes); d_pattern the expression index (as d_part_pattern); after a scan with segments d_segment and d_first_entry (n_seg + 1:
 * file s owns the entries [first_entry[s], first_entry[s + 1])), both NULL otherwise.  Zero parts is a success with n_entries =
 * n_bytes = 0 and entry_off[0] = 0.
 * Identities: with flags 0 and no marks n_entries = n_parts and n_bytes is the sum of to - from; HG_PARTS_LINE alone gives the
 * bytes hg_gather_lines gives with flags 0 on the same scan.
 * HG_ERR_ARG, with nothing launched and the reason in hg_scanner_error: no successful scan on this scanner yet (or the last
 * one failed); d_text or nbytes differ from the last scan's; the last scan was not one with parts; unknown flag bits; a mark
 * length above HG_PARTS_MARK_MAX; byte_base != 0 after a scan with segments; params == NULL or result == NULL.
 * Lifetime.  The result stays valid until the next scan or hg_gather_parts on this scanner.  The stage has buffers of its own:
 * the scan's results, a previous hg_gather_lines and a previous hg_count_records stay as they are.  gather_us: the stage in
 * microseconds (HIP events; the host synchronisation that sizes the output included).
 * The stage runs on the GPU (hypergrep_amd/csrc/hg_partlines.hip): an entry pass, a lane per part (a lower bound into the
 * records, first / last from the neighbouring parts, the fields and the 64-bit size); an exclusive scan of the sizes; and a
 * copy pass divided by OUTPUT bytes, HG_GATHER_TILE per workgroup, which finds its entries by binary search and writes whole
 * aligned 16-byte words.  The text is read inside the pieces that have parts only (whole aligned dwords: never past nbytes
 * rounded up to 4). */
#define HG_PARTS_NUMBER 1u      /* the decimal line_number + 1 and ':' in front (line mode: of a piece's first part) */
#define HG_PARTS_BYTE_OFFSET 2u /* the decimal byte offset and ':' in front (line mode: of a piece's first part) */
#define HG_PARTS_TERMINATE 4u   /* a '\n' behind an entry (line mode: a piece's last) whose last text byte is not one */
#define HG_PARTS_LINE 8u        /* line mode: the whole line, its parts between the marks */
#define HG_PART_FIRST 1u
#define HG_PART_LAST 2u
#define HG_PARTS_MARK_MAX 16
typedef struct hg_part_lines_params { /* sizeof 56 */
    uint32_t flags;                   /* HG_PARTS_* */
    uint32_t reserved;
    uint64_t byte_base;               /* added to the offset prefix: the offset of d_text in a larger text */
    uint32_t mark_on_len, mark_off_len;
    uint8_t mark_on[16], mark_off[16];
} hg_part_lines_params_t;
typedef struct hg_part_lines_result { /* sizeof 80 */
    uint64_t n_entries, n_bytes;
    const uint8_t *d_bytes;        /* DEVICE, valid until the next scan or hg_gather_parts on this scanner */
    const uint64_t *d_entry_off;   /* n_entries + 1 */
    const uint64_t *d_line_number; /* as in the parts (file-relative after a scan with segments) */
    const uint32_t *d_kind;        /* HG_PART_FIRST | HG_PART_LAST */
    const uint32_t *d_pattern;     /* expression index of each entry's part */
    const uint32_t *d_segment;     /* NULL unless the last scan had segments */
    const uint64_t *d_first_entry; /* n_seg + 1, NULL unless segments */
    uint32_t gather_us, reserved;
} hg_part_lines_result_t;
int hg_gather_parts(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, const hg_part_lines_params_t *params, void *stream,
                    hg_part_lines_result_t *result);
/* Copy the last parts gather's first max_bytes bytes and the per-entry arrays of its first max_entries entries to host memory
 * (any pointer may be NULL; entry_off receives min(n_entries, max_entries) + 1 values).  HG_ERR_ARG without a parts gather
 * since the last scan, and for `segment` after a scan without segments. */
int hg_copy_part_lines(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *entry_off, uint64_t *line_number, uint32_t *kind,
                       uint32_t *pattern, uint32_t *segment, uint64_t max_entries);
/* first_entry (n_seg + 1 values) of the last parts gather; HG_ERR_ARG unless it followed a scan with segments. */
int hg_copy_part_lines_first(hg_scanner_t *scanner, uint64_t *first_entry);
/* The bytes (the first max_bytes of them) into a DEVICE buffer, asynchronously on `stream`. */
int hg_copy_part_lines_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream);

/* Distinct matched parts and how often each occurs (grep -o | sort | uniq -c): the parts of the last scan with parts on this
 * scanner, grouped by their bytes on the GPU, so that only the distinct values go to the host.  The stage runs after
 * hg_scan_device_parts or hg_scan_device_segments_parts, on that scan's records; it scans nothing and changes nothing about
 * scanning or about any other stage.
 * Value.  The value of part q is text[S + from, S + to), S as for hg_gather_parts: hg_hit_aux_t.start of the record of the
 * part's piece, plus seg_start[segment] after a scan with segments (the segments' d_seg_start array must still be valid).  A
 * part whose piece has no record is not counted (the parts stage never leaves one).
 * Key.  The value's bytes; with HG_VALUES_BY_PATTERN the pair (expression index d_part_pattern[q], bytes).  The segment is
 * never part of the key: after a scan of many files equal values in different files are one group.
 * Per group: count, the number of parts with the key; first, the smallest part index with it; pattern, line_number and
 * segment those of part `first` (without HG_VALUES_BY_PATTERN the pattern is that of the first part only).  Groups are ordered
 * by ascending first; d_bytes holds the values joined in that order, value j being d_bytes[d_off[j], d_off[j + 1]).  Every
 * output is a function of the input alone: two runs give identical arrays.  Zero parts is a success with n_values = 0 and
 * off[0] = 0.
 * params (NULL: all defaults).  hash_bits: 0 means 64; 1 .. 64 cut the hash to that many low bits before any use, which makes
 * distinct keys collide (a knob for tests and experiments: the result is the same, only slower).  table_log2: 0 means the
 * smallest power of two that is at least 2 * n_parts and at least 2^10; an explicit value must satisfy 2^table_log2 > n_parts
 * and be at most 40 (a nearly full table: long probes, same result).
 * HG_ERR_ARG, with nothing launched and the reason in hg_scanner_error: no successful scan on this scanner yet (or the last
 * one failed); d_text or nbytes differ from the last scan's; the last scan was not one with parts; unknown flag bits;
 * hash_bits above 64; table_log2 too small or above 40; scanner == NULL or result == NULL.  HG_ERR_NOMEM when the buffers do
 * not fit (a part costs 44 bytes, a slot 32, a value 72 plus its bytes).
 * Lifetime.  The result stays valid until the next scan or hg_count_values on this scanner.  The stage has buffers of its
 * own: the scan's results, a previous hg_gather_lines, hg_gather_parts and hg_count_records stay as they are.  values_us: the
 * stage in microseconds (HIP events; its two host synchronisations included).
 * The stage runs on the GPU (hypergrep_amd/csrc/hg_values.hip): a hash pass (a lane per part, a wavefront per part longer
 * than 256 bytes), an insert pass into an open-addressing table of 64-bit slots claimed by compare-and-swap, with integer
 * atomics for count and first, a compaction and a sort by first, and the gathers' copy pass divided by output bytes.  Text is
 * read inside the parts only (whole aligned dwords: never past nbytes rounded up to 4).
 * Not offered: case folding, and anything for the databases the parts stage refuses.  Values per file, an order by count and
 * a cut to the most frequent are hg_rank_values' (below); accumulation across scans is hg_accumulate_values' (further below). */
#define HG_VALUES_BY_PATTERN 1u /* the expression index is part of the key */
typedef struct hg_values_params { /* sizeof 16 */
    uint32_t flags;               /* HG_VALUES_* */
    uint32_t hash_bits;           /* 0: 64 */
    uint32_t table_log2;          /* 0: from n_parts */
    uint32_t reserved;
} hg_values_params_t;
typedef struct hg_values_result { /* sizeof 88 */
    uint64_t n_values, n_parts, n_bytes;
    const uint8_t *d_bytes;        /* DEVICE, valid until the next scan or hg_count_values on this scanner */
    const uint64_t *d_off;         /* n_values + 1 */
    const uint64_t *d_count;       /* parts per value */
    const uint64_t *d_first;       /* the smallest part index per value, ascending */
    const uint32_t *d_pattern;     /* expression index of part `first` */
    const uint64_t *d_line_number; /* line_number of part `first` */
    const uint32_t *d_segment;     /* segment of part `first`; NULL unless the last scan had segments */
    uint32_t table_log2, values_us; /* the table the stage used */
} hg_values_result_t;
int hg_count_values(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, const hg_values_params_t *params, void *stream,
                    hg_values_result_t *result);
/* Copy the last value count's first max_bytes bytes and the per-value arrays of its first max_values values to host memory
 * (any pointer may be NULL; off receives min(n_values, max_values) + 1 values).  HG_ERR_ARG without a value count since the
 * last scan (a refused or failed hg_count_values leaves none: the count before it is gone), and for `segment` after a scan
 * without segments. */
int hg_copy_values(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *off, uint64_t *count, uint64_t *first,
                   uint32_t *pattern, uint64_t *line_number, uint32_t *segment, uint64_t max_values);
/* The bytes (the first max_bytes of them) into a DEVICE buffer, asynchronously on `stream`. */
int hg_copy_values_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream);
/* The same for a file: hg_hyperscan_counts' arguments, reader, chunking (256 MiB chunks cut at piece boundaries),
 * decompression and database cache, with the parts stage and the values stage behind every chunk's scan.  Only each chunk's
 * distinct values are downloaded (bytes, offsets, counts, expression indices) and merged on the host by key; no part record
 * and no line leaves the GPU.  There is no max_match_count: the counts describe the whole file.  params as for
 * hg_count_values (NULL: defaults; an explicit table_log2 must serve every chunk's parts).  On success on_values is called
 * once, with the merged groups in the order in which their keys first occur in the file: value j is bytes[off[j], off[j + 1]),
 * pattern[j] the expression index of its first part (part of the key with HG_VALUES_BY_PATTERN).  The pointers are valid
 * during the call only.  Return codes are hg_hyperscan_ext's: a set that does not compile or that the parts stage refuses
 * (HYPERSCANNER_DB) and a file that cannot be opened are answered before any device resource is taken; bad params or
 * on_values == NULL give the code of a bad buffer_count. */
typedef void (*hg_values_event)(void *context, const uint8_t *bytes, const uint64_t *off, const uint64_t *count, const uint32_t *pattern,
                                uint64_t n_values);
int hg_hyperscan_values(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                        const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements,
                        const int buffer_size, const hg_values_params_t *params, hg_values_event on_values, void *context);

/* The matched values ranked by count, per file if asked, and cut to the most frequent on the GPU (grep -o | sort | uniq -c |
 * sort -rn | head): the distinct values of the last scan with parts on this scanner, ordered by count, of which only the kept
 * rows' bytes are gathered and go to the host.  The stage runs after hg_scan_device_parts or hg_scan_device_segments_parts,
 * on that scan's records, as hg_count_values does; it scans nothing and changes nothing about scanning or any other stage.
 * Value.  As for hg_count_values.  A part whose piece has no record is not counted.
 * Key.  The value's bytes; with HG_RANK_BY_PATTERN the pair (expression index, bytes); with HG_RANK_PER_SEGMENT additionally
 * the part's segment, so that equal values in two files are two groups.
 * Per group: count, the number of parts with the key; first, the smallest part index with it; pattern, line_number and
 * segment those of part `first`.
 * Order.  Ascending segment (only with HG_RANK_PER_SEGMENT), then descending count, then ascending first.  first is unique,
 * so the order is total and every output is a function of the input alone: two runs give identical arrays.
 * Cut.  top == 0 keeps every group.  Otherwise the first `top` groups of the whole scan are kept, or the first `top` of every
 * segment with HG_RANK_PER_SEGMENT; a tie in count at the cut is decided by first (the smaller stays).
 * Result.  The kept groups in that order, n_values of them: d_bytes holds their values joined, row j being
 * d_bytes[d_off[j], d_off[j + 1]); d_count, d_first, d_pattern, d_line_number per row, d_segment too unless the last scan had
 * no segments (NULL then).  With HG_RANK_PER_SEGMENT also d_first_value (n_seg + 1: segment s owns the rows
 * [first_value[s], first_value[s + 1]); a file without parts owns an empty range), d_seg_distinct (n_seg: the segment's
 * distinct values before the cut) and d_seg_parts (n_seg: the sum of the segment's groups' counts before the cut, so that a
 * share can be computed from a cut result); all three NULL, and n_seg 0, without the flag.  n_distinct is the number of
 * groups before the cut, n_parts the scan's parts, n_bytes the kept rows' bytes.  Zero parts is a success with n_values = 0.
 * params (NULL: all defaults).  hash_bits and table_log2 mean what they mean in hg_values_params_t.
 * HG_ERR_ARG, with nothing launched and the reason in hg_scanner_error: everything hg_count_values refuses (no successful
 * scan, another text, a scan without parts, hash_bits above 64, table_log2 too small or above 40, scanner == NULL or
 * result == NULL); unknown flag bits; HG_RANK_PER_SEGMENT after a scan without segments.  HG_ERR_NOMEM when the buffers do
 * not fit (a part costs 44 bytes, a slot 32, a group 120, a segment 40, plus the kept rows' bytes; HG_RANK_PER_SEGMENT adds 8
 * bytes a part and 24 a group).
 * Lifetime.  The stage has buffers of its own.  The result stays valid until the next scan or hg_rank_values on this scanner;
 * a refused or failed call leaves no earlier ranking behind.  The scan's results and any earlier hg_count_values,
 * hg_gather_lines, hg_gather_parts or hg_count_records stay as they are.  rank_us: the stage in microseconds (HIP events; its
 * host synchronisations included).
 * The stage runs on the GPU: the values stage's hash, insert and compaction passes with the segment as a third key component
 * (hypergrep_amd/csrc/hg_values.hip), two stable radix sorts, and the kernels of hypergrep_amd/csrc/hg_rank.hip (a lane per
 * group or per segment; no atomics, no text reads), then the gathers' copy pass over the kept rows.
 * Not offered: case folding, a tie-break by value bytes, ranking across GPUs.  Accumulation across scans is
 * hg_accumulate_values' (below). */
#define HG_RANK_BY_PATTERN 1u  /* the expression index is part of the key */
#define HG_RANK_PER_SEGMENT 2u /* the segment is part of the key; order and cut are per segment */
typedef struct hg_rank_params { /* sizeof 24 */
    uint32_t flags;             /* HG_RANK_* */
    uint32_t hash_bits;         /* 0: 64 */
    uint32_t table_log2;        /* 0: from n_parts */
    uint32_t reserved;
    uint64_t top;               /* 0: no cut */
} hg_rank_params_t;
typedef struct hg_rank_result { /* sizeof 128 */
    uint64_t n_values, n_distinct, n_parts, n_bytes;
    const uint8_t *d_bytes;         /* DEVICE, valid until the next scan or hg_rank_values on this scanner */
    const uint64_t *d_off;          /* n_values + 1 */
    const uint64_t *d_count;        /* parts per row */
    const uint64_t *d_first;        /* the smallest part index per row */
    const uint32_t *d_pattern;      /* expression index of part `first` */
    const uint64_t *d_line_number;  /* line_number of part `first` */
    const uint32_t *d_segment;      /* segment of part `first`; NULL unless the last scan had segments */
    const uint64_t *d_first_value;  /* n_seg + 1; NULL without HG_RANK_PER_SEGMENT, as the next two */
    const uint64_t *d_seg_distinct; /* n_seg */
    const uint64_t *d_seg_parts;    /* n_seg */
    uint32_t n_seg, table_log2, rank_us, reserved;
} hg_rank_result_t;
int hg_rank_values(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, const hg_rank_params_t *params, void *stream,
                   hg_rank_result_t *result);
/* Copy the last ranking's first max_bytes bytes and the per-row arrays of its first max_values rows to host memory (any
 * pointer may be NULL; off receives min(n_values, max_values) + 1 values).  HG_ERR_ARG without a ranking since the last scan,
 * and for `segment` after a scan without segments. */
int hg_copy_ranked_values(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *off, uint64_t *count, uint64_t *first,
                          uint32_t *pattern, uint64_t *line_number, uint32_t *segment, uint64_t max_values);
/* first_value (n_seg + 1 values), seg_distinct and seg_parts (n_seg each) of the last ranking (any pointer may be NULL);
 * HG_ERR_ARG unless it was one with HG_RANK_PER_SEGMENT. */
int hg_copy_ranked_segments(hg_scanner_t *scanner, uint64_t *first_value, uint64_t *seg_distinct, uint64_t *seg_parts);
/* The bytes (the first max_bytes of them) into a DEVICE buffer, asynchronously on `stream`. */
int hg_copy_ranked_values_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream);
/* The same for many files in one call: hg_hyperscan_files_parts' arguments, reader and packing (small plain files share one
 * buffer and one GPU scan), with the parts stage and the rank stage behind every pack's scan, the latter with
 * HG_RANK_PER_SEGMENT and params->top (params->flags may carry HG_RANK_BY_PATTERN only; NULL: defaults).  Only the kept rows
 * are downloaded (bytes, offsets, counts, expression indices) and three numbers per file; no part record and no line leaves the
 * GPU.  on_file is called once per file, in file order: row j of the file is bytes[off[j], off[j + 1]) (off[0] need not be 0),
 * with count[j] and pattern[j]; n_values rows are kept of the file's n_distinct values, n_parts is the sum of the counts of all
 * of them (before the cut).  A file without parts and a file that cannot be opened are called too, with zero rows; the latter
 * has its own rc in `summaries`.  The pointers are valid during the call only.  Files of the per-file route (gzip, zstd, larger
 * than a pack, every file when buffer_size < 2) go through hg_hyperscan_values' chunk merge inside the call, and the host
 * applies the same order (count descending, then first occurrence in the file) and the same cut: a file's rows do not depend
 * on the route it took.  summaries as for hg_hyperscan_files_parts (n_selected is 0 for a file of the per-file route).  Return
 * codes and early refusals are hg_hyperscan_files_parts' and hg_hyperscan_values': bad params or on_file == NULL give the code
 * of a bad buffer_count. */
typedef void (*hg_file_values_event)(void *context, unsigned int file_index, const uint8_t *bytes, const uint64_t *off, const uint64_t *count,
                                     const uint32_t *pattern, uint64_t n_values, uint64_t n_distinct, uint64_t n_parts);
int hg_hyperscan_files_values(const char *const *file_names, unsigned int n_files, const char *const *patterns,
                              const unsigned int *pattern_flags, const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext,
                              const unsigned int elements, const int buffer_size, const hg_rank_params_t *params,
                              hg_file_values_event on_file, void *context, hg_file_summary_t *summaries);

/* Matched values accumulated across scans, with a cut to the most frequent (grep -o | sort | uniq -c | sort -rn | head over a
 * text that arrives in many buffers): a value store on the scanner, a device-resident table of distinct values that survives
 * scans.  hg_accumulate_values adds the parts of the last scan with parts (hg_scan_device_parts or
 * hg_scan_device_segments_parts); hg_rank_accumulated orders the store and cuts it, so that only the kept rows go to the host.
 * Definition.  Let the accumulated calls since the last reset be 1 .. k and P their scans' parts, one list after the other; a
 * part's ordinal is the number of parts of the earlier calls plus its index in its own call.  The store's groups are the groups
 * hg_count_values defines over P, by its Value and Key rules: a part whose piece has no record is not counted, the segment is
 * never in the key, the expression index is with HG_ACC_BY_PATTERN.  Per group: count, the number of parts in it; first, the
 * smallest ordinal in it; pattern and line_number those of part `first` (the caller chains line_base across buffers, as for
 * counts).  A scan that is accumulated twice counts twice.  Every output is a function of the inputs alone.
 * Cut identity.  A text cut at piece boundaries into buffers that are scanned in order with chained line_base and accumulated one
 * by one leaves the store the whole text accumulated once leaves: every array of every ranking is equal, first included.
 * Rank.  hg_rank_accumulated orders the groups by descending count, then ascending first (with HG_ACC_ORDER_FIRST by ascending
 * first only) and keeps the first `top` (0: all).  Only the kept rows' bytes are gathered: row j is d_bytes[d_off[j],
 * d_off[j + 1]).  n_distinct is the number of groups before the cut, n_parts the parts of all accumulated calls (counted or
 * not), n_bytes the kept rows' bytes.  The result stays valid until the next hg_accumulate_values, hg_rank_accumulated or
 * hg_reset_accumulated on the scanner; scans do not disturb it, and it changes nothing in the store.
 * params (NULL: all defaults).  hash_bits and table_log2 mean what they mean in hg_values_params_t and govern the call's own
 * grouping.  store_log2 == 0 lets the store's table grow on its own: the smallest power of two that is at least twice the
 * distinct values and at least 2^10, never smaller than before.  An explicit store_log2 fixes the table size (for tests); if it
 * does not hold the values with one slot to spare the call returns HG_ERR_NOMEM.  HG_ACC_BY_PATTERN and hash_bits are fixed
 * when a store begins: a call that differs from them without HG_ACC_RESET is refused.  HG_ACC_RESET empties the store first.
 * HG_ERR_ARG, with nothing launched and the reason in hg_scanner_error: everything hg_count_values refuses; unknown flag bits;
 * an explicit store_log2 above 40; a changed HG_ACC_BY_PATTERN or hash_bits without HG_ACC_RESET; a rank or copy call with no
 * accumulation since the last reset (for the copies also: no ranking since the last accumulation).
 * Atomicity.  A refused call and a call that runs out of memory leave the store exactly as it was, HG_ACC_RESET or not.  A
 * HIP error (HG_ERR_HIP) behind that point leaves it empty, as after hg_reset_accumulated, and says so.
 * Isolation.  The store has buffers of its own, a values stage of its own among them: the scan's results and an earlier
 * hg_count_values, hg_rank_values, gather or count stay as they are.
 * The stage runs on the GPU (hypergrep_amd/csrc/hg_valstore.hip): hg_count_values' grouping of the call's parts, a read-only
 * lookup of every group in the store's table (a lane per group, a wavefront per value longer than 256 bytes; the text against
 * the store's byte arena by whole aligned dwords of both), two scans that size the new values, a rehash when the table grows,
 * an apply pass (a found group adds its count, a new one claims a slot by compare-and-swap) and the gathers' copy pass from
 * the text to the arena; a ranking is one stable radix sort, a place pass and the copy pass over the kept rows.  acc_us and
 * rank_us: the calls in microseconds (HIP events; their host synchronisations included).
 * Not offered: per-segment keys in the store, case folding, ranking across GPUs. */
#define HG_ACC_BY_PATTERN 1u   /* the expression index is part of the key */
#define HG_ACC_RESET 2u        /* empty the store first */
#define HG_ACC_ORDER_FIRST 1u  /* hg_rank_accumulated: keep the store's order, which is first occurrence */
typedef struct hg_acc_params { /* sizeof 16 */
    uint32_t flags;            /* HG_ACC_BY_PATTERN, HG_ACC_RESET */
    uint32_t hash_bits;        /* 0: 64 */
    uint32_t table_log2;       /* 0: from the call's parts */
    uint32_t store_log2;       /* 0: from the store's distinct values */
} hg_acc_params_t;
typedef struct hg_acc_result { /* sizeof 56 */
    uint64_t n_distinct;       /* the store's distinct values after the call */
    uint64_t n_added;          /* of them new with this call */
    uint64_t n_groups;         /* this call's groups */
    uint64_t n_parts;          /* this call's parts */
    uint64_t n_parts_total;    /* the parts accumulated so far */
    uint64_t n_bytes;          /* the bytes of the store's values */
    uint32_t store_log2, acc_us; /* the table the store has now */
} hg_acc_result_t;
typedef struct hg_acc_rank_result { /* sizeof 88 */
    uint64_t n_values, n_distinct, n_parts, n_bytes;
    const uint8_t *d_bytes;        /* DEVICE, valid until the next accumulate, rank or reset on this scanner */
    const uint64_t *d_off;         /* n_values + 1 */
    const uint64_t *d_count;       /* parts per row */
    const uint64_t *d_first;       /* the smallest ordinal per row */
    const uint32_t *d_pattern;     /* expression index of part `first` */
    const uint64_t *d_line_number; /* line_number of part `first` */
    uint32_t store_log2, rank_us;
} hg_acc_rank_result_t;
int hg_accumulate_values(hg_scanner_t *scanner, const void *d_text, uint64_t nbytes, const hg_acc_params_t *params, void *stream,
                         hg_acc_result_t *result);
int hg_rank_accumulated(hg_scanner_t *scanner, uint64_t top, uint32_t flags, void *stream, hg_acc_rank_result_t *result);
/* Copy the last ranking's first max_bytes bytes and the per-row arrays of its first max_values rows to host memory (any pointer
 * may be NULL; off receives min(n_values, max_values) + 1 values). */
int hg_copy_accumulated(hg_scanner_t *scanner, uint8_t *bytes, uint64_t max_bytes, uint64_t *off, uint64_t *count, uint64_t *first,
                        uint32_t *pattern, uint64_t *line_number, uint64_t max_values);
/* The bytes (the first max_bytes of them) into a DEVICE buffer, asynchronously on `stream`. */
int hg_copy_accumulated_device(hg_scanner_t *scanner, void *d_dst, uint64_t max_bytes, void *stream);
/* Empty the store (its buffers stay with the scanner).  HG_ERR_ARG for scanner == NULL only. */
int hg_reset_accumulated(hg_scanner_t *scanner);
/* hg_hyperscan_values with the store behind every chunk's scan and one ranking at the end: its arguments, reader, chunking,
 * decompression and database cache, plus `top` (0: all).  Every chunk's parts are accumulated where they lie; on success
 * on_values is called once, with the kept rows by (count descending, first occurrence in the file).  *n_distinct and *n_parts
 * (either may be NULL) receive the file's distinct values and its parts, both before the cut (two out-pointers, so that the
 * callback keeps hg_values_event's signature).  No part record, no line and no
 * per-chunk value list leaves the GPU.  Return codes and early refusals are hg_hyperscan_values'. */
int hg_hyperscan_values_top(char *file_name, const char *const *patterns, const unsigned int *pattern_flags,
                            const unsigned int *pattern_ids, const hs_expr_ext_t *const *ext, const unsigned int elements,
                            const int buffer_size, const hg_values_params_t *params, uint64_t top, hg_values_event on_values,
                            void *context, uint64_t *n_distinct, uint64_t *n_parts);

/* Counts per report id (hg_count_records): which expressions fired, and on how many lines, without moving the record list.
 * Bins.  A bin is a distinct report id of the database, in ascending id order (hg_db_report_ids; n_bins <= n_patterns).
 * Expressions that share an id share a bin; the id of a combination is a bin; the id of a QUIET expression is a bin that
 * always stays 0, because QUIET reports are never delivered.
 * Definition.  Take the records of the last scan on the scanner: the final hits, or the surviving records of a scan with
 * segments (context lists and parts are ignored).  For bin b with id v, n_reports[b] is the number of records with id == v and
 * n_lines[b] the number of distinct (segment, line_number) among them.  By the records' order, (segment, line_number, id,
 * to), a record counts as a new line for its bin iff it is record 0 or differs from the record before it in segment,
 * line_number or id.
 * HG_COUNTS_ACCUMULATE adds to the totals already on the scanner instead of zeroing them first: buffers of one text that are
 * cut at piece boundaries never share a line piece, so the sums of a chained scan are the counts of the whole text.  The first
 * call after hg_scanner_create starts from zero either way.  HG_COUNTS_PER_SEGMENT, only after a scan with segments, also
 * fills two row-major n_seg x n_bins uint32_t matrices, lines and reports per file (a pack is at most 256 MiB, so 32 bits
 * suffice); they are never accumulated, each call overwrites them; n_seg * n_bins above 2^28 cells is HG_ERR_ARG.
 * HG_ERR_ARG, with nothing launched and the reason in hg_scanner_error: no successful scan on this scanner yet; the last scan
 * was inverted (its records carry HG_ID_INVERT and no expression); unknown flag bits; HG_COUNTS_PER_SEGMENT after a scan
 * without segments; result == NULL.
 * Zero records is a success with all-zero counts.  The stage leaves the scan's own results and a previous gather untouched,
 * and every hg_copy_* works after it as before.  All sizes are known before the launch; the call blocks once, at the end.
 * counts_us: the stage in microseconds (HIP events).
 * The stage is one kernel (hypergrep_amd/csrc/hg_counts.hip): a workgroup per run of records counts in LDS up to
 * HG_COUNTS_LDS_BINS bins (in memory above), a wave that agrees on one bin adds once, and integer atomics make the result
 * exact whatever the order.  Only the 16-byte hit records are read. */
#define HG_COUNTS_ACCUMULATE 1u
#define HG_COUNTS_PER_SEGMENT 2u
#define HG_COUNTS_LDS_BINS 4096u /* up to this many bins a workgroup counts in LDS */
typedef struct hg_counts_result { /* sizeof 64 */
    uint32_t n_bins, n_seg;       /* n_seg 0 without HG_COUNTS_PER_SEGMENT */
    uint64_t n_records;           /* records this call counted */
    const uint32_t *d_ids;        /* DEVICE, n_bins ascending; valid until the next scan or count */
    const uint64_t *d_n_lines, *d_n_reports;     /* n_bins totals (accumulated with the flag) */
    const uint32_t *d_seg_lines, *d_seg_reports; /* n_seg x n_bins, NULL without the flag */
    uint32_t counts_us, reserved;
} hg_counts_result_t;
int hg_count_records(hg_scanner_t *scanner, uint32_t flags, void *stream, hg_counts_result_t *result);
/* The bins and totals of the last count (the first min(n_bins, max_bins) of them; any pointer may be NULL) to host memory.
 * HG_ERR_ARG without a count on this scanner. */
int hg_copy_counts(hg_scanner_t *scanner, uint32_t *ids, uint64_t *n_lines, uint64_t *n_reports, uint32_t max_bins);
/* Rows [first_seg, first_seg + n) of the last count's matrices (n x n_bins values each; either pointer may be NULL).
 * HG_ERR_ARG unless the last count had HG_COUNTS_PER_SEGMENT and no scan followed it, or when the rows are out of range. */
int hg_copy_segment_counts(hg_scanner_t *scanner, uint32_t *seg_lines, uint32_t *seg_reports, uint32_t first_seg, uint32_t n);
/* host only, needs no GPU: the bins of a compiled database (the first min(max, *n_bins) ids; ids may be NULL) */
int hg_db_report_ids(const hg_database_t *db, uint32_t *ids, uint32_t max, uint32_t *n_bins);

/* Copy the last scan's first `max` hits (and aux records, if aux != NULL) to host memory. */
int hg_copy_hits(hg_scanner_t *scanner, hg_hit_t *hits, hg_hit_aux_t *aux, uint64_t max);

/* Copy the last scan's first `max` hit records (16 B each) into another DEVICE buffer, asynchronously on
 * `stream` (e.g. a tensor that is then sent over RCCL). */
int hg_copy_hits_device(hg_scanner_t *scanner, void *d_dst, uint64_t max, void *stream);

/* Start of match of the last scan's first `max` hits, one uint32_t per hit in hit order, the same origin as `to`
 * (offsets inside the scanned bytes, i.e. relative to hg_hit_aux_t.start).  Hits of expressions compiled with
 * HS_FLAG_SOM_LEFTMOST carry the leftmost start of their match; all others 0.  The starts are computed by a pass that runs
 * after the hits are final, only when the database has SOM expressions (hg_scan_device then includes it). */
int hg_copy_hit_starts(hg_scanner_t *scanner, uint32_t *from, uint64_t max);
/* The same into a DEVICE buffer, asynchronously on `stream`. */
int hg_copy_hit_starts_device(hg_scanner_t *scanner, void *d_dst, uint64_t max, void *stream);

/* Deterministic synthetic log used by bench.py and the parity tests: writes nbytes at d_text (device)
 * or text (host) from the same counter-based generator; see hypergrep_amd/csrc/hg_synth.h. */
typedef struct hg_synth_spec {
    uint64_t seed;
    uint64_t first_block;    /* index of the first 64 KiB block (shard offset) */
    uint32_t hit_per_million; /* probability that a line carries a needle, in 1e-6 units */
    uint32_t n_needles;
    const uint8_t *needles;       /* n_needles strings, concatenated */
    const uint32_t *needle_off;   /* n_needles + 1 offsets into needles */
} hg_synth_spec_t;
int hg_synth_device(void *d_text, uint64_t nbytes, const hg_synth_spec_t *spec, int device, void *stream);
int hg_synth_host(uint8_t *text, uint64_t nbytes, const hg_synth_spec_t *spec);

/* ---- diagnostics (tests, tools) ------------------------------------------------------------------------------------
 * A device buffer of `nbytes` (rounded up to 16) whose end is followed by reserved, unmapped address space: a read or
 * write past it is a GPU memory fault instead of a silent pass.  The parity tests run on such buffers so that an
 * over-read in any kernel fails where it happens.  hg_debug_upload / hg_debug_download: blocking copies to / from it. */
int hg_debug_alloc_guarded(uint64_t nbytes, int device, void **d_ptr, void **guard_handle);
void hg_debug_free_guarded(void *guard_handle);
int hg_debug_upload(void *d_dst, const void *src, uint64_t nbytes);
int hg_debug_download(void *dst, const void *d_src, uint64_t nbytes);
/* What the finalize stage of the scanner's last pass did (the last segment's pass, for a buffer scanned in segments), for
 * tests that must know which of its paths ran.  The host notes it while it plans and queues a pass: a scan launches and
 * copies nothing for it.  path: how the reports were ordered; fin_shift / fin_nb / fin_cap: buckets of 2^fin_shift text bytes
 * by line start, their number, the records each may hold; id_bits / to_bits: the key fields' widths.  fill (may be NULL)
 * receives the raw reports of the first min(max_fill, fin_nb) buckets, copied from the device when the call is made, and
 * info->n_fill their number (0 unless the last pass was bucketed). */
#define HG_FIN_PATH_NONE 0u           /* no pass yet */
#define HG_FIN_PATH_BUCKETED 1u       /* every bucket ordered on its own */
#define HG_FIN_PATH_COMPACT_PACKED 2u /* compact array, one sort of a packed 64-bit key */
#define HG_FIN_PATH_COMPACT_WIDE 3u   /* compact array, two sorts: (id, to), then line */
typedef struct hg_finalize_info {
    uint32_t path;
    uint32_t fin_shift, fin_nb, fin_cap, id_bits, to_bits;
    uint32_t early_buckets; /* buckets finalized before the last pipeline chunk's side passes were through (the early range) */
    uint32_t early_beside_stream; /* ... those of them finalized beside the last stream launch, in front of its joiner */
    uint32_t scan_blocks;   /* blocks the position scan used for the pass's largest bucket range */
    uint32_t left_bucketed; /* the scanner has left bucketed emission: its later passes are compact */
    uint32_t n_fill;
    uint32_t reserved;
} hg_finalize_info_t;
int hg_debug_finalize_info(hg_scanner_t *scanner, hg_finalize_info_t *info, uint32_t *fill, uint32_t max_fill);
/* Face B bookkeeping, for tests and HYPERGREP_TRACE: the device the next scan context would be created on for a node of
 * `ndev` GPUs (HYPERGREP_DEVICE pins one, otherwise files round-robin; advances the round-robin), and the cache counters
 * {database cache hits, misses, entries, window tunings, contexts created, reused, re-bound to another pattern set, alive}. */
int hg_faceb_next_device(int ndev);
void hg_faceb_stats(uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
