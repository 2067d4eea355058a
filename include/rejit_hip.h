/* include/rejit_hip.h -- the C ABI of librejit_hip.so: the drop-in boundary between a
 * host program and the MI355X kernels.
 *
 * In the reference the boundary is a set of raw function pointers into JIT-generated x86
 * code, one per match type (src/regexp.h:533-536):
 *
 *     bool     (*MatchFullFunc)    (const char* text, size_t size);
 *     bool     (*MatchAnywhereFunc)(const char* text, size_t size);
 *     bool     (*MatchFirstFunc)   (const char* text, size_t size, Match*);
 *     unsigned (*MatchAllFunc)     (const char* text, size_t size, std::vector<Match>*);
 *
 * produced by Regej::Compile (src/rejit.cc:229-267) and called by Regej::Match*
 * (src/rejit.cc:150-208).  The entry points below replace exactly those: rj_compile takes
 * the place of Parser::Parse + Codegen::Compile, rj_match_* of the four generated
 * functions.  Offsets are returned instead of pointers (the C++ wrapper in
 * include/rejit.h converts).  Plain C types only; no HIP or torch types in signatures
 * (streams are passed as void*).
 *
 * Errors never throw and never abort: every call returns a negative rj_status and
 * rj_last_error() holds a message (thread-local).
 */
#ifndef REJIT_HIP_H_
#define REJIT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  RJ_OK = 0,
  RJ_PARSER_ERROR = -1,  /* == rejit::ParserError, include/rejit.h:98-102 of the reference */
  RJ_TOO_LARGE = -2,     /* pattern expands beyond the device automaton limits */
  RJ_DEVICE_ERROR = -3,  /* HIP failure (no GPU, out of memory, launch error, ...) */
  RJ_BAD_ARGUMENT = -4
} rj_status;

typedef struct rj_program rj_program; /* a compiled pattern: immutable, shareable across threads */
typedef struct rj_scan rj_scan;       /* per-caller device scratch + results; NOT thread-safe   */

typedef struct {
  int32_t n_positions;     /* automaton positions (one per pattern byte)            */
  int32_t n_words;         /* 32-bit words of automaton state                       */
  int32_t has_assertions;  /* pattern contains ^ or $                               */
  int32_t scan_mode;       /* 0 dense (every position), 1 fast-forward windows       */
  int32_t n_windows;       /* number of 4-byte window constants                     */
  uint32_t window_offset;  /* byte offset of the windows inside a match             */
  uint32_t window_len;     /* bytes compared per window                             */
  uint64_t min_len;        /* shortest match                                         */
  uint64_t max_len;        /* longest match, UINT64_MAX when unbounded               */
  int32_t ring_artefact_risk; /* 1: the reference's answer on this pattern can depend on its ring artefact (DESIGN.md
                              * section 6).  A RANGE of such a pattern (rj_scan_run with own_begin / own_end) owns the whole
                              * segments between synchronisation points, [first point >= own_begin, first point >= own_end),
                              * and takes the text buffer to be the WHOLE text: give every rank the text up to its end
                              * (rejit_amd/sharding.py: visible_range(..., whole_text=True)), not a fixed halo.
                              * Where the artefact can apply (a candidate begins where another ends) and no exact replay can
                              * take the call, the call fails with RJ_TOO_LARGE and rj_last_error() names the ring artefact and
                              * the limit: the answer is the reference's or none, never the documented semantics in its place.
                              * The limits are budgets of one-lane work (rejit_amd/csrc/engine_internal.h): about 2.4 s for
                              * automata of more than 1024 positions (one lane over the whole text), about 2 s for rings of more
                              * than 448 slots (one lane per stretch without a synchronisation point), and up to about 15 s for a
                              * long stretch whose parts the parallel replay could not take (more order patterns at its cuts than
                              * rounds, snapshots that do not fit), which is then replayed on one lane; beyond, and for a stretch
                              * of more than 1 GiB or a grown batch whose scratch does not fit, RJ_TOO_LARGE.  An own range that
                              * the replay cannot serve is answered from the text's beginning (the run covers the starts before
                              * own_end) when no candidate there begins where another ends. */
  int32_t reserved;
} rj_info;

typedef struct {
  uint64_t n_hits;         /* candidate starts produced by the scan kernel           */
  uint64_t n_candidates;   /* verified (begin,end) candidates before selection       */
  uint64_t n_matches;      /* final left-most-longest, non-overlapping matches       */
  float scan_ms;           /* start-to-end time of the scan kernel(s), from their dispatch timestamps (count_path 1: first
                              workgroup's entry to last workgroup's exit by the device's wall clock, see rj_scan_set_timing) */
  float total_ms;          /* host clock: first launch to final synchronise of the run */
  int32_t retries;         /* runs repeated because a device list had to grow        */
  int32_t large_path;      /* 1 when the rocPRIM sort path was taken                 */
  int32_t exact_path;      /* 1 when the exact replay replaced the result, 2 when it took a long segment in parts */
  int32_t linear_path;    /* 1 when a candidate outlived the parallel verifier's walk and the linear-time carry scan ran */
  int32_t stream_path;    /* 1 when the bit-stream dense kernel produced the result (one pass, pairs written once) */
  int32_t slow_starts;    /* that kernel: starts that outlived its register steps and took the scalar walk (saturating) */
  int32_t count_path;     /* 1 when the one-kernel count (plane_count.hip) answered: a count and bounds, no span list (round 6) */
  int32_t run_path;       /* 1 when the run kernels (run_scan.hip: one long-lived thread in one loop position -- `[acgt]+`, `a.*b`)
                           * produced the result: two passes over the text, linear whatever the runs' length (round 6); 2: the pair
                           * kernels of the same file (`"[^"]*"`: the same class at both ends, none of it inside the loop) */
} rj_stats;

/* ---- compile (replaces Regej::Regej + Regej::Compile, src/rejit.cc:127-137,229-267) */
int rj_compile(const char* regexp, rj_program** out);
void rj_program_free(rj_program* prog);
int rj_program_info(const rj_program* prog, rj_info* info);
const char* rj_last_error(void);

/* ---- host text: one call = H2D copy + device pipeline + D2H of the results.
 * These four replace the four JIT function pointers above. */
/* 1 = the whole text matches, 0 = it does not, <0 = rj_status */
int rj_match_full(const rj_program* prog, const char* text, size_t n);
/* 1 / 0 / <0 */
int rj_match_anywhere(const rj_program* prog, const char* text, size_t n);
/* 1 (begin/end offsets written) / 0 / <0; left-most longest match */
int rj_match_first(const rj_program* prog, const char* text, size_t n, uint64_t* begin, uint64_t* end);
/* number of matches (>= 0) or rj_status.  *spans receives a malloc'ed array of
 * 2*count offsets (begin0,end0,begin1,...) to be released with rj_free_spans; pass NULL
 * to only count. */
int64_t rj_match_all(const rj_program* prog, const char* text, size_t n, uint64_t** spans);
void rj_free_spans(uint64_t* spans);
/* rj_stats of the calling thread's last rj_match_all / rj_match_first / rj_replace_all ... of `prog` (which kernels answered:
 * count_path, stream_path, linear_path, ...), as rj_scan_stats_sized.  RJ_BAD_ARGUMENT when this thread has made no such
 * call (calls of several threads combined into one batch are accounted to the thread that led the batch). */
int rj_host_stats(const rj_program* prog, void* stats, size_t struct_size);

/* A batch of independent texts in ONE device pass -- replaces the per-file loop of a grep-like
 * caller (`for each file: re->MatchAll(file, size, &matches)`, sample/jrep.cc:261-313), whose
 * per-call latency (~50 us + a PCIe copy each) a GPU cannot afford for many small files.  Every
 * text is matched on its own: no match crosses a text boundary, `^` / `$` see each text's own
 * begin and end.  counts[i] receives the number of matches of text i; *spans (may be NULL to only
 * count) a malloc'ed array of 2 * total offsets, text after text, RELATIVE to their own text;
 * release with rj_free_spans.  Returns the total number of matches or rj_status. */
int64_t rj_match_all_batch(const rj_program* prog, const char* const* texts, const size_t* sizes, size_t n_texts,
                           uint64_t* counts, uint64_t** spans);

/* The same for a batch its owner lays out ITSELF, so that no text is copied twice: text i is
 * packed[offsets[i] .. offsets[i] + sizes[i]), offsets ascending, and EVERY byte of packed[0 .. total_bytes) that
 * belongs to no text -- at least one behind every text, the last one included -- holds rj_batch_separator(prog).
 * `packed` is uploaded as it is: from memory of rj_host_alloc (pinned) at the PCIe rate, from ordinary memory
 * through the runtime's staging copy.  A native grep reads its files straight into such a buffer
 * (samples/jrep_gpu.cc); the reference's loop has no counterpart (one mmap + MatchAll per file,
 * sample/jrep.cc:261-313).  counts / spans / return value as for rj_match_all_batch.  A pattern for which
 * rj_batch_separator is -1 (every byte value can be consumed by some position of an automaton with assertions, or
 * the pattern is at risk of the ring artefact) is matched text by text. */
int rj_batch_separator(const rj_program* prog);
int64_t rj_match_all_packed(const rj_program* prog, const char* packed, const uint64_t* offsets, const size_t* sizes, size_t n_texts,
                            uint64_t total_bytes, uint64_t* counts, uint64_t** spans);
void* rj_host_alloc(size_t bytes);   /* pinned host memory (NULL when there is none to be had) */
void rj_host_free(void* p);

/* ReplaceAll (replaces MatchAll + rejit::Replace, src/rejit.cc:97-112,220-226): every match is
 * replaced by with[0..with_len).  Returns the number of matches (>= 0) or rj_status; *out receives
 * a malloc'ed copy of the new text (NUL-terminated for convenience, *out_len excludes the NUL),
 * to be released with rj_free_text.  Only the new text crosses PCIe, not the match list. */
int64_t rj_replace_all(const rj_program* prog, const char* text, size_t n, const char* with, size_t with_len, char** out,
                       size_t* out_len);
void rj_free_text(char* text);
/* The same in two steps, for a caller that owns the buffer the new text goes to (Regej::ReplaceAll rewrites its std::string:
 * include/rejit.h; reference src/rejit.cc:220-226): _begin uploads, matches and replaces on the device and returns the number
 * of matches (or rj_status) with the new text's length in *out_len; _fetch -- same thread, same program, once -- copies the
 * new text into dst[0 .. out_len) (dst_cap >= out_len; no NUL is written).  dst may be the memory `text` pointed to: the
 * device holds its own copy by then.  Measured on the GPU box (1 GB): malloc + download + free of the one-call form cost
 * 50 + 80 ms, the download into pages the caller already owns 18 ms. */
int64_t rj_replace_all_begin(const rj_program* prog, const char* text, size_t n, const char* with, size_t with_len, size_t* out_len);
int rj_replace_all_fetch(const rj_program* prog, char* dst, size_t dst_cap);

/* ---- device-resident text (what bench.py and the multi-GPU driver use; no copies).
 * d_text must be 16-byte aligned device memory with bytes [0, n) readable.  Matches whose
 * BEGIN lies in [own_begin, own_end) are reported (own_end may be n + 1 to include the
 * empty match at the end of the text); the automaton may read up to n, so a shard passes
 * its halo inside [0, n).  carry_cur / carry_prev_end / have_prev describe the last match
 * selected before own_begin (0,0,0 for the first shard). */
int rj_scan_create(const rj_program* prog, rj_scan** out);
void rj_scan_destroy(rj_scan* scan);
/* rj_stats.scan_ms (and rj_multi_scan_ms) is the scan kernel's own duration, from a start and an end event stamped by the
 * launch.  The end event is free; the START event costs 6-9 us per call (measured, round 4: 32-37 -> 26-28 us for texts of
 * 32 KB .. 16 MiB; ~6.5 us between two kernels of the regexdna step).  So it is OFF unless asked for -- per object, or for
 * every object created from now on (rj_set_default_timing returns the previous default; environment RJ_KERNEL_TIMING=1 sets
 * the initial one) -- and scan_ms reads 0 without it.  The Python binding (rejit_amd/api.py: bench.py, the tests and the
 * tools read scan_ms) switches the default on when it loads the library.
 * The one-kernel counts path (rj_multi_set_counts_only, rj_scan_count, rj_match_all(..., NULL) with count_path == 1) takes
 * no start event: there scan_ms runs from the first workgroup's entry into the kernel to the last workgroup's exit, read from
 * the device's constant-rate wall clock (100 MHz on gfx950: 10 ns resolution; hipDeviceAttributeWallClockRate) by the kernel
 * itself.  That costs nothing on the stream, timing on or off.  Every other path -- and a counts run that was void and was
 * answered by the span pipeline -- still uses the events. */
int rj_scan_set_timing(rj_scan* scan, int on);
int rj_set_default_timing(int on);
int64_t rj_scan_run(rj_scan* scan, const void* d_text, uint64_t n, uint64_t own_begin, uint64_t own_end,
                    uint64_t carry_cur, uint64_t carry_prev_end, int have_prev, void* hip_stream);
/* The same whole-text run in two halves, so that a caller with several patterns (or texts) in
 * flight does not serialise on every call's latency-bound tail: rj_scan_start enqueues the scan on
 * hip_stream and the verify / gather kernels behind it on the scan's own stream, rj_scan_finish
 * waits and returns the count (results as after rj_scan_run).  One start per scan at a time; scans
 * started back to back on one stream run their scan kernels one after the other while the tails of
 * earlier ones overlap them. */
int rj_scan_start(rj_scan* scan, const void* d_text, uint64_t n, void* hip_stream);
int64_t rj_scan_finish(rj_scan* scan);
/* MatchAllCount over device text (Regej::MatchAllCount, reference src/rejit.cc:203-208, is MatchAll with a NULL vector: the
 * caller wants the NUMBER of matches).  A pattern with the shape the one-kernel count takes (plane_count.hip; every regexdna
 * pattern, sample/regexdna.cc:51-61) is answered by that kernel -- the text read once, nothing written but the count;
 * rj_stats.count_path reads 1, rj_scan_device_spans NULL, and rj_scan_copy_spans / rj_scan_replace refuse with
 * RJ_BAD_ARGUMENT (there is no list).  Any other pattern, and a text on which the kernel voids its run, takes rj_scan_run's
 * pipeline (whole text, no carry).  rj_match_all(prog, text, n, NULL) does the same for host texts.  Returns the count or
 * rj_status. */
int64_t rj_scan_count(rj_scan* scan, const void* d_text, uint64_t n, void* hip_stream);
/* results of the last run: device pointer to 2*count uint64 offsets, or a copy (host_spans may be host or
 * device memory; returns the number of matches, copies at most cap of them) */
const uint64_t* rj_scan_device_spans(const rj_scan* scan);
int64_t rj_scan_copy_spans(const rj_scan* scan, uint64_t* host_spans, uint64_t cap);
/* Replace over device text: the matches of the LAST rj_scan_run on this scan (which must have
 * covered d_text[0..n) ) are replaced by `with` (host bytes); the result is written to d_out
 * (device, out_cap bytes).  Returns the new length or rj_status. */
int64_t rj_scan_replace(rj_scan* scan, const void* d_text, uint64_t n, const char* with, uint64_t with_len, void* d_out,
                        uint64_t out_cap, void* hip_stream);
int rj_scan_stats(const rj_scan* scan, rj_stats* stats);
/* rj_stats has grown (stream_path, slow_starts: round 4) and may grow again: rj_scan_stats writes sizeof(rj_stats) of the
 * header the LIBRARY was built from.  A caller that may meet a newer library passes the size of ITS struct: at most
 * struct_size bytes are written; returns the library's sizeof(rj_stats) (> struct_size: fields the caller does not know
 * were left out) or rj_status. */
int rj_scan_stats_sized(const rj_scan* scan, void* stats, size_t struct_size);
/* 1 / 0 / <0: kMatchFull over device text */
int rj_scan_match_full(rj_scan* scan, const void* d_text, uint64_t n, void* hip_stream);

/* ---- per-record answers over device-resident text (rejit_amd/csrc/record_join.hip): what a grep-like
 * or dataframe-like caller wants -- how many matches each record (line, string of a column, text of a packed batch) has, which
 * records match, where a record's matches sit in the list -- without a download of the list.  Records are
 * d_text[rec_begin[i], rec_end[i]), ascending and not overlapping: rec_begin[i] <= rec_end[i] <= rec_begin[i + 1], rec_end[last]
 * <= n; gaps between records are allowed, so are records that touch.  ONE ordinary whole-text run (rj_scan_run(scan, d_text, n,
 * 0, n + 1, 0, 0, 0, stream)), then every match goes by its BEGIN b to the last record i with rec_begin[i] <= b, and is kept
 * when b <= rec_end[i] (else it lies in a gap and belongs to no record) -- the rule of rj_match_all_packed: an empty match at a
 * record's end is that record's when a gap follows, the next record's when the two touch.  A kept match that ends beyond
 * rec_end[i] still counts for record i and is tallied in n_crossing: the library does not make records independent, the caller's
 * layout does (every byte outside a record holds rj_batch_separator(prog), as for rj_match_all_packed; n_crossing == 0 tells).
 * Record i's matches are spans[first[i] .. first[i] + count[i]) of the run's own list, as offsets into d_text. */
typedef struct {
  uint64_t n_kept;       /* matches that belong to a record                       */
  uint64_t n_matching;   /* records with at least one match                       */
  uint64_t n_crossing;   /* kept matches that end beyond their record's end       */
  uint64_t n_matches;    /* the whole-text run's matches (kept + in gaps)         */
} rj_record_stats;

/* d_rec_begin / d_rec_end: device, n_records uint64 each.  d_counts: device, n_records uint32 (saturating at
 * UINT32_MAX), may be NULL.  d_first: device, n_records uint64, may be NULL.  Returns n_kept or rj_status;
 * RJ_BAD_ARGUMENT with a message naming the first bad row when the table is not ascending / inside the text.
 * Afterwards rj_scan_device_spans / _copy_spans / rj_scan_stats are those of the whole-text run.  Every output is written
 * by exactly one lane: nothing has to be cleared first.  A refusal of the run itself (RJ_TOO_LARGE) passes through. */
int64_t rj_scan_records(rj_scan* scan, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                        const uint64_t* d_rec_end, uint64_t n_records, uint32_t* d_counts, uint64_t* d_first,
                        rj_record_stats* stats, void* hip_stream);
/* indices (ascending) of the records of the LAST rj_scan_records on this scan with a match (invert != 0: without);
 * d_indices: device, cap uint64; returns how many there are (writes at most cap) or rj_status.  Reads the counts of that
 * join: the caller's d_counts (which must still hold them) or, when that was NULL, the scan's own copy.  RJ_BAD_ARGUMENT when
 * the scan's last run was anything but a successful rj_scan_records. */
int64_t rj_scan_records_select(rj_scan* scan, int invert, uint64_t* d_indices, uint64_t cap, void* hip_stream);
/* Records of a device text gathered into a NEW contiguous device text (rejit_amd/csrc/record_pack.hip):
 * what a grep-like caller prints (the selected lines, fill = '\n') and what makes the strings of a column whose records touch
 * independent (fill = rj_batch_separator(prog)) -- without a download.  With k = d_indices ? n_indices : n_records,
 * r(j) = d_indices ? d_indices[j] : j and len(j) = rec_end[r(j)] - rec_begin[r(j)]:
 *     ob(0) = lead, ob(j + 1) = ob(j) + len(j) + gap, total = ob(k)       (k == 0: total = lead)
 *     d_out[ob(j), ob(j) + len(j)) = the bytes of text record r(j); every other byte of d_out[0, total) = fill
 *     d_out_begin[j] = ob(j), d_out_end[j] = ob(j) + len(j)               (k uint64 each; either may be NULL)
 * d_indices: any order, repeats allowed (a permutation, a take; rj_scan_records_select's output is the common case); a
 * non-NULL d_indices with n_indices == 0 packs nothing.  Rows need not be in order with each other; every packed row must
 * keep begin <= end <= n and every index must be < n_records: RJ_BAD_ARGUMENT with a message naming the first bad j -- a bad
 * row is never followed outside the text or the output.  fill: 0..255; gap may be 0.  d_out: 16-byte aligned, out_cap
 * bytes, not overlapping the text.  Returns total WHATEVER out_cap is and never writes at or beyond out_cap; d_out == NULL
 * with out_cap == 0 is the size query (the tables are still written when given).  With total <= out_cap the result is
 * complete: every byte of [0, total) and every table row is written exactly once, nothing has to be cleared first, nothing
 * behind total is touched.  n + gap must stay below 2^42 and lead + k * (n + gap) below 2^62.  The scan lends scratch only: its span list, its
 * stats and the state of its last rj_scan_records (rj_scan_records_select included) stay as they were. */
int64_t rj_scan_records_pack(rj_scan* scan, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                             const uint64_t* d_rec_end, uint64_t n_records, const uint64_t* d_indices, uint64_t n_indices,
                             int fill, uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin,
                             uint64_t* d_out_end, void* hip_stream);
/* The pack above in which every packed record has its OWN matches replaced by `with` (rejit_amd/csrc/record_replace.hip,
 * DESIGN.md section 4.15): `sed 's/RE/with/g'` over lines, `str.replace` over a column, with the new record table, in one call
 * and without a download.  k, r(j), lead, gap, fill, d_indices, out_cap, the size query and the tables are exactly those of
 * rj_scan_records_pack.  The match list is the list of the scan's last run (rj_scan_device_spans, m = its count); d_counts /
 * d_first are what rj_scan_records wrote for THIS record table on that run: record r's matches are spans[first[r] .. first[r] +
 * count[r]).  R(r) = the bytes of text[rec_begin[r], rec_end[r]) with each of those matches replaced by `with` (host bytes), left
 * to right -- what the reference's rejit::Replace (src/rejit.cc:97-112) gives on the record alone with the record-relative spans;
 * an empty match inserts `with` at its position.  With len'(j) = len(j) - (bytes of r(j)'s matches) + count[r(j)] * with_len:
 *     ob(0) = lead, ob(j + 1) = ob(j) + len'(j) + gap, total = ob(k)
 *     d_out[ob(j), ob(j) + len'(j)) = R(r(j)); every other byte of d_out[0, total) = fill
 *     d_out_begin[j] = ob(j), d_out_end[j] = ob(j) + len'(j)
 * Bytes of a record inside a match that belongs to another record or to a gap are copied as text: only the record's own matches
 * are replaced.  Returns total WHATEVER out_cap is, never writes at or beyond out_cap; with total <= out_cap every byte of
 * [0, total) and every table row is written exactly once.  The scan lends scratch only: spans, stats and the state of its last
 * rj_scan_records (rj_scan_records_select included) stay as they were.
 * Refusals (RJ_BAD_ARGUMENT; one that names a row gives the first bad j as "row <j> "; a refused call copies nothing and is never
 * led outside the text, the list or the output): a bad index or row, by the pack's rules; first[r] + count[r] > m; count[r] ==
 * UINT32_MAX (saturated: the range is unknown); the row's first match begins before rec_begin[r]; the row's last match ends
 * beyond rec_end[r] -- a crossing match: the records are not independent, rj_scan_records_pack with the separator makes them so
 * (the list is an ordered non-overlapping selection, so the first begin and the last end bound every match of the row);
 * d_counts or d_first NULL while k > 0; with == NULL with with_len > 0; a last run that left no list (counts-only); the
 * argument refusals of the pack; n + (m + 1) * with_len + gap >= 2^42, or lead + k * that >= 2^62 (and k >= 2^60). */
int64_t rj_scan_records_replace(rj_scan* scan, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                                const uint64_t* d_rec_end, uint64_t n_records, const uint32_t* d_counts, const uint64_t* d_first,
                                const uint64_t* d_indices, uint64_t n_indices, const char* with, uint64_t with_len, int fill,
                                uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin,
                                uint64_t* d_out_end, void* hip_stream);
/* The FIELDS of records -- the pieces between a record's own matches: `awk -F RE`, `cut`, str.split, Arrow's
 * split_pattern_regex -- or the MATCHES themselves per record (`grep -o`, str.findall), as a piece table: a record table over
 * the same device text whose rows are the pieces, plus Arrow-style offsets that say which pieces belong to which row
 * (rejit_amd/csrc/record_split.hip).  The text is not an argument, only its length n (for the row
 * checks): the call reads tables and the scan's span list and nothing else.  k, r(j) and d_indices are those of
 * rj_scan_records_pack: any order, repeats allowed, non-NULL with n_indices == 0 is no rows.  The match list is the list of the
 * scan's last run, of length m; d_counts / d_first are what rj_scan_records wrote for THIS record table on that run.  Record
 * r = r(j) is [rb, re), with f = first[r], c = count[r] and own matches (b_t, e_t) = spans[f + t], t < c:
 *     RJ_SPLIT_BETWEEN: row j has c + 1 pieces, piece t = [t == 0 ? rb : e_{t-1}, t == c ? re : b_t)
 *     RJ_SPLIT_MATCHES: row j has c pieces,     piece t = [b_t, e_t)          (a row without a match has none)
 *     piece_first[0] = 0, piece_first[j + 1] = piece_first[j] + (pieces of row j), P = piece_first[k]
 * The BETWEEN pieces are the parts of the record that rj_scan_records_replace copies as text: joining them with `with` gives
 * exactly that call's R(r).  Empty pieces are pieces (two matches that touch, a match at the record's begin or end), and an
 * empty match at p cuts at p.  d_piece_first: device, k + 1 uint64, may be NULL (the scan then keeps its own, as the pack does
 * with its begins).  Row j's pieces are rows piece_first[j] .. piece_first[j + 1] of d_piece_begin / d_piece_end (device,
 * piece_cap uint64 each), as offsets into the text.  Returns P WHATEVER piece_cap is and never writes a piece row at or beyond
 * piece_cap; d_piece_begin == d_piece_end == NULL with piece_cap == 0 is the size query (d_piece_first is still written when
 * given).  With P <= piece_cap every row of the three tables is written exactly once, nothing has to be cleared first.  The
 * scan lends scratch only: spans, stats and the state of its last rj_scan_records (rj_scan_records_select included) stay as
 * they were.  Without d_indices both tables are ascending and not overlapping: valid record tables for rj_scan_records (a
 * second pattern per field), and rj_scan_records_pack over them prints the fields or the matches.
 * Refusals (RJ_BAD_ARGUMENT; one that names a row gives the first bad j as "row <j> "; a refused call writes no piece row and
 * is never led outside the list or the tables): for both values of `what` the six of rj_scan_records_replace -- a bad index; a
 * bad row (begin <= end <= n); count[r] == UINT32_MAX; first[r] + count[r] > m; a first match that begins before rec_begin[r];
 * a last match that ends beyond rec_end[r] (the records are not independent: rj_scan_records_pack with the separator makes
 * them so) --; a null argument; d_counts or d_first NULL while k > 0; a table that is not 8-byte aligned (d_counts: 4-byte);
 * `what` outside {0, 1}; a last run that left no list (counts-only); k >= 2^60, or k * (m + 1) >= 2^62. */
enum { RJ_SPLIT_BETWEEN = 0, RJ_SPLIT_MATCHES = 1 };
int64_t rj_scan_records_split(rj_scan* scan, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end,
                              uint64_t n_records, const uint32_t* d_counts, const uint64_t* d_first,
                              const uint64_t* d_indices, uint64_t n_indices, int what, uint64_t* d_piece_first,
                              uint64_t* d_piece_begin, uint64_t* d_piece_end, uint64_t piece_cap, void* hip_stream);
/* The rows of a record table GROUPED BY THEIR BYTES (rejit_amd/csrc/record_group.hip): which records are
 * equal -- `sort | uniq -c`, `awk '{c[$3]++}'`, Arrow's dictionary_encode / unique / value_counts over a string column -- exactly
 * (lengths and bytes are compared; a hash only finds the candidates) and deterministically, without a download.  Any record
 * table over the text serves: rj_scan_records_split's pieces (matches, fields), lines, the strings of a column.  k, r(j) and
 * d_indices are those of rj_scan_records_pack: any order, repeats allowed, non-NULL with n_indices == 0 is no rows.  Row j is
 * the byte string text[rec_begin[r(j)], rec_end[r(j)]); two rows are equal when their lengths and bytes are; empty rows are
 * equal to each other; a row's identity is j, not r(j).  With the distinct strings numbered g = 0 .. G - 1 in order of first
 * appearance:
 *     d_group[j]       = the group of row j                              (k uint64, may be NULL)
 *     d_rep[g]         = the smallest j with that string, so strictly ascending       (group_cap uint64)
 *     d_group_count[g] = the number of rows in group g; the counts add up to k        (group_cap uint64)
 * d_group are the indices of a dictionary encoding, the dictionary is rj_scan_records_pack over the rows d_rep (composed with
 * d_indices when there are any).  Returns G WHATEVER group_cap is and never writes d_rep / d_group_count at or beyond
 * group_cap; d_rep == d_group_count == NULL with group_cap == 0 is the size query (d_group is still written when given).
 * With G <= group_cap every row of the three tables is written exactly once, nothing has to be cleared first, nothing behind
 * G or k is touched.  k == 0 returns 0.  The scan lends scratch only (44 to 68 bytes per row): spans, stats and the state of
 * its last rj_scan_records (rj_scan_records_select included) stay as they were.  One synchronise per call.
 * Refusals (RJ_BAD_ARGUMENT; one that names a row gives the first bad j as "row <j> "; a refused call writes no output row and
 * is never led outside the text or a table): an index >= n_records; a row without begin <= end <= n; a null argument (d_text
 * with n > 0, the tables with n_records > 0, d_rep or d_group_count with group_cap > 0); a table that is not 8-byte aligned.
 * k >= 2^31: RJ_TOO_LARGE (rows and slots share 32-bit words in the scratch).
 * Two knobs for tests, read from the environment at every call: RJ_GROUP_HASH_BITS=b keeps only the low b bits of every hash
 * (different strings then share probe chains: the byte compare decides), RJ_GROUP_LONG_BYTES=L moves the length above which
 * a row is walked by a wave instead of a lane (default 64). */
int64_t rj_scan_records_group(rj_scan* scan, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                              const uint64_t* d_rec_end, uint64_t n_records, const uint64_t* d_indices, uint64_t n_indices,
                              uint64_t* d_group, uint64_t* d_rep, uint64_t* d_group_count, uint64_t group_cap,
                              void* hip_stream);
/* The rows of a record table IN THE ORDER OF THEIR BYTES (rejit_amd/csrc/record_sort.hip): `sort`,
 * ORDER BY over a string column, a sorted dictionary, the input of a merge join -- and, over the rows d_rep of
 * rj_scan_records_group, `sort -u` and `sort | uniq -c` -- exactly, without a download.  k, r(j) and d_indices are those of
 * rj_scan_records_pack and rj_scan_records_group: any order, repeats allowed, non-NULL with n_indices == 0 is no rows; a row's
 * identity is j, not r(j).  Row j is the byte string text[rec_begin[r(j)], rec_end[r(j)]).  d_order (k uint64) receives THE
 * permutation of 0 .. k - 1 with row(order[i]) <= row(order[i + 1]):
 *     bytes compare as unsigned values (memcmp, `LC_ALL=C sort`);  a proper prefix sorts before the longer row;
 *     rows with equal bytes come in ascending j (the sort is stable).
 * The answer is unique and depends on the rows alone; rj_scan_records_pack with d_order as its index list (composed with
 * d_indices when there are any) prints the sorted table.  Returns k.  Every row of d_order is written exactly once, nothing
 * has to be cleared first, nothing behind k is touched.  k == 0 returns 0.  The scan lends scratch only (63 bytes per row and
 * the radix sort's temporary storage): spans, stats and the state of its last rj_scan_records (rj_scan_records_select
 * included) stay as they were.  One synchronise per refinement round: a round reads 7 more bytes of every row that still
 * shares everything read so far with another one, behind the prefix ALL rows of such a segment share (skipped from the
 * second round on); at most G + 1 rounds for G distinct strings, 1 to 3 on columns of short strings.
 * `stats` (may be NULL) receives what the call did.
 * Refusals (RJ_BAD_ARGUMENT; one that names a row gives the first bad j as "row <j> "; a refused call writes no output row and
 * is never led outside the text or a table): an index >= n_records; a row without begin <= end <= n; a null argument (d_text
 * with n > 0, the tables with n_records > 0, d_order with k > 0); a table that is not 8-byte aligned.
 * k >= 2^31: RJ_TOO_LARGE (rows and segments share 32-bit words in the scratch).
 * Two knobs for tests, read from the environment at every call: RJ_SORT_SKIP=0 turns the prefix skip off (7 bytes per round,
 * whatever the rows share), RJ_SORT_LONG_BYTES=L moves the number of bytes a lane compares before it hands the row to a wave
 * (default 64). */
typedef struct {
  uint64_t rounds;     /* refinement rounds run (0 when k < 2)                          */
  uint64_t keyed_rows; /* rows given a key, summed over the rounds                      */
  uint64_t skip_rows;  /* rows compared against their segment's head by the prefix skip */
  uint64_t long_rows;  /* of those, rows handed to the wave tier                        */
} rj_sort_stats;
int64_t rj_scan_records_sort(rj_scan* scan, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                             const uint64_t* d_rec_end, uint64_t n_records, const uint64_t* d_indices, uint64_t n_indices,
                             uint64_t* d_order, rj_sort_stats* stats /* may be NULL */, void* hip_stream);
/* The rows of one record table LOOKED UP IN ANOTHER (rejit_amd/csrc/record_lookup.hip): `grep -F -x -f
 * KEYS`, `awk 'NR==FNR{s[$0];next} $3 in s'`, `comm`, Arrow's is_in / index_in, a semi-, anti- or inner join on a string key,
 * a new batch encoded against an existing dictionary -- exactly (lengths and bytes are compared; a hash only finds the
 * candidates), without a download.  Two record tables, the SET table over d_set_text[0, set_n) and the PROBE table over
 * d_text[0, n), each with the row rules of rj_scan_records_pack / rj_scan_records_group: any order, repeats allowed through the
 * index list, a non-NULL index list with count 0 is no rows.  The two texts may be the same buffer, overlap, or be unrelated.
 * ks is the number of set rows, kp of probe rows; set row i is set_text[set_begin[rs(i)], set_end[rs(i)]), probe row j is
 * text[rec_begin[r(j)], rec_end[r(j)]); a row's identity is its position i or j, not its record.  Two rows are equal when
 * their lengths and bytes are; empty rows are equal to each other; "ab" and "ab\0" are different.
 *     d_index[j]    = the smallest i whose set row equals probe row j, or RJ_LOOKUP_NONE     (kp uint64; index_in, first occurrence)
 *     d_set_hits[i] = when i is the smallest set row with its string, the number of probe rows j with d_index[j] == i; for a
 *                     later duplicate 0.  The hits add up to n_found                          (ks uint64, may be NULL)
 * The answer is unique and depends on the rows alone.  The set rows whose d_set_hits is 0 at a first occurrence are the
 * anti-join's right side (`comm -13`).  Returns n_found, the number of probe rows whose string is in the set.  Every row of
 * d_index, and of d_set_hits when given, is written exactly once, nothing has to be cleared first, nothing behind kp or ks is
 * touched.  ks == 0: every index is RJ_LOOKUP_NONE and the call returns 0.  kp == 0: returns 0, and d_set_hits, when given,
 * is still written (all zero).  `stats` (may be NULL) receives what the call found.
 * Composition: a lookup against the group call's dictionary -- the set rows d_rep of rj_scan_records_group over the set table,
 * passed as d_set_indices (composed with that call's d_indices when there were any) -- gives every probe row its GROUP NUMBER
 * directly: a new batch encoded against an existing dictionary, and the key step of an inner join (records.join_rows).
 * The scan lends scratch only (the group call's 44 to 68 bytes per set row, 4 bytes per slot of hit counts, 8 bytes per probe
 * row): spans, stats and the state of its last rj_scan_records (rj_scan_records_select included) stay as they were.  One
 * synchronise per call.  Without d_set_hits and stats (is_in) the probes issue no atomic on the table or the counts.
 * Refusals (RJ_BAD_ARGUMENT; a refused call writes no output row and is never led outside a text or a table): an index at or
 * beyond its table's record count; a row without begin <= end <= its text's length -- the message names the table and the
 * first bad row, "set row <i> " for the set, which is checked first, "row <j> " for the probe --; a null argument (per side:
 * the text with a length > 0, the tables with a record count > 0; d_index with kp > 0); a table that is not 8-byte aligned.
 * An output that overlaps an input is undefined, as elsewhere in the family.
 * ks >= 2^31 or kp >= 2^31: RJ_TOO_LARGE (hit counts and the long list are 32-bit words in the scratch).
 * The group call's knobs are read at every call: RJ_GROUP_HASH_BITS, RJ_GROUP_LONG_BYTES (both sides), RJ_GROUP_PEEL=0 (the
 * set's inserts and the probes' hit counts each issue their own atomics).  No knobs of its own. */
#define RJ_LOOKUP_NONE (~0ull)
typedef struct {
  uint64_t n_found;        /* probe rows whose string is in the set                        */
  uint64_t n_set_distinct; /* distinct strings among the set rows (the group call's G)     */
  uint64_t n_set_hit;      /* of those, strings that at least one probe row has            */
  uint64_t long_rows;      /* probe rows handed to the wave tier                           */
} rj_lookup_stats;
int64_t rj_scan_records_lookup(rj_scan* scan, const void* d_set_text, uint64_t set_n, const uint64_t* d_set_begin,
                               const uint64_t* d_set_end, uint64_t n_set_records, const uint64_t* d_set_indices,
                               uint64_t n_set_indices, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                               const uint64_t* d_rec_end, uint64_t n_records, const uint64_t* d_indices, uint64_t n_indices,
                               uint64_t* d_index, uint64_t* d_set_hits /* may be NULL */,
                               rj_lookup_stats* stats /* may be NULL */, void* hip_stream);
/* The rows of a record table read AS NUMBERS (rejit_amd/csrc/record_parse.hip): `awk '{s[$1] += $3}'`,
 * `awk '$9 >= 500'`, `sort -n`, Arrow's cast(utf8 -> int64 / uint64 / float64) -- exactly, or not at all, without a download.
 * The row rules are those of rj_scan_records_pack / rj_scan_records_group: any order, repeats allowed through the index list, a
 * non-NULL index list with count 0 is no rows; k is the number of rows, row j is text[rec_begin[r(j)], rec_end[r(j)]).
 *     d_value[j]  = the row's int64, its uint64, or the IEEE-754 bits of its double; 0 when the status is not OK   (k uint64)
 *     d_status[j] = RJ_PARSE_OK, or why the row has no value                                          (k bytes, may be NULL)
 * D is [0-9].  With RJ_PARSE_TRIM the ASCII spaces and tabs before and behind the number are dropped first; without it they
 * are ordinary bytes.  Nothing else is skipped: no underscores, no locale, no inf / nan / hex; a NUL is an ordinary byte.  The
 * statuses, decided in this order:
 *     RJ_PARSE_EMPTY      no bytes are left
 *     RJ_PARSE_MALFORMED  the bytes are not in the kind's grammar: INT64 [+-]?D+, UINT64 \+?D+ (a `-` is malformed, `-0`
 *                         included), FLOAT64 [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?
 *     RJ_PARSE_RANGE      integer kinds: the value is outside [-2^63, 2^63 - 1] / [0, 2^64 - 1] (leading zeros do not count);
 *                         FLOAT64 under RJ_PARSE_WIDE only (below): the correctly rounded double is infinite
 *     RJ_PARSE_INEXACT    FLOAT64: with the row's exact decimal value written as +-m x 10^q, m not divisible by 10 -- a property
 *                         of the value, not of its spelling: 1.50, 15e-1 and 0.0015e3 are (15, -1) --, the row is OK when m = 0
 *                         (+-0.0 whatever the exponent says) or when m <= 2^53 and -22 <= q <= 22; everything else is INEXACT
 * An OK value is what Python's int() / float() and strtod make of the row, bit for bit: inside the window double(m) and 10^|q|
 * are exact and the value is one IEEE multiplication or division of the two, hence correctly rounded.  A row never gets a
 * nearby value.
 * With RJ_PARSE_WIDE (FLOAT64; accepted and without effect for the integer kinds, so one flags word serves every column) the
 * window is widened to every decimal the walk can hold, by integer arithmetic (the Eisel-Lemire product over a table of 128-bit
 * powers of five).  Grammar, TRIM, EMPTY and MALFORMED are as before.  Let S be the row's significant
 * digits, from the first non-zero mantissa digit to the last, and the value int(S) x 10^q -- the (m, q) above:
 *     no such digit          OK with +-0.0, as without the flag
 *     int(S) <= 2^64 - 1     the row is decided: OK with the correctly rounded double -- float()'s bits; subnormals, and +-0.0 for
 *                            1e-400, included --, or RJ_PARSE_RANGE (value 0) when that double is infinite: 1e309 and
 *                            1.7976931348623159e308 are RANGE, 1.7976931348623158e308 is OK.  Every spelling with up to 19
 *                            significant digits is decided, and many with 20.
 *     otherwise              with P the longest prefix of S that fits 64 bits and r = len(S) - len(P), the value lies strictly
 *                            between P x 10^(q + r) and (P + 1) x 10^(q + r): when both ends round to one double the row is OK with
 *                            it (rounding is monotone); when both are infinite it is RANGE; when they differ, or P = 2^64 - 1, it
 *                            is RJ_PARSE_INEXACT -- a property of the value, not of its spelling or of where the row is cut.
 * So under RJ_PARSE_WIDE a FLOAT64 row can be RJ_PARSE_RANGE (n_range counts it), every row that is OK without the flag keeps its
 * bits, and INEXACT is left to the few rows of more than 64 bits of mantissa whose bracket straddles a rounding boundary.
 * Without the flag nothing changes.  A row still never gets a value that is not the correctly rounded one.
 * Returns n_ok.  Every row of d_value, and of d_status when given, is written exactly once, nothing has to be cleared first,
 * nothing behind k is touched; k == 0 returns 0.  `stats` (may be NULL) receives the five counts; they add up to k.  A row of
 * any length is legal (one lane walks it).  The scan lends scratch only: spans, stats and the state of its last rj_scan_records
 * (rj_scan_records_select included) stay as they were.  One synchronise per call.
 * Refusals (RJ_BAD_ARGUMENT; a refused call writes no output row and is never led outside the text or a table): an index >=
 * n_records; a row without begin <= end <= n -- the message names the first bad row, "row <j> " --; a null argument (d_text
 * with n > 0, the tables with n_records > 0, d_value with k > 0); a table or d_value that is not 8-byte aligned; an unknown
 * kind, or a flag bit other than RJ_PARSE_TRIM and RJ_PARSE_WIDE.  An output that overlaps an input is undefined, as elsewhere in the family.
 * k >= 2^31: RJ_TOO_LARGE, as in the rest of the family's row calls. */
#define RJ_PARSE_INT64 0
#define RJ_PARSE_UINT64 1
#define RJ_PARSE_FLOAT64 2
#define RJ_PARSE_TRIM 1u /* flags: ASCII space (0x20) and tab (0x09) before and behind the number are skipped */
#define RJ_PARSE_WIDE 4u /* flags: FLOAT64 rows outside the exact window get their correctly rounded double (above); 2u is reserved */
enum { RJ_PARSE_OK = 0, RJ_PARSE_EMPTY = 1, RJ_PARSE_MALFORMED = 2, RJ_PARSE_RANGE = 3, RJ_PARSE_INEXACT = 4 };
typedef struct {
  uint64_t n_ok, n_empty, n_malformed, n_range, n_inexact;
} rj_parse_stats;
int64_t rj_scan_records_parse(rj_scan* scan, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                              const uint64_t* d_rec_end, uint64_t n_records, const uint64_t* d_indices, uint64_t n_indices,
                              int kind, unsigned flags, uint64_t* d_value, uint8_t* d_status /* may be NULL */,
                              rj_parse_stats* stats /* may be NULL */, void* hip_stream);
/* The rows of a record table read AS TIMESTAMPS (rejit_amd/csrc/record_time.hip): the first column of a
 * log -- `10/Oct/2000:13:55:36 -0700`, `2026-10-20T17:15:00.123Z` --, Arrow's strptime / cast(utf8 -> timestamp[unit]): "requests
 * per minute", "the lines between two instants", "order by time" -- exactly, or not at all, without a download.  The parse's
 * fourth value kind: everything that is not about time is rj_scan_records_parse's, word for word -- the row rules, k, the
 * status enum, rj_parse_stats, the refusals of rows and arguments.
 *     d_value[j]  = the row's instant as an int64 count of `unit`s since 1970-01-01T00:00:00Z (negative before it); 0 when the
 *                   status is not OK                                                                              (k uint64)
 *     d_status[j] = RJ_PARSE_OK, or why the row has no value                                          (k bytes, may be NULL)
 * `format` (format_len bytes, 1..64; it need not end in a NUL, and a NUL inside is a literal) is a strptime-style format.  A
 * row is matched against it from its first byte to its last; D is [0-9]:
 *     %Y   exactly DDDD, 0001..9999 (0000 is RANGE)          %H %M %S   exactly DD each: 00..23, 00..59, 00..59 (a second of
 *     %m   exactly DD, 01..12                                           60 is RANGE: there are no leap seconds)
 *     %b   exactly 3 ASCII letters, jan..dec in any case;    %f   1 to 9 digits, as many as the row has there (greedy): the
 *          other letters or bytes are MALFORMED                   fraction of a second
 *     %d   exactly DD, 01..the last day of that month in     %z   `Z` (upper case only), or [+-]DD, an optional `:`, DD: hours
 *          that year (proleptic Gregorian leap rule)              00..23, minutes 00..59 (else RANGE).  The offset is subtracted;
 *     %%   a `%`                                                  -00:00 is +00:00.  An offset with seconds is MALFORMED
 *     any other byte, NUL included: itself, exactly.  A blank in the format is one such byte, not "any white space".
 * Fields the format does not name are 0; without %z the fields are UTC.  With RJ_PARSE_TRIM the ASCII spaces and tabs before
 * and behind the row are dropped first; without it they are ordinary bytes.  The statuses, decided in this order:
 *     RJ_PARSE_EMPTY      no bytes are left
 *     RJ_PARSE_MALFORMED  the row ends before the format does, a byte does not fit its directive or literal, or bytes remain
 *                         behind the format's last one
 *     RJ_PARSE_RANGE      a field is outside its range above (the day is judged against its month and year wherever they
 *                         stand in the row); or the instant is outside int64 in `unit` -- only RJ_TIME_NANO can do that: before
 *                         1677-09-21T00:12:43.145224192Z or after 2262-04-11T23:47:16.854775807Z
 *     RJ_PARSE_INEXACT    %f has a non-zero digit below `unit`: the instant is not representable.  Never truncated or rounded
 * An OK value is what Python's datetime.strptime makes of the same bytes and format -- the civil fields as UTC, or the aware
 * value under %z -- as (dt - epoch) // unit, computed in integers (days from the civil date by the 400-year-era formula, no
 * table of years).  Python accepts more (one-digit fields, runs of white space, other letter cases of literals, offsets with
 * seconds): those rows are MALFORMED here.  No row that is OK here has another value there, and no row Python rejects is OK
 * here, except for %f with 7 to 9 digits, which Python does not read.
 * Returns n_ok.  Every row of d_value, and of d_status when given, is written exactly once, nothing has to be cleared first,
 * nothing behind k is touched; k == 0 returns 0.  `stats` (may be NULL) receives the five counts; they add up to k.  A row of
 * any length is legal (one lane walks it; a malformed row stops at its first bad byte).  The scan lends scratch only: spans,
 * stats and the state of its last rj_scan_records (rj_scan_records_select included) stay as they were.  One synchronise per call.
 * Refusals (RJ_BAD_ARGUMENT; a refused call writes no output row and is never led outside the text or a table): the parse's --
 * an index >= n_records; a row without begin <= end <= n, the message names the first bad row, "row <j> "; a null argument
 * (also `format` with format_len > 0); a table or d_value that is not 8-byte aligned --; a unit that is not RJ_TIME_*; a flag
 * bit other than RJ_PARSE_TRIM; and a format that is refused, the message naming the byte offset, "format byte <i>: ": an
 * empty format (0); more than 64 bytes (64); an unknown directive or a `%` as the last byte (the `%`); a directive given twice,
 * or %m together with %b (the second one's `%`); %f directly followed by a digit literal or by one of %Y %m %d %H %M %S (that
 * byte: the greedy read would be ambiguous); a format without %Y, %d and one of %m / %b (format_len: time-of-day-only formats
 * stay out).  k >= 2^31: RJ_TOO_LARGE.
 * The inverse (timestamps as text) is rj_scan_records_format_time, below.  What stays out: %y %j %e %a %p, named zones,
 * locales, leap seconds. */
#define RJ_TIME_SECOND 0
#define RJ_TIME_MILLI 1
#define RJ_TIME_MICRO 2
#define RJ_TIME_NANO 3
int64_t rj_scan_records_parse_time(rj_scan* scan, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                                   const uint64_t* d_rec_end, uint64_t n_records, const uint64_t* d_indices,
                                   uint64_t n_indices, const char* format, uint64_t format_len, int unit, unsigned flags,
                                   uint64_t* d_value, uint8_t* d_status /* may be NULL */,
                                   rj_parse_stats* stats /* may be NULL */, void* hip_stream);
/* A column of numbers written AS DECIMAL TEXT (rejit_amd/csrc/record_format.hip): the inverse of
 * rj_scan_records_parse -- the sums of an aggregation, line numbers, Arrow's cast(int64 / uint64 / float64 -> utf8) -- as a new
 * device text and its record table, without a download.  d_value: n_values 64-bit words, read by `kind` (the kind numbers of
 * RJ_PARSE_*): an int64, a uint64, or the IEEE-754 bits of a double.  With k = d_indices ? n_indices : n_values and
 * r(j) = d_indices ? d_indices[j] : j (a take, a permutation, the order of a top-K; repeats allowed; a non-NULL list with count 0
 * is no rows), row j's bytes T(j) are made from d_value[r(j)], and the layout is rj_scan_records_pack's with len(j) = |T(j)|:
 *     ob(0) = lead, ob(j + 1) = ob(j) + len(j) + gap, total = ob(k)       (k == 0: total = lead)
 *     d_out[ob(j), ob(j) + len(j)) = T(j); every other byte of d_out[0, total) = fill
 *     d_out_begin[j] = ob(j), d_out_end[j] = ob(j) + len(j)               (k uint64 each; either may be NULL)
 * T(j), byte for byte what Python writes:
 *     INT64, UINT64   str(int): a `-` for negatives only, no `+`, no leading zeros, 1 to 20 bytes
 *     FLOAT64         repr(float).  The digits are the shortest string of 1 to 17 that reads back as the same double, and
 *                     among the strings of that length the one closest to the exact value (the even one at a tie).  With the
 *                     value written 0.d1d2... x 10^decpt the form is positional for -4 < decpt <= 16, `.0` appended when
 *                     there is no fraction (9999999999999998.0, 0.0001, 1000000000000000.5), else d[.ddd]e+-XX with a sign and
 *                     at least two exponent digits (1e+16, 1e-05, 1.2345678901234568e+17, 5e-324).  -0.0 is `-0.0`.  The
 *                     non-finite values are `inf`, `-inf` and `nan`, whatever the NaN's sign and payload: THESE THREE
 *                     rj_scan_records_parse DOES NOT READ BACK (its grammar has digits only: they are MALFORMED there).
 *                     The longest row has 24 bytes (-2.9205048131065683e-196).
 *     d_status given  a row whose d_status[r(j)] (n_values bytes: parse's status column, unchanged) is not RJ_PARSE_OK is the
 *                     EMPTY row: zero bytes, an empty CSV field, Arrow's null.
 * For every finite double, rj_scan_records_parse(RJ_PARSE_FLOAT64, RJ_PARSE_WIDE) of the output returns the input's bits with
 * status OK; the integer kinds likewise return the value.  The digits are computed in integers only (Schubfach over a table of
 * 128-bit powers of ten, rejit_amd/csrc/pow10_table.h); there is no fallback and no floating-point operation.
 * flags must be 0: every bit is refused, later styles have room.  fill: 0..255; gap may be 0.  d_out: 16-byte aligned, out_cap
 * bytes.  Returns total WHATEVER out_cap is and never writes at or beyond out_cap; d_out == NULL with out_cap == 0 is the size
 * query (the tables are still written when given).  With total <= out_cap the result is complete: every byte of [0, total) and
 * every table row is written exactly once, nothing has to be cleared first, nothing behind total or behind row k is touched.
 * The scan lends scratch only: spans, stats and the state of its last rj_scan_records (rj_scan_records_select included) stay as
 * they were.  One synchronise per call.
 * Refusals (RJ_BAD_ARGUMENT; a refused call writes no output byte and no table row): an index >= n_values -- the message names
 * the first bad row, "row <j> " --; a null d_value with n_values > 0, a null d_out with out_cap > 0; a table, d_value or
 * d_indices that is not 8-byte aligned; a d_out that is not 16-byte aligned; an unknown kind, any flag bit, a fill outside
 * 0..255; 24 + gap >= 2^42, or lead + k * (24 + gap) >= 2^62.  k >= 2^31: RJ_TOO_LARGE, as in the rest of the family's row
 * calls.  An output that overlaps an input is undefined, as elsewhere in the family. */
#define RJ_FORMAT_INT64 0 /* the kind numbers of RJ_PARSE_* */
#define RJ_FORMAT_UINT64 1
#define RJ_FORMAT_FLOAT64 2
int64_t rj_scan_records_format(rj_scan* scan, const uint64_t* d_value, const uint8_t* d_status /* may be NULL */,
                               uint64_t n_values, const uint64_t* d_indices, uint64_t n_indices, int kind, unsigned flags,
                               int fill, uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap,
                               uint64_t* d_out_begin, uint64_t* d_out_end, void* hip_stream);
/* Several columns of records put SIDE BY SIDE into lines (rejit_amd/csrc/record_zip.hip): the inverse
 * of rj_scan_records_split -- Arrow's binary_join_element_wise, `paste -d`, `awk '{print $3, $1}'`, the "%7d %s %s\n" of
 * `sort | uniq -c` -- as a new device text and its record table, without a download.  cols: n_cols (1..16) columns, a HOST
 * array.  Column c is a record table over a device text of its own -- d_text (n bytes), d_rec_begin, d_rec_end (n_records) --,
 * an optional index list and a width; its rows are rj_scan_records_pack's: row j is record d_indices ? d_indices[j] : j, any
 * order, repeats allowed, a non-NULL list with count 0 is no rows; every row keeps begin <= end <= n, every index is
 * < n_records.  Columns may share one text and one table (two fields of one split).  Every column has the same row count
 * k = d_indices ? n_indices : n_records.  With P(c, j) the bytes of column c's row j:
 *     F(c, j) = P(c, j) padded to |width| bytes with the byte `pad`: a positive width pads on the LEFT (%7d), a negative one
 *               on the RIGHT (%-7s); width 0, or a piece already that long, adds nothing; nothing is ever truncated
 *     T(j)    = F(0, j) sep F(1, j) sep ... F(C-1, j)        sep: sep_len (0..64) HOST bytes, the same between every pair
 * and the layout is rj_scan_records_pack's with len(j) = |T(j)|:
 *     ob(0) = lead, ob(j + 1) = ob(j) + len(j) + gap, total = ob(k)       (k == 0: total = lead)
 *     d_out[ob(j), ob(j) + len(j)) = T(j); every other byte of d_out[0, total) = fill
 *     d_out_begin[j] = ob(j), d_out_end[j] = ob(j) + len(j)               (k uint64 each; either may be NULL)
 * With n_cols = 1 and width 0 the output is rj_scan_records_pack's for the same arguments, byte for byte and table row for
 * table row, whatever sep is.  The columns and the separator travel as kernel arguments: no upload, no allocation for them.
 * flags must be 0.  pad, fill: 0..255; gap may be 0.  d_out: 16-byte aligned, out_cap bytes.  Returns total WHATEVER out_cap
 * is and never writes at or beyond out_cap; d_out == NULL with out_cap == 0 is the size query (the tables are still written
 * when given).  With total <= out_cap the result is complete: every byte of [0, total) and every table row is written exactly
 * once, nothing has to be cleared first, nothing behind total or behind row k is touched.  The scan lends scratch only (8 +
 * 16 n_cols bytes per row): spans, stats and the state of its last rj_scan_records stay as they were.  One synchronise per call.
 * Refusals (RJ_BAD_ARGUMENT; a refused call writes no output byte and no table row): a bad index or a bad row in any column
 * -- the message names the first one, "row <j> column <c> ": the smallest j, and at that j the smallest c --; n_cols outside
 * 1..16; columns whose k differ (both are named); sep == NULL with sep_len > 0; sep_len > 64; |width| > 4096; reserved != 0;
 * any flag bit; pad or fill outside 0..255; a null text with n > 0, a null table with k > 0, a null d_out with out_cap > 0; a
 * table or index list that is not 8-byte aligned; a d_out that is not 16-byte aligned; R >= 2^42 with R = sum over the columns
 * of max(n, |width|) + (n_cols - 1) sep_len + gap, or lead + k R >= 2^62.  k >= 2^31: RJ_TOO_LARGE.  An output that overlaps
 * an input is undefined, as elsewhere in the family. */
typedef struct rj_zip_column {
  const void* d_text;
  uint64_t n;
  const uint64_t* d_rec_begin;
  const uint64_t* d_rec_end;
  uint64_t n_records;
  const uint64_t* d_indices; /* may be NULL */
  uint64_t n_indices;
  int32_t width;
  int32_t reserved; /* must be 0 */
} rj_zip_column;    /* 64 bytes */
int64_t rj_scan_records_zip(rj_scan* scan, const rj_zip_column* cols, int n_cols, const char* sep, uint64_t sep_len, int pad,
                            unsigned flags, int fill, uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap,
                            uint64_t* d_out_begin, uint64_t* d_out_end, void* hip_stream);
/* A column of int64 INSTANTS written AS TEXT (rejit_amd/csrc/record_time_format.hip): the inverse of
 * rj_scan_records_parse_time -- the buckets of "requests per minute" as `2026-10-20T17:15`, a time column that was filtered or
 * sorted on the device, Arrow's strftime / cast(timestamp[unit] -> utf8) -- as a new device text and its record table, without
 * a download.  Everything that is not about time is rj_scan_records_format's, word for word: d_value (n_values 64-bit words),
 * k = d_indices ? n_indices : n_values, r(j) = d_indices ? d_indices[j] : j (repeats allowed; a non-NULL list with count 0 is
 * no rows), row j's bytes T(j) made from d_value[r(j)], and the layout with len(j) = |T(j)|:
 *     ob(0) = lead, ob(j + 1) = ob(j) + len(j) + gap, total = ob(k)       (k == 0: total = lead)
 *     d_out[ob(j), ob(j) + len(j)) = T(j); every other byte of d_out[0, total) = fill
 *     d_out_begin[j] = ob(j), d_out_end[j] = ob(j) + len(j)               (k uint64 each; either may be NULL)
 * The value is an int64 count of `unit`s (RJ_TIME_SECOND .. RJ_TIME_NANO) since 1970-01-01T00:00:00Z.  Its civil instant is
 * floor(value / units per second) seconds plus a non-negative rest -- the floor goes toward minus infinity: -1 ns is
 * 1969-12-31T23:59:59.999999999 --, shifted by zone_minutes (-1439..1439, one fixed offset for the whole column; 0 is UTC) and
 * split by the inverse of the parse's days-from-civil: the 400-year-era formula in integers, no table of years.  `format`
 * (format_len bytes, 1..64; it need not end in a NUL, and a NUL inside is a literal) has the parse's own directives, every one
 * of a fixed width:
 *     %Y   4 digits, zero-padded                             %f   the unit's fraction digits: 3 under MILLI, 6 under MICRO, 9
 *     %m %d %H %M %S   2 digits each                              under NANO, six zeros under SECOND (Python's %f)
 *     %b   Jan..Dec                                          %z   +hhmm / -hhmm of zone_minutes, +0000 for 0 (Python's form; the
 *     %%   a `%`                                                  parse reads it back, its colon is optional)
 *     any other byte, NUL included: itself
 * Fields the format does not name are dropped, as strftime drops them: a floor to the finest named field.  Every OK row of a
 * call therefore has the SAME length L, which depends on the format and the unit only; the longest possible L is 77 (64 format
 * bytes, + 2 for %Y, + 1 for %b, + 7 for %f, + 3 for %z).  A row is the EMPTY row (zero bytes) in two cases:
 *     d_status given  d_status[r(j)] (n_values bytes: parse's status column, unchanged) is not RJ_PARSE_OK      (n_null)
 *     out of range    the SHIFTED instant's year is outside 0001..9999 -- never a nearby or wrapped value       (n_range)
 *                     Only SECOND, MILLI and MICRO can produce it: every int64 under NANO lies inside 1677..2262.
 * An OK row is, byte for byte, what Python's datetime.strftime writes for the same instant and format, with two differences:
 * %Y is isoformat()'s four digits (on glibc datetime(1, 1, 1).strftime('%Y') is '1'), and %f has the unit's digits, where
 * Python's datetime knows microseconds only.  For every format that names %Y, a month, %d, %H, %M, %S, and %f where the unit
 * is finer than a second (and %z unless zone_minutes is 0), rj_scan_records_parse_time of the output returns the value with
 * status OK.  `stats` (may be NULL) receives n_ok, n_null and n_range; they add up to k.
 * flags must be 0: every bit is refused.  fill: 0..255; gap may be 0.  d_out: 16-byte aligned, out_cap bytes.  Returns total
 * WHATEVER out_cap is and never writes at or beyond out_cap; d_out == NULL with out_cap == 0 is the size query (the tables are
 * still written when given).  With total <= out_cap the result is complete: every byte of [0, total) and every table row is
 * written exactly once, nothing has to be cleared first, nothing behind total or behind row k is touched.  The scan lends
 * scratch only (16 bytes per row): spans, stats and the state of its last rj_scan_records (rj_scan_records_select included)
 * stay as they were.  One synchronise per call.
 * Refusals (RJ_BAD_ARGUMENT; a refused call writes no output byte, no table row and no stats): rj_scan_records_format's -- an
 * index >= n_values, the message names the first bad row, "row <j> "; a null d_value with n_values > 0, a null d_out with
 * out_cap > 0; a table, d_value or d_indices that is not 8-byte aligned; a d_out that is not 16-byte aligned; any flag bit; a
 * fill outside 0..255 --; a null `format` with format_len > 0; a unit that is not RJ_TIME_*; zone_minutes outside -1439..1439;
 * a format that is refused, the message naming the byte offset, "format byte <i>: ": an empty format (0); more than 64 bytes
 * (64); an unknown directive or a `%` as the last byte (the `%`); a directive given twice, or %m together with %b (the second
 * one's `%`) -- the parse's two other refusals do not apply to writing: %f may stand before a digit, and `%H:%M` is a fine
 * format --; 77 + gap >= 2^42, or lead + k * (77 + gap) >= 2^62.  k >= 2^31: RJ_TOO_LARGE.  An output that overlaps an input
 * is undefined, as elsewhere in the family.
 * What stays out: %y %j %e %a %p, named zones and daylight saving, per-row offsets, locales, leap seconds. */
typedef struct rj_format_time_stats {
  uint64_t n_ok, n_null, n_range; /* they add up to k */
} rj_format_time_stats;
int64_t rj_scan_records_format_time(rj_scan* scan, const uint64_t* d_value, const uint8_t* d_status /* may be NULL */,
                                    uint64_t n_values, const uint64_t* d_indices, uint64_t n_indices, const char* format,
                                    uint64_t format_len, int unit, int zone_minutes, unsigned flags, int fill, uint64_t lead,
                                    uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin, uint64_t* d_out_end,
                                    rj_format_time_stats* stats /* may be NULL */, void* hip_stream);
/* The rows of a record table through a byte map and a drop set into a NEW packed device text (rejit_amd/csrc/
 * record_translate.hip): `tr A-Z a-z`, `tr -d '\r'`, pandas str.lower / str.upper / str.translate,
 * Arrow's ascii_lower / ascii_upper, Python's bytes.translate(table, delete) -- without a download, and in front of
 * rj_scan_records_group / _sort / _lookup their case-insensitive forms.  The contract is rj_scan_records_pack's, word for word;
 * only a row's bytes differ.  k, r(j), d_indices (any order, repeats allowed, non-NULL with n_indices == 0 is no rows), lead,
 * gap and fill are the pack's.  Row j's bytes are
 *     T(j) = bytes(text[rec_begin[r(j)], rec_end[r(j)])).translate(map, delete)       in Python's meaning:
 * a byte in the drop set is removed -- judged on the SOURCE byte, before the map -- and every other byte b becomes map[b]; a
 * NUL is an ordinary byte.  map: host, 256 bytes, NULL is the identity.  drop: host, 32 bytes = 256 bits, byte b is dropped
 * when bit (b & 7) of drop[b >> 3] is set; NULL drops nothing.  Both travel as kernel arguments: no upload, no allocation.
 * The layout is the pack's with len'(j) = |T(j)|:
 *     ob(0) = lead, ob(j + 1) = ob(j) + len'(j) + gap, total = ob(k)                    (k == 0: total = lead)
 *     d_out[ob(j), ob(j) + len'(j)) = T(j); every other byte of d_out[0, total) = fill
 *     d_out_begin[j] = ob(j), d_out_end[j] = ob(j) + len'(j)                            (k uint64 each; either may be NULL)
 * Returns total WHATEVER out_cap is and never writes at or beyond out_cap; d_out == NULL with out_cap == 0 is the size query
 * (the tables and the stats are still written).  With total <= out_cap every byte of [0, total) and every table row is
 * written exactly once, nothing has to be cleared first, nothing behind total or k is touched.  The scan lends scratch only:
 * its span list, its stats and the state of its last rj_scan_records (rj_scan_records_select included) stay as they were.
 * One synchronise per call.
 * Refusals (RJ_BAD_ARGUMENT) are the pack's: a null argument, a table that is not 8-byte aligned, d_out not 16-byte aligned,
 * fill outside 0..255, n + gap >= 2^42 or lead + k * (n + gap) >= 2^62 (also with gap 1), and an index >= n_records or a row
 * without begin <= end <= n: the message's "row <j> " names the first bad j.  A refused call writes no output byte and no
 * table row and is never led outside the text.  A d_out that overlaps the text is undefined, as elsewhere in the family.
 * What stays out: UTF-8 case mapping, `tr -s` (that is rj_scan_records_replace with `x+`), multi-byte maps, in-place
 * translation. */
typedef struct {
  uint64_t bytes_in;       /* source bytes of the k rows                          */
  uint64_t bytes_dropped;  /* of those, bytes in the drop set                     */
  uint64_t bytes_changed;  /* kept bytes b with map[b] != b                       */
} rj_translate_stats;
int64_t rj_scan_records_translate(rj_scan* scan, const void* d_text, uint64_t n, const uint64_t* d_rec_begin,
                                  const uint64_t* d_rec_end, uint64_t n_records, const uint64_t* d_indices, uint64_t n_indices,
                                  const uint8_t* map /* host, 256 bytes; NULL: identity */,
                                  const uint8_t* drop /* host, 32 bytes = 256 bits; NULL: none */, int fill, uint64_t lead,
                                  uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin, uint64_t* d_out_end,
                                  rj_translate_stats* stats /* may be NULL */, void* hip_stream);
/* The rows and fields of a device-resident CSV text with QUOTED fields (RFC 4180: the quote byte around a field, doubled inside
 * it) as record tables (rejit_amd/csrc/record_csv.hip) -- the family's front door for texts in which
 * a field may hold the delimiter or a line break.  Let ins(p) be the parity of the quote bytes in text[0, p) (quote == -1:
 * always 0).  Byte p is STRUCTURAL when ins(p) == 0 and it is the delimiter or \n.  Fields are the stretches between
 * structural bytes; a \n also ends a row; a \r directly before a row-ending \n belongs to neither.  A text that does not end
 * in a structural \n has a last row that ends at n, one that does has no extra row, n == 0 has no rows; every row has at
 * least one field (an empty line is one empty field).  For the raw field [fb, fe):
 *     begin = fb + 1 when fb < fe and text[fb] is the quote, else fb
 *     end   = fe - 1 when fe > begin, text[fe - 1] is the quote and the field is not the last one of a text with ins(n) == 1,
 *             else fe
 * and its flags are the OR over its bytes of
 *     RJ_CSV_BAD_QUOTE  a quote at p with ins(p) == 0 that is neither at fb nor directly behind a quote
 *     RJ_CSV_ESCAPED    a quote at p with ins(p) == 0, not at fb, directly behind a quote (the second byte of a `""`)
 *     RJ_CSV_BAD_CLOSE  a quote at p with ins(p) == 1 not followed by the text's end, the delimiter, \n, \r\n or a quote
 *     RJ_CSV_BARE_CR    a \r with ins(p) == 0 that is not followed by \n
 *     RJ_CSV_OPEN       on the last field when ins(n) == 1
 * If no field carries an RJ_CSV_MALFORMED flag, rows and values are those of Python's csv.reader(strict=True) exactly (a
 * field's value: its bytes, `""` read as `"` where it is ESCAPED; an empty line is ['']); otherwise every row before the
 * first flagged row is.  On flagged fields and behind them the rule above is the meaning.  With quote == -1 and no \r other
 * than in \r\n the fields are line.split(delimiter) of the lines.
 *     d_row_first[0] = 0, d_row_first[r + 1] = d_row_first[r] + (fields of row r)        (row_cap + 1 uint64: Arrow's offsets)
 *     d_row_begin[r], d_row_end[r]: the raw row without its line break                   (row_cap uint64 each)
 *     d_field_begin[f], d_field_end[f], d_field_flags[f]: field f in text order          (field_cap each; the flags 4 bytes)
 * Rows and fields ascend and do not overlap: each pair is a record table for every other call of the family.  Every table
 * may be NULL and is then not written.  Returns n_fields WHATEVER the caps are; never writes a row at or beyond row_cap or
 * a field at or beyond field_cap; all tables NULL with both caps 0 is the size query, and `stats` (host, required) is complete
 * in it too.  With n_rows <= row_cap and n_fields <= field_cap every entry below the counts is written exactly once as the
 * caller sees it (d_field_flags is cleared by the call), nothing has to be cleared first, nothing behind the counts is
 * touched.  The scan lends scratch only: its span list, its stats and the state of its last rj_scan_records stay as they
 * were.  One synchronise per call.  stats.first_bad: the offset of the first byte that raised BAD_QUOTE, BAD_CLOSE or
 * BARE_CR, n for a text that is only OPEN, UINT64_MAX when nothing is malformed.
 * Refusals (RJ_BAD_ARGUMENT, no byte written): a null scan, a null text with n > 0, stats == NULL, a table that is not 8-byte
 * aligned (the flags: 4-byte), delimiter outside 0..255, quote outside -1..255, delimiter or quote equal to \n or \r,
 * delimiter equal to quote, n >= 2^42.
 * What stays out: a text range other than [0, n), multi-byte delimiters, backslash escapes, skipinitialspace, comment lines,
 * skipping blank lines, header handling (drop row 0 with `indices`), type inference, and unescaping inside this call (pack
 * the fields, then rj_scan_records_replace `""` by `"`). */
typedef struct rj_csv_stats {
  uint64_t n_rows, n_fields;
  uint64_t n_quoted;     /* fields whose first raw byte is the quote byte                */
  uint64_t n_escapes;    /* doubled quotes inside quoted fields (events, not fields)     */
  uint64_t n_bad_quote, n_bad_close, n_bare_cr;   /* events                              */
  uint64_t open_at_end;  /* 1: the text ends inside quotes                               */
  uint64_t first_bad;    /* text offset of the first offending byte, UINT64_MAX: none    */
} rj_csv_stats;
enum { RJ_CSV_ESCAPED = 1, RJ_CSV_BAD_QUOTE = 2, RJ_CSV_BAD_CLOSE = 4, RJ_CSV_BARE_CR = 8, RJ_CSV_OPEN = 16 };
#define RJ_CSV_MALFORMED (RJ_CSV_BAD_QUOTE | RJ_CSV_BAD_CLOSE | RJ_CSV_BARE_CR | RJ_CSV_OPEN)
int64_t rj_scan_records_csv(rj_scan* scan, const void* d_text, uint64_t n, int delimiter, int quote /* -1: none */,
                            uint64_t* d_row_first /* row_cap + 1 */, uint64_t* d_row_begin, uint64_t* d_row_end /* row_cap each */,
                            uint64_t row_cap, uint64_t* d_field_begin, uint64_t* d_field_end,
                            uint32_t* d_field_flags /* field_cap each */, uint64_t field_cap, rj_csv_stats* stats /* host, required */,
                            void* hip_stream);
/* Several columns of records written AS QUOTED CSV LINES (rejit_amd/csrc/record_csv_format.hip): the
 * inverse of rj_scan_records_csv -- Python's csv.writer, Arrow's write_csv -- as a new device text and its record table,
 * without a download.  cols: n_cols (1..16) columns, a HOST array of rj_zip_column exactly as rj_scan_records_zip takes it
 * (rows as rj_scan_records_pack's: any order, repeats allowed, a non-NULL list with count 0 is no rows; columns may share a
 * text and a table; every column has the same row count k); width and reserved must be 0.  With P the bytes of column c's
 * row j, d = delimiter and q = quote (0..255 each, neither \n nor \r, different from each other):
 *     special(P)  P holds d, q, \r or \n
 *     need(c, j)  bit c of always_mask is set, or special(P), or n_cols == 1 and P is empty (csv.writer's lone empty field: "")
 *     F(c, j)     VALUE column (bit c of raw_mask clear): need ? q + P with every q doubled + q : P
 *                 RAW column (bit c of raw_mask set):     need ? q + P + q : P -- nothing is doubled: the caller states that P
 *                 is the interior of a field as rj_scan_records_csv delimits it, its "" still in place; for a field without
 *                 an RJ_CSV_MALFORMED flag this equals the value rule applied to the field's unescaped value
 *     T(j)        F(0, j) d F(1, j) d ... F(C-1, j)
 * and the layout is rj_scan_records_pack's with len(j) = |T(j)|:
 *     ob(0) = lead, ob(j + 1) = ob(j) + len(j) + gap, total = ob(k)       (k == 0: total = lead)
 *     d_out[ob(j), ob(j) + len(j)) = T(j); every other byte of d_out[0, total) = fill
 *     d_out_begin[j] = ob(j), d_out_end[j] = ob(j) + len(j)               (k uint64 each; either may be NULL)
 * With no always and no raw bits line j is what csv.writer(delimiter=d, quotechar=q, lineterminator="\r\n") writes for the
 * row, without its terminator; with all always bits the same under quoting=csv.QUOTE_ALL.  A NUL is an ordinary byte.  A
 * column may be in both masks.  With n_cols = 1 and no piece that needs quotes the output is rj_scan_records_pack's.
 * flags must be 0.  fill: 0..255; gap may be 0.  d_out: 16-byte aligned, out_cap bytes.  Returns total WHATEVER out_cap is and
 * never writes at or beyond out_cap; d_out == NULL with out_cap == 0 is the size query (the tables are still written when
 * given).  With total <= out_cap the result is complete: every byte of [0, total) and every table row is written exactly once,
 * nothing has to be cleared first, nothing behind total or behind row k is touched.  stats (host, may be NULL): n_rows = k,
 * n_fields = k n_cols, n_quoted = the fields with need, n_doubled = the quote bytes doubled, total.  Every piece's bytes are
 * read once to classify them and once to copy them (a value piece of 8 KiB or more with quote bytes inside once more, to count
 * them in front of every 4-KiB chunk of the output).  The scan lends scratch only (8 + 16 n_cols bytes per row and 16 bytes per
 * 4 KiB of min(out_cap, lead + k R) with the R of the refusals below -- pass the size query's total as out_cap, not "a large
 * number", where rows repeat long records --, shared with rj_scan_records_zip): spans, stats and the state of its last rj_scan_records stay as they were.
 * One synchronise per call.
 * Refusals (RJ_BAD_ARGUMENT; a refused call writes no output byte and no table row): a bad index or a bad row in any column
 * -- the message names the first one, "row <j> column <c> ": the smallest j, and at that j the smallest c --; n_cols outside
 * 1..16; columns whose k differ (both are named); width != 0; reserved != 0; any flag bit; fill, delimiter or quote outside
 * 0..255; a delimiter or quote that is \n or \r; delimiter == quote; a mask bit at or above n_cols; a null text with n > 0, a
 * null table with k > 0, a null d_out with out_cap > 0; a table or index list that is not 8-byte aligned; a d_out that is not
 * 16-byte aligned; R >= 2^42 with R = sum over the columns of (2 n + 2) + (n_cols - 1) + gap, or lead + k R >= 2^62.
 * k >= 2^31: RJ_TOO_LARGE.  An output that overlaps an input is undefined, as elsewhere in the family.
 * What stays out: no quoting at all (quote == -1) and escape characters -- rj_scan_records_zip joins without quoting;
 * QUOTE_NONNUMERIC as a mode (set always_mask for the columns that hold strings); multi-byte delimiters; a line terminator
 * other than what fill and gap give; per-row nulls; header lines. */
typedef struct rj_csv_format_stats {
  uint64_t n_rows, n_fields;
  uint64_t n_quoted;    /* fields written inside quotes                        */
  uint64_t n_doubled;   /* quote bytes doubled inside them (value columns)     */
  uint64_t total;
} rj_csv_format_stats;
int64_t rj_scan_records_format_csv(rj_scan* scan, const rj_zip_column* cols, int n_cols, int delimiter, int quote,
                                   uint32_t always_mask, uint32_t raw_mask, unsigned flags, int fill, uint64_t lead, uint64_t gap,
                                   void* d_out, uint64_t out_cap, uint64_t* d_out_begin, uint64_t* d_out_end,
                                   rj_csv_format_stats* stats /* host, may be NULL */, void* hip_stream);

/* ---- several patterns over the same device-resident text (regexdna: nine MatchAllCount calls on
 * one text, sample/regexdna.cc:56-70).  When every pattern has a nibble-form window set (DESIGN.md
 * section 4) the text is read ONCE for all of them; otherwise the patterns run one after another.
 * Results are those of rj_scan_run per pattern: rj_multi_scan(m, i) is an ordinary rj_scan holding
 * pattern i's spans / stats after rj_multi_run. */
typedef struct rj_multi rj_multi;   /* like rj_scan: per caller, NOT thread-safe */
int rj_multi_create(const rj_program* const* progs, int n_progs, rj_multi** out);
void rj_multi_destroy(rj_multi* multi);
/* counts[i] = matches of pattern i over d_text[0..n).  Returns how the set was run: 1 = one fused scan
 * kernel for all patterns; 3 = scan + classification + counting in one kernel (rj_multi_set_counts_only); 2 = one scan kernel per pattern queued back to back, then the verify /
 * gather tails of all patterns in two launches and a single synchronise (any set of fixed-window
 * patterns); 0 = one complete pipeline after the other; <0 = rj_status */
int rj_multi_run(rj_multi* multi, const void* d_text, uint64_t n, uint64_t* counts, void* hip_stream);
/* the same for the matches whose begin lies in [own_begin, own_end) -- a shard with its halo inside
 * [0, n), as for rj_scan_run; no selection state is carried in (first shard / independent ranges) */
int rj_multi_run_range(rj_multi* multi, const void* d_text, uint64_t n, uint64_t own_begin, uint64_t own_end,
                       uint64_t* counts, void* hip_stream);
/* rj_multi_run in two halves: rj_multi_start enqueues the run's kernels on hip_stream and returns, rj_multi_finish
 * waits for them and collects the counts (its return value is rj_multi_run's).  One run in flight per rj_multi; a
 * caller that alternates between TWO rj_multi objects of the same patterns keeps the device busy while the host
 * turns a result around (the reference's counterpart: regexdna-multithread.cc keeps one thread per pattern busy,
 * sample/regexdna-multithread.cc:65-78) -- bench.py's headline loop does that.  The text must stay unchanged until
 * rj_multi_finish.  [own_begin, own_end) as for rj_multi_run_range (0, n + 1: the whole text). */
int rj_multi_start(rj_multi* multi, const void* d_text, uint64_t n, uint64_t own_begin, uint64_t own_end, void* hip_stream);
int rj_multi_finish(rj_multi* multi, uint64_t* counts);
/* For two rj_multi objects run alternately on two streams: the scan kernel of `multi`'s runs is queued behind the
 * scan kernel of `before`'s run in flight (a stream-wait on that kernel's end), so that the two HBM-bound scans never
 * share the memory system while the latency-bound tails of one run execute under the scan of the other.  before =
 * NULL removes the order.  The objects must outlive each other's runs. */
int rj_multi_order_after(rj_multi* multi, rj_multi* before);
/* on != 0: rj_multi_start queues only the scan kernel on the caller's stream and everything behind it (the
 * latency-bound classify / gather tails) on a stream of the object's own, ordered by the scan kernel's end event.  A
 * caller that alternates two rj_multi objects on ONE stream then has the HBM-bound scan kernels back to back on that
 * stream -- in order, no cross-stream wait between them -- while each run's tails execute under the next scan.
 * rj_multi_finish is unchanged (it waits for the run's last kernel, wherever it is).  Not with mode 2. */
int rj_multi_set_tail_stream(rj_multi* multi, int on);
/* on != 0: the caller wants COUNTS -- what Regej::MatchAllCount answers (reference src/rejit.cc:203-208; regexdna asks
 * nothing else of its nine patterns, sample/regexdna.cc:65).  For the pattern sets the one-pass scan takes AND whose
 * patterns all match exactly 8 bytes within one byte of the scan's base windows (k-mers with one degenerate position,
 * both strands: regexdna's nine) rj_multi_run / _run_range / _start + _finish then run ONE kernel (plane_count.hip): the
 * text once, every candidate's eight bytes looked up in a table, nothing written but the counts.  Their return value is
 * 3 for such a run.  Afterwards counts[] and rj_multi_bounds / _bounds_device / rj_multi_device_counts work as ever (every
 * workgroup of the kernel records its first / last match per pattern: nothing is read again, the text may be gone);
 * rj_scan_device_spans(rj_multi_scan(m, i)) is NULL (no span list was made) and rj_scan_copy_spans / rj_scan_replace on it
 * return RJ_BAD_ARGUMENT.  Exactness: the counts are those of the left-most-longest, non-overlapping selection.  Two matches
 * of ONE pattern fewer than 8 bytes apart (`agggtaaagggtaaa`) are resolved inside the kernel when they form an isolated
 * pair; a longer chain of such neighbours, or a pair across two waves' spans, makes the kernel void its run, and THAT call
 * is answered by the span pipeline (return value 1) -- the next call tries the kernel again.  Any other pattern set ignores
 * the switch.  An rj_multi of ONE pattern takes the switch too.
 * Returns 1 when runs will take the one-kernel path, 0 when the set does not have the shape, < 0 rj_status. */
int rj_multi_set_counts_only(rj_multi* multi, int on);
/* rj_scan_set_timing for every pattern of the object (rj_multi_scan_ms reads 0 when off).  On the one-kernel counts path the
 * duration comes from the device's wall clock and switching it on puts nothing on the stream (see rj_scan_set_timing). */
int rj_multi_set_timing(rj_multi* multi, int on);
rj_scan* rj_multi_scan(rj_multi* multi, int i);
/* First and last match of every pattern's result after rj_multi_run / _run_range: bounds[4*i .. 4*i+3] =
 * first begin, first end, last begin, last end (all UINT64_MAX when pattern i has no match).  This is what
 * neighbouring shards exchange to carry the left-most-longest selection over a cut: a shard whose first
 * match begins before its left neighbour's last end re-runs that pattern with rj_scan_run(rj_multi_scan(m, i),
 * ..., carry) -- 32 bytes per pattern instead of the match list. */
int rj_multi_bounds(rj_multi* multi, uint64_t* bounds, void* hip_stream);
/* The rows of an exchange that stays on the device (one process per GPU, torch.distributed / RCCL): d_rows[8 * i ..]
 * = what a rank contributes per pattern to the carry exchange between shards: count | first begin, first end (written
 * only when first_round != 0: the result under the empty carry) | last begin, last end (-1 without a match) | the
 * carry the result was selected under (cur, prev_end, have: zeroed when first_round != 0, kept by the caller when
 * it re-runs a pattern); begins and ends plus `offset` (the shard's position in the whole text).  Written by a kernel
 * queued on hip_stream -- no synchronisation, the collective that gathers the rows is queued behind it. */
int rj_multi_bounds_device(rj_multi* multi, int64_t offset, int first_round, int64_t* d_rows, void* hip_stream);
/* The decision every rank takes from the gathered rows d_all[world][n_patterns][8] = count, first begin / end under
 * the EMPTY carry, current last begin / end, carry the current result was selected under (cur, prev_end, have):
 * out (device or pinned host memory, 4 * n_patterns + 1 integers) = job-wide counts | 1 where `rank` has to select
 * the pattern again | the (cur, prev_end) to select it under | 1 when any rank re-runs anything.  One kernel on
 * hip_stream; the caller synchronises once per round. */
int rj_carry_decide(const int64_t* d_all, int world, int rank, int n_patterns, int64_t* out, void* hip_stream);
/* The whole exchange step behind one call, for C++ callers with one process (or thread) per GPU and one shard of the
 * text resident on each (the reference's counterpart is the per-pattern thread pool of sample/regexdna-multithread.cc:
 * 65-78; across devices the unit is the byte range): runs the patterns over this rank's shard (arguments as for
 * rj_multi_run_range; `offset` = the position of d_text[0] in the whole text), then carries the left-most-longest
 * selection over the cuts -- per round one all-gather of 8 integers per pattern, written and evaluated by kernels on
 * hip_stream, one synchronise -- re-running the (rare) pattern whose first match begins inside its left neighbour's
 * last one.  counts[i] = matches of pattern i over the WHOLE text, on every rank; rj_multi_scan(m, i) holds this
 * shard's final spans.  rccl_comm is the caller's ncclComm_t (RCCL is bound with dlopen at the first call: the copy
 * the process has loaded already, else librccl.so.1 / $RJ_RCCL_LIBRARY); every rank of the communicator must call.
 * Ring-artefact-risk patterns need their shard's buffer to reach the end of the text (rj_program_info). */
int rj_multi_device_counts(rj_multi* multi, const void* d_text, uint64_t n, uint64_t own_begin, uint64_t own_end,
                           int64_t offset, void* rccl_comm, int rank, int world, uint64_t* counts, void* hip_stream);
/* The same over any all-gather: d_send (bytes_per_rank bytes, device) of every rank, in rank order, into d_recv
 * (world * bytes_per_rank bytes, device), queued on hip_stream or complete on return; 0 = success. */
typedef int (*rj_allgather_fn)(void* ctx, const void* d_send, void* d_recv, uint64_t bytes_per_rank, void* hip_stream);
int rj_multi_device_counts_via(rj_multi* multi, const void* d_text, uint64_t n, uint64_t own_begin, uint64_t own_end,
                               int64_t offset, rj_allgather_fn allgather, void* ctx, int rank, int world, uint64_t* counts,
                               void* hip_stream);

/* MatchAll of ONE pattern over a text that is sharded across ranks (one process or thread per GPU, a shard of the text
 * resident on each), the ordered match list gathered on `root` -- SURVEY 8e / BASELINE configs[3] (the complex regex
 * over 50 GB on 8 GPUs); the reference's result is that list (src/codegen.cc:36-86, include/rejit.h:65-68).  Arguments
 * as for rj_multi_device_counts: this rank owns the match begins [own_begin, own_end) of its buffer d_text[0..n), which
 * starts at `offset` of the whole text and holds a halo of max_len - 1 bytes behind own_end.  Runs the shard, carries
 * the left-most-longest selection over the cuts (rounds of one 64-byte all-gather), then every rank sends its pairs --
 * as GLOBAL offsets -- straight to their place in the root's list (ncclSend / ncclRecv in one group: peer -> root, no
 * ring).  Returns the job-wide number of matches on every rank (or rj_status); on `root`
 * rj_scan_gathered_spans(scan, &count) is the device pointer to the 2 * count offsets in text order (valid until the
 * scan's next run), NULL elsewhere.  rj_scan_device_spans(scan) stays this shard's own (local) result. */
int64_t rj_scan_gather_spans(rj_scan* scan, const void* d_text, uint64_t n, uint64_t own_begin, uint64_t own_end, int64_t offset,
                             void* rccl_comm, int rank, int world, int root, void* hip_stream);
/* The same over any pair of collectives (MPI, a test harness with several shards on one device): the all-gather of
 * rj_multi_device_counts_via, and a gather of byte ranges to the root -- d_send[0..send_bytes) of every rank to
 * d_recv + recv_offsets[rank] on the root (d_recv is NULL elsewhere; recv_offsets / recv_bytes list all ranks, on all
 * ranks), queued on hip_stream or complete on return; 0 = success. */
typedef int (*rj_gatherv_fn)(void* ctx, const void* d_send, uint64_t send_bytes, void* d_recv, const uint64_t* recv_offsets,
                             const uint64_t* recv_bytes, int root, void* hip_stream);
int64_t rj_scan_gather_spans_via(rj_scan* scan, const void* d_text, uint64_t n, uint64_t own_begin, uint64_t own_end, int64_t offset,
                                 rj_allgather_fn allgather, rj_gatherv_fn gatherv, void* ctx, int rank, int world, int root, void* hip_stream);
const uint64_t* rj_scan_gathered_spans(const rj_scan* scan, uint64_t* count);
/* a copy of that list (host_spans: host or device memory, cap pairs at most); returns the number of pairs gathered (0 on a
 * rank that is not the root) or rj_status */
int64_t rj_scan_copy_gathered_spans(const rj_scan* scan, uint64_t* host_spans, uint64_t cap);
/* mode 0 (default): fuse when possible; mode 1: never fuse -- every pattern scans the whole text on its own,
 * all of them in ONE launch when the patterns have the regexdna shape (scan_windows_train), else one kernel
 * per pattern back to back on the caller's stream; mode 2: one kernel per pattern, alternating between the
 * caller's stream and a second one so that consecutive kernels overlap at their boundaries; mode 3: one
 * kernel per pattern back to back (measurement: the per-kernel HBM roofline); mode 4: mode 0 with the scan and
 * the classification of its candidates in ONE kernel (round 4: measured no faster, kept selectable) */
int rj_multi_set_mode(rj_multi* multi, int mode);
/* duration of the last run's scan kernel(s) in ms, summed (0 when the patterns ran one by one) */
float rj_multi_scan_ms(const rj_multi* multi);

/* number of visible HIP devices (0 when there is none), for callers that want to probe */
int rj_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* REJIT_HIP_H_ */
