// rejit_amd/csrc/record_csv_format.hip -- rj_scan_records_format_csv: the rows of up to 16 record tables put side by side into
// the lines of a NEW contiguous device text with its record table, every field quoted exactly where Python's csv.writer quotes
// it, laid out as rj_scan_records_pack lays records out -- the inverse of rj_scan_records_csv, without a download.
// record_csv_format.h has the rule and the arithmetic.  The columns, the delimiter, the quote and the masks are kernel
// ARGUMENTS.  Two memsets (the summary, the look-back's words) and four launches on one stream, one synchronise:
//
// Classify: one lane per output row.  The lane resolves its C rows with record_rows.h's resolver and reads every piece's bytes
//   ONCE, 16 at a time: is one of them the delimiter, the quote, \r or \n, and how many are the quote.  A piece of
//   csvf::kWaveBytes or more is taken by the lane's whole wave instead, 64 lanes x 16 bytes a step (the two tiers of the group
//   call's hash pass).  It stages 16 bytes per piece (source, length, quote count, need), the row's length, and leaves the
//   first bad (row, column) in the summary: one atomic max per wave.  It writes no table row: the check stands in front of the plan.
// Plan: record_frame.h's plan_staged_lengths (plan_units over the staged lengths); ob / oe and the total.  Returns at once behind a bad row.
// Checkpoint: returns at once unless the classify met an expanding piece of csvf::kCheckpointBytes or more.  A wave per row:
//   lane c places column c's field from the staged pieces (a wave prefix sum of the field lengths), and every such piece is
//   walked ONCE by the wave, 64 lanes x 16 bytes a step, counting its quote bytes: where a step's output holds a chunk's first
//   byte, it leaves (the step, the quote bytes in front of it) as that chunk's checkpoint -- 16 bytes per 4-KiB chunk of
//   min(out_cap, lead + k R), the most the emit can write.  A chunk's first byte lies in one piece at the most: every entry has one writer, and nothing is cleared first.
// Emit: record_frame.h's emit_chunks -- output-major and persistent in chunks of 4 KiB through an image in LDS --, the zip's policy
//   with three tiers (csvf::tier_of) and a phase between the rows and the store:
//     bytes   every row of the chunk once, by its own lane: delimiters, the quotes around a field, the short pieces (doubled
//             inline), the partial groups at the two ends of a piece that streams (csvf::row_edges)
//     expand  a long value piece with quote bytes inside: the row's lane only lists it; then one wave per listed piece walks
//             its source 64 lanes x 16 bytes a step, a lane's output offset being its source offset plus the wave prefix sum
//             of the quote counts in front of it, and writes the bytes that land in the chunk into the image
//             (csvf::expand_group).  A chunk that begins inside such a piece starts the walk at its CHECKPOINT (below); inside
//             a piece shorter than csvf::kCheckpointBytes it walks the few steps in front of it too, counting only.  No
//             single lane ever loops over a long piece's length, and no piece is walked more than three times
//     stream  only in a chunk that a streaming piece touches: every lane looks up the row around its OWN 16 output bytes and,
//             where one such piece covers them whole, takes 16 source bytes through DeviceText's streaming read
//   and every lane stores its 16 aligned bytes: the streamed ones, else the image's.  Plain vector stores, no byte stores to
//   memory but the last group's below the total, no atomics on memory (the chunk's list is counted in LDS).
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_csv_format.h"
#include "record_frame.h"
#include "record_rows.h"

namespace rejit_amd {

namespace {

static_assert(csvf::kEmitChunk == kImageChunk, "the header's chunk is the frame's");
static_assert(csvf::kWaveStep == kWave * rows::kGroupBytes, "a wave's step is 64 lanes x 16 bytes");

// the call's counts in the summary (words the frame's calls leave to their callers)
enum { kSumQuoted = kSumKept, kSumDoubled = kSumMatching, kSumCheckpointed = kSumSelected };

// One step of the expand walk: the lane's group of the kWaveStep source bytes at s of the piece (w, *valid of its bytes), its
// quote bytes (*qbits) and how many quote bytes of the step lie in the lanes below (*below).  Returns the step's quote bytes
// (wave-uniform).
__device__ __forceinline__ uint32_t walk_step(const DeviceText& text, const csvf::Piece& pc, uint64_t s, int lane, uint32_t quote, uint32_t w[4],
                                              uint32_t* valid, uint32_t* qbits, uint32_t* below) {
  const uint64_t g = s + static_cast<uint64_t>(lane) * rows::kGroupBytes;
  *valid = g >= pc.len ? 0u : pc.len - g < rows::kGroupBytes ? static_cast<uint32_t>(pc.len - g) : 16u;
  w[0] = w[1] = w[2] = w[3] = 0;
  if (*valid) rows::load_at(text, text.n, pc.src + g, w);
  *qbits = *valid ? csvf::quote_bits(w, *valid, quote) : 0u;
  const uint32_t mine = csv::popcount(*qbits);
  const uint32_t through = wave_inclusive_sum(mine);
  *below = through - mine;
  return wave_last_lane(through);
}

__global__ __launch_bounds__(kThreads) void record_csv_format_classify_kernel(const csvf::Columns cols, uint32_t n_cols, uint32_t delimiter, uint32_t quote,
                                                                              uint32_t always_mask, uint32_t raw_mask, uint64_t k, uint64_t n_units,
                                                                              csvf::Staged* __restrict__ stage, uint64_t* __restrict__ row_len,
                                                                              unsigned long long* summary, uint32_t want_stats) {
  const int lane = lane_id();
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    bool good = j < k, bad = false;
    uint32_t bad_col = 0;
    uint64_t len = 0, quoted = 0, doubled = 0;
    for (uint32_t c = 0; c < n_cols; c++) {   // (every lane of the wave runs every column: the long pieces are the wave's)
      const csvf::Column& col = cols.col[c];
      const DeviceText text{col.text, col.n};
      rows::Row row{false, 0, 0};
      if (good) {
        row = rows::resolve(col.rec_begin, col.rec_end, col.indices, col.n_records, col.n, j);
        if (row.bad) good = false, bad = true, bad_col = c;
      }
      const uint64_t piece_len = good ? row.len() : 0;
      const bool wide = good && piece_len >= csvf::kWaveBytes;
      bool special = false;
      uint64_t quotes = 0;
      if (good && !wide) csvf::classify_groups(text, col.n, row.rb, piece_len, 0, 1, delimiter, quote, &special, &quotes);
      for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1) {   // a long piece: the wave walks it, its lane keeps the result
        const int owner = __builtin_ctzll(todo);
        const uint64_t src = lane_value(row.rb, owner), src_len = lane_value(piece_len, owner);
        bool sp = false;
        uint64_t qs = 0;
        csvf::classify_groups(text, col.n, src, src_len, static_cast<uint64_t>(lane), kWave, delimiter, quote, &sp, &qs);
        const bool any = __ballot(sp) != 0;
        const uint64_t sum = wave_sum64(qs);
        if (lane == owner) special = any, quotes = sum;
      }
      if (good) {
        const csvf::Piece pc{row.rb, piece_len, quotes, csvf::need_quotes(n_cols, always_mask, c, piece_len, special)};
        const bool raw = csvf::is_raw(raw_mask, c);
        if (stage) stage[j * n_cols + c] = csvf::stage_piece(pc);
        len += csvf::field_length(c, pc, raw);
        quoted += pc.need ? 1 : 0;
        doubled += csvf::doubles(pc, raw) ? quotes : 0;
        if (csvf::checkpointed(pc, raw)) summary[kSumCheckpointed] = 1;   // (every writer writes 1)
      }
    }
    if (j < k) row_len[j] = len;
    note_bad_word(bad, zip::bad_word(j, bad_col), &summary[kSumBadWord]);
    if (want_stats) {   // one add per wave and word (a refused call's counts are not read)
      const uint64_t q = wave_sum64(good ? quoted : 0), d = wave_sum64(good ? doubled : 0);
      if (lane == 0 && q) atomicAdd(&summary[kSumQuoted], static_cast<unsigned long long>(q));
      if (lane == 0 && d) atomicAdd(&summary[kSumDoubled], static_cast<unsigned long long>(d));
    }
  }
}

__global__ __launch_bounds__(kThreads) void record_csv_format_plan_kernel(const uint64_t* __restrict__ row_len, uint64_t k, uint64_t lead, uint64_t gap,
                                                                          unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                                          uint64_t* __restrict__ out_begin, uint64_t* __restrict__ out_end,
                                                                          unsigned long long* summary) {
  plan_staged_lengths(row_len, k, lead, gap, granules, ticket, n_units, out_begin, out_end, summary);
}

// record_csv_format.h's Source over the kernel's arguments and the stage
struct DeviceSource {
  const csvf::Columns& cols;
  const csvf::Staged* __restrict__ stage;
  uint32_t n_cols;
  __device__ __forceinline__ csvf::Piece piece(uint64_t j, uint32_t c) const {
    const ulonglong2 v = reinterpret_cast<const ulonglong2*>(stage)[j * n_cols + c];
    return csvf::staged_piece(csvf::Staged{v.x, v.y});
  }
  __device__ __forceinline__ uint32_t text_byte(uint32_t c, uint64_t s) const { return cols.col[c].text[s]; }
  __device__ __forceinline__ void load16(uint32_t c, uint64_t s, uint32_t w[4]) const { DeviceText{cols.col[c].text, cols.col[c].n}.load16(s, w); }
};

__global__ __launch_bounds__(kThreads) void record_csv_format_checkpoint_kernel(const csvf::Columns cols, uint32_t n_cols, uint32_t quote, uint32_t raw_mask,
                                                                                const csvf::Staged* __restrict__ stage, uint64_t k,
                                                                                const uint64_t* __restrict__ ob, uint64_t out_cap,
                                                                                csvf::Checkpoint* __restrict__ checkpoints, const unsigned long long* summary) {
  if (refused(summary) || summary[kSumCheckpointed] == 0) return;
  const uint64_t total = summary[kSumTotal];
  const uint64_t limit = total < out_cap ? total : out_cap;
  const int lane = lane_id();
  const DeviceSource src{cols, stage, n_cols};
  const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); j < k; j += n_waves) {
    const bool mine = static_cast<uint32_t>(lane) < n_cols;
    const uint32_t c = mine ? static_cast<uint32_t>(lane) : 0u;   // (a lane without a column computes column 0's places and drops them)
    const csvf::Piece own = mine ? src.piece(j, c) : csvf::Piece{0, 0, 0, false};
    const bool raw = csvf::is_raw(raw_mask, c);
    const uint64_t own_len = mine ? csvf::field_length(c, own, raw) : 0;
    const uint64_t at = ob[j] + wave_inclusive_sum64(own_len) - own_len;
    const uint64_t own_data0 = csvf::field_at(at, c, own, raw).data0;
    for (uint64_t todo = __ballot(mine && csvf::checkpointed(own, raw) && own_data0 < limit); todo; todo &= todo - 1) {
      const int owner = __builtin_ctzll(todo);
      const csvf::Piece pc{lane_value(own.src, owner), lane_value(own.len, owner), 0, true};
      const uint64_t data0 = lane_value(own_data0, owner);
      const DeviceText text{cols.col[owner].text, cols.col[owner].n};
      uint64_t before = 0;
      for (uint64_t s = 0; s < pc.len; s += csvf::kWaveStep) {
        const uint64_t step_out = data0 + s + before;
        if (step_out >= limit) break;
        uint32_t w[4], valid, qbits, below;
        const uint32_t in_step = walk_step(text, pc, s, lane, quote, w, &valid, &qbits, &below);
        const uint64_t step_bytes = pc.len - s < csvf::kWaveStep ? pc.len - s : csvf::kWaveStep;
        const uint64_t step_end = step_out + step_bytes + in_step;   // (at most 2 kWaveStep behind step_out: one boundary at the most)
        const uint64_t b = csvf::boundary_from(step_out, csvf::kEmitChunk);
        if (lane == 0 && b < step_end && b < limit) checkpoints[b / csvf::kEmitChunk] = csvf::Checkpoint{s, before};
        before += in_step;
      }
    }
  }
}

// The emit: record_frame.h's emit_chunks with the zip's stream tier and, between the rows and the store, the expand walk over
// the pieces the rows' lanes listed (the chunk's list, LDS).
struct ExpandList {
  uint64_t row[csvf::kMaxExpand], at[csvf::kMaxExpand];
  uint32_t col[csvf::kMaxExpand];
};
struct CsvFormatEmit : StreamingImagePolicy {
  uint32_t& s_expands;   // the pieces listed (they fit: kMaxExpand's assert)
  ExpandList& list;
  const csvf::Columns& cols;
  const DeviceSource& src;
  const uint64_t* __restrict__ ob;
  const csvf::Checkpoint* __restrict__ checkpoints;
  uint32_t n_cols, delimiter, quote, raw_mask;
  int lane;   // (made once in front of the chunks: made in `between`, the walk's loop compiles to other, slower code)
  __device__ __forceinline__ void reset() const { s_streams = 0, s_expands = 0; }
  // bytes: the row's edges; the pieces that expand are listed
  __device__ __forceinline__ bool row(uint64_t j, uint64_t c0, uint64_t c1, const ImagePut& put) const {
    const uint64_t at = ob[j];
    if (at >= c1) return false;
    return csvf::row_edges(src, n_cols, delimiter, quote, raw_mask, j, at, c0, c1, put, [&](uint64_t row, uint32_t col, uint64_t data0) {
      const uint32_t i = atomicAdd(&s_expands, 1u);   // (LDS)
      if (i < csvf::kMaxExpand) list.row[i] = row, list.at[i] = data0, list.col[i] = col;
    });
  }
  // expand: a wave per listed piece
  __device__ __forceinline__ void between(uint64_t c, uint64_t c0, uint64_t c1, const ImagePut& put) const {
    const uint32_t n_expands = s_expands < csvf::kMaxExpand ? s_expands : csvf::kMaxExpand;   // workgroup-uniform
    if (!n_expands) return;
    for (uint32_t i = threadIdx.x >> 6; i < n_expands; i += kWaves) {
      const uint32_t col = list.col[i];
      const uint64_t data0 = list.at[i];
      const csvf::Piece pc = src.piece(list.row[i], col);
      const DeviceText text{cols.col[col].text, cols.col[col].n};
      const csvf::Checkpoint from = csvf::resumes(pc, csvf::is_raw(raw_mask, col), data0, c0) ? checkpoints[c] : csvf::Checkpoint{0, 0};
      uint64_t before = from.before;   // the quote bytes of the piece in front of the step
      for (uint64_t s = from.s; s < pc.len; s += csvf::kWaveStep) {
        const uint64_t step_out = data0 + s + before;
        if (step_out >= c1) break;
        uint32_t w[4], valid, qbits, below;
        const uint32_t in_step = walk_step(text, pc, s, lane, quote, w, &valid, &qbits, &below);
        const uint64_t step_bytes = pc.len - s < csvf::kWaveStep ? pc.len - s : csvf::kWaveStep;
        if (valid && step_out + step_bytes + in_step > c0)
          csvf::expand_group(w, valid, qbits, quote, step_out + static_cast<uint64_t>(lane) * rows::kGroupBytes + below, c0, c1, put);
        before += in_step;
      }
    }
    __syncthreads();
  }
  __device__ __forceinline__ bool group16(uint64_t j, uint64_t at, uint64_t p, uint32_t w[4]) const {
    return csvf::group_streamed(src, n_cols, raw_mask, j, at, p, w);
  }
};
__global__ __launch_bounds__(kThreads) void record_csv_format_emit_kernel(const csvf::Columns cols, uint32_t n_cols, uint32_t delimiter, uint32_t quote,
                                                                          uint32_t raw_mask, const csvf::Staged* __restrict__ stage, uint64_t k,
                                                                          const uint64_t* __restrict__ ob, const csvf::Checkpoint* __restrict__ checkpoints,
                                                                          uint32_t fill, uint8_t* __restrict__ out, uint64_t out_cap,
                                                                          const unsigned long long* summary) {
  __shared__ uint32_t s_streams, s_expands;
  __shared__ ExpandList s_list;
  const DeviceSource src{cols, stage, n_cols};
  emit_chunks(CsvFormatEmit{StreamingImagePolicy(s_streams), s_expands, s_list, cols, src, ob, checkpoints, n_cols, delimiter, quote, raw_mask, lane_id()}, k, ob, fill, out,
              out_cap, summary);
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_format_csv(rj_scan* s, const rj_zip_column* columns, int n_cols, int delimiter, int quote, uint32_t always_mask, uint32_t raw_mask,
                                   unsigned flags, int fill, uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin,
                                   uint64_t* d_out_end, rj_csv_format_stats* stats, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_format_csv";
  static_assert(sizeof(rj_zip_column) == sizeof(csvf::Column), "record_zip.h's Column is rj_zip_column");
  if (!s) return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", kCall);
  const csvf::Column* given = reinterpret_cast<const csvf::Column*>(columns);
  const csvf::Refusal why = csvf::check_call(given, n_cols, delimiter, quote, always_mask, raw_mask, flags, fill, lead, gap, d_out, out_cap, d_out_begin, d_out_end);
  const uint64_t k = given && n_cols >= 1 ? zip::rows_of(given[0]) : 0;
  if (why.code != csvf::kFine) {
    char msg[320];
    csvf::refusal_message(msg, sizeof(msg), kCall, why, k, n_cols);
    return rj_fail(why.code == csvf::kTooManyRows ? RJ_TOO_LARGE : RJ_BAD_ARGUMENT, "%s", msg);
  }
  csvf::Columns cols = {};
  for (int c = 0; c < n_cols; c++) cols.col[c] = given[c];
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  const bool copies = out_cap != 0;
  // what the emit can write: the caller's out_cap may be any "large enough" number, the output is never longer than lead + k R
  const uint64_t most = csvf::most_total(k, given, n_cols, lead, gap), most_bytes = out_cap < most ? out_cap : most;
  const uint32_t C = static_cast<uint32_t>(n_cols);
  int rc;
  uint64_t *ob = nullptr, *row_len = nullptr;
  csvf::Staged* stage = nullptr;
  csvf::Checkpoint* checkpoints = nullptr;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, then the look-back's words
  if ((rc = pack_begin_table(s, d_out_begin, copies, k, &ob)) != RJ_OK) return rc;
  if (k) {   // the rows' lengths, then (a call that copies) the pieces and a checkpoint per chunk of min(out_cap, lead + k R): the zip's scratch
    const uint64_t len_bytes = rows::align16(k * sizeof(uint64_t)), stage_bytes = copies ? k * C * sizeof(csvf::Staged) : 0;
    RJ_HIP(s->rec_zip_stage.reserve(len_bytes + stage_bytes + (copies ? chunks_of(most_bytes, kImageChunk) * sizeof(csvf::Checkpoint) : 0)));
    row_len = s->rec_zip_stage.as<uint64_t>();
    if (copies) {
      stage = reinterpret_cast<csvf::Staged*>(s->rec_zip_stage.as<uint8_t>() + len_bytes);
      checkpoints = reinterpret_cast<csvf::Checkpoint*>(s->rec_zip_stage.as<uint8_t>() + len_bytes + stage_bytes);
    }
  }
  if ((rc = records_begin(s, 1 + lookback::granule_words(n_units), st, &scratch, &summary)) != RJ_OK) return rc;
  const dim3 block(kThreads), units(unit_grid(n_units));
  if (k)
    hipLaunchKernelGGL(record_csv_format_classify_kernel, units, block, 0, st, cols, C, static_cast<uint32_t>(delimiter), static_cast<uint32_t>(quote),
                       always_mask, raw_mask, k, n_units, stage, row_len, summary, stats ? 1u : 0u);
  hipLaunchKernelGGL(record_csv_format_plan_kernel, units, block, 0, st, static_cast<const uint64_t*>(row_len), k, lead, gap, scratch + 1, scratch, n_units,
                     ob, d_out_end, summary);
  if (copies && k) {
    const uint64_t row_groups = (k + kWaves - 1) / kWaves;   // a wave per row
    hipLaunchKernelGGL(record_csv_format_checkpoint_kernel, dim3(unit_grid(row_groups)), block, 0, st, cols, C, static_cast<uint32_t>(quote), raw_mask,
                       static_cast<const csvf::Staged*>(stage), k, static_cast<const uint64_t*>(ob), out_cap, checkpoints, summary);
  }
  if (copies)
    hipLaunchKernelGGL(record_csv_format_emit_kernel, dim3(image_grid(most_bytes)), block, 0, st, cols, C, static_cast<uint32_t>(delimiter),
                       static_cast<uint32_t>(quote), raw_mask, static_cast<const csvf::Staged*>(stage), k, static_cast<const uint64_t*>(ob),
                       static_cast<const csvf::Checkpoint*>(checkpoints), static_cast<uint32_t>(fill), static_cast<uint8_t*>(d_out), out_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0) {
    char msg[320];
    csvf::bad_row_message(msg, sizeof(msg), kCall, s->rec_host[kSumBadWord]);
    return rj_fail(RJ_BAD_ARGUMENT, "%s", msg);
  }
  if (stats) {
    stats->n_rows = k;
    stats->n_fields = k * C;
    stats->n_quoted = s->rec_host[kSumQuoted];
    stats->n_doubled = s->rec_host[kSumDoubled];
    stats->total = s->rec_host[kSumTotal];
  }
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
