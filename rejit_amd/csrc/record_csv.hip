// rejit_amd/csrc/record_csv.hip -- rj_scan_records_csv: the rows and fields of a device-resident CSV text with quoted fields
// as record tables (row offsets in the Arrow style, the raw rows, the fields without their quotes, a word of flags per
// field).  record_csv.h has the arithmetic and the rule.  One memset (the stats words) and three or four launches on one
// stream, one synchronise; no look-back, no ticket: nothing waits for another workgroup.
//
// Summarise: every wave of the grid owns one contiguous span of the text (whole units of RJ_CSV_UNIT bytes) and streams it
//   once, 16 bytes per lane and step: the masks of quote, delimiter and \n, the lane's summary under both entry parities, the
//   lanes' parities joined by one ballot, the step's counts by two wave sums.  It leaves one Summary per span.
// Resolve: one wave composes the spans' summaries in order (at most a few thousand): every span's entry -- ins() at its
//   first byte, the structural bytes and the row ends before it -- and the counts.  It writes row_first[0].
// Clear:  field_flags below min(n_fields, field_cap) zeroed (the counts are on the device only: no memset from the host).
// Emit:   the same walk with the entry known and a halo of one byte back and two ahead from the neighbouring lanes: every
//   lane knows the field and row number of each of its bytes (the wave's running counts + a prefix sum over the lanes + a
//   popcount), writes the tables' entries its structural bytes own (csv::emit_group), ORs the events' flags into their
//   fields atomically and counts the events.  In a size query it only counts.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_csv.h"
#include "record_frame.h"

namespace rejit_amd {

namespace {

static_assert(csv::kLanes == kWave && csv::kWavesPerGroup == kWaves, "a wave takes a step, a workgroup has four");
static_assert(csv::kUnit % csv::kStep == 0, "a span is whole steps, but for the text's end");

// the stats words (device, and their pinned copy)
enum { kCsvRows = 0, kCsvFields, kCsvQuoted, kCsvEscapes, kCsvBadQuote, kCsvBadClose, kCsvBareCr, kCsvOpen, kCsvFirstBad, kCsvWords = 16 };

struct Walk {
  const uint8_t* text;
  uint64_t n, unit;
  int delimiter, quote;
  csv::Geometry geo;
};

// the lane's 16 bytes of the step at p (no halo); beyond the span's end: nothing
__device__ __forceinline__ csv::Group load_core(const DeviceText& src, uint64_t p0, uint64_t span_end) {
  csv::Group g;
  g.w[0] = g.w[1] = g.w[2] = g.w[3] = 0;
  g.prev = g.next1 = g.next2 = -1;
  g.valid = p0 >= span_end ? 0u : span_end - p0 < csv::kGroup ? static_cast<uint32_t>(span_end - p0) : csv::kGroup;
  if (g.valid == csv::kGroup) src.load16(p0, g.w);
  else if (g.valid != 0) src.load16_guarded(p0, g.w);
  return g;
}

__global__ __launch_bounds__(kThreads) void record_csv_summarise_kernel(const Walk W, csv::Summary* __restrict__ summaries) {
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (wave >= W.geo.waves) return;
  const int lane = lane_id();
  const uint64_t s0 = csv::span_begin(W.geo, W.unit, W.n, wave), s1 = csv::span_begin(W.geo, W.unit, W.n, wave + 1);
  const DeviceText src{W.text, W.n};
  csv::Summary run = csv::nothing();
  for (uint64_t p = s0; p < s1; p += csv::kStep) {
    const csv::Group g = load_core(src, p + static_cast<uint64_t>(lane) * csv::kGroup, s1);
    const csv::LaneSummary l = csv::lane_summary(csv::make_masks(g, W.delimiter, W.quote));
    const uint64_t odd = __ballot(l.parity != 0);
    const uint32_t entry = lanes_below(odd) & 1u;   // relative to the step's first byte
    const uint32_t c0 = wave_total(entry ? l.c[1] : l.c[0]), c1 = wave_total(entry ? l.c[0] : l.c[1]);
    run = csv::compose(run, csv::widen(static_cast<uint32_t>(__popcll(odd)) & 1u, c0, c1));
  }
  if (lane == 0) summaries[wave] = run;
}

// one wave: lane l composes the spans [l * per, (l + 1) * per), the lanes' parities go through one ballot, their counts through
// a prefix sum, and every lane walks its spans again with the entry known
__global__ __launch_bounds__(kWave) void record_csv_resolve_kernel(const Walk W, const csv::Summary* __restrict__ summaries, csv::Entry* __restrict__ entries,
                                                                   uint64_t* __restrict__ row_first, unsigned long long* stats) {
  const uint64_t lane = static_cast<uint64_t>(lane_id());
  const uint64_t per = (W.geo.waves + kWave - 1) / kWave;
  const uint64_t a = lane * per < W.geo.waves ? lane * per : W.geo.waves;
  const uint64_t b = a + per < W.geo.waves ? a + per : W.geo.waves;
  csv::Summary mine = csv::nothing();
  for (uint64_t i = a; i < b; i++) mine = csv::compose(mine, summaries[i]);
  const uint64_t odd = __ballot(mine.parity != 0);
  const uint32_t entry = lanes_below(odd) & 1u;
  const uint64_t fields = entry ? mine.fields[1] : mine.fields[0], rows = entry ? mine.rows[1] : mine.rows[0];
  csv::Entry e{entry, wave_inclusive_sum64(fields) - fields, wave_inclusive_sum64(rows) - rows};
  for (uint64_t i = a; i < b; i++) {
    entries[i] = e;
    e = csv::advance(e, summaries[i]);
  }
  if (lane == kWave - 1) {   // (its spans are the last ones, or none: e is the state at the text's end)
    const uint64_t tail = csv::tail_row(W.n, W.n ? W.text[W.n - 1] : 0u, e);
    stats[kCsvRows] = e.rows + tail;
    stats[kCsvFields] = e.fields + tail;
    stats[kCsvOpen] = e.parity;
    stats[kCsvFirstBad] = e.parity ? W.n : ~0ull;   // (a text that ends inside quotes: the closing quote is missing at n)
    if (row_first) row_first[0] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void record_csv_clear_kernel(uint32_t* __restrict__ flags, uint64_t field_cap, const unsigned long long* stats) {
  const uint64_t fields = stats[kCsvFields];
  const uint64_t k = fields < field_cap ? fields : field_cap;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < k; i += static_cast<uint64_t>(gridDim.x) * kThreads) flags[i] = 0;
}

// the caller's tables: nothing at or beyond a cap, nothing into a table that is not there
struct Tables {
  uint64_t *rows_first, *rows_begin, *rows_end;
  uint64_t row_cap;
  uint64_t *begins, *ends;
  uint32_t* flags;
  uint64_t field_cap;
  __device__ __forceinline__ void field_begin(uint64_t f, uint64_t v) const {
    if (begins && f < field_cap) begins[f] = v;
  }
  __device__ __forceinline__ void field_end(uint64_t f, uint64_t v) const {
    if (ends && f < field_cap) ends[f] = v;
  }
  __device__ __forceinline__ void flag(uint64_t f, uint32_t bits) const {
    if (flags && f < field_cap) atomicOr(&flags[f], bits);
  }
  __device__ __forceinline__ void row_begin(uint64_t r, uint64_t v) const {
    if (rows_begin && r < row_cap) rows_begin[r] = v;
  }
  __device__ __forceinline__ void row_end(uint64_t r, uint64_t v) const {
    if (rows_end && r < row_cap) rows_end[r] = v;
  }
  // (row_first has row_cap + 1 entries)
  __device__ __forceinline__ void row_first(uint64_t r, uint64_t v) const {
    if (rows_first && r <= row_cap) rows_first[r] = v;
  }
};

// (no scratch: profiles/csv_kernel_resources.txt)
__global__ __launch_bounds__(kThreads) void record_csv_emit_kernel(const Walk W, const csv::Entry* __restrict__ entries, const Tables T, unsigned long long* stats) {
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (wave >= W.geo.waves) return;
  const int lane = lane_id();
  const uint64_t s0 = csv::span_begin(W.geo, W.unit, W.n, wave), s1 = csv::span_begin(W.geo, W.unit, W.n, wave + 1);
  const DeviceText src{W.text, W.n};
  csv::Entry at = entries[wave];                                  // wave-uniform: the state at the step's first byte
  int32_t prev_tail = s0 > 0 ? static_cast<int32_t>(W.text[s0 - 1]) : -1;   // the byte before the step
  csv::Tally tally;
  csv::tally_init(&tally);
  for (uint64_t p = s0; p < s1; p += csv::kStep) {
    const uint64_t p0 = p + static_cast<uint64_t>(lane) * csv::kGroup;
    csv::Group g = load_core(src, p0, s1);
    // ---- the halo: the lane below's last byte, the lane above's first two (a lane with bytes has a full lane below it)
    const uint32_t last = g.w[3] >> 24;
    const uint32_t below = wave_from_lane_below(last);
    const uint32_t above = wave_from_lane_above((g.w[0] & 0xFFFFu) | (g.valid << 16));
    g.prev = lane == 0 ? prev_tail : static_cast<int32_t>(below);
    if (lane == kWave - 1) {   // the next step's bytes, or another span's
      g.next1 = p0 + 16 < W.n ? static_cast<int32_t>(W.text[p0 + 16]) : -1;
      g.next2 = p0 + 17 < W.n ? static_cast<int32_t>(W.text[p0 + 17]) : -1;
    } else {
      const uint32_t has = above >> 16;
      g.next1 = has >= 1 ? static_cast<int32_t>(above & 0xFFu) : -1;
      g.next2 = has >= 2 ? static_cast<int32_t>((above >> 8) & 0xFFu) : -1;
    }
    prev_tail = static_cast<int32_t>(wave_last_lane(last));
    // ---- the lane's entry parity and its marks
    const csv::Masks m = csv::make_masks(g, W.delimiter, W.quote);
    const uint64_t odd = __ballot((csv::popcount(m.q & m.in & csv::kCore) & 1u) != 0);
    const uint32_t entry = (static_cast<uint32_t>(at.parity) ^ lanes_below(odd)) & 1u;
    const csv::Marks k = csv::make_marks(m, entry, p0 == 0);
    // ---- the fields and rows before the lane
    const uint32_t counts = csv::lane_counts(k);
    const uint32_t upto = wave_inclusive_sum(counts);
    const uint32_t before = upto - counts;
    csv::emit_group(k, p0, g.valid, W.n, at.fields + (before & 0xFFFFu), at.rows + (before >> 16), T);
    csv::tally_add(&tally, k, p0);
    const uint32_t all = wave_last_lane(upto);
    at.parity ^= static_cast<uint64_t>(__popcll(odd)) & 1u;
    at.fields += all & 0xFFFFu;
    at.rows += all >> 16;
  }
  // ---- the events
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint64_t sum = wave_sum64(tally.n[i]);
    if (lane == 0 && sum) atomicAdd(&stats[kCsvQuoted + i], static_cast<unsigned long long>(sum));
  }
  if (tally.first_bad != ~0ull) atomicMin(&stats[kCsvFirstBad], static_cast<unsigned long long>(tally.first_bad));
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_csv(rj_scan* s, const void* d_text, uint64_t n, int delimiter, int quote, uint64_t* d_row_first, uint64_t* d_row_begin, uint64_t* d_row_end,
                            uint64_t row_cap, uint64_t* d_field_begin, uint64_t* d_field_end, uint32_t* d_field_flags, uint64_t field_cap, rj_csv_stats* stats,
                            void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_csv";
  switch (csv::check_call(s, d_text, n, delimiter, quote, d_row_first, d_row_begin, d_row_end, d_field_begin, d_field_end, d_field_flags, stats)) {
    case csv::kFine: break;
    case csv::kNull: return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", kCall);
    case csv::kStats: return rj_fail(RJ_BAD_ARGUMENT, "%s: stats is NULL", kCall);
    case csv::kTableAlign: return rj_fail(RJ_BAD_ARGUMENT, "%s: a table is not 8-byte aligned", kCall);
    case csv::kFlagsAlign: return rj_fail(RJ_BAD_ARGUMENT, "%s: d_field_flags is not 4-byte aligned", kCall);
    case csv::kDelimiter: return rj_fail(RJ_BAD_ARGUMENT, "%s: delimiter %d is not a byte (0..255)", kCall, delimiter);
    case csv::kQuote: return rj_fail(RJ_BAD_ARGUMENT, "%s: quote %d is neither a byte (0..255) nor -1", kCall, quote);
    case csv::kLineBreak: return rj_fail(RJ_BAD_ARGUMENT, "%s: \\n and \\r are the line break, neither delimiter nor quote", kCall);
    case csv::kSame: return rj_fail(RJ_BAD_ARGUMENT, "%s: delimiter and quote are the same byte %d", kCall, delimiter);
    case csv::kTooLong: return rj_fail(RJ_BAD_ARGUMENT, "%s: a text of %llu bytes (2^42 or more)", kCall, static_cast<unsigned long long>(n));
  }
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  // the geometry: test knobs, read at every call.  A unit is whole steps; a span stays below 2^32 bytes (a lane's event counts)
  uint64_t unit = env_number("RJ_CSV_UNIT", static_cast<uint32_t>(csv::kUnit), 1u << 30);
  unit = unit < csv::kStep ? csv::kStep : (unit + csv::kStep - 1) / csv::kStep * csv::kStep;
  uint64_t grid = env_number("RJ_CSV_GRID", csv::kGrid, 1u << 16);
  const uint64_t least = (n >> 32) / kWaves + 1;
  grid = grid < least ? least : grid;
  const uint64_t wave_cap = grid * kWaves;
  Walk W{static_cast<const uint8_t*>(d_text), n, unit, delimiter, quote, csv::geometry(n, unit, wave_cap)};
  // the scan's scratch: the stats words, a summary and an entry per span
  const uint64_t stage = kCsvWords * sizeof(unsigned long long) + W.geo.waves * (sizeof(csv::Summary) + sizeof(csv::Entry));
  RJ_HIP(s->rec_csv_stage.reserve(stage));
  if (!s->rec_csv_host) RJ_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->rec_csv_host), kCsvWords * sizeof(unsigned long long)));
  unsigned long long* d_stats = s->rec_csv_stage.as<unsigned long long>();
  csv::Summary* summaries = reinterpret_cast<csv::Summary*>(d_stats + kCsvWords);
  csv::Entry* entries = reinterpret_cast<csv::Entry*>(summaries + W.geo.waves);
  RJ_HIP(hipMemsetAsync(d_stats, 0, kCsvWords * sizeof(unsigned long long), st));
  const dim3 blocks(static_cast<unsigned>(W.geo.waves ? (W.geo.waves + kWaves - 1) / kWaves : 1)), block(kThreads);
  const Tables T{d_row_first, d_row_begin, d_row_end, row_cap, d_field_begin, d_field_end, d_field_flags, field_cap};
  hipLaunchKernelGGL(record_csv_summarise_kernel, blocks, block, 0, st, W, summaries);
  hipLaunchKernelGGL(record_csv_resolve_kernel, dim3(1), dim3(kWave), 0, st, W, static_cast<const csv::Summary*>(summaries), entries, d_row_first, d_stats);
  if (d_field_flags && field_cap) {
    const uint64_t most = n + 1 < field_cap ? n + 1 : field_cap;   // (a text of n bytes has at most n + 1 fields)
    hipLaunchKernelGGL(record_csv_clear_kernel, dim3(unit_grid((most + kThreads * 4 - 1) / (kThreads * 4))), block, 0, st, d_field_flags, field_cap,
                       static_cast<const unsigned long long*>(d_stats));
  }
  hipLaunchKernelGGL(record_csv_emit_kernel, blocks, block, 0, st, W, static_cast<const csv::Entry*>(entries), T, d_stats);
  RJ_HIP(hipMemcpyAsync(s->rec_csv_host, d_stats, kCsvWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  RJ_HIP(hipStreamSynchronize(st));
  RJ_HIP(hipGetLastError());
  const unsigned long long* h = s->rec_csv_host;
  stats->n_rows = h[kCsvRows], stats->n_fields = h[kCsvFields];
  stats->n_quoted = h[kCsvQuoted], stats->n_escapes = h[kCsvEscapes];
  stats->n_bad_quote = h[kCsvBadQuote], stats->n_bad_close = h[kCsvBadClose], stats->n_bare_cr = h[kCsvBareCr];
  stats->open_at_end = h[kCsvOpen], stats->first_bad = h[kCsvFirstBad];
  return static_cast<int64_t>(h[kCsvFields]);
}

}  // extern "C"
