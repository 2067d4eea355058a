// rejit_amd/csrc/record_time_format.hip -- rj_scan_records_format_time: a column of int64 instants -- every value, or the rows an
// index list names -- written as TEXT under a strftime-style format into a new contiguous device text with its record table,
// laid out exactly as rj_scan_records_format lays its rows out: the inverse of rj_scan_records_parse_time, without a download.
// record_time_format.h has the meaning (the split of an instant into civil fields, the layout table the format is compiled
// into, a row's bytes through it); the frame is record_format.hip's: two memsets (the summary, the look-back's words) and up
// to three launches on one stream, one synchronise:
//
// Check (with an index list only): one lane per row, index < n_values; the first bad row wins (note_bad_row).  A refused call
//   writes no table row and no byte: the two kernels behind it return at once.
// Plan: record_frame.h's plan_units, one lane per row, a unit = 256 rows, the decoupled look-back.  A lane reads its index,
//   status and value and splits the instant ONCE -- the kernel is instantiated per unit of time, so every divisor is a
//   constant and no division is a call --, stored as 16 bytes of stage per row: the packed civil fields with the row's
//   class, and the nanoseconds.  The row's length, L or 0, goes into the scan; ob / oe and the total are written.  The three
//   classes (OK, null status, out of range) are counted with ballots: one LDS atomic per wave, unit and class that occurred,
//   one global atomic per workgroup and class, into summary words of this call's own.
// Emit: record_format.hip's shape, output-major in chunks of 4 KiB (one pass of 256 lanes x 16 bytes), the chunk built in LDS:
//   its rows from one pair of searches over ob, every row written once by its own lane through the layout table -- copied to
//   LDS once per workgroup from a kernel argument, by constant indices -- into an image of the chunk that was filled with the
//   fill byte, then one 16-byte store of the image per lane.  No byte stores to memory but the last group's below the total,
//   no atomics.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_time_format.h"

namespace rejit_amd {

namespace {

constexpr uint64_t kEmitChunk = 4096;

// the summary words of a call: a count per class (kSumBadWord, kSumTotal and kSumTimedOut keep their meaning)
enum { kSumOk = kSumKept, kSumNull = kSumMatching, kSumRange = kSumCrossing };
static_assert(kSumRange < kSumBadWord && kSumRange < kSumTotal && kSumRange < kSumTimedOut, "summary words of its own");
__device__ __forceinline__ uint32_t class_word(uint32_t cls) { return cls == timeformat::kOk ? kSumOk : cls == timeformat::kNull ? kSumNull : kSumRange; }

__global__ __launch_bounds__(kThreads) void record_time_format_check_kernel(const uint64_t* __restrict__ indices, uint64_t n_values, uint64_t k, uint64_t n_units,
                                                                            unsigned long long* summary) {
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    const bool bad = j < k && indices[j] >= n_values;
    note_bad_row(bad, j, &summary[kSumBadWord]);
  }
}

template <int kUnit>
__global__ __launch_bounds__(kThreads) void record_time_format_plan_kernel(const uint64_t* __restrict__ value, const uint8_t* __restrict__ status,
                                                                           const uint64_t* __restrict__ indices, uint64_t k, int32_t zone_seconds, uint32_t L,
                                                                           uint64_t lead, uint64_t gap, unsigned long long* granules, unsigned long long* ticket,
                                                                           uint64_t n_units, ulonglong2* __restrict__ stage, uint64_t* __restrict__ out_begin,
                                                                           uint64_t* __restrict__ out_end, unsigned long long* summary) {
  __shared__ uint32_t s_count[timeformat::kClasses];
  if (refused(summary)) return;
  if (threadIdx.x < timeformat::kClasses) s_count[threadIdx.x] = 0;
  __syncthreads();
  const auto row = [=](uint64_t j) {   // (every index has passed the check)
    const uint64_t r = indices ? indices[j] : j;
    const timeformat::Fields f = (status && status[r] != timeformat::kStatusOk) ? timeformat::null_row() : timeformat::split<kUnit>(value[r], zone_seconds);
    if (stage) stage[j] = make_ulonglong2(f.packed, f.nanos);
    const uint32_t cls = timeformat::class_of(f);
#pragma unroll
    for (uint32_t c = 0; c < timeformat::kClasses; c++) {   // (the lanes that have a row: the others are masked off here)
      const uint64_t lanes = __ballot(cls == c);
      if (lanes && lane_id() == __builtin_ctzll(lanes)) atomicAdd(&s_count[c], static_cast<uint32_t>(__popcll(lanes)));
    }
    return PlannedRow{0, timeformat::row_len(f, L)};
  };
  plan_units(row, k, lead, gap, granules, ticket, n_units, out_begin, out_end, summary);
  __syncthreads();
  if (threadIdx.x < timeformat::kClasses && s_count[threadIdx.x])
    atomicAdd(&summary[class_word(threadIdx.x)], static_cast<unsigned long long>(s_count[threadIdx.x]));
}

// The emit: record_format.hip's -- output-major, persistent, the total read from the summary, the rows of a chunk from the
// pair of searches, the chunk's image in LDS -- with the row's bytes from the layout table: byte i of every OK row is entry i,
// a literal or a byte of the row's Source.  The rows of a chunk are not bounded (empty rows with gap 0): the lanes take them
// 256 at a time.
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void record_time_format_emit_kernel(
    const ulonglong2* __restrict__ stage, uint64_t k, const uint64_t* __restrict__ ob, timeformat::Layout layout, uint32_t fill, uint8_t* __restrict__ out,
    uint64_t out_cap, const unsigned long long* summary) {
  static_assert(kEmitChunk == kThreads * pack::kGroupBytes, "one pass of the workgroup fills or stores the chunk's image");
  __shared__ uint4 s_image[kThreads];
  __shared__ uint64_t s_rows[2];
  __shared__ uint32_t s_layout[timeformat::kLayoutWords];
  if (refused(summary)) return;
  if (threadIdx.x == kThreads - 1) {
#pragma unroll
    for (uint32_t i = 0; i < timeformat::kLayoutWords; i++) s_layout[i] = layout.words[i];
  }
  const uint16_t* entries = reinterpret_cast<const uint16_t*>(s_layout);
  const uint32_t L = layout.len;
  const uint64_t total = summary[kSumTotal];
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint64_t n_chunks = (limit + kEmitChunk - 1) / kEmitChunk;
  const uint32_t tid = threadIdx.x;
  const pack::View table{ob, nullptr, nullptr, nullptr, 0, k, total};
  uint8_t* image = reinterpret_cast<uint8_t*>(s_image);
  const uint32_t fw = pack::fill_word(fill);
  for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t c0 = c * kEmitChunk;
    const uint64_t c1 = c0 + kEmitChunk < limit ? c0 + kEmitChunk : limit;
    // ---- the rows that touch the chunk (two searches side by side), and the image all fill
    if (tid == 0) s_rows[0] = pack::chunk_first_row(table, k, c0);
    if (tid == kWave) s_rows[1] = pack::chunk_end_row(table, k, 0, c1);
    s_image[tid] = make_uint4(fw, fw, fw, fw);
    __syncthreads();   // (the first one also publishes s_layout)
    const uint64_t j0 = s_rows[0], j1 = s_rows[1] > j0 ? s_rows[1] : j0;   // (j1 <= k)
    // ---- every row once: its bytes inside the chunk
    for (uint64_t j = j0 + tid; j < j1; j += kThreads) {
      const ulonglong2 staged = stage[j];
      const timeformat::Fields f{staged.x, staged.y};
      const uint64_t at = ob[j];
      uint32_t lo, hi;
      if (!timeformat::chunk_part(at, timeformat::row_len(f, L), c0, c1, &lo, &hi)) continue;
      const timeformat::Source src = timeformat::unfold(f);
      for (uint32_t i = lo; i < hi; i++) {
        const uint64_t in_image = at + i - c0;
        if (in_image < kEmitChunk && i < timeformat::kMaxRowBytes) image[in_image] = static_cast<uint8_t>(timeformat::char_at(src, entries[i]));   // (always: chunk_part)
      }
    }
    __syncthreads();
    // ---- 16 aligned output bytes per lane
    const uint64_t p = c0 + static_cast<uint64_t>(tid) * pack::kGroupBytes;
    if (p < c1) {
      const uint32_t bytes = pack::group_store_bytes(p, limit);
      if (bytes == pack::kGroupBytes) {
        *reinterpret_cast<uint4*>(out + p) = s_image[tid];
      } else {
        for (uint32_t b = 0; b < bytes; b++) out[p + b] = image[tid * pack::kGroupBytes + b];
      }
    }
    __syncthreads();   // (the next chunk rewrites s_rows and the image)
  }
}

inline unsigned emit_grid(uint64_t out_cap) {
  const uint64_t cap_chunks = (out_cap + kEmitChunk - 1) / kEmitChunk;
  return static_cast<unsigned>(cap_chunks < kCopyGrid ? cap_chunks : kCopyGrid);
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_format_time(rj_scan* s, const uint64_t* d_value, const uint8_t* d_status, uint64_t n_values, const uint64_t* d_indices,
                                    uint64_t n_indices, const char* format, uint64_t format_len, int unit, int zone_minutes, unsigned flags, int fill,
                                    uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin, uint64_t* d_out_end,
                                    rj_format_time_stats* stats, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_format_time";
  const uint64_t k = d_indices ? n_indices : n_values;
  if (!s) return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", kCall);
  timeformat::Refusal refusal = timeformat::check_arguments(d_value, n_values, d_indices, format, format_len, unit, zone_minutes, flags, fill, d_out, out_cap,
                                                            d_out_begin, d_out_end);
  timeparse::Program program{};
  if (refusal == timeformat::kFine) {
    uint32_t at = 0;
    const int bad_format = timeparse::compile_mode(reinterpret_cast<const uint8_t*>(format), format_len, true, &program, &at);
    if (bad_format != timeparse::kFormatOk) return rj_fail(RJ_BAD_ARGUMENT, "%s: format byte %u: %s", kCall, at, timeparse::format_error_text(bad_format));
    refusal = timeformat::check_sizes(k, lead, gap);
  }
  switch (refusal) {
    case timeformat::kFine: break;
    case timeformat::kNullArgument: return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", kCall);
    case timeformat::kTableAlign: return rj_fail(RJ_BAD_ARGUMENT, "%s: a table, d_value or d_indices is not 8-byte aligned", kCall);
    case timeformat::kOutAlign: return rj_fail(RJ_BAD_ARGUMENT, "%s: d_out is not 16-byte aligned", kCall);
    case timeformat::kBadUnit:
      return rj_fail(RJ_BAD_ARGUMENT, "%s: unit %d is not RJ_TIME_SECOND, RJ_TIME_MILLI, RJ_TIME_MICRO or RJ_TIME_NANO", kCall, unit);
    case timeformat::kBadZone: return rj_fail(RJ_BAD_ARGUMENT, "%s: zone_minutes %d is outside -1439..1439", kCall, zone_minutes);
    case timeformat::kBadFlags: return rj_fail(RJ_BAD_ARGUMENT, "%s: flags %#x: no flag is defined, flags must be 0", kCall, flags);
    case timeformat::kBadFill: return rj_fail(RJ_BAD_ARGUMENT, "%s: fill %d is not a byte (0..255)", kCall, fill);
    case timeformat::kBadSums:
      return rj_fail(RJ_BAD_ARGUMENT, "%s: %llu rows can exceed 2^62 output bytes (lead + k * (77 + gap)), or 77 + gap reaches 2^42", kCall,
                     static_cast<unsigned long long>(k));
    case timeformat::kTooManyRows:
      return rj_fail(RJ_TOO_LARGE, "%s: %llu rows: the record calls that read rows take fewer than 2^31 of them", kCall, static_cast<unsigned long long>(k));
  }
  const timeformat::Layout layout = timeformat::make_layout(program, unit, zone_minutes);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  const bool copies = out_cap != 0;
  int rc;
  uint64_t* ob = nullptr;
  ulonglong2* stage = nullptr;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, then the look-back's words
  if ((rc = pack_begin_table(s, d_out_begin, copies, k, &ob)) != RJ_OK) return rc;
  if (copies && k) {
    RJ_HIP(s->rec_format_stage.reserve(k * sizeof(ulonglong2)));
    stage = s->rec_format_stage.as<ulonglong2>();
  }
  if ((rc = records_begin(s, 1 + lookback::granule_words(n_units), st, &scratch, &summary)) != RJ_OK) return rc;
  const dim3 block(kThreads), units(unit_grid(n_units));
  const int32_t zone_seconds = zone_minutes * 60;
  if (d_indices && k) hipLaunchKernelGGL(record_time_format_check_kernel, units, block, 0, st, d_indices, n_values, k, n_units, summary);
#define RJ_TIME_FORMAT_PLAN(UNIT)                                                                                                                  \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(record_time_format_plan_kernel<UNIT>), units, block, 0, st, d_value, d_status, d_indices, k, zone_seconds, \
                     layout.len, lead, gap, scratch + 1, scratch, n_units, stage, ob, d_out_end, summary)
  switch (unit) {
    case timeparse::kSecond: RJ_TIME_FORMAT_PLAN(timeparse::kSecond); break;
    case timeparse::kMilli: RJ_TIME_FORMAT_PLAN(timeparse::kMilli); break;
    case timeparse::kMicro: RJ_TIME_FORMAT_PLAN(timeparse::kMicro); break;
    default: RJ_TIME_FORMAT_PLAN(timeparse::kNano); break;
  }
#undef RJ_TIME_FORMAT_PLAN
  if (copies)
    hipLaunchKernelGGL(record_time_format_emit_kernel, dim3(emit_grid(out_cap)), block, 0, st, static_cast<const ulonglong2*>(stage), k,
                       static_cast<const uint64_t*>(ob), layout, static_cast<uint32_t>(fill), static_cast<uint8_t*>(d_out), out_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0)
    return rj_fail(RJ_BAD_ARGUMENT, "%s: row %llu names no value (index < n_values)", kCall, static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
  if (stats) *stats = rj_format_time_stats{s->rec_host[kSumOk], s->rec_host[kSumNull], s->rec_host[kSumRange]};
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
