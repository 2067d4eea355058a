// rejit_amd/csrc/record_time_format.hip -- rj_scan_records_format_time: a column of int64 instants -- every value, or the rows an
// index list names -- written as TEXT under a strftime-style format into a new contiguous device text with its record table,
// laid out exactly as rj_scan_records_format lays its rows out: the inverse of rj_scan_records_parse_time, without a download.
// record_time_format.h has the meaning (the split of an instant into civil fields, the layout table the format is compiled
// into, a row's bytes through it); the frame is record_format.hip's (record_frame.h's value_rows_begin, check_indices, plan_units, emit_chunks): two memsets (the summary, the look-back's words) and up
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
// Emit: record_frame.h's emit_chunks, as record_format.hip's: output-major in chunks of 4 KiB (one pass of 256 lanes x 16 bytes), the chunk built in LDS:
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

// the summary words of a call: a count per class (kSumBadWord, kSumTotal and kSumTimedOut keep their meaning)
enum { kSumOk = kSumKept, kSumNull = kSumMatching, kSumRange = kSumCrossing };
static_assert(kSumRange < kSumBadWord && kSumRange < kSumTotal && kSumRange < kSumTimedOut, "summary words of its own");
__device__ __forceinline__ uint32_t class_word(uint32_t cls) { return cls == timeformat::kOk ? kSumOk : cls == timeformat::kNull ? kSumNull : kSumRange; }

__global__ __launch_bounds__(kThreads) void record_time_format_check_kernel(const uint64_t* __restrict__ indices, uint64_t n_values, uint64_t k, uint64_t n_units,
                                                                            unsigned long long* summary) {
  check_indices(indices, n_values, k, n_units, summary);
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

// The emit: record_frame.h's emit_chunks; byte i of every OK row is the layout table's entry i, a literal or a byte of the
// row's Source.  The table is copied to LDS once per workgroup from a kernel argument, by constant indices.
struct TimeFormatEmit : ImagePolicy {
  const ulonglong2* __restrict__ stage;
  const uint64_t* __restrict__ ob;
  const uint16_t* entries;   // (LDS)
  uint32_t L;
  __device__ __forceinline__ bool row(uint64_t j, uint64_t c0, uint64_t c1, const ImagePut& put) const {
    const ulonglong2 staged = stage[j];
    const timeformat::Fields f{staged.x, staged.y};
    const uint64_t at = ob[j];
    uint32_t lo, hi;
    if (!pack::chunk_part(at, timeformat::row_len(f, L), c0, c1, &lo, &hi)) return false;
    const timeformat::Source src = timeformat::unfold(f);
    for (uint32_t i = lo; i < hi; i++)
      if (put.holds(at + i - c0) && i < timeformat::kMaxRowBytes) put(at + i - c0, timeformat::char_at(src, entries[i]));   // (always: chunk_part, hi <= L)
    return false;
  }
};
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void record_time_format_emit_kernel(
    const ulonglong2* __restrict__ stage, uint64_t k, const uint64_t* __restrict__ ob, timeformat::Layout layout, uint32_t fill, uint8_t* __restrict__ out,
    uint64_t out_cap, const unsigned long long* summary) {
  __shared__ uint32_t s_layout[timeformat::kLayoutWords];
  if (threadIdx.x == kThreads - 1) {   // (the first chunk's first barrier publishes it)
#pragma unroll
    for (uint32_t i = 0; i < timeformat::kLayoutWords; i++) s_layout[i] = layout.words[i];
  }
  emit_chunks(TimeFormatEmit{{}, stage, ob, reinterpret_cast<const uint16_t*>(s_layout), layout.len}, k, ob, fill, out, out_cap, summary);
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
  if ((rc = value_rows_begin(s, d_out_begin, copies, k, n_units, st, &ob, &stage, &scratch, &summary)) != RJ_OK) return rc;
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
    hipLaunchKernelGGL(record_time_format_emit_kernel, dim3(image_grid(out_cap)), block, 0, st, static_cast<const ulonglong2*>(stage), k,
                       static_cast<const uint64_t*>(ob), layout, static_cast<uint32_t>(fill), static_cast<uint8_t*>(d_out), out_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0) return bad_index_failure(s, kCall);
  if (stats) *stats = rj_format_time_stats{s->rec_host[kSumOk], s->rec_host[kSumNull], s->rec_host[kSumRange]};
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
