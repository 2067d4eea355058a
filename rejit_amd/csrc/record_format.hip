// rejit_amd/csrc/record_format.hip -- rj_scan_records_format: a column of 64-bit values -- int64, uint64 or the bits of doubles;
// every value, or the rows an index list names -- written as decimal TEXT into a new contiguous device text with its record
// table, laid out as rj_scan_records_pack lays records out: the inverse of rj_scan_records_parse, without a download.  The
// bytes are Python's str(int) / repr(float).  record_format.h has the arithmetic (the digits of an integer, the shortest digits
// of a double by Schubfach over pow10_table.h, the closed form of a row's bytes); two memsets (the summary, the look-back's
// words) and up to three launches on one stream, one synchronise:
//
// Check (with an index list only): one lane per row, index < n_values; the first bad row wins (note_bad_row).  A refused call
//   writes no table row and no byte: the two kernels behind it return at once.
// Plan: record_frame.h's plan_units, one lane per row, a unit = 256 rows, the decoupled look-back.  A lane reads its index,
//   status and value and converts ONCE: for a double the shortest digits (three 64 x 128 products with two table words, fetched
//   per lane through the vector caches), for an integer its magnitude and digit count, stored as 16 bytes of scratch per row
//   -- the decimal mantissa, and decpt, sign, class and length.  (An integer could be read again by the emit instead; with
//   the index, the status and the digit count in it that kernel needs 98 VGPRs, four waves per SIMD, against 60 and eight:
//   the 32 bytes per row of the stage are the cheaper price.)  The row's length goes into the scan; ob / oe and the total are
//   written.
// Emit: record_frame.h's emit_chunks -- output-major as copy_chunks, in chunks of 4 KiB (one pass of 256 lanes x 16 bytes), the chunk
//   built in LDS: its rows from one pair of searches over ob, every row converted once by its own lane -- the digits from the
//   staged Small (or from the integer itself) by the header's closed form -- into an image of the chunk that was filled with
//   the fill byte, then one 16-byte store of the image per lane.  No byte stores to memory but the last group's below the total,
//   no atomics.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_format.h"
#include "record_frame.h"

namespace rejit_amd {

namespace {

__global__ __launch_bounds__(kThreads) void record_format_check_kernel(const uint64_t* __restrict__ indices, uint64_t n_values, uint64_t k, uint64_t n_units,
                                                                       unsigned long long* summary) {
  check_indices(indices, n_values, k, n_units, summary);
}

// the row's value as a Small; every index has passed the check
template <bool kFloat>
__device__ __forceinline__ numformat::Small small_of_row(const uint64_t* __restrict__ value, const uint8_t* __restrict__ status,
                                                         const uint64_t* __restrict__ indices, int kind, uint64_t j) {
  const uint64_t r = indices ? indices[j] : j;
  if (status && status[r] != numformat::kStatusOk) return numformat::empty_row();
  return kFloat ? numformat::small_of_double(value[r]) : numformat::small_of_int(value[r], kind);
}

template <bool kFloat>
__global__ __launch_bounds__(kThreads) void record_format_plan_kernel(const uint64_t* __restrict__ value, const uint8_t* __restrict__ status,
                                                                      const uint64_t* __restrict__ indices, uint64_t k, int kind, uint64_t lead, uint64_t gap,
                                                                      unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                                      ulonglong2* __restrict__ stage, uint64_t* __restrict__ out_begin,
                                                                      uint64_t* __restrict__ out_end, unsigned long long* summary) {
  if (refused(summary)) return;
  const auto row = [=](uint64_t j) {
    const numformat::Small s = small_of_row<kFloat>(value, status, indices, kind, j);
    if (stage) stage[j] = make_ulonglong2(s.digits, s.meta);
    return PlannedRow{0, numformat::small_len(s)};
  };
  plan_units(row, k, lead, gap, granules, ticket, n_units, out_begin, out_end, summary);
}

// The emit: record_frame.h's emit_chunks; a row's bytes are the digits of the staged Small by the header's closed form.
struct FormatEmit : ImagePolicy {
  const ulonglong2* __restrict__ stage;
  const uint64_t* __restrict__ ob;
  __device__ __forceinline__ bool row(uint64_t j, uint64_t c0, uint64_t c1, const ImagePut& put) const {
    const ulonglong2 staged = stage[j];
    const numformat::Small s{staged.x, staged.y};
    const uint64_t at = ob[j];
    uint32_t lo, hi;
    if (!pack::chunk_part(at, numformat::small_len(s), c0, c1, &lo, &hi)) return false;
    const numformat::Row row = numformat::unfold(s);
    // (holds: always, by chunk_part -- but char_at made AHEAD of a test is hoisted and unswitched on the row's class, and the kernel
    // spills 428 registers)
    for (uint32_t i = lo; i < hi; i++)
      if (put.holds(at + i - c0)) put(at + i - c0, numformat::char_at(row, i));
    return false;
  }
};
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void record_format_emit_kernel(
    const ulonglong2* __restrict__ stage, uint64_t k, const uint64_t* __restrict__ ob, uint32_t fill, uint8_t* __restrict__ out, uint64_t out_cap,
    const unsigned long long* summary) {
  emit_chunks(FormatEmit{{}, stage, ob}, k, ob, fill, out, out_cap, summary);
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_format(rj_scan* s, const uint64_t* d_value, const uint8_t* d_status, uint64_t n_values, const uint64_t* d_indices, uint64_t n_indices,
                               int kind, unsigned flags, int fill, uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin,
                               uint64_t* d_out_end, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_format";
  const uint64_t k = d_indices ? n_indices : n_values;
  if (!s) return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", kCall);
  switch (numformat::check_call(d_value, d_status, n_values, d_indices, n_indices, kind, flags, fill, lead, gap, d_out, out_cap, d_out_begin, d_out_end)) {
    case numformat::kFine: break;
    case numformat::kNullArgument: return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", kCall);
    case numformat::kTableAlign: return rj_fail(RJ_BAD_ARGUMENT, "%s: a table, d_value or d_indices is not 8-byte aligned", kCall);
    case numformat::kOutAlign: return rj_fail(RJ_BAD_ARGUMENT, "%s: d_out is not 16-byte aligned", kCall);
    case numformat::kBadKind: return rj_fail(RJ_BAD_ARGUMENT, "%s: kind %d is not RJ_FORMAT_INT64, RJ_FORMAT_UINT64 or RJ_FORMAT_FLOAT64", kCall, kind);
    case numformat::kBadFlags: return rj_fail(RJ_BAD_ARGUMENT, "%s: flags %#x: no flag is defined, flags must be 0", kCall, flags);
    case numformat::kBadFill: return rj_fail(RJ_BAD_ARGUMENT, "%s: fill %d is not a byte (0..255)", kCall, fill);
    case numformat::kBadSums:
      return rj_fail(RJ_BAD_ARGUMENT, "%s: %llu rows can exceed 2^62 output bytes (lead + k * (24 + gap)), or 24 + gap reaches 2^42", kCall,
                     static_cast<unsigned long long>(k));
    case numformat::kTooManyRows:
      return rj_fail(RJ_TOO_LARGE, "%s: %llu rows: the record calls that read rows take fewer than 2^31 of them", kCall, static_cast<unsigned long long>(k));
  }
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  const bool copies = out_cap != 0;
  int rc;
  uint64_t* ob = nullptr;
  ulonglong2* stage = nullptr;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, then the look-back's words
  if ((rc = value_rows_begin(s, d_out_begin, copies, k, n_units, st, &ob, &stage, &scratch, &summary)) != RJ_OK) return rc;
  const dim3 block(kThreads), units(unit_grid(n_units));
  if (d_indices && k) hipLaunchKernelGGL(record_format_check_kernel, units, block, 0, st, d_indices, n_values, k, n_units, summary);
#define RJ_FORMAT_PLAN(FLOAT)                                                                                                                \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(record_format_plan_kernel<FLOAT>), units, block, 0, st, d_value, d_status, d_indices, k, kind, lead, gap, \
                     scratch + 1, scratch, n_units, stage, ob, d_out_end, summary)
  if (kind == numformat::kFloat64) RJ_FORMAT_PLAN(true);
  else RJ_FORMAT_PLAN(false);
#undef RJ_FORMAT_PLAN
  if (copies)
    hipLaunchKernelGGL(record_format_emit_kernel, dim3(image_grid(out_cap)), block, 0, st, static_cast<const ulonglong2*>(stage), k,
                       static_cast<const uint64_t*>(ob), static_cast<uint32_t>(fill), static_cast<uint8_t*>(d_out), out_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0) return bad_index_failure(s, kCall);
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
