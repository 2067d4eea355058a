// rejit_amd/csrc/record_parse.hip -- rj_scan_records_parse: the rows of a record table over a device text -- the fields of
// rj_scan_records_split, lines, the strings of a column; every row, or the rows an index list names -- read as NUMBERS:
// d_value[j] (an int64, a uint64 or the bits of a double) and d_status[j] (why a row has no value), exactly and without a
// download.  record_parse.h has the grammar, the state a row is walked with and the exact window of the doubles; one memset
// (the summary) and two launches on one stream, one synchronise; no scratch beyond the summary's words:
//
// Check: one lane per row, the pack's checks (rows::resolve; the first bad row wins, note_bad_row).  It reads the tables only.
// Parse: one lane per row, units of 256 rows taken by a persistent grid (eight waves per SIMD).  It returns at once when the
//   summary holds a bad row (a refused call writes no output row), else walks its row's 16-byte groups (rows::load_group over
//   DeviceText: the guarded load at the text's end, any alignment of the row's begin) through numparse::step until the row ends
//   or is malformed -- the next group's load is issued before the current one is stepped: the load does not depend on the
//   state --, and stores numparse::finish's value (8 bytes) and status (1 byte).  A row of any length is legal and costs its
//   lane's walk; there is no wave tier: the state of a number is carried from byte to byte.  The five statuses are counted
//   with ballots into wave-uniform registers; at its end a wave adds its counts to the workgroup's (LDS), and the workgroup
//   issues ONE atomic add per class that occurred -- a few thousand adds on a summary word per call, not one per 64 rows
//   (156 250 adds on one address were the whole run time of 10^7 rows: profiles/parse_probe.txt).
//   FLOAT64 under RJ_PARSE_WIDE has an instantiation of its own (kWide): the same walk with the wide state's digit rule, and a
//   finish that gives the lanes outside Clinger's window their Eisel-Lemire product -- a count of leading zeros, one or two
//   64 x 64 -> 128 products and two words of pow5_table.h's 10 KB table, fetched per lane through the vector caches.  The
//   three kernels without the flag are compiled from the *_as<false> functions: the code they always had.
// Nothing here waits for another lane's progress.  The rows, the text and the refusal are record_frame.h's.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_parse.h"
#include "record_rows.h"

namespace rejit_amd {

namespace {

// the summary words of a parse: a count per status (kSumBadWord, between them, and kSumTimedOut keep their meaning)
__device__ __forceinline__ uint32_t status_word(uint32_t status) { return status < kSumBadWord ? status : status + 1; }
static_assert(kSumKept == 0 && kSumMatching == 1 && kSumCrossing == 2 && kSumBadWord == 3 && kSumSelected == 4 && kSumTotal == 5, "status_word");
constexpr unsigned kParseGrid = 256 * 8;   // persistent: eight workgroups (a wave per SIMD each) for each of the 256 CUs
// the wide instantiation needs 69 VGPRs, seven waves per SIMD (profiles/parse_wide_kernel_resources.txt): a grid of eight
// workgroups per CU would leave every eighth one to run its whole share behind the others
constexpr unsigned kParseWideGrid = 256 * 7;

__global__ __launch_bounds__(kThreads) void record_parse_check_kernel(Rows R, uint64_t n_records, uint64_t n, uint64_t k, uint64_t n_units,
                                                                      unsigned long long* summary) {
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    const bool bad = j < k && rows::resolve(R.rec_begin, R.rec_end, R.indices, n_records, n, j).bad;
    note_bad_row(bad, j, &summary[kSumBadWord]);
  }
}

template <int kKind, bool kWide>
__global__ __launch_bounds__(kThreads) void record_parse_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint64_t n_records, uint64_t k,
                                                                uint64_t n_units, unsigned flags, uint64_t* __restrict__ value,
                                                                uint8_t* __restrict__ status, unsigned long long* summary) {
  __shared__ uint32_t s_count[numparse::kStatuses];
  if (refused(summary)) return;
  if (threadIdx.x < numparse::kStatuses) s_count[threadIdx.x] = 0;
  __syncthreads();
  const DeviceText src{text, n};
  uint32_t count[numparse::kStatuses] = {0, 0, 0, 0, 0};   // (wave-uniform; a wave sees fewer than 2^31 rows)
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    uint32_t st = numparse::kStatuses;   // (a lane without a row counts nowhere)
    if (j < k) {
      const rows::Row row = rows::resolve(R.rec_begin, R.rec_end, R.indices, n_records, n, j);
      numparse::Result res{numparse::kMalformed, 0};
      if (!row.bad) {   // (every row passed the check; a lane is still never led outside the text)
        const uint64_t len = row.len(), groups = rows::n_groups(len);
        numparse::State s = numparse::start_as<kWide>(kKind, flags);
        uint32_t w[4] = {0, 0, 0, 0};
        if (groups) rows::load_group(src, n, row.rb, len, 0, w);
        for (uint64_t g = 0; g < groups && !numparse::done(s); g++) {
          uint32_t next[4] = {0, 0, 0, 0};
          if (g + 1 < groups) rows::load_group(src, n, row.rb, len, g + 1, next);
          const uint64_t left = len - g * rows::kGroupBytes;
          numparse::step_as<kWide>(s, w, left < rows::kGroupBytes ? static_cast<uint32_t>(left) : static_cast<uint32_t>(rows::kGroupBytes));
          w[0] = next[0], w[1] = next[1], w[2] = next[2], w[3] = next[3];
        }
        res = numparse::finish_as<kWide>(s, kKind);
      }
      st = res.status;
      value[j] = res.bits;
      if (status) status[j] = static_cast<uint8_t>(st);
    }
#pragma unroll
    for (uint32_t c = 0; c < numparse::kStatuses; c++) count[c] += static_cast<uint32_t>(__popcll(__ballot(st == c)));
  }
  if (lane_id() == 0) {
#pragma unroll
    for (uint32_t c = 0; c < numparse::kStatuses; c++)
      if (count[c]) atomicAdd(&s_count[c], count[c]);
  }
  __syncthreads();
  if (threadIdx.x < numparse::kStatuses && s_count[threadIdx.x])
    atomicAdd(&summary[status_word(threadIdx.x)], static_cast<unsigned long long>(s_count[threadIdx.x]));
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_parse(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                              const uint64_t* d_indices, uint64_t n_indices, int kind, unsigned flags, uint64_t* d_value, uint8_t* d_status,
                              rj_parse_stats* stats, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_parse";
  const uint64_t k = d_indices ? n_indices : n_records;
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) || (k && !d_value))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse: null argument");
  if (!aligned8(d_rec_begin, d_rec_end, d_indices, d_value)) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse: a table is not 8-byte aligned");
  if (!numparse::kind_known(kind))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse: kind %d is not RJ_PARSE_INT64, RJ_PARSE_UINT64 or RJ_PARSE_FLOAT64", kind);
  if (!numparse::flags_known(flags)) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse: flags %#x: the flags are RJ_PARSE_TRIM and RJ_PARSE_WIDE", flags);
  if (!rows::rows_fit(k))
    return rj_fail(RJ_TOO_LARGE, "rj_scan_records_parse: %llu rows: the record calls that read rows take fewer than 2^31 of them",
                   static_cast<unsigned long long>(k));
  if (stats) *stats = rj_parse_stats{0, 0, 0, 0, 0};
  if (k == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  int rc;
  unsigned long long *scratch = nullptr, *summary = nullptr;
  if ((rc = records_begin(s, 0, st, &scratch, &summary)) != RJ_OK) return rc;
  const Rows R{d_rec_begin, d_rec_end, d_indices};
  const uint8_t* text = static_cast<const uint8_t*>(d_text);
  const bool wide = kind == numparse::kFloat64 && (flags & numparse::kWideFlag);   // (RJ_PARSE_WIDE is inert for the integer kinds)
  const dim3 block(kThreads), grid(static_cast<unsigned>(n_units < kParseGrid ? n_units : kParseGrid));
  const dim3 wide_grid(static_cast<unsigned>(n_units < kParseWideGrid ? n_units : kParseWideGrid));
  hipLaunchKernelGGL(record_parse_check_kernel, dim3(unit_grid(n_units)), block, 0, st, R, n_records, n, k, n_units, summary);
#define RJ_PARSE_LAUNCH(KIND, WIDE) \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(record_parse_kernel<KIND, WIDE>), WIDE ? wide_grid : grid, block, 0, st, text, n, R, n_records, k, n_units, flags, d_value, d_status, summary)
  if (kind == numparse::kInt64) RJ_PARSE_LAUNCH(numparse::kInt64, false);
  else if (kind == numparse::kUint64) RJ_PARSE_LAUNCH(numparse::kUint64, false);
  else if (wide) RJ_PARSE_LAUNCH(numparse::kFloat64, true);
  else RJ_PARSE_LAUNCH(numparse::kFloat64, false);
#undef RJ_PARSE_LAUNCH
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse: row %llu names no record or a record outside the text (index < n_records, begin <= end <= n)",
                   static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
  if (stats) {
    stats->n_ok = s->rec_host[kSumKept];
    stats->n_empty = s->rec_host[kSumMatching];
    stats->n_malformed = s->rec_host[kSumCrossing];
    stats->n_range = s->rec_host[kSumSelected];
    stats->n_inexact = s->rec_host[kSumTotal];
  }
  return static_cast<int64_t>(s->rec_host[kSumKept]);
}

}  // extern "C"
