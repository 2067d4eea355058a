// rejit_amd/csrc/record_time.hip -- rj_scan_records_parse_time: the rows of a record table over a device text -- the fields of
// rj_scan_records_split, lines, the strings of a column; every row, or the rows an index list names -- read as TIMESTAMPS
// under a strptime-style format: d_value[j] (an int64 count of the call's unit since 1970-01-01T00:00:00Z) and d_status[j]
// (why a row has no value), exactly and without a download.  record_time.h has the directives, the format's compiler, the
// state a row is walked with and the calendar; the frame is rj_scan_records_parse's (record_parse.hip): one memset (the
// summary) and two launches on one stream, one synchronise; no scratch beyond the summary's words:
//
// Check: one lane per row, the pack's checks (rows::resolve; the first bad row wins, note_bad_row).  It reads the tables only.
//   (The parse's check kernel, word for word; it lives in that unit's anonymous namespace, so this unit has a copy.)
// Time: one lane per row, units of 256 rows taken by a persistent grid (kTimeGrid, from the kernel's resource line:
//   profiles/time_kernel_resources.txt).  It returns at once when the summary holds a bad row (a refused call writes no output
//   row), else walks its row's 16-byte groups (rows::load_group over DeviceText: the guarded load at the text's end, any
//   alignment of the row's begin) through timeparse::step until the row ends or is malformed -- the next group's load is
//   issued before the current one is stepped --, and stores timeparse::finish's value (8 bytes) and status (1 byte).
//   The compiled format arrives as a kernel argument of 16 words and a length.  Every lane has a program counter of its own
//   (%f's length, `Z` against `+hh:mm` and trimmed blanks make lanes diverge), and an argument indexed by a per-lane value
//   would be copied to scratch: one lane copies the 16 words to LDS once per workgroup, by constant indices, and every lane
//   reads its step's one or two bytes from there.
//   A row of any length is legal and costs its lane's walk.  The five statuses are counted with ballots into wave-uniform
//   registers; at its end a wave adds its counts to the workgroup's (LDS), and the workgroup issues ONE atomic add per class
//   that occurred, as the parse does.
// Nothing here waits for another lane's progress.  The rows, the text and the refusal are record_frame.h's.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_rows.h"
#include "record_time.h"

namespace rejit_amd {

namespace {

// the summary words of a call: a count per status (kSumBadWord, between them, and kSumTimedOut keep their meaning)
__device__ __forceinline__ uint32_t status_word(uint32_t status) { return status < kSumBadWord ? status : status + 1; }
static_assert(kSumKept == 0 && kSumMatching == 1 && kSumCrossing == 2 && kSumBadWord == 3 && kSumSelected == 4 && kSumTotal == 5, "status_word");
// persistent: a workgroup is a wave per SIMD; the kernel needs 76 VGPRs, six waves per SIMD (profiles/time_kernel_resources.txt),
// so six workgroups for each of the 256 CUs are resident at once -- a seventh would run its whole share behind the others
constexpr unsigned kTimeGrid = 256 * 6;

__global__ __launch_bounds__(kThreads) void record_time_check_kernel(Rows R, uint64_t n_records, uint64_t n, uint64_t k, uint64_t n_units,
                                                                     unsigned long long* summary) {
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    const bool bad = j < k && rows::resolve(R.rec_begin, R.rec_end, R.indices, n_records, n, j).bad;
    note_bad_row(bad, j, &summary[kSumBadWord]);
  }
}

__global__ __launch_bounds__(kThreads) void record_time_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint64_t n_records, uint64_t k,
                                                               uint64_t n_units, timeparse::Program program, int unit_of_time, unsigned flags,
                                                               uint64_t* __restrict__ value, uint8_t* __restrict__ status, unsigned long long* summary) {
  __shared__ uint32_t s_count[timeparse::kStatuses];
  __shared__ uint32_t s_program[timeparse::kMaxFormat / 4];
  if (refused(summary)) return;
  if (threadIdx.x < timeparse::kStatuses) s_count[threadIdx.x] = 0;
  if (threadIdx.x == kThreads - 1) {
#pragma unroll
    for (uint32_t i = 0; i < timeparse::kMaxFormat / 4; i++) s_program[i] = program.words[i];
  }
  __syncthreads();
  const uint8_t* code = reinterpret_cast<const uint8_t*>(s_program);
  const uint32_t code_len = program.len;
  const DeviceText src{text, n};
  uint32_t count[timeparse::kStatuses] = {0, 0, 0, 0, 0};   // (wave-uniform; a wave sees fewer than 2^31 rows)
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    uint32_t st = timeparse::kStatuses;   // (a lane without a row counts nowhere)
    if (j < k) {
      const rows::Row row = rows::resolve(R.rec_begin, R.rec_end, R.indices, n_records, n, j);
      timeparse::Result res{timeparse::kMalformed, 0};
      if (!row.bad) {   // (every row passed the check; a lane is still never led outside the text)
        const uint64_t len = row.len(), groups = rows::n_groups(len);
        timeparse::State s = timeparse::start(flags);
        uint32_t w[4] = {0, 0, 0, 0};
        if (groups) rows::load_group(src, n, row.rb, len, 0, w);
        for (uint64_t g = 0; g < groups && !timeparse::done(s); g++) {
          uint32_t next[4] = {0, 0, 0, 0};
          if (g + 1 < groups) rows::load_group(src, n, row.rb, len, g + 1, next);
          const uint64_t left = len - g * rows::kGroupBytes;
          timeparse::step(s, code, code_len, w, left < rows::kGroupBytes ? static_cast<uint32_t>(left) : static_cast<uint32_t>(rows::kGroupBytes));
          w[0] = next[0], w[1] = next[1], w[2] = next[2], w[3] = next[3];
        }
        res = timeparse::finish(s, code_len, unit_of_time);
      }
      st = res.status;
      value[j] = res.bits;
      if (status) status[j] = static_cast<uint8_t>(st);
    }
#pragma unroll
    for (uint32_t c = 0; c < timeparse::kStatuses; c++) count[c] += static_cast<uint32_t>(__popcll(__ballot(st == c)));
  }
  if (lane_id() == 0) {
#pragma unroll
    for (uint32_t c = 0; c < timeparse::kStatuses; c++)
      if (count[c]) atomicAdd(&s_count[c], count[c]);
  }
  __syncthreads();
  if (threadIdx.x < timeparse::kStatuses && s_count[threadIdx.x])
    atomicAdd(&summary[status_word(threadIdx.x)], static_cast<unsigned long long>(s_count[threadIdx.x]));
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_parse_time(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                                   const uint64_t* d_indices, uint64_t n_indices, const char* format, uint64_t format_len, int unit, unsigned flags,
                                   uint64_t* d_value, uint8_t* d_status, rj_parse_stats* stats, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_parse_time";
  const uint64_t k = d_indices ? n_indices : n_records;
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) || (k && !d_value) || (!format && format_len))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse_time: null argument");
  if (!aligned8(d_rec_begin, d_rec_end, d_indices, d_value))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse_time: a table is not 8-byte aligned");
  timeparse::Program program;
  uint32_t at = 0;
  const int bad_format = timeparse::compile(reinterpret_cast<const uint8_t*>(format), format_len, &program, &at);
  if (bad_format != timeparse::kFormatOk)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse_time: format byte %u: %s", at, timeparse::format_error_text(bad_format));
  if (!timeparse::unit_known(unit))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse_time: unit %d is not RJ_TIME_SECOND, RJ_TIME_MILLI, RJ_TIME_MICRO or RJ_TIME_NANO", unit);
  if (!timeparse::flags_known(flags)) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_parse_time: flags %#x: the only flag is RJ_PARSE_TRIM", flags);
  if (!rows::rows_fit(k))
    return rj_fail(RJ_TOO_LARGE, "rj_scan_records_parse_time: %llu rows: the record calls that read rows take fewer than 2^31 of them",
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
  const dim3 block(kThreads), grid(static_cast<unsigned>(n_units < kTimeGrid ? n_units : kTimeGrid));
  hipLaunchKernelGGL(record_time_check_kernel, dim3(unit_grid(n_units)), block, 0, st, R, n_records, n, k, n_units, summary);
  hipLaunchKernelGGL(record_time_kernel, grid, block, 0, st, text, n, R, n_records, k, n_units, program, unit, flags, d_value, d_status, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0)
    return rj_fail(RJ_BAD_ARGUMENT,
                   "rj_scan_records_parse_time: row %llu names no record or a record outside the text (index < n_records, begin <= end <= n)",
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
