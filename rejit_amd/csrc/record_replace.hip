// rejit_amd/csrc/record_replace.hip -- rj_scan_records_replace: the pack of record_pack.hip in which every packed record has
// its own matches replaced by `with` -- `sed 's/RE/with/g'` over lines, `str.replace` over a column -- with the new record
// table, in one call and without a download.  record_replace.h has the arithmetic; three launches on one stream:
//
// Table: match-major, one match per lane, a unit = 256 matches.  A lane's match length, then record_frame.h's
// unit_exclusive_sum (a 64-bit wave scan, the unit's place from the decoupled look-back of tile_lookback.h).  It writes
// D[g] = begin_g - removed[g] + g * with_len for g in [0, m].  16 bytes per match read, 8 written.
//
// Plan: record_frame.h's plan_units -- the pack's plan -- with a row's length = len'(j): one row per lane; a row with matches
// reads two spans and two table entries more.  It checks its rows (index, row, a saturated count, first + count <= m, the
// first match's begin, the last match's end), writes ob / oe and leaves the total and the first bad row with its kind in the
// summary.
//
// Copy: record_frame.h's copy_chunks, output-major, in chunks of 16 KiB (one synchronise per call).  A chunk stages ob, source
// begin, first, count and base of its rows, and every lane produces 16 aligned output bytes at a time: the row by a search
// in the stage, the piece by a search in the row's slice of D (global memory: a line's matches sit in one or two cache
// lines), then -- 16 bytes inside one text piece -- the pack's misaligned 16-byte read and one 16-byte store.  A group with a
// replacement or a seam in it goes byte by byte.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_pack.h"
#include "record_replace.h"

namespace rejit_amd {

namespace {

static_assert(kThreads == replace::kTableUnit, "a unit of the table is one match per lane");

struct DeviceMem {
  const uint64_t* rec_begin_;
  const uint64_t* rec_end_;
  const uint64_t* first_;
  const uint32_t* counts_;
  const uint64_t* indices_;
  const uint64_t* spans_;
  const uint64_t* table_;
  const uint8_t* with_;
  __device__ __forceinline__ uint64_t rec_begin(uint64_t r) const { return rec_begin_[r]; }
  __device__ __forceinline__ uint64_t rec_end(uint64_t r) const { return rec_end_[r]; }
  __device__ __forceinline__ uint64_t first(uint64_t r) const { return first_[r]; }
  __device__ __forceinline__ uint32_t count(uint64_t r) const { return counts_[r]; }
  __device__ __forceinline__ uint64_t index(uint64_t j) const { return indices_[j]; }
  __device__ __forceinline__ uint64_t span_begin(uint64_t g) const { return spans_[2 * g]; }
  __device__ __forceinline__ uint64_t span_end(uint64_t g) const { return spans_[2 * g + 1]; }
  __device__ __forceinline__ uint64_t table(uint64_t g) const { return table_[g]; }
  __device__ __forceinline__ uint32_t with_byte(uint64_t i) const { return with_[i]; }
};

__global__ __launch_bounds__(kThreads) void record_replace_table_kernel(const uint64_t* __restrict__ spans, uint64_t m, uint64_t n, uint64_t with_len,
                                                                        unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                                        uint64_t* __restrict__ table, unsigned long long* summary) {
  __shared__ UnitSum s_unit;
  unit_init(s_unit.place);
  for (uint64_t tk; unit_take(s_unit.place, ticket, n_units, &tk);) {
    const uint64_t g = tk * kThreads + threadIdx.x;
    uint64_t begin = n, len = 0;
    if (g < m) {
      begin = spans[2 * g];
      len = replace::match_length(begin, spans[2 * g + 1], n);
    }
    uint64_t removed, unit_end;
    const bool ok = unit_exclusive_sum(s_unit, len, tk, n_units, granules, summary, &removed, &unit_end);
    if (ok && g <= m) table[g] = replace::table_entry(begin, removed, g, with_len);
  }
}

__global__ __launch_bounds__(kThreads) void record_replace_plan_kernel(DeviceMem M, uint64_t n_records, uint64_t k, uint64_t n, uint64_t m, uint64_t lead,
                                                                       uint64_t gap, unsigned long long* granules, unsigned long long* ticket,
                                                                       uint64_t n_units, uint64_t* __restrict__ out_begin, uint64_t* __restrict__ out_end,
                                                                       unsigned long long* summary) {
  if (summary[kSumTimedOut] != 0) return;   // the table is not whole: nothing is planned, nothing copied
  const auto row = [=](uint64_t j) {
    const replace::RowPlan p = replace::plan_row(M, j, M.indices_ != nullptr, n_records, n, m);
    return PlannedRow{p.kind == replace::kOk ? 0 : replace::bad_word(j, p.kind), p.len};
  };
  plan_units(row, k, lead, gap, granules, ticket, n_units, out_begin, out_end, summary);
}

// what a chunk of the copy stages: 18 KiB of LDS, eight workgroups per CU
struct ReplaceCopy {
  static constexpr uint32_t kRows = 512;
  struct Stage {
    uint64_t ob[kRows + 1], src[kRows], first[kRows], base[kRows];
    uint32_t count[kRows];
  };
  DeviceMem M;
  uint64_t with_len;
  __device__ __forceinline__ pack::View table(const uint64_t* ob, uint64_t k, uint64_t total) const {
    return pack::View{ob, nullptr, nullptr, nullptr, 0, k, total};
  }
  __device__ __forceinline__ void stage_row(Stage& s, uint64_t i, const pack::View&, uint64_t j) const {
    const replace::RowInfo x = replace::row_info(M, j, M.indices_ != nullptr);
    s.src[i] = x.rb;
    s.first[i] = x.f;
    s.base[i] = x.base;
    s.count[i] = x.c;
  }
  __device__ __forceinline__ replace::Stage staged(const Stage& s) const { return replace::Stage{s.first, s.base, s.count}; }
  __device__ __forceinline__ replace::Stage unstaged() const { return replace::Stage{nullptr, nullptr, nullptr}; }
  __device__ __forceinline__ void group16(const pack::View& view, const replace::Stage& stage, const pack::Rows& rows, uint64_t p, uint64_t limit,
                                          uint64_t gap, uint32_t fill, const DeviceText& src, uint32_t w[4]) const {
    replace::group16(view, stage, M, M.indices_ != nullptr, rows, p, limit, gap, fill, with_len, src, w);
  }
};

__global__ __launch_bounds__(kThreads) void record_replace_copy_kernel(const uint8_t* __restrict__ text, uint64_t n, DeviceMem M, uint64_t k,
                                                                       const uint64_t* __restrict__ ob, uint64_t gap, uint32_t fill, uint64_t with_len,
                                                                       uint64_t chunk, uint32_t stage_cap, uint8_t* __restrict__ out, uint64_t out_cap,
                                                                       const unsigned long long* summary) {
  copy_chunks(ReplaceCopy{M, with_len}, text, n, k, ob, gap, fill, chunk, stage_cap, out, out_cap, summary);
}

int refuse_row(unsigned long long word) {
  const unsigned long long j = replace::bad_word_row(word);
  switch (replace::bad_word_kind(word)) {
    case replace::kBadIndex:
    case replace::kBadRow:
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: row %llu of the pack names no record or a record outside the text (index < n_records, begin <= end <= n)", j);
    case replace::kBadRange:
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: row %llu has first + count beyond the scan's list: d_counts / d_first are not those of the scan's last rj_scan_records", j);
    case replace::kSaturated:
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: row %llu has a saturated count (UINT32_MAX): the range of its matches is unknown", j);
    case replace::kBeginsBefore:
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: row %llu has a first match that begins before its record: d_counts / d_first are not those of this table", j);
    default:
      return rj_fail(RJ_BAD_ARGUMENT,
                     "rj_scan_records_replace: row %llu has a match that ends beyond its record: the records are not independent (rj_scan_records_pack "
                     "with rj_batch_separator as fill makes them so)", j);
  }
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_replace(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                                const uint32_t* d_counts, const uint64_t* d_first, const uint64_t* d_indices, uint64_t n_indices, const char* with,
                                uint64_t with_len, int fill, uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin,
                                uint64_t* d_out_end, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_replace";
  if (!with && with_len) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: null argument");
  int rc = check_pack_call(kCall, s, d_text, n, d_rec_begin, d_rec_end, n_records, d_out, out_cap, fill);
  if (rc != RJ_OK) return rc;
  if (!aligned8(d_rec_begin, d_rec_end, d_indices, d_first, d_out_begin, d_out_end) || (reinterpret_cast<uintptr_t>(d_counts) & 3u))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: a table is not 8-byte aligned (d_counts: 4-byte)");
  const uint64_t k = d_indices ? n_indices : n_records;
  if (k && (!d_counts || !d_first)) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: d_counts and d_first (as rj_scan_records wrote them) are needed");
  const uint64_t m = s->result_count;
  const uint64_t* spans = s->result;
  if (m && !spans)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: the last run was counts-only: there is no span list to replace (rj_multi_set_counts_only / rj_scan_count)");
  if (!replace::sums_fit(k, n, m, with_len, lead, gap))
    return rj_fail(RJ_BAD_ARGUMENT,
                   "rj_scan_records_replace: %llu rows of a text of %llu bytes with %llu matches can exceed 2^62 output bytes (or n + (matches + 1) * with_len + gap reaches 2^42)",
                   static_cast<unsigned long long>(k), static_cast<unsigned long long>(n), static_cast<unsigned long long>(m));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t table_units = (m + 1 + kThreads - 1) / kThreads;
  const uint64_t row_units = (k + kThreads - 1) / kThreads;
  const uint64_t table_words = lookback::granule_words(table_units);
  RJ_HIP(s->rec_repl_table.reserve((m + 1) * sizeof(uint64_t)));
  RJ_HIP(s->with_buf.reserve(std::max<uint64_t>(with_len, 16)));
  const bool copies = out_cap != 0;
  uint64_t* ob = nullptr;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the two tickets, then the table's look-back words, then the plan's
  if ((rc = pack_begin_table(s, d_out_begin, copies, k, &ob)) != RJ_OK) return rc;
  if ((rc = records_begin(s, 2 + table_words + lookback::granule_words(row_units), st, &scratch, &summary)) != RJ_OK) return rc;
  uint64_t* table = s->rec_repl_table.as<uint64_t>();
  if (with_len && copies) RJ_HIP(hipMemcpyAsync(s->with_buf.p, with, with_len, hipMemcpyHostToDevice, st));
  const DeviceMem mem{d_rec_begin, d_rec_end, d_first, d_counts, d_indices, spans, table, s->with_buf.as<uint8_t>()};
  hipLaunchKernelGGL(record_replace_table_kernel, dim3(unit_grid(table_units)), dim3(kThreads), 0, st, spans, m, n, with_len, scratch + 2, scratch,
                     table_units, table, summary);
  hipLaunchKernelGGL(record_replace_plan_kernel, dim3(unit_grid(row_units)), dim3(kThreads), 0, st, mem, n_records, k, n, m, lead, gap,
                     scratch + 2 + table_words, scratch + 1, row_units, ob, d_out_end, summary);
  if (copies)
    hipLaunchKernelGGL(record_replace_copy_kernel, dim3(copy_grid(out_cap)), dim3(kThreads), 0, st, static_cast<const uint8_t*>(d_text), n, mem, k, ob, gap,
                       static_cast<uint32_t>(fill), with_len, kCopyChunk, ReplaceCopy::kRows, static_cast<uint8_t*>(d_out), out_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0) return refuse_row(s->rec_host[kSumBadWord]);
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
