// rejit_amd/csrc/record_replace.hip -- rj_scan_records_replace: the pack of record_pack.hip in which every packed record has
// its own matches replaced by `with` -- `sed 's/RE/with/g'` over lines, `str.replace` over a column -- with the new record
// table, in one call and without a download.  record_replace.h has the arithmetic; three launches on one stream:
//
// Table: match-major, one match per lane, a unit = 256 matches.  A lane's match length, a 64-bit wave scan, the unit's place
// from the decoupled look-back of tile_lookback.h (tickets in arrival order, publish BEFORE resolve, as record_pack.hip's
// plan).  It writes D[g] = begin_g - removed[g] + g * with_len for g in [0, m].  16 bytes per match read, 8 written.
//
// Plan: the pack's plan with row_advance = len'(j) + gap: one row per lane; a row with matches reads two spans and two table
// entries more.  It checks its rows (index, row, a saturated count, first + count <= m, the first match's begin, the last
// match's end), writes ob / oe and leaves the total and the first bad row with its kind in the summary.
//
// Copy: output-major, 16 KiB chunks, a persistent grid, the total read from the summary (one synchronise per call).  Per
// chunk the rows that touch it are staged in LDS when they fit -- ob, source begin, first, count and base of each --, and
// every lane produces 16 aligned output bytes at a time: the row by a search in the stage, the piece by a search in the
// row's slice of D (global memory: a line's matches sit in one or two cache lines), then -- 16 bytes inside one text piece
// -- the pack's misaligned 16-byte read and one 16-byte store.  A group with a replacement or a seam in it goes byte by byte.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_internal.h"
#include "kernel_util.h"
#include "record_pack.h"
#include "record_replace.h"
#include "record_text.h"
#include "stream_load.h"
#include "tile_lookback.h"
#include "wave_ops.h"

namespace rejit_amd {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr uint64_t kCopyChunk = 16384;    // output bytes per chunk: four passes of 256 lanes x 16 bytes
constexpr uint32_t kStageRows = 512;      // rows a chunk stages: 18 KiB of LDS, eight workgroups per CU
constexpr unsigned kCopyGrid = 256 * 8;   // persistent: eight workgroups for each of the 256 CUs
static_assert(kThreads == replace::kTableUnit, "a unit of the table is one match per lane");

// the summary the three kernels share (device words, copied to the scan's pinned copy; eight words, as record_pack.hip's)
enum { kSumTotal = 0, kSumBad /* replace::bad_word of the first bad row, 0: none */, kSumTimedOut, kSumWords = 8 };

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

// One unit of a scan in arrival order: `add` per lane -> the sum of everything before this lane (all units before, all lanes
// before).  s_wave / s_before / s_timed_out are the caller's LDS words.  False: the look-back timed out (workgroup-uniform).
__device__ __forceinline__ bool unit_exclusive_sum(uint64_t add, uint64_t tk, uint64_t n_units, unsigned long long* granules, unsigned long long* s_wave,
                                                   unsigned long long* s_before, uint32_t* s_timed_out, unsigned long long* summary, uint64_t* before_lane,
                                                   uint64_t* unit_end) {
  const int wv = static_cast<int>(threadIdx.x) >> 6;
  const int lane = lane_id();
  const uint64_t inc = wave_inclusive_sum64(add);
  if (lane == kWave - 1) s_wave[wv] = inc;
  __syncthreads();
  if (wv == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) total += s_wave[w];
    if (lane == 0) lookback::publish(granules, n_units, tk, total);
    unsigned long long before = 0;
    const bool ok = lookback::resolve(granules, n_units, tk, &before);
    if (lane == 0) {
      s_before[0] = before;
      s_before[1] = before + total;
      if (!ok) {
        *s_timed_out = 1;
        summary[kSumTimedOut] = 1;
      }
    }
  }
  __syncthreads();
  uint64_t at = s_before[0] + inc - add;
#pragma unroll
  for (int w = 0; w < kWaves; w++)
    if (w < wv) at += s_wave[w];
  *before_lane = at;
  *unit_end = s_before[1];
  return *s_timed_out == 0;
}

__global__ __launch_bounds__(kThreads) void record_replace_table_kernel(const uint64_t* __restrict__ spans, uint64_t m, uint64_t n, uint64_t with_len,
                                                                        unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                                        uint64_t* __restrict__ table, unsigned long long* summary) {
  __shared__ unsigned long long s_ticket, s_before[2];
  __shared__ unsigned long long s_wave[kWaves];
  __shared__ uint32_t s_timed_out;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_timed_out = 0;
  for (;;) {
    if (tid == 0) s_ticket = atomicAdd(ticket, 1ull);
    __syncthreads();
    const uint64_t tk = s_ticket;
    if (tk >= n_units) return;
    const uint64_t g = tk * kThreads + tid;
    uint64_t begin = n, len = 0;
    if (g < m) {
      begin = spans[2 * g];
      len = replace::match_length(begin, spans[2 * g + 1], n);
    }
    uint64_t removed, unit_end;
    const bool ok = unit_exclusive_sum(len, tk, n_units, granules, s_wave, s_before, &s_timed_out, summary, &removed, &unit_end);
    if (ok && g <= m) table[g] = replace::table_entry(begin, removed, g, with_len);
  }
}

__global__ __launch_bounds__(kThreads) void record_replace_plan_kernel(DeviceMem M, uint64_t n_records, uint64_t k, uint64_t n, uint64_t m, uint64_t lead,
                                                                       uint64_t gap, unsigned long long* granules, unsigned long long* ticket,
                                                                       uint64_t n_units, uint64_t* __restrict__ out_begin, uint64_t* __restrict__ out_end,
                                                                       unsigned long long* summary) {
  __shared__ unsigned long long s_ticket, s_before[2];
  __shared__ unsigned long long s_wave[kWaves];
  __shared__ uint32_t s_timed_out;
  const uint32_t tid = threadIdx.x;
  const int lane = lane_id();
  if (summary[kSumTimedOut] != 0) return;   // the table is not whole: nothing is planned, nothing copied
  if (n_units == 0) {                       // no rows: the output is the lead
    if (blockIdx.x == 0 && tid == 0) summary[kSumTotal] = lead;
    return;
  }
  if (tid == 0) s_timed_out = 0;
  for (;;) {
    if (tid == 0) s_ticket = atomicAdd(ticket, 1ull);
    __syncthreads();
    const uint64_t tk = s_ticket;
    if (tk >= n_units) return;
    const uint64_t j = tk * kThreads + tid;
    replace::RowPlan row{replace::kOk, 0};
    uint64_t add = 0;
    if (j < k) {
      row = replace::plan_row(M, j, M.indices_ != nullptr, n_records, n, m);
      add = row.kind == replace::kOk ? row.len + gap : 0;   // (a bad row adds nothing: the sums of a refused call cannot overflow)
    }
    const uint64_t bad_lanes = __ballot(row.kind != replace::kOk);
    if (bad_lanes && lane == __builtin_ctzll(bad_lanes))
      atomicMax(&summary[kSumBad], static_cast<unsigned long long>(replace::bad_word(j, row.kind)));
    uint64_t before, unit_end;
    const bool ok = unit_exclusive_sum(add, tk, n_units, granules, s_wave, s_before, &s_timed_out, summary, &before, &unit_end);
    if (ok && tk == n_units - 1 && tid == 0) summary[kSumTotal] = lead + unit_end;
    if (ok && j < k) {
      if (out_begin) out_begin[j] = lead + before;
      if (out_end) out_end[j] = lead + before + row.len;
    }
  }
}

__global__ __launch_bounds__(kThreads) void record_replace_copy_kernel(const uint8_t* __restrict__ text, uint64_t n, DeviceMem M, uint64_t k,
                                                                       const uint64_t* __restrict__ ob, uint64_t gap, uint32_t fill, uint64_t with_len,
                                                                       uint64_t chunk, uint32_t stage_cap, uint8_t* __restrict__ out, uint64_t out_cap,
                                                                       const unsigned long long* summary) {
  __shared__ uint64_t s_ob[kStageRows + 1];
  __shared__ uint64_t s_src[kStageRows];
  __shared__ uint64_t s_first[kStageRows];
  __shared__ uint64_t s_base[kStageRows];
  __shared__ uint32_t s_count[kStageRows];
  __shared__ uint64_t s_rows[2];
  if (summary[kSumBad] != 0 || summary[kSumTimedOut] != 0) return;   // a refused plan: its tables are not followed anywhere
  const uint64_t total = summary[kSumTotal];
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint64_t n_chunks = (limit + chunk - 1) / chunk;
  const uint32_t tid = threadIdx.x;
  const bool have_indices = M.indices_ != nullptr;
  const pack::View table{ob, nullptr, nullptr, nullptr, 0, k, total};
  const DeviceText src{text, n};
  for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t c0 = c * chunk;
    const uint64_t c1 = c0 + chunk < limit ? c0 + chunk : limit;
    // ---- the rows that touch the chunk: two searches side by side, the second one from row 0 (it does not wait for the first)
    if (tid == 0) s_rows[0] = pack::chunk_first_row(table, k, c0);
    if (tid == kWave) s_rows[1] = pack::chunk_end_row(table, k, 0, c1);
    __syncthreads();
    pack::Rows rows;
    rows.j0 = s_rows[0];
    rows.j1 = s_rows[1] > rows.j0 ? s_rows[1] : rows.j0;
    const bool staged = pack::chunk_fits_stage(rows, stage_cap);   // workgroup-uniform
    pack::View view = table;
    replace::Stage stage{nullptr, nullptr, nullptr};
    if (staged) {
      for (uint64_t i = tid; i <= rows.j1 - rows.j0; i += kThreads) {
        s_ob[i] = table.ob_at(rows.j0 + i);
        if (rows.j0 + i < rows.j1) {
          const replace::RowInfo x = replace::row_info(M, rows.j0 + i, have_indices);
          s_src[i] = x.rb;
          s_first[i] = x.f;
          s_base[i] = x.base;
          s_count[i] = x.c;
        }
      }
      __syncthreads();
      view = pack::View{s_ob, s_src, nullptr, nullptr, rows.j0, ~0ull, total};
      stage = replace::Stage{s_first, s_base, s_count};
    }
    // ---- 16 aligned output bytes per lane and pass
    for (uint64_t p = c0 + static_cast<uint64_t>(tid) * pack::kGroupBytes; p < c1; p += static_cast<uint64_t>(kThreads) * pack::kGroupBytes) {
      uint32_t w[4];
      replace::group16(view, stage, M, have_indices, rows, p, limit, gap, fill, with_len, src, w);
      const uint32_t bytes = pack::group_store_bytes(p, limit);
      if (bytes == pack::kGroupBytes) {
        *reinterpret_cast<uint4*>(out + p) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (uint32_t b = 0; b < bytes; b++) out[p + b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
      }
    }
    __syncthreads();   // (the next chunk rewrites s_rows and the stage)
  }
}

int ensure_summary(rj_scan* s) {
  if (!s->rec_host) RJ_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->rec_host), kSumWords * sizeof(unsigned long long)));
  RJ_HIP(s->rec_summary.reserve(kSumWords * sizeof(unsigned long long)));
  return RJ_OK;
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
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) || (!d_out && out_cap) || (!with && with_len))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: null argument");
  if (fill < 0 || fill > 255) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: fill %d is not a byte (0..255)", fill);
  if (reinterpret_cast<uintptr_t>(d_out) & 15u) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_replace: d_out is not 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(d_rec_begin) | reinterpret_cast<uintptr_t>(d_rec_end) | reinterpret_cast<uintptr_t>(d_indices) |
        reinterpret_cast<uintptr_t>(d_first) | reinterpret_cast<uintptr_t>(d_out_begin) | reinterpret_cast<uintptr_t>(d_out_end)) & 7u) ||
      (reinterpret_cast<uintptr_t>(d_counts) & 3u))
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
  int rc = ensure_summary(s);
  if (rc != RJ_OK) return rc;
  const uint64_t table_units = (m + 1 + kThreads - 1) / kThreads;
  const uint64_t plan_units = (k + kThreads - 1) / kThreads;
  // scratch: the two tickets, then the table's look-back words, then the plan's
  const uint64_t table_words = lookback::granule_words(table_units);
  const size_t scratch_bytes = (2 + table_words + lookback::granule_words(plan_units)) * sizeof(unsigned long long);
  RJ_HIP(s->rec_granules.reserve(scratch_bytes));
  RJ_HIP(s->rec_repl_table.reserve((m + 1) * sizeof(uint64_t)));
  RJ_HIP(s->with_buf.reserve(std::max<uint64_t>(with_len, 16)));
  const bool copies = out_cap != 0;
  uint64_t* ob = d_out_begin;
  if (!ob && copies && k) {   // (the copy needs the table)
    RJ_HIP(s->rec_pack_begin.reserve(k * sizeof(uint64_t)));
    ob = s->rec_pack_begin.as<uint64_t>();
  }
  unsigned long long* scratch = s->rec_granules.as<unsigned long long>();
  unsigned long long* summary = s->rec_summary.as<unsigned long long>();
  uint64_t* table = s->rec_repl_table.as<uint64_t>();
  RJ_HIP(hipMemsetAsync(scratch, 0, scratch_bytes, st));
  RJ_HIP(hipMemsetAsync(summary, 0, kSumWords * sizeof(unsigned long long), st));
  if (with_len && copies) RJ_HIP(hipMemcpyAsync(s->with_buf.p, with, with_len, hipMemcpyHostToDevice, st));
  const DeviceMem mem{d_rec_begin, d_rec_end, d_first, d_counts, d_indices, spans, table, s->with_buf.as<uint8_t>()};
  const unsigned table_grid = static_cast<unsigned>(std::min<uint64_t>(table_units, 1024));   // persistent: workgroups take units
  hipLaunchKernelGGL(record_replace_table_kernel, dim3(table_grid), dim3(kThreads), 0, st, spans, m, n, with_len, scratch + 2, scratch, table_units, table,
                     summary);
  const unsigned plan_grid = static_cast<unsigned>(std::min<uint64_t>(std::max<uint64_t>(plan_units, 1), 1024));
  hipLaunchKernelGGL(record_replace_plan_kernel, dim3(plan_grid), dim3(kThreads), 0, st, mem, n_records, k, n, m, lead, gap, scratch + 2 + table_words,
                     scratch + 1, plan_units, ob, d_out_end, summary);
  if (copies) {
    const uint64_t cap_chunks = (out_cap + kCopyChunk - 1) / kCopyChunk;
    const unsigned copy_grid = static_cast<unsigned>(std::min<uint64_t>(cap_chunks, kCopyGrid));
    hipLaunchKernelGGL(record_replace_copy_kernel, dim3(copy_grid), dim3(kThreads), 0, st, static_cast<const uint8_t*>(d_text), n, mem, k, ob, gap,
                       static_cast<uint32_t>(fill), with_len, kCopyChunk, kStageRows, static_cast<uint8_t*>(d_out), out_cap, summary);
  }
  RJ_HIP(hipMemcpyAsync(s->rec_host, summary, kSumWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  RJ_HIP(hipStreamSynchronize(st));
  RJ_HIP(hipGetLastError());
  if (s->rec_host[kSumTimedOut] != 0) return rj_fail(RJ_DEVICE_ERROR, "rj_scan_records_replace: the look-back timed out");
  if (s->rec_host[kSumBad] != 0) return refuse_row(s->rec_host[kSumBad]);
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
