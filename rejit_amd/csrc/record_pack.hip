// rejit_amd/csrc/record_pack.hip -- rj_scan_records_pack: a list of records of one device text -- every record, or the rows
// rj_scan_records_select listed, or any permutation / take -- gathered into a NEW contiguous device text, `gap` fill bytes
// behind each record and `lead` in front, with the new record table.  It is what a grep-like caller prints (the selected
// lines, fill = '\n') and what makes the strings of an Arrow-layout column independent of each other (fill = the program's
// rj_batch_separator) without a trip to the host.  record_pack.h has the arithmetic; two launches:
//
// Plan: record-major, one row per lane, a unit = 256 rows.  A lane's length + gap, a 64-bit wave scan (wave_ops.h), the
// unit's place from the decoupled look-back of tile_lookback.h (tickets in arrival order; a unit publishes BEFORE it looks
// back, exactly as record_select_kernel).  It writes ob / oe, checks its rows, leaves the total and the first bad row in the
// summary.  16 bytes per row read (+ 8 with indices), 8 to 16 written.
//
// Copy: output-major, so a workgroup's work does not depend on the records' sizes.  The output [0, min(total, out_cap)) is cut
// into chunks of 16 KiB; the grid is persistent and reads the total from the summary (the host has not seen it yet: one
// synchronise per call).  Per chunk two lanes search the ob table for the rows that touch it, the rows' ob and source begins
// are staged in LDS when they fit (else every lane searches the table), and every lane produces 16 aligned output bytes at a
// time: one search for its piece, then -- the common case, 16 bytes inside one record -- two aligned 16-byte loads around the
// source, a byte funnel shift, one 16-byte store.  Text in, output out, once each.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_internal.h"
#include "kernel_util.h"
#include "record_pack.h"
#include "record_text.h"
#include "stream_load.h"
#include "tile_lookback.h"
#include "wave_ops.h"

namespace rejit_amd {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr uint64_t kCopyChunk = 16384;    // output bytes per chunk: four passes of 256 lanes x 16 bytes
constexpr uint32_t kStageRows = 1024;     // rows a chunk stages: 2 x 8 KiB of LDS, eight workgroups per CU
constexpr unsigned kCopyGrid = 256 * 8;   // persistent: eight workgroups for each of the 256 CUs

// the summary both kernels share (device words, copied to the scan's pinned copy; eight words, as record_join.hip's)
enum { kSumTotal = 0, kSumBadRow /* ~(first bad row), 0: none */, kSumTimedOut, kSumWords = 8 };

__global__ __launch_bounds__(kThreads) void record_pack_plan_kernel(const uint64_t* __restrict__ rec_begin, const uint64_t* __restrict__ rec_end,
                                                                    uint64_t n_records, const uint64_t* __restrict__ indices, uint64_t k, uint64_t n,
                                                                    uint64_t lead, uint64_t gap, unsigned long long* granules, unsigned long long* ticket,
                                                                    uint64_t n_units, uint64_t* __restrict__ out_begin, uint64_t* __restrict__ out_end,
                                                                    unsigned long long* summary) {
  __shared__ unsigned long long s_ticket, s_before;
  __shared__ unsigned long long s_wave[kWaves];
  __shared__ uint32_t s_timed_out;
  const uint32_t tid = threadIdx.x;
  const int wv = static_cast<int>(tid) >> 6;
  const int lane = lane_id();
  if (n_units == 0) {   // no rows: the output is the lead
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
    uint64_t len = 0, add = 0;
    bool bad = false;
    if (j < k) {
      const uint64_t r = indices ? indices[j] : j;
      bad = pack::bad_index(r, n_records);
      uint64_t rb = 0, re = 0;
      if (!bad) {
        rb = rec_begin[r];
        re = rec_end[r];
        bad = pack::bad_row(rb, re, n);
      }
      add = pack::row_advance(bad, rb, re, gap);
      len = bad ? 0 : re - rb;
    }
    const uint64_t inc = wave_inclusive_sum64(add);
    if (lane == kWave - 1) s_wave[wv] = inc;
    const uint64_t bad_lanes = __ballot(bad);
    if (bad_lanes && lane == 0)
      atomicMax(&summary[kSumBadRow],
                static_cast<unsigned long long>(~(tk * kThreads + static_cast<uint64_t>(wv) * kWave + static_cast<uint64_t>(__builtin_ctzll(bad_lanes)))));
    __syncthreads();
    if (wv == 0) {
      unsigned long long total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; w++) total += s_wave[w];
      if (lane == 0) lookback::publish(granules, n_units, tk, total);
      unsigned long long before = 0;
      const bool ok = lookback::resolve(granules, n_units, tk, &before);
      if (lane == 0) {
        s_before = before;
        if (!ok) {
          s_timed_out = 1;
          summary[kSumTimedOut] = 1;
        } else if (tk == n_units - 1) {
          summary[kSumTotal] = lead + before + total;
        }
      }
    }
    __syncthreads();
    if (s_timed_out == 0 && j < k) {
      uint64_t at = lead + s_before + inc - add;
#pragma unroll
      for (int w = 0; w < kWaves; w++)
        if (w < wv) at += s_wave[w];
      if (out_begin) out_begin[j] = at;
      if (out_end) out_end[j] = at + len;
    }
  }
}

__global__ __launch_bounds__(kThreads) void record_pack_copy_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ rec_begin,
                                                                    const uint64_t* __restrict__ indices, uint64_t k, const uint64_t* __restrict__ ob,
                                                                    uint64_t gap, uint32_t fill, uint64_t chunk, uint32_t stage_cap,
                                                                    uint8_t* __restrict__ out, uint64_t out_cap, const unsigned long long* summary) {
  __shared__ uint64_t s_ob[kStageRows + 1];
  __shared__ uint64_t s_src[kStageRows];
  __shared__ uint64_t s_rows[2];
  if (summary[kSumBadRow] != 0 || summary[kSumTimedOut] != 0) return;   // a refused plan: its table is not followed anywhere
  const uint64_t total = summary[kSumTotal];
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint64_t n_chunks = (limit + chunk - 1) / chunk;
  const uint32_t tid = threadIdx.x;
  const pack::View table{ob, nullptr, rec_begin, indices, 0, k, total};
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
    if (staged) {
      for (uint64_t i = tid; i <= rows.j1 - rows.j0; i += kThreads) {
        s_ob[i] = table.ob_at(rows.j0 + i);
        if (rows.j0 + i < rows.j1) s_src[i] = table.src_at(rows.j0 + i);
      }
      __syncthreads();
      view = pack::View{s_ob, s_src, nullptr, nullptr, rows.j0, ~0ull, total};
    }
    // ---- 16 aligned output bytes per lane and pass
    for (uint64_t p = c0 + static_cast<uint64_t>(tid) * pack::kGroupBytes; p < c1; p += static_cast<uint64_t>(kThreads) * pack::kGroupBytes) {
      uint32_t w[4];
      pack::group16(view, rows, p, limit, gap, fill, src, w);
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

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_pack(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                             const uint64_t* d_indices, uint64_t n_indices, int fill, uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap,
                             uint64_t* d_out_begin, uint64_t* d_out_end, void* hip_stream) {
  ErrnoGuard errno_guard;
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) || (!d_out && out_cap))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: null argument");
  if (fill < 0 || fill > 255) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: fill %d is not a byte (0..255)", fill);
  if (reinterpret_cast<uintptr_t>(d_out) & 15u) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: d_out is not 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_rec_begin) | reinterpret_cast<uintptr_t>(d_rec_end) | reinterpret_cast<uintptr_t>(d_indices) |
       reinterpret_cast<uintptr_t>(d_out_begin) | reinterpret_cast<uintptr_t>(d_out_end)) & 7u)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: a table is not 8-byte aligned");
  const uint64_t k = d_indices ? n_indices : n_records;
  if (!pack::sums_fit(k, n, lead, gap))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: %llu rows of a text of %llu bytes can exceed 2^62 output bytes (or n + gap reaches 2^42)",
                   static_cast<unsigned long long>(k), static_cast<unsigned long long>(n));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  int rc = ensure_summary(s);
  if (rc != RJ_OK) return rc;
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  const size_t scratch_bytes = (lookback::granule_words(n_units) + 1) * sizeof(unsigned long long);   // the ticket, then the look-back's words
  RJ_HIP(s->rec_granules.reserve(scratch_bytes));
  const bool copies = out_cap != 0;
  uint64_t* ob = d_out_begin;
  if (!ob && copies && k) {   // (the copy needs the table)
    RJ_HIP(s->rec_pack_begin.reserve(k * sizeof(uint64_t)));
    ob = s->rec_pack_begin.as<uint64_t>();
  }
  unsigned long long* scratch = s->rec_granules.as<unsigned long long>();
  unsigned long long* summary = s->rec_summary.as<unsigned long long>();
  RJ_HIP(hipMemsetAsync(scratch, 0, scratch_bytes, st));
  RJ_HIP(hipMemsetAsync(summary, 0, kSumWords * sizeof(unsigned long long), st));
  const unsigned plan_grid = static_cast<unsigned>(std::min<uint64_t>(std::max<uint64_t>(n_units, 1), 1024));   // persistent: workgroups take units
  hipLaunchKernelGGL(record_pack_plan_kernel, dim3(plan_grid), dim3(kThreads), 0, st, d_rec_begin, d_rec_end, n_records, d_indices, k, n, lead, gap,
                     scratch + 1, scratch, n_units, ob, d_out_end, summary);
  if (copies) {
    const uint64_t cap_chunks = (out_cap + kCopyChunk - 1) / kCopyChunk;
    const unsigned copy_grid = static_cast<unsigned>(std::min<uint64_t>(cap_chunks, kCopyGrid));
    hipLaunchKernelGGL(record_pack_copy_kernel, dim3(copy_grid), dim3(kThreads), 0, st, static_cast<const uint8_t*>(d_text), n, d_rec_begin, d_indices, k,
                       ob, gap, static_cast<uint32_t>(fill), kCopyChunk, kStageRows, static_cast<uint8_t*>(d_out), out_cap, summary);
  }
  RJ_HIP(hipMemcpyAsync(s->rec_host, summary, kSumWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  RJ_HIP(hipStreamSynchronize(st));
  RJ_HIP(hipGetLastError());
  if (s->rec_host[kSumTimedOut] != 0) return rj_fail(RJ_DEVICE_ERROR, "rj_scan_records_pack: the look-back timed out");
  if (s->rec_host[kSumBadRow] != 0)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: row %llu of the pack names no record or a record outside the text (index < n_records, begin <= end <= n)",
                   static_cast<unsigned long long>(~s->rec_host[kSumBadRow]));
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
