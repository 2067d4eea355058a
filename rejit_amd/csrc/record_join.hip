// rejit_amd/csrc/record_join.hip -- per-record answers over device-resident text: rj_scan_records hands the matches of one
// whole-text run to the caller's records (counts, first match, a four-word summary), rj_scan_records_select lists the
// records with (or without) a match.  Text, match list and record table are all in HBM already; what lies between them
// and a small answer is a sorted join (record_join.h has the rule), and that join is a kernel here instead of a download
// of both lists and a merge on one CPU thread (finish_packed, host_api.hip; samples/jrep_gpu.*).
//
// Join: record-major.  A workgroup owns a tile of 256 records, one per lane: exactly one lane writes a record's outputs,
// nothing has to be cleared first.  Two lanes (of two waves, side by side) search the scan's list for the tile's first and
// last bound; the begins in between are staged in LDS when they fit (32 KiB) and every lane makes its two searches there,
// else every lane searches the list itself (a record with more matches than LDS holds, a tile of huge records).  The same
// lanes check the table.  Per workgroup: wave reductions (wave_ops.h) of kept / matching / crossing / first bad row, summed
// over the workgroup's tiles, then one atomic instruction into the summary.
// Traffic: the begins of the list once (8 bytes per match, in lines that also hold the ends), 16 bytes per record read,
// 4 to 12 written; one more 8-byte read per record WITH a match (the end of its last match: does it cross).  The text is
// not touched.
//
// Selection: one pass, the final place of a tile's indices from the decoupled look-back of tile_lookback.h through
// record_frame.h's unit_take / unit_place (tickets in arrival order; a unit publishes its count BEFORE it looks back): no
// sort, no device-wide slot counter.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_join.h"

namespace rejit_amd {

namespace {

constexpr uint32_t kStageBegins = 4096;   // begins a tile stages: 32 KiB of LDS, four to five workgroups per CU
constexpr int kSelectRows = 8;            // selection: rows of 256 records per unit of the look-back
constexpr uint64_t kSelectUnit = static_cast<uint64_t>(kSelectRows) * kThreads;

__global__ __launch_bounds__(kThreads) void record_join_kernel(const uint64_t* __restrict__ spans, uint64_t m, const uint64_t* __restrict__ rec_begin,
                                                               const uint64_t* __restrict__ rec_end, uint64_t n_records, uint64_t n,
                                                               uint32_t stage_cap, uint32_t* __restrict__ counts, uint64_t* __restrict__ first,
                                                               unsigned long long* summary) {
  __shared__ uint64_t s_stage[kStageBegins];
  __shared__ uint64_t s_range[2];
  __shared__ unsigned long long s_part[kWaves][4];
  const uint32_t tid = threadIdx.x;
  const int wv = static_cast<int>(tid) >> 6;
  const records::Begins list{spans, 2, 0};
  const uint64_t n_tiles = (n_records + kThreads - 1) / kThreads;
  uint64_t acc_kept = 0, acc_matching = 0, acc_crossing = 0, acc_bad = ~0ull;   // wave-uniform; acc_bad: the first bad row
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t r0 = t * kThreads;
    const uint64_t r1 = r0 + kThreads < n_records ? r0 + kThreads : n_records;
    // ---- the tile's range of the list: its first and its last bound, searched side by side (records::tile_range)
    if (tid == 0) s_range[0] = records::lower_bound(list, 0, m, rec_begin[r0]);
    if (tid == kWave) {
      const uint64_t last = r1 - 1;
      const bool has_next = last + 1 < n_records;
      s_range[1] = records::lower_bound(list, 0, m, records::upper_key(rec_end[last], has_next, has_next ? rec_begin[last + 1] : 0));
    }
    __syncthreads();
    const uint64_t lo = s_range[0];
    const uint64_t hi = s_range[1] > lo ? s_range[1] : lo;   // (a bad table must not turn the range inside out)
    const bool staged = hi - lo <= stage_cap;                // workgroup-uniform
    if (staged) {
      for (uint64_t k = tid; k < hi - lo; k += kThreads) s_stage[k] = spans[2 * (lo + k)];
      __syncthreads();
    }
    // ---- one record per lane
    const uint64_t i = r0 + tid;
    uint64_t f = 0, c = 0;
    bool bad = false, cross = false;
    if (i < r1) {
      const uint64_t rb = rec_begin[i], re = rec_end[i];
      const bool has_next = i + 1 < n_records;
      const uint64_t nb = has_next ? rec_begin[i + 1] : 0;
      bad = records::bad_row(rb, re, has_next, nb, n);
      const uint64_t key = records::upper_key(re, has_next, nb);
      if (staged) records::join_row(records::Begins{s_stage, 1, lo}, lo, hi, rb, key, &f, &c);
      else records::join_row(list, lo, hi, rb, key, &f, &c);
      if (c) cross = records::crosses(spans[2 * (f + c - 1) + 1], re);
      counts[i] = records::saturate32(c);
      if (first) first[i] = f;
    }
    // ---- the workgroup's share of the summary (all lanes: a lane without a record adds nothing)
    acc_kept += wave_sum64(c);
    acc_matching += static_cast<uint64_t>(__popcll(__ballot(c != 0)));
    acc_crossing += static_cast<uint64_t>(__popcll(__ballot(cross)));
    const uint64_t bad_lanes = __ballot(bad);
    if (bad_lanes) {
      const uint64_t row = r0 + static_cast<uint64_t>(wv) * kWave + static_cast<uint64_t>(__builtin_ctzll(bad_lanes));
      if (row < acc_bad) acc_bad = row;
    }
    __syncthreads();   // (the next tile rewrites s_range and s_stage)
  }
  if (lane_id() == 0) {
    s_part[wv][kSumKept] = acc_kept;
    s_part[wv][kSumMatching] = acc_matching;
    s_part[wv][kSumCrossing] = acc_crossing;
    s_part[wv][kSumBadWord] = ~acc_bad;   // (the largest complement is the smallest row; 0: none)
  }
  __syncthreads();
  if (tid < 4) {
    unsigned long long v = 0;
    for (int w = 0; w < kWaves; w++) v = tid == kSumBadWord ? (s_part[w][tid] > v ? s_part[w][tid] : v) : v + s_part[w][tid];
    if (v != 0) {
      if (tid == kSumBadWord) atomicMax(&summary[tid], v);
      else atomicAdd(&summary[tid], v);
    }
  }
}

// The indices of the records whose count is non-zero (invert: zero), ascending, at most cap of them written; their number
// in summary[kSumSelected].  A unit = 8 rows of 256 records; row by row a lane's place is (everything before the unit) +
// (the rows and waves before its own) + (the selected lanes below it).
__global__ __launch_bounds__(kThreads) void record_select_kernel(const uint32_t* __restrict__ counts, uint64_t n_records, int invert,
                                                                 unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                                 uint64_t* __restrict__ out, uint64_t cap, unsigned long long* summary) {
  __shared__ UnitPlace s_unit;
  __shared__ uint32_t s_count[kSelectRows][kWaves];
  const uint32_t tid = threadIdx.x;
  const int wv = static_cast<int>(tid) >> 6;
  const int lane = lane_id();
  unit_init(s_unit);
  for (uint64_t tk; unit_take(s_unit, ticket, n_units, &tk);) {
    const uint64_t base = tk * kSelectUnit;
    uint64_t mask[kSelectRows];
#pragma unroll
    for (int j = 0; j < kSelectRows; j++) {
      const uint64_t i = base + static_cast<uint64_t>(j) * kThreads + tid;
      const bool sel = i < n_records && ((counts[i] != 0) != (invert != 0));
      mask[j] = __ballot(sel);
      if (lane == 0) s_count[j][wv] = static_cast<uint32_t>(__popcll(mask[j]));
    }
    __syncthreads();
    const uint32_t total = wv == 0 ? wave_total(lane < kSelectRows * kWaves ? s_count[lane / kWaves][lane % kWaves] : 0u) : 0u;
    if (unit_place(s_unit, total, tk, n_units, granules, summary)) {
      if (tk == n_units - 1 && tid == 0) summary[kSumSelected] = s_unit.end;
      uint64_t at = s_unit.before;
#pragma unroll
      for (int j = 0; j < kSelectRows; j++) {
        uint32_t waves_before = 0, row = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
          const uint32_t k = s_count[j][w];
          if (w < wv) waves_before += k;
          row += k;
        }
        if ((mask[j] >> lane) & 1ull) {
          const uint64_t p = at + waves_before + lanes_below(mask[j]);
          if (p < cap) out[p] = base + static_cast<uint64_t>(j) * kThreads + tid;
        }
        at += row;
      }
    }
  }
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                        uint32_t* d_counts, uint64_t* d_first, rj_record_stats* stats, void* hip_stream) {
  ErrnoGuard errno_guard;
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end))) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records: null argument");
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  // the ordinary whole-text run (never the one-kernel count: the join needs the list); a refusal passes through
  int rc = run_pipeline(s, static_cast<const uint8_t*>(d_text), n, 0, n + 1, 0, 0, 0, st);
  if (rc != RJ_OK) return rc;
  const uint64_t m = s->result_count;
  if (m && !s->result) return rj_fail(RJ_DEVICE_ERROR, "rj_scan_records: internal: the run left no span list");
  rj_record_stats out{};
  out.n_matches = m;
  if (n_records) {
    uint32_t* counts = d_counts;
    if (!counts) {
      RJ_HIP(s->rec_counts.reserve(n_records * sizeof(uint32_t)));
      counts = s->rec_counts.as<uint32_t>();
    }
    unsigned long long *scratch = nullptr, *summary = nullptr;
    if ((rc = records_begin(s, 0, st, &scratch, &summary)) != RJ_OK) return rc;
    const uint64_t n_tiles = (n_records + kThreads - 1) / kThreads;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(n_tiles, 1u << 20));   // (more tiles: a workgroup takes several)
    hipLaunchKernelGGL(record_join_kernel, dim3(grid), dim3(kThreads), 0, st, s->result, m, d_rec_begin, d_rec_end, n_records, n, kStageBegins,
                       counts, d_first, summary);
    if ((rc = records_finish(s, "rj_scan_records", st)) != RJ_OK) return rc;
    if (s->rec_host[kSumBadWord] != 0)
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records: row %llu of the record table is not ascending or not inside the text (begin <= end <= next begin, end <= n)",
                     static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
    out.n_kept = s->rec_host[kSumKept];
    out.n_matching = s->rec_host[kSumMatching];
    out.n_crossing = s->rec_host[kSumCrossing];
    s->rec_select_counts = counts;
  }
  s->rec_n = n_records;
  s->rec_valid = true;
  if (stats) *stats = out;
  return static_cast<int64_t>(out.n_kept);
}

int64_t rj_scan_records_select(rj_scan* s, int invert, uint64_t* d_indices, uint64_t cap, void* hip_stream) {
  ErrnoGuard errno_guard;
  if (!s) return rj_fail(RJ_BAD_ARGUMENT, "null scan");
  if (!s->rec_valid) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_select: the scan's last run was not a successful rj_scan_records");
  if (cap && !d_indices) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_select: null argument");
  if (s->rec_n == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (s->rec_n + kSelectUnit - 1) / kSelectUnit;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, then the look-back's words
  int rc = records_begin(s, 1 + lookback::granule_words(n_units), st, &scratch, &summary);
  if (rc != RJ_OK) return rc;
  hipLaunchKernelGGL(record_select_kernel, dim3(unit_grid(n_units)), dim3(kThreads), 0, st, s->rec_select_counts, s->rec_n, invert, scratch + 1, scratch,
                     n_units, d_indices, cap, summary);
  if ((rc = records_finish(s, "rj_scan_records_select", st)) != RJ_OK) return rc;
  return static_cast<int64_t>(s->rec_host[kSumSelected]);
}

}  // extern "C"
