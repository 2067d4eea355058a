// rejit_amd/csrc/record_split.hip -- rj_scan_records_split: the fields (the text BETWEEN a record's own matches: `awk -F RE`,
// `cut`, str.split) or the matches themselves (`grep -o`, str.findall) of the chosen records as a piece table over the same
// device text, with Arrow-style offsets per row -- in one call and without a download.  record_split.h has the arithmetic;
// two launches on one stream:
//
// Plan: record_frame.h's plan_units -- the pack's plan -- over k + 1 rows with a row's length = its pieces (c + 1 or c), lead 0
// and gap 0: one row per lane, the checks of replace::plan_row, piece_first[j] out of the unit scan.  Row k is the table's
// closing row: it has no pieces, so the scan leaves piece_first[k] = P there.  P and the first bad row with its kind go to the
// summary.  28 bytes per row read (index 8 more), 8 written; a row with matches reads two spans more.
//
// Emit: piece-major, so a workgroup's work does not depend on how the pieces are spread over the rows.  [0, min(P, piece_cap))
// is cut into chunks of kEmitChunk pieces; the grid is persistent and reads P from the summary.  Per chunk two lanes of two
// waves search piece_first for the rows that touch it; their piece_first, begin, end, first and count are staged in LDS when
// they fit (else every lane searches the table in memory), and a lane owns one piece per pass: one search for its row, one
// or two 8-byte reads of the list, two coalesced 8-byte stores.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_pack.h"
#include "record_replace.h"
#include "record_split.h"

namespace rejit_amd {

namespace {

// A chunk of kEmitChunk pieces, a stage of kEmitRows rows (23 KiB of LDS).  kBetween gives every row a piece, so a chunk
// touches at most kEmitChunk rows and always stages them; kMatches leaves the stage when more than kEmitRows - 1 rows without
// a match lie between the pieces of one chunk (a sparse pattern over many lines).
constexpr uint64_t kEmitChunk = 512;
constexpr uint32_t kEmitRows = 640;
static_assert(kEmitChunk < kEmitRows, "a chunk of rows with one piece each fits the stage");

struct DeviceMem {
  const uint64_t* rec_begin_;
  const uint64_t* rec_end_;
  const uint64_t* first_;
  const uint32_t* counts_;
  const uint64_t* indices_;
  const uint64_t* spans_;
  __device__ __forceinline__ uint64_t rec_begin(uint64_t r) const { return rec_begin_[r]; }
  __device__ __forceinline__ uint64_t rec_end(uint64_t r) const { return rec_end_[r]; }
  __device__ __forceinline__ uint64_t first(uint64_t r) const { return first_[r]; }
  __device__ __forceinline__ uint32_t count(uint64_t r) const { return counts_[r]; }
  __device__ __forceinline__ uint64_t index(uint64_t j) const { return indices_[j]; }
  __device__ __forceinline__ uint64_t span_begin(uint64_t g) const { return spans_[2 * g]; }
  __device__ __forceinline__ uint64_t span_end(uint64_t g) const { return spans_[2 * g + 1]; }
  __device__ __forceinline__ uint64_t table(uint64_t) const { return 0; }   // (record_split.h: the split has no table D)
};

__global__ __launch_bounds__(kThreads) void record_split_plan_kernel(DeviceMem M, int what, uint64_t n_records, uint64_t k, uint64_t n, uint64_t m,
                                                                     unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                                     uint64_t* __restrict__ piece_first, unsigned long long* summary) {
  const auto row = [=](uint64_t j) {
    if (j == k) return PlannedRow{0, 0};   // the closing row
    const split::RowPlan p = split::plan_row(M, what, j, M.indices_ != nullptr, n_records, n, m);
    return PlannedRow{p.kind == replace::kOk ? 0 : replace::bad_word(j, p.kind), p.pieces};
  };
  plan_units(row, k + 1, 0, 0, granules, ticket, n_units, piece_first, nullptr, summary);
}

struct EmitStage {
  uint64_t pf[kEmitRows + 1], rb[kEmitRows], re[kEmitRows], first[kEmitRows];
  uint32_t count[kEmitRows];
};

__global__ __launch_bounds__(kThreads) void record_split_emit_kernel(DeviceMem M, int what, uint64_t k, const uint64_t* __restrict__ piece_first,
                                                                     uint64_t chunk, uint32_t stage_cap, uint64_t* __restrict__ piece_begin,
                                                                     uint64_t* __restrict__ piece_end, uint64_t piece_cap,
                                                                     const unsigned long long* summary) {
  __shared__ EmitStage s_stage;
  __shared__ uint64_t s_rows[2];
  if (refused(summary)) return;
  const uint64_t total = summary[kSumTotal];
  const uint64_t limit = total < piece_cap ? total : piece_cap;
  const uint64_t n_chunks = (limit + chunk - 1) / chunk;
  const uint32_t tid = threadIdx.x;
  const bool have_indices = M.indices_ != nullptr;
  const pack::View table{piece_first, nullptr, nullptr, nullptr, 0, k, total};
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
    split::Stage stage{nullptr, nullptr, nullptr, nullptr};
    if (staged) {
      for (uint64_t i = tid; i <= rows.j1 - rows.j0; i += kThreads) {
        s_stage.pf[i] = table.ob_at(rows.j0 + i);
        if (rows.j0 + i < rows.j1) {
          const split::RowInfo x = split::row_info(M, rows.j0 + i, have_indices);
          s_stage.rb[i] = x.rb;
          s_stage.re[i] = x.re;
          s_stage.first[i] = x.f;
          s_stage.count[i] = x.c;
        }
      }
      __syncthreads();
      view = pack::View{s_stage.pf, nullptr, nullptr, nullptr, rows.j0, ~0ull, total};
      stage = split::Stage{s_stage.rb, s_stage.re, s_stage.first, s_stage.count};
    }
    // ---- one piece per lane and pass
    for (uint64_t p = c0 + tid; p < c1; p += kThreads) {
      const split::Piece pc = split::piece(view, stage, M, what, have_indices, rows, p);
      piece_begin[p] = pc.begin;
      piece_end[p] = pc.end;
    }
    __syncthreads();   // (the next chunk rewrites s_rows and the stage)
  }
}

int refuse_row(unsigned long long word) {
  const unsigned long long j = replace::bad_word_row(word);
  switch (replace::bad_word_kind(word)) {
    case replace::kBadIndex:
    case replace::kBadRow:
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: row %llu names no record or a record outside the text (index < n_records, begin <= end <= n)", j);
    case replace::kBadRange:
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: row %llu has first + count beyond the scan's list: d_counts / d_first are not those of the scan's last rj_scan_records", j);
    case replace::kSaturated:
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: row %llu has a saturated count (UINT32_MAX): the range of its matches is unknown", j);
    case replace::kBeginsBefore:
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: row %llu has a first match that begins before its record: d_counts / d_first are not those of this table", j);
    default:
      return rj_fail(RJ_BAD_ARGUMENT,
                     "rj_scan_records_split: row %llu has a match that ends beyond its record: the records are not independent (rj_scan_records_pack "
                     "with rj_batch_separator as fill makes them so)", j);
  }
}

inline unsigned emit_grid(uint64_t piece_cap) {
  const uint64_t cap_chunks = (piece_cap + kEmitChunk - 1) / kEmitChunk;
  return static_cast<unsigned>(cap_chunks < kCopyGrid ? cap_chunks : kCopyGrid);
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_split(rj_scan* s, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records, const uint32_t* d_counts,
                              const uint64_t* d_first, const uint64_t* d_indices, uint64_t n_indices, int what, uint64_t* d_piece_first,
                              uint64_t* d_piece_begin, uint64_t* d_piece_end, uint64_t piece_cap, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_split";
  if (!s || (n_records && (!d_rec_begin || !d_rec_end)) || (piece_cap && (!d_piece_begin || !d_piece_end)))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: null argument");
  if (what != RJ_SPLIT_BETWEEN && what != RJ_SPLIT_MATCHES)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: what %d is neither RJ_SPLIT_BETWEEN nor RJ_SPLIT_MATCHES", what);
  if (!aligned8(d_rec_begin, d_rec_end, d_indices, d_first, d_piece_first, d_piece_begin, d_piece_end) || (reinterpret_cast<uintptr_t>(d_counts) & 3u))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: a table is not 8-byte aligned (d_counts: 4-byte)");
  const uint64_t k = d_indices ? n_indices : n_records;
  if (k && (!d_counts || !d_first)) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: d_counts and d_first (as rj_scan_records wrote them) are needed");
  const uint64_t m = s->result_count;
  const uint64_t* spans = s->result;
  if (m && !spans)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: the last run was counts-only: there is no span list to split by (rj_multi_set_counts_only / rj_scan_count)");
  if (!split::sums_fit(k, m))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_split: %llu rows with %llu matches can exceed 2^62 pieces (or there are 2^60 rows)",
                   static_cast<unsigned long long>(k), static_cast<unsigned long long>(m));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t row_units = (k + 1 + kThreads - 1) / kThreads;   // (k + 1: the closing row)
  uint64_t* piece_first = d_piece_first;
  if (!piece_first) {   // the scan's own, as the pack's begins
    RJ_HIP(s->rec_pack_begin.reserve((k + 1) * sizeof(uint64_t)));
    piece_first = s->rec_pack_begin.as<uint64_t>();
  }
  int rc;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, then the plan's look-back words
  if ((rc = records_begin(s, 1 + lookback::granule_words(row_units), st, &scratch, &summary)) != RJ_OK) return rc;
  const DeviceMem mem{d_rec_begin, d_rec_end, d_first, d_counts, d_indices, spans};
  hipLaunchKernelGGL(record_split_plan_kernel, dim3(unit_grid(row_units)), dim3(kThreads), 0, st, mem, what, n_records, k, n, m, scratch + 1, scratch,
                     row_units, piece_first, summary);
  if (piece_cap)
    hipLaunchKernelGGL(record_split_emit_kernel, dim3(emit_grid(piece_cap)), dim3(kThreads), 0, st, mem, what, k, piece_first, kEmitChunk, kEmitRows,
                       d_piece_begin, d_piece_end, piece_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0) return refuse_row(s->rec_host[kSumBadWord]);
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
