// rejit_amd/csrc/record_pack.hip -- rj_scan_records_pack: a list of records of one device text -- every record, or the rows
// rj_scan_records_select listed, or any permutation / take -- gathered into a NEW contiguous device text, `gap` fill bytes
// behind each record and `lead` in front, with the new record table.  It is what a grep-like caller prints (the selected
// lines, fill = '\n') and what makes the strings of an Arrow-layout column independent of each other (fill = the program's
// rj_batch_separator) without a trip to the host.  record_pack.h has the arithmetic; two launches:
//
// Plan: record-major, one row per lane, a unit = 256 rows.  A lane's length + gap, then record_frame.h's plan_units: a
// 64-bit wave scan and the unit's place from the decoupled look-back of tile_lookback.h (tickets in arrival order; a unit
// publishes BEFORE it looks back).  It writes ob / oe, checks its rows, leaves the total and the first bad row in the
// summary.  16 bytes per row read (+ 8 with indices), 8 to 16 written.
//
// Copy: record_frame.h's copy_chunks, output-major, in chunks of 16 KiB (one synchronise per call).  A chunk stages the ob
// and source begins of its rows, and every lane produces 16 aligned output bytes at a time: one search for its piece, then
// -- the common case, 16 bytes inside one record -- two aligned 16-byte loads around the source, a byte funnel shift, one
// 16-byte store.  Text in, output out, once each.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_pack.h"

namespace rejit_amd {

namespace {

__global__ __launch_bounds__(kThreads) void record_pack_plan_kernel(const uint64_t* __restrict__ rec_begin, const uint64_t* __restrict__ rec_end,
                                                                    uint64_t n_records, const uint64_t* __restrict__ indices, uint64_t k, uint64_t n,
                                                                    uint64_t lead, uint64_t gap, unsigned long long* granules, unsigned long long* ticket,
                                                                    uint64_t n_units, uint64_t* __restrict__ out_begin, uint64_t* __restrict__ out_end,
                                                                    unsigned long long* summary) {
  const auto row = [=](uint64_t j) {
    const uint64_t r = indices ? indices[j] : j;
    if (pack::bad_index(r, n_records)) return PlannedRow{~j, 0};
    const uint64_t rb = rec_begin[r], re = rec_end[r];
    if (pack::bad_row(rb, re, n)) return PlannedRow{~j, 0};
    return PlannedRow{0, re - rb};
  };
  plan_units(row, k, lead, gap, granules, ticket, n_units, out_begin, out_end, summary);
}

// what a chunk of the copy stages: 2 x 8 KiB of LDS, eight workgroups per CU
struct PackCopy {
  static constexpr uint32_t kRows = 1024;
  struct Stage {
    uint64_t ob[kRows + 1], src[kRows];
  };
  const uint64_t* rec_begin;
  const uint64_t* indices;
  __device__ __forceinline__ pack::View table(const uint64_t* ob, uint64_t k, uint64_t total) const {
    return pack::View{ob, nullptr, rec_begin, indices, 0, k, total};
  }
  __device__ __forceinline__ void stage_row(Stage& s, uint64_t i, const pack::View& table, uint64_t j) const { s.src[i] = table.src_at(j); }
  struct Extras {};   // (ob and src are all a row has, and the view holds them)
  __device__ __forceinline__ Extras staged(const Stage&) const { return Extras{}; }
  __device__ __forceinline__ Extras unstaged() const { return Extras{}; }
  __device__ __forceinline__ void group16(const pack::View& view, const Extras&, const pack::Rows& rows, uint64_t p, uint64_t limit, uint64_t gap,
                                          uint32_t fill, const DeviceText& src, uint32_t w[4]) const {
    pack::group16(view, rows, p, limit, gap, fill, src, w);
  }
};

__global__ __launch_bounds__(kThreads) void record_pack_copy_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ rec_begin,
                                                                    const uint64_t* __restrict__ indices, uint64_t k, const uint64_t* __restrict__ ob,
                                                                    uint64_t gap, uint32_t fill, uint64_t chunk, uint32_t stage_cap,
                                                                    uint8_t* __restrict__ out, uint64_t out_cap, const unsigned long long* summary) {
  copy_chunks(PackCopy{rec_begin, indices}, text, n, k, ob, gap, fill, chunk, stage_cap, out, out_cap, summary);
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_pack(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                             const uint64_t* d_indices, uint64_t n_indices, int fill, uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap,
                             uint64_t* d_out_begin, uint64_t* d_out_end, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_pack";
  int rc = check_pack_call(kCall, s, d_text, n, d_rec_begin, d_rec_end, n_records, d_out, out_cap, fill);
  if (rc != RJ_OK) return rc;
  if (!aligned8(d_rec_begin, d_rec_end, d_indices, d_out_begin, d_out_end)) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: a table is not 8-byte aligned");
  const uint64_t k = d_indices ? n_indices : n_records;
  if (!pack::sums_fit(k, n, lead, gap))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: %llu rows of a text of %llu bytes can exceed 2^62 output bytes (or n + gap reaches 2^42)",
                   static_cast<unsigned long long>(k), static_cast<unsigned long long>(n));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  const bool copies = out_cap != 0;
  uint64_t* ob = nullptr;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, then the look-back's words
  if ((rc = pack_begin_table(s, d_out_begin, copies, k, &ob)) != RJ_OK) return rc;
  if ((rc = records_begin(s, 1 + lookback::granule_words(n_units), st, &scratch, &summary)) != RJ_OK) return rc;
  hipLaunchKernelGGL(record_pack_plan_kernel, dim3(unit_grid(n_units)), dim3(kThreads), 0, st, d_rec_begin, d_rec_end, n_records, d_indices, k, n, lead,
                     gap, scratch + 1, scratch, n_units, ob, d_out_end, summary);
  if (copies)
    hipLaunchKernelGGL(record_pack_copy_kernel, dim3(copy_grid(out_cap)), dim3(kThreads), 0, st, static_cast<const uint8_t*>(d_text), n, d_rec_begin,
                       d_indices, k, ob, gap, static_cast<uint32_t>(fill), kCopyChunk, PackCopy::kRows, static_cast<uint8_t*>(d_out), out_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_pack: row %llu of the pack names no record or a record outside the text (index < n_records, begin <= end <= n)",
                   static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
