// rejit_amd/csrc/record_zip.hip -- rj_scan_records_zip: the rows of up to 16 record tables -- each over a device text of its
// own, or several over one -- put side by side into the lines of a NEW contiguous device text with its record table, laid out
// as rj_scan_records_pack lays records out: Arrow's binary_join_element_wise, `paste -d`, `awk '{print $3, $1}'`, the
// "%7d %s %s\n" of `sort | uniq -c`, without a download.  record_zip.h has the rule and the arithmetic.  The columns and the
// separator are kernel ARGUMENTS (16 x 64 + 64 bytes): no upload, no allocation for them.  Two memsets (the summary, the
// look-back's words) and three launches on one stream, one synchronise:
//
// Resolve: one lane per output row.  The lane resolves its C rows with record_rows.h's resolver, stages (source begin,
//   length) per piece -- 16 C bytes per row of scan scratch, so that the emit does not walk index -> begin -> end again for
//   every chunk a row touches -- and the row's length, and leaves the first bad (row, column) in the summary: one atomic max
//   per wave.  It writes no table row: a refused call leaves ob / oe as they were, which a plan that writes its rows unit by
//   unit cannot promise -- so the check stands in front of the plan, as in record_format.hip.
// Plan: record_frame.h's plan_staged_lengths -- plan_units over the staged lengths, one lane per row, a unit = 256 rows, the decoupled look-back;
//   ob / oe and the total.  Returns at once behind a bad row.
// Emit: record_frame.h's emit_chunks, the frame of the format's emit -- output-major and persistent, a sibling of copy_chunks: chunks of 4 KiB (one pass of 256
//   lanes x 16 bytes), the total from the summary, a chunk's rows from the pair of searches over ob.  Two tiers inside it, by a
//   segment's length (zip::kStreamBytes = 32):
//     bytes   every row of the chunk once, by its own lane: the separators, the short pieces and paddings, and the partial
//             groups at the two ends of the long ones, as byte writes into the chunk's image in LDS (zip::row_edges)
//     stream  only in a chunk that a long segment touches: every lane looks up the row around its OWN 16 output bytes and,
//             where one long piece (or padding) covers them whole, takes 16 source bytes through DeviceText's streaming read
//             (zip::group_streamed) -- registers, not LDS
//   and every lane stores its 16 aligned bytes: the streamed ones, else the image's.  No byte stores to memory but the last
//   group's below the total, no atomics, no loop over a long piece's length.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_rows.h"
#include "record_zip.h"

namespace rejit_amd {

namespace {

static_assert(zip::kEmitChunk == kImageChunk, "the header's chunk is the frame's");

__global__ __launch_bounds__(kThreads) void record_zip_resolve_kernel(const zip::Columns cols, uint32_t n_cols, uint64_t sep_len, uint64_t k, uint64_t n_units,
                                                                      ulonglong2* __restrict__ stage, uint64_t* __restrict__ row_len,
                                                                      unsigned long long* summary) {
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    bool bad = false;
    uint32_t bad_col = 0;
    uint64_t len = 0;
    if (j < k) {
      for (uint32_t c = 0; c < n_cols; c++) {
        const zip::Column& col = cols.col[c];
        const rows::Row row = rows::resolve(col.rec_begin, col.rec_end, col.indices, col.n_records, col.n, j);
        if (row.bad) {
          bad = true, bad_col = c;
          break;
        }
        if (stage) stage[j * n_cols + c] = make_ulonglong2(row.rb, row.len());
        len += zip::field_length(c, row.len(), col.width, sep_len);
      }
      row_len[j] = len;
    }
    note_bad_word(bad, zip::bad_word(j, bad_col), &summary[kSumBadWord]);
  }
}

__global__ __launch_bounds__(kThreads) void record_zip_plan_kernel(const uint64_t* __restrict__ row_len, uint64_t k, uint64_t lead, uint64_t gap,
                                                                   unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                                   uint64_t* __restrict__ out_begin, uint64_t* __restrict__ out_end,
                                                                   unsigned long long* summary) {
  plan_staged_lengths(row_len, k, lead, gap, granules, ticket, n_units, out_begin, out_end, summary);
}

// record_zip.h's Source over the kernel's arguments and the stage
struct DeviceSource {
  const zip::Columns& cols;
  const zip::Sep& sep;
  const ulonglong2* __restrict__ stage;
  uint32_t n_cols;
  __device__ __forceinline__ zip::Piece piece(uint64_t j, uint32_t c) const {
    const ulonglong2 v = stage[j * n_cols + c];
    return zip::Piece{v.x, v.y};
  }
  __device__ __forceinline__ int32_t width(uint32_t c) const { return cols.col[c].width; }
  __device__ __forceinline__ uint32_t sep_byte(uint32_t i) const { return sep.byte[i]; }
  __device__ __forceinline__ uint32_t text_byte(uint32_t c, uint64_t s) const { return cols.col[c].text[s]; }
  __device__ __forceinline__ void load16(uint32_t c, uint64_t s, uint32_t w[4]) const { DeviceText{cols.col[c].text, cols.col[c].n}.load16(s, w); }
};

// The emit: record_frame.h's emit_chunks with a stream tier -- the rows' edges into the image, the long segments from registers
struct ZipEmit : StreamingImagePolicy {
  const DeviceSource& src;
  const uint64_t* __restrict__ ob;
  uint32_t n_cols;
  uint64_t sep_len;
  uint32_t pad;
  __device__ __forceinline__ bool row(uint64_t j, uint64_t c0, uint64_t c1, const ImagePut& put) const {
    const uint64_t at = ob[j];
    if (at >= c1) return false;
    return zip::row_edges(src, n_cols, sep_len, pad, j, at, c0, c1, put);
  }
  __device__ __forceinline__ bool group16(uint64_t j, uint64_t at, uint64_t p, uint32_t w[4]) const {
    return zip::group_streamed(src, n_cols, sep_len, pad, j, at, p, w);
  }
};
// (73 VGPRs, six waves per SIMD: held to 64 for eight, the compiler spills 10 of them to scratch memory -- not worth two waves)
__global__ __launch_bounds__(kThreads) void record_zip_emit_kernel(
    const zip::Columns cols, const zip::Sep sep, uint32_t n_cols, uint64_t sep_len, uint32_t pad, const ulonglong2* __restrict__ stage, uint64_t k,
    const uint64_t* __restrict__ ob, uint32_t fill, uint8_t* __restrict__ out, uint64_t out_cap, const unsigned long long* summary) {
  __shared__ uint32_t s_streams;
  const DeviceSource src{cols, sep, stage, n_cols};
  emit_chunks(ZipEmit{StreamingImagePolicy(s_streams), src, ob, n_cols, sep_len, pad}, k, ob, fill, out, out_cap, summary);
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_zip(rj_scan* s, const rj_zip_column* columns, int n_cols, const char* sep, uint64_t sep_len, int pad, unsigned flags, int fill,
                            uint64_t lead, uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin, uint64_t* d_out_end, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_zip";
  static_assert(sizeof(rj_zip_column) == sizeof(zip::Column), "record_zip.h's Column is rj_zip_column");
  if (!s) return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", kCall);
  const zip::Column* given = reinterpret_cast<const zip::Column*>(columns);
  const zip::Refusal why = zip::check_call(given, n_cols, sep, sep_len, pad, flags, fill, lead, gap, d_out, out_cap, d_out_begin, d_out_end);
  const uint64_t k = given && n_cols >= 1 ? zip::rows_of(given[0]) : 0;
  if (why.code != zip::kFine) {
    char msg[320];
    zip::refusal_message(msg, sizeof(msg), kCall, why, k);
    return rj_fail(why.code == zip::kTooManyRows ? RJ_TOO_LARGE : RJ_BAD_ARGUMENT, "%s", msg);
  }
  zip::Columns cols = {};
  zip::Sep sep_bytes = {};
  for (int c = 0; c < n_cols; c++) cols.col[c] = given[c];
  for (uint64_t i = 0; i < sep_len; i++) sep_bytes.byte[i] = static_cast<uint8_t>(sep[i]);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  const bool copies = out_cap != 0;
  const uint32_t C = static_cast<uint32_t>(n_cols);
  int rc;
  uint64_t *ob = nullptr, *row_len = nullptr;
  ulonglong2* stage = nullptr;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, then the look-back's words
  if ((rc = pack_begin_table(s, d_out_begin, copies, k, &ob)) != RJ_OK) return rc;
  if (k) {   // the rows' lengths, then (a call that copies) the pieces
    const uint64_t len_bytes = rows::align16(k * sizeof(uint64_t));
    RJ_HIP(s->rec_zip_stage.reserve(len_bytes + (copies ? k * C * sizeof(ulonglong2) : 0)));
    row_len = s->rec_zip_stage.as<uint64_t>();
    if (copies) stage = reinterpret_cast<ulonglong2*>(s->rec_zip_stage.as<uint8_t>() + len_bytes);
  }
  if ((rc = records_begin(s, 1 + lookback::granule_words(n_units), st, &scratch, &summary)) != RJ_OK) return rc;
  const dim3 block(kThreads), units(unit_grid(n_units));
  if (k) hipLaunchKernelGGL(record_zip_resolve_kernel, units, block, 0, st, cols, C, sep_len, k, n_units, stage, row_len, summary);
  hipLaunchKernelGGL(record_zip_plan_kernel, units, block, 0, st, static_cast<const uint64_t*>(row_len), k, lead, gap, scratch + 1, scratch, n_units, ob,
                     d_out_end, summary);
  if (copies)
    hipLaunchKernelGGL(record_zip_emit_kernel, dim3(image_grid(out_cap)), block, 0, st, cols, sep_bytes, C, sep_len, static_cast<uint32_t>(pad),
                       static_cast<const ulonglong2*>(stage), k, static_cast<const uint64_t*>(ob), static_cast<uint32_t>(fill), static_cast<uint8_t*>(d_out),
                       out_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0) {
    char msg[320];
    zip::bad_row_message(msg, sizeof(msg), kCall, s->rec_host[kSumBadWord]);
    return rj_fail(RJ_BAD_ARGUMENT, "%s", msg);
  }
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
