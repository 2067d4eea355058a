// rejit_amd/csrc/record_translate.hip -- rj_scan_records_translate: the rows of a record table through a 256-byte map and a
// 256-bit drop set (Python's bytes.translate(table, delete), `tr A-Z a-z`, `tr -d '\r'`, ascii_lower / ascii_upper) into a NEW
// packed device text with its record table, laid out as rj_scan_records_pack lays records out.  It is the family's first call
// whose output length depends on every source byte: a stream compaction.  record_translate.h has the arithmetic.  The map
// and the drop set are a kernel ARGUMENT (288 bytes): no upload, no allocation for them.  Two memsets (the summary, the
// look-backs' words) and up to three launches on one stream, one synchronise:
//
// Rows:  record_frame.h's plan_units, unchanged, over the source lengths with lead 0 and gap 1: row j's place sb(j) in the
//   virtual stream V (its bytes, then one terminator), S in the summary, the rows checked and the first bad one left there.
// Count: source-major and persistent, units in ticket order; a unit is r consecutive slabs of 4096 positions (r = 1 unless
//   rows overlap or repeat so much that S exceeds the text and its rows: record_translate.h).  A slab finds its rows on sb by
//   the pack's two searches; every lane takes 16 positions (one 16-byte read where they lie in one row), forms its kept mask
//   from the drop set in LDS; the unit's kept bytes go through record_frame.h's unit_place (publish, then look back) and
//   leave kp[unit]; the lane that holds a row's terminator writes the row's end and the next row's begin.  The last unit
//   leaves the total and the stats.  Without a drop set (and without a caller who asks for bytes_changed) the launch is
//   replaced by the layout kernel: len' = len, the tables are arithmetic on sb.
// Emit:  slab by slab again, no unit waits for another: the kept bytes go through the map in LDS into an image of the slab's
//   output range, in turns of 4 KiB.  A turn presets the image to fill; a lane's 16 bytes are in registers, and a lane whose
//   places miss the turn's window leaves at once, so a large gap or many terminators cost turns -- work in proportion to the
//   output -- and no LDS.  The image is stored 16 bytes per lane; the ragged edges of the range, which the neighbouring slab
//   shares a group with, byte by byte.  Slab 0 owns the lead.  Nothing is stored at or beyond out_cap.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_rows.h"
#include "record_translate.h"

namespace rejit_amd {

namespace {

static_assert(translate::kSlab == kThreads * translate::kGroup, "a slab is one pass of the workgroup, 16 positions per lane");
static_assert(translate::kImage == kThreads * sizeof(uint4), "one pass of the workgroup presets or stores the image");

// the summary's words as this call uses them: kSumTotal = S (the rows' plan), kSumSelected = the output's total,
// kSumKept = the bytes kept, kSumCrossing = the kept bytes the map changes
enum { kSumOutTotal = kSumSelected, kSumChanged = kSumCrossing };

__global__ __launch_bounds__(kThreads) void record_translate_rows_kernel(const uint64_t* __restrict__ rec_begin, const uint64_t* __restrict__ rec_end,
                                                                         uint64_t n_records, const uint64_t* __restrict__ indices, uint64_t k, uint64_t n,
                                                                         unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                                         uint64_t* __restrict__ sb, unsigned long long* summary) {
  const auto row = [=](uint64_t j) {
    const rows::Row r = rows::resolve(rec_begin, rec_end, indices, n_records, n, j);
    return r.bad ? PlannedRow{~j, 0} : PlannedRow{0, r.len()};
  };
  plan_units(row, k, 0, 1, granules, ticket, n_units, sb, nullptr, summary);
}

// nothing is dropped: row j keeps its length, ob(j) = lead + sb(j) - j + j * gap
__global__ __launch_bounds__(kThreads) void record_translate_layout_kernel(const uint64_t* __restrict__ sb, uint64_t k, uint64_t lead, uint64_t gap,
                                                                           uint64_t* __restrict__ out_begin, uint64_t* __restrict__ out_end,
                                                                           unsigned long long* summary) {
  if (refused(summary)) return;
  const uint64_t S = summary[kSumTotal];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    summary[kSumKept] = S - k;
    summary[kSumOutTotal] = translate::place(lead, gap, S - k, k);
  }
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; j < k; j += static_cast<uint64_t>(gridDim.x) * kThreads) {
    const uint64_t at = sb[j], next = j + 1 < k ? sb[j + 1] : S;
    if (out_begin) out_begin[j] = translate::place(lead, gap, at - j, j);
    if (out_end) out_end[j] = translate::place(lead, gap, next - 1 - j, j);
  }
}

// the tables in LDS: the map 256 bytes at a 256-byte boundary (64 dwords, one per bank: two lanes on a bank are on one dword),
// the drop set 8 dwords
struct LdsTables {
  alignas(256) uint8_t map[256];
  uint32_t drop[8];
};
__device__ __forceinline__ void tables_to_lds(const translate::Tables& t, LdsTables& l) {
  l.map[threadIdx.x] = t.map[threadIdx.x];
  if (threadIdx.x < 8) l.drop[threadIdx.x] = t.drop[threadIdx.x];
}

// the slab's rows by the pack's two searches, side by side (a barrier in front: the words' last readers are through)
__device__ __forceinline__ void slab_rows(const pack::View& sb, uint64_t k, uint64_t c0, uint64_t c1, uint64_t s_rows[2], uint64_t* j_lo, uint64_t* j_hi) {
  __syncthreads();
  if (threadIdx.x == 0) s_rows[0] = pack::chunk_first_row(sb, k, c0);
  if (threadIdx.x == kWave) s_rows[1] = pack::chunk_end_row(sb, k, 0, c1);
  __syncthreads();
  *j_lo = s_rows[0];
  *j_hi = s_rows[1] > s_rows[0] ? s_rows[1] : s_rows[0];
}

// x per lane -> the sum of the lanes before this one, and the workgroup's total
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t x, uint32_t s_wave[kWaves], uint32_t* total) {
  const int wv = static_cast<int>(threadIdx.x) >> 6;
  const uint32_t inc = wave_inclusive_sum(x);
  __syncthreads();
  if (lane_id() == kWave - 1) s_wave[wv] = inc;
  __syncthreads();
  uint32_t before = inc - x, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    const uint32_t v = s_wave[w];
    all += v;
    if (w < wv) before += v;
  }
  *total = all;
  return before;
}

struct Geometry {
  uint64_t S, slabs, per_unit, units;
};
__device__ __forceinline__ Geometry geometry(const unsigned long long* summary, uint64_t unit_cap) {
  Geometry g;
  g.S = summary[kSumTotal];
  g.slabs = translate::n_slabs(g.S, translate::kSlab);
  g.per_unit = translate::slabs_per_unit(g.slabs, unit_cap);
  g.units = translate::n_units(g.slabs, g.per_unit);
  return g;
}

__global__ __launch_bounds__(kThreads) void record_translate_count_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ rec_begin,
                                                                          const uint64_t* __restrict__ indices, uint64_t k, const uint64_t* __restrict__ sb_table,
                                                                          const translate::Tables tables, uint64_t lead, uint64_t gap, uint64_t unit_cap,
                                                                          unsigned long long* granules, unsigned long long* ticket,
                                                                          unsigned long long* __restrict__ kp, uint64_t* __restrict__ out_begin,
                                                                          uint64_t* __restrict__ out_end, unsigned long long* summary) {
  __shared__ LdsTables s_tables;
  __shared__ UnitPlace s_place;
  __shared__ unsigned long long s_kept[kWaves];
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint64_t s_rows[2];
  if (refused(summary)) return;
  const Geometry G = geometry(summary, unit_cap);
  const uint32_t tid = threadIdx.x;
  if (G.units == 0) {   // no rows: the output is the lead
    if (blockIdx.x == 0 && tid == 0) summary[kSumOutTotal] = lead;
    return;
  }
  tables_to_lds(tables, s_tables);
  const translate::TableView tab{s_tables.map, s_tables.drop};
  const pack::View sb{sb_table, nullptr, rec_begin, indices, 0, k, G.S};
  const DeviceText src{text, n};
  unit_init(s_place);
  for (uint64_t tk; unit_take(s_place, ticket, G.units, &tk);) {
    const uint64_t slab0 = tk * G.per_unit;
    const uint64_t slab1 = slab0 + G.per_unit < G.slabs ? slab0 + G.per_unit : G.slabs;
    // ---- the unit's kept bytes (with one slab per unit the lane's group stays in registers for the tables)
    translate::Group g;
    uint32_t kept = 0;
    uint64_t j_lo = 0, j_hi = 0, lane_kept = 0, lane_changed = 0;
    for (uint64_t c = slab0; c < slab1; c++) {
      const uint64_t c0 = c * translate::kSlab;
      const uint64_t c1 = c0 + translate::kSlab < G.S ? c0 + translate::kSlab : G.S;
      slab_rows(sb, k, c0, c1, s_rows, &j_lo, &j_hi);
      g = translate::load_group(sb, j_lo, j_hi, c0 + static_cast<uint64_t>(tid) * translate::kGroup, G.S, src);
      kept = translate::kept_mask(g, tab);
      lane_kept += translate::popcount16(kept);
      lane_changed += translate::popcount16(translate::changed_mask(g, kept, tab));
    }
    const uint64_t wave_kept = wave_sum64(lane_kept), wave_changed = wave_sum64(lane_changed);
    if (lane_id() == 0) {
      s_kept[tid >> 6] = wave_kept;
      if (wave_changed) atomicAdd(&summary[kSumChanged], static_cast<unsigned long long>(wave_changed));
    }
    __syncthreads();
    unsigned long long unit_kept = 0;
    if (tid < kWave) {
#pragma unroll
      for (int w = 0; w < kWaves; w++) unit_kept += s_kept[w];
    }
    if (!unit_place(s_place, unit_kept, tk, G.units, granules, summary)) continue;   // (timed out: nothing is written, the call fails)
    if (tid == 0) {
      kp[tk] = s_place.before;
      if (tk == G.units - 1) {
        summary[kSumKept] = s_place.end;
        summary[kSumOutTotal] = translate::place(lead, gap, s_place.end, k);
      }
    }
    // ---- the tables: the lane that holds a row's terminator writes the row's end and the next row's begin
    if (!out_begin && !out_end) continue;
    uint64_t running = s_place.before;
    for (uint64_t c = slab0; c < slab1; c++) {
      const uint64_t c0 = c * translate::kSlab;
      if (G.per_unit != 1) {
        const uint64_t c1 = c0 + translate::kSlab < G.S ? c0 + translate::kSlab : G.S;
        slab_rows(sb, k, c0, c1, s_rows, &j_lo, &j_hi);
        g = translate::load_group(sb, j_lo, j_hi, c0 + static_cast<uint64_t>(tid) * translate::kGroup, G.S, src);
        kept = translate::kept_mask(g, tab);
      }
      uint32_t sums;
      const uint32_t before = block_exclusive_sum(translate::lane_sums(g, kept), s_wave, &sums);
      if (c0 == 0 && tid == 0 && out_begin) out_begin[0] = lead;
      translate::row_ends(g, kept, running + translate::sums_kept(before), lead, gap, [=](uint64_t j, uint64_t oe) {
        if (out_end) out_end[j] = oe;
        if (out_begin && j + 1 < k) out_begin[j + 1] = oe + gap;
      });
      running += translate::sums_kept(sums);
    }
  }
}

// (101 VGPRs, four waves per SIMD, no scratch: profiles/translate_kernel_resources.txt)
__global__ __launch_bounds__(kThreads) void record_translate_emit_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ rec_begin,
                                                                         const uint64_t* __restrict__ indices, uint64_t k, const uint64_t* __restrict__ sb_table,
                                                                         const translate::Tables tables, uint64_t lead, uint64_t gap, uint32_t fill,
                                                                         uint64_t unit_cap, const unsigned long long* __restrict__ kp /* null: nothing dropped */,
                                                                         uint8_t* __restrict__ out, uint64_t out_cap, const unsigned long long* summary) {
  __shared__ uint4 s_image[kThreads];
  __shared__ LdsTables s_tables;
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint64_t s_rows[2];
  if (refused(summary)) return;
  const Geometry G = geometry(summary, unit_cap);
  const uint64_t total = summary[kSumOutTotal];
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint32_t tid = threadIdx.x;
  if (G.units == 0) {   // no rows: the lead alone
    if (blockIdx.x == 0)
      for (uint64_t p = tid; p < limit; p += kThreads) out[p] = static_cast<uint8_t>(fill);
    return;
  }
  tables_to_lds(tables, s_tables);
  const translate::TableView tab{s_tables.map, s_tables.drop};
  const pack::View sb{sb_table, nullptr, rec_begin, indices, 0, k, G.S};
  const DeviceText src{text, n};
  uint8_t* image = reinterpret_cast<uint8_t*>(s_image);
  const uint32_t fw = pack::fill_word(fill);
  for (uint64_t u = blockIdx.x; u < G.units; u += gridDim.x) {
    const uint64_t slab0 = u * G.per_unit;
    const uint64_t slab1 = slab0 + G.per_unit < G.slabs ? slab0 + G.per_unit : G.slabs;
    uint64_t running = 0;
    for (uint64_t c = slab0; c < slab1; c++) {
      const uint64_t c0 = c * translate::kSlab;
      const uint64_t c1 = c0 + translate::kSlab < G.S ? c0 + translate::kSlab : G.S;
      uint64_t j_lo, j_hi;
      slab_rows(sb, k, c0, c1, s_rows, &j_lo, &j_hi);
      if (c == slab0) running = kp ? kp[u] : c0 - j_lo;   // (nothing dropped: every position before c0 but the terminators)
      const translate::Group g = translate::load_group(sb, j_lo, j_hi, c0 + static_cast<uint64_t>(tid) * translate::kGroup, G.S, src);
      const uint32_t kept = translate::kept_mask(g, tab);
      uint32_t sums;
      const uint32_t before = block_exclusive_sum(translate::lane_sums(g, kept), s_wave, &sums);
      const uint64_t at = translate::place(lead, gap, running + translate::sums_kept(before), g.j);
      const translate::Range range = translate::slab_range(c0, lead, gap, running, j_lo, sums);
      running += translate::sums_kept(sums);
      const uint64_t stop = range.o1 < limit ? range.o1 : limit;
      // ---- turns: preset, place, store (a lane presets and stores its own 16 bytes: two barriers a turn)
      for (uint64_t w0 = translate::first_window(range); w0 < stop; w0 += translate::kImage) {
        s_image[tid] = make_uint4(fw, fw, fw, fw);
        __syncthreads();
        translate::place_group(g, kept, at, gap, w0, translate::kImage, tab, [=](uint64_t in_image, uint32_t byte) { image[in_image] = static_cast<uint8_t>(byte); });
        __syncthreads();
        const uint64_t p = w0 + static_cast<uint64_t>(tid) * translate::kGroup;
        const translate::Store st = translate::group_store(p, range, limit);
        if (st.hi - st.lo == translate::kGroup) {
          *reinterpret_cast<uint4*>(out + p) = s_image[tid];
        } else {
          for (uint32_t b = st.lo; b < st.hi; b++) out[p + b] = image[tid * translate::kGroup + b];
        }
      }
    }
  }
}

inline unsigned slab_grid(uint64_t unit_cap) { return static_cast<unsigned>(unit_cap < kCopyGrid ? unit_cap : kCopyGrid); }

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_translate(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                                  const uint64_t* d_indices, uint64_t n_indices, const uint8_t* map, const uint8_t* drop, int fill, uint64_t lead,
                                  uint64_t gap, void* d_out, uint64_t out_cap, uint64_t* d_out_begin, uint64_t* d_out_end, rj_translate_stats* stats,
                                  void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_translate";
  const uint64_t k = d_indices ? n_indices : n_records;
  int rc;
  switch (translate::check_call(s, d_text, n, d_rec_begin, d_rec_end, n_records, d_indices, n_indices, fill, lead, gap, d_out, out_cap, d_out_begin, d_out_end)) {
    case translate::kFine: break;
    case translate::kNull: return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", kCall);
    case translate::kFill: return rj_fail(RJ_BAD_ARGUMENT, "%s: fill %d is not a byte (0..255)", kCall, fill);
    case translate::kOutAlign: return rj_fail(RJ_BAD_ARGUMENT, "%s: d_out is not 16-byte aligned", kCall);
    case translate::kTableAlign: return rj_fail(RJ_BAD_ARGUMENT, "%s: a table is not 8-byte aligned", kCall);
    case translate::kSums:
      return rj_fail(RJ_BAD_ARGUMENT, "%s: %llu rows of a text of %llu bytes can exceed 2^62 output bytes (or n + gap reaches 2^42)", kCall,
                     static_cast<unsigned long long>(k), static_cast<unsigned long long>(n));
  }
  translate::Tables tables;
  bool identity, drops;
  translate::make_tables(map, drop, &tables, &identity, &drops);
  const bool counts = drops || (stats && !identity);   // else len' = len, and bytes_changed is 0 or not asked for
  const bool copies = out_cap != 0;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_row_units = (k + kThreads - 1) / kThreads;
  const uint64_t unit_cap = translate::unit_cap(n, k, translate::kSlab);
  // the scan's scratch: sb (8 bytes per row), then kp (8 bytes per unit); two tickets and two look-backs' words
  const uint64_t sb_bytes = rows::align16(k * sizeof(uint64_t));
  RJ_HIP(s->rec_translate_stage.reserve(sb_bytes + unit_cap * sizeof(unsigned long long) + 16));
  uint64_t* sb = s->rec_translate_stage.as<uint64_t>();
  unsigned long long* kp = reinterpret_cast<unsigned long long*>(s->rec_translate_stage.as<uint8_t>() + sb_bytes);
  const uint64_t row_words = 1 + lookback::granule_words(n_row_units);
  unsigned long long *scratch = nullptr, *summary = nullptr;
  if ((rc = records_begin(s, row_words + 1 + lookback::granule_words(unit_cap), st, &scratch, &summary)) != RJ_OK) return rc;
  const dim3 block(kThreads);
  const uint8_t* text = static_cast<const uint8_t*>(d_text);
  hipLaunchKernelGGL(record_translate_rows_kernel, dim3(unit_grid(n_row_units)), block, 0, st, d_rec_begin, d_rec_end, n_records, d_indices, k, n, scratch + 1,
                     scratch, n_row_units, sb, summary);
  if (counts)
    hipLaunchKernelGGL(record_translate_count_kernel, dim3(slab_grid(unit_cap)), block, 0, st, text, n, d_rec_begin, d_indices, k,
                       static_cast<const uint64_t*>(sb), tables, lead, gap, unit_cap, scratch + row_words + 1, scratch + row_words, kp, d_out_begin, d_out_end,
                       summary);
  else
    hipLaunchKernelGGL(record_translate_layout_kernel, dim3(unit_grid(n_row_units)), block, 0, st, static_cast<const uint64_t*>(sb), k, lead, gap, d_out_begin,
                       d_out_end, summary);
  if (copies)
    hipLaunchKernelGGL(record_translate_emit_kernel, dim3(slab_grid(unit_cap)), block, 0, st, text, n, d_rec_begin, d_indices, k,
                       static_cast<const uint64_t*>(sb), tables, lead, gap, static_cast<uint32_t>(fill), unit_cap,
                       counts ? static_cast<const unsigned long long*>(kp) : nullptr, static_cast<uint8_t*>(d_out), out_cap, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0)
    return rj_fail(RJ_BAD_ARGUMENT, "%s: row %llu of the call names no record or a record outside the text (index < n_records, begin <= end <= n)", kCall,
                   static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
  if (stats) {
    stats->bytes_in = s->rec_host[kSumTotal] - k;
    stats->bytes_dropped = stats->bytes_in - s->rec_host[kSumKept];
    stats->bytes_changed = counts ? s->rec_host[kSumChanged] : 0;
  }
  return static_cast<int64_t>(s->rec_host[kSumOutTotal]);
}

}  // extern "C"
