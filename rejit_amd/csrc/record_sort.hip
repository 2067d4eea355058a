// rejit_amd/csrc/record_sort.hip -- rj_scan_records_sort: the rows of a record table over a device text -- lines, the pieces
// of rj_scan_records_split, the representatives of rj_scan_records_group; every row, or the rows an index list names -- put
// in the order of their bytes: d_order, THE stable permutation (`LC_ALL=C sort -s`), exactly and without a download.
// record_sort.h has the arithmetic: a most-significant-first refinement over 7-byte windows with a common-prefix skip.  A round
// is these launches on one stream and ONE synchronise, which brings back the numbers of open rows and open segments:
//
// Init (first round only): the pack's checks (rows::resolve; the first bad row wins, note_bad_row); perm = the identity, one
//   open segment.
// Compact: record_frame.h's unit scan over the positions' flags -> the dense list of open (position, segment, row).
// Skip (lane), from the second round on: one listed row per lane against its segment's first row, at most L bytes; one
//   atomic min into the segment's depth where the lane knows less than the word says; rows that agreed on all L bytes and
//   have more are appended to a list (wave_append).
// Skip (wave): one wave per such row, 64 lanes x 16 bytes = 1 KiB per iteration, a ballot ends it at the first difference.
// Key: one listed row per lane, key(row, depth of its segment) beside the row.
// Order: rocPRIM's radix sort, stable: by key, then -- when there is more than one segment -- by the bits of the segment number.
// Cut: one sorted entry per lane: the new flags of its position; a position that closes gets its d_order row, ONCE.
// Every kernel behind the first returns at once when the summary holds a bad row: a refused call writes no output row.
// The rows, the text, the refusal, the two wave idioms and the knobs' parser are record_frame.h's.
#include <hip/hip_runtime.h>

#include <cstring>  // must precede rocprim (its texture iterator uses ::memset)

#include <rocprim/rocprim.hpp>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_rows.h"
#include "record_sort.h"

namespace rejit_amd {

namespace {

// the words of the call's summary a round leaves: open rows and open segments behind its cut, the rows its wave tier took
enum { kSortOpenRows = kSumKept, kSortOpenSegments = kSumMatching, kSortLongRows = kSumCrossing };

// the scratch of a call (sort::layout)
struct Scratch {
  uint8_t* flags;
  uint32_t* perm;
  uint64_t* pos_depth;
  uint32_t* act_pos;
  uint64_t* key;                 // the list as the compaction and the key pass leave it ...
  uint64_t* seg_row;
  uint32_t* long_list;
  uint64_t* seg_depth;
  unsigned long long* seg_cur;
  uint32_t* seg_head;
};
// ... and as the radix passes leave it
struct SortedList {
  const uint64_t* __restrict__ keys;
  const uint64_t* __restrict__ seg_rows;
  __device__ __forceinline__ uint32_t seg(uint64_t i) const { return sort::seg_of(seg_rows[i]); }
  __device__ __forceinline__ uint64_t key(uint64_t i) const { return keys[i]; }
};

// ---------------------------------------------------------------------------------------------------------------- init
__global__ __launch_bounds__(kThreads) void record_sort_init_kernel(uint64_t n, Rows R, uint64_t n_records, uint64_t k, uint64_t n_units, Scratch S,
                                                                    uint64_t* __restrict__ order, unsigned long long* summary) {
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    bool bad = false;
    if (j < k) {
      bad = rows::resolve(R.rec_begin, R.rec_end, R.indices, n_records, n, j).bad;
      S.perm[j] = static_cast<uint32_t>(j);
      S.flags[j] = k < 2 ? 0 : static_cast<uint8_t>(sort::kOpen | (j == 0 ? sort::kHead : 0));
      if (j == 0) S.pos_depth[0] = 0;
      if (k == 1 && !bad) order[0] = 0;   // (one row: nothing to compare)
    }
    note_bad_row(bad, j, &summary[kSumBadWord]);
  }
}

// ---------------------------------------------------------------------------------------------------------------- compact
__global__ __launch_bounds__(kThreads) void record_sort_compact_kernel(uint64_t k, uint64_t n_units, bool skip, Scratch S, unsigned long long* granules,
                                                                       unsigned long long* ticket, unsigned long long* summary) {
  __shared__ UnitSum s_unit;
  // Only the bad word, not refused(): kSumTimedOut is written by this kernel's own unit scan and by nothing before it in the
  // call, so it can be set here only by another workgroup of this launch -- and a workgroup that starts behind a time-out
  // still takes its units and publishes them (nobody waits on words it left out); the call fails at its end either way.
  if (summary[kSumBadWord] != 0) return;
  unit_init(s_unit.place);
  for (uint64_t tk; unit_take(s_unit.place, ticket, n_units, &tk);) {
    const uint64_t p = tk * kThreads + threadIdx.x;
    const uint8_t flags = p < k ? S.flags[p] : 0;
    uint64_t before, unit_end;
    const bool ok = unit_exclusive_sum(s_unit, sort::place_add(flags), tk, n_units, granules, summary, &before, &unit_end);
    if (ok && (flags & sort::kOpen)) {
      const sort::Place at = sort::place(before, flags);
      S.act_pos[at.at] = static_cast<uint32_t>(p);
      S.seg_row[at.at] = sort::seg_row(at.seg, S.perm[p]);
      if (flags & sort::kHead) {
        const uint64_t depth = S.pos_depth[p];
        S.seg_depth[at.seg] = depth;
        S.seg_cur[at.seg] = skip ? sort::kNoDepth : depth;   // (the skip's atomic min starts from "nothing known")
        S.seg_head[at.seg] = at.at;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- skip
struct RowPair {
  uint64_t hb, hl, rb, rl, D;
  uint32_t seg;
};
__device__ __forceinline__ RowPair row_pair(const Rows& R, const Scratch& S, uint64_t a) {
  const uint64_t sr = S.seg_row[a];
  RowPair q;
  q.seg = sort::seg_of(sr);
  const uint64_t r = R.record(sort::row_of(sr));
  const uint64_t h = R.record(sort::row_of(S.seg_row[S.seg_head[q.seg]]));
  q.rb = R.rec_begin[r], q.rl = R.rec_end[r] - q.rb;
  q.hb = R.rec_begin[h], q.hl = R.rec_end[h] - q.hb;
  q.D = S.seg_depth[q.seg];
  return q;
}
// seg_cur[s] <- min(seg_cur[s], depth); the read first: most rows of a segment know no less than the word already says
__device__ __forceinline__ void depth_min(unsigned long long* word, uint64_t depth) {
  if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > depth) atomicMin(word, static_cast<unsigned long long>(depth));
}

__global__ __launch_bounds__(kThreads) void record_sort_skip_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint64_t n_active, uint64_t n_units,
                                                                    uint32_t long_bytes, Scratch S, unsigned long long* summary) {
  if (refused(summary)) return;
  const DeviceText src{text, n};
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t a = unit * kThreads + threadIdx.x;
    bool more = false;
    if (a < n_active) {
      const RowPair q = row_pair(R, S, a);
      const uint64_t depth = sort::skip_row(src, n, q.hb, q.hl, q.rb, q.rl, q.D, long_bytes, &more);
      if (!more) depth_min(&S.seg_cur[q.seg], depth);   // (a listed row's word comes from its wave: the segment's depth stays exact)
    }
    wave_append(more, static_cast<uint32_t>(a), &summary[kSortLongRows], S.long_list);
  }
}

__global__ __launch_bounds__(kThreads) void record_sort_skip_long_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint32_t long_bytes, Scratch S,
                                                                         const unsigned long long* summary) {
  if (refused(summary)) return;
  const DeviceText src{text, n};
  const uint64_t n_long = summary[kSortLongRows];
  const int lane = lane_id();
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); i < n_long; i += waves) {
    const RowPair q = row_pair(R, S, S.long_list[i]);
    const uint64_t both = q.hl < q.rl ? q.hl : q.rl;
    uint64_t depth = both;
    for (uint64_t d0 = q.D + long_bytes; d0 < both; d0 += kWave * sort::kGroupBytes) {
      const uint64_t at = sort::wave_group(src, n, q.hb, q.rb, both, d0, static_cast<uint64_t>(lane));
      const uint64_t differ = __ballot(at != sort::kNoDepth);
      if (differ) {   // the lanes' groups ascend with the lanes: the lowest of these lanes has the first difference
        depth = lane_value(at, __builtin_ctzll(differ));
        break;
      }
    }
    if (lane == 0) depth_min(&S.seg_cur[q.seg], depth);
  }
}

// ---------------------------------------------------------------------------------------------------------------- key
__global__ __launch_bounds__(kThreads) void record_sort_key_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint64_t n_active, uint64_t n_units,
                                                                   Scratch S, const unsigned long long* summary) {
  if (refused(summary)) return;
  const DeviceText src{text, n};
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t a = unit * kThreads + threadIdx.x;
    if (a >= n_active) continue;
    const uint64_t sr = S.seg_row[a];
    const uint64_t r = R.record(sort::row_of(sr));
    const uint64_t rb = R.rec_begin[r];
    S.key[a] = sort::key(src, n, rb, R.rec_end[r] - rb, S.seg_cur[sort::seg_of(sr)]);
  }
}

// ---------------------------------------------------------------------------------------------------------------- cut
// record_sort.h's Mem: plain stores, every position has one lane
struct CutMem {
  Scratch S;
  uint64_t* __restrict__ order;
  __device__ __forceinline__ void set_flags(uint64_t p, uint8_t f) const { S.flags[p] = f; }
  __device__ __forceinline__ void set_perm(uint64_t p, uint32_t row) const { S.perm[p] = row; }
  __device__ __forceinline__ void set_depth(uint64_t p, uint64_t d) const { S.pos_depth[p] = d; }
  __device__ __forceinline__ void set_order(uint64_t p, uint32_t row) const { order[p] = row; }
};

__global__ __launch_bounds__(kThreads) void record_sort_cut_kernel(uint64_t n_active, uint64_t n_units, SortedList list, Scratch S,
                                                                   uint64_t* __restrict__ order, unsigned long long* summary) {
  if (refused(summary)) return;
  const CutMem M{S, order};
  uint32_t open_rows = 0, open_heads = 0;   // of this wave, over all its units: two atomics per wave and launch, not per unit
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t a = unit * kThreads + threadIdx.x;
    uint8_t flags = 0;
    if (a < n_active) {
      flags = sort::cut(list, a, n_active);
      const uint64_t sr = list.seg_rows[a];
      sort::settle(M, S.act_pos[a], flags, sort::row_of(sr), S.seg_cur[sort::seg_of(sr)]);
    }
    open_rows += __popcll(__ballot((flags & sort::kOpen) != 0));
    open_heads += __popcll(__ballot((flags & sort::kOpen) && (flags & sort::kHead)));
  }
  if (open_rows && lane_id() == 0) {
    atomicAdd(&summary[kSortOpenRows], static_cast<unsigned long long>(open_rows));
    atomicAdd(&summary[kSortOpenSegments], static_cast<unsigned long long>(open_heads));
  }
}

// the stable sort of the list's n_active entries by (segment, key): key_a / segrow_a -> *keys / *seg_rows
int order_list(rj_scan* s, const sort::Layout& lay, uint8_t* base, uint64_t n_active, uint64_t n_segments, hipStream_t st, const uint64_t** keys,
               const uint64_t** seg_rows) {
  uint64_t *key_a = reinterpret_cast<uint64_t*>(base + lay.key_a), *key_b = reinterpret_cast<uint64_t*>(base + lay.key_b);
  uint64_t *sr_a = reinterpret_cast<uint64_t*>(base + lay.segrow_a), *sr_b = reinterpret_cast<uint64_t*>(base + lay.segrow_b);
  const unsigned bits = sort::seg_bits(n_segments);
  size_t by_key = 0, by_seg = 0;
  RJ_HIP(rocprim::radix_sort_pairs(nullptr, by_key, key_a, key_b, sr_a, sr_b, n_active, 0, 64, st));
  if (bits) RJ_HIP(rocprim::radix_sort_pairs(nullptr, by_seg, sr_b, sr_a, key_b, key_a, n_active, 32, 32 + bits, st));
  RJ_HIP(s->sort_tmp.reserve(std::max<size_t>(std::max(by_key, by_seg), 16)));
  RJ_HIP(rocprim::radix_sort_pairs(s->sort_tmp.p, by_key, key_a, key_b, sr_a, sr_b, n_active, 0, 64, st));
  *keys = key_b, *seg_rows = sr_b;
  if (bits) {
    RJ_HIP(rocprim::radix_sort_pairs(s->sort_tmp.p, by_seg, sr_b, sr_a, key_b, key_a, n_active, 32, 32 + bits, st));
    *keys = key_a, *seg_rows = sr_a;
  }
  return RJ_OK;
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_sort(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                             const uint64_t* d_indices, uint64_t n_indices, uint64_t* d_order, rj_sort_stats* stats, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_sort";
  if (stats) *stats = rj_sort_stats{0, 0, 0, 0};
  const uint64_t k = d_indices ? n_indices : n_records;
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) || (k && !d_order))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_sort: null argument");
  if (!aligned8(d_rec_begin, d_rec_end, d_indices, d_order)) return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_sort: a table is not 8-byte aligned");
  if (!rows::rows_fit(k))
    return rj_fail(RJ_TOO_LARGE, "rj_scan_records_sort: %llu rows: rows and segments share 32-bit words in the scratch (fewer than 2^31 rows)",
                   static_cast<unsigned long long>(k));
  if (k == 0) return 0;
  // the test knobs, read at every call: RJ_SORT_LONG_BYTES, RJ_SORT_SKIP=0
  const uint32_t long_bytes = env_number("RJ_SORT_LONG_BYTES", sort::kLongBytes, rows::kMaxLongBytes);
  const bool skip = env_number("RJ_SORT_SKIP", 1, 1) != 0;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  const uint64_t scratch_words = 1 + lookback::granule_words(n_units);   // the ticket, the look-back's words
  const sort::Layout lay = sort::layout(k);
  RJ_HIP(s->rec_repl_table.reserve(lay.bytes));
  uint8_t* base = s->rec_repl_table.as<uint8_t>();
  Scratch S;
  S.flags = base + lay.flags;
  S.perm = reinterpret_cast<uint32_t*>(base + lay.perm);
  S.pos_depth = reinterpret_cast<uint64_t*>(base + lay.pos_depth);
  S.act_pos = reinterpret_cast<uint32_t*>(base + lay.act_pos);
  S.key = reinterpret_cast<uint64_t*>(base + lay.key_a);
  S.seg_row = reinterpret_cast<uint64_t*>(base + lay.segrow_a);
  S.long_list = reinterpret_cast<uint32_t*>(base + lay.long_list);
  S.seg_depth = reinterpret_cast<uint64_t*>(base + lay.seg_depth);
  S.seg_cur = reinterpret_cast<unsigned long long*>(base + lay.seg_cur);
  S.seg_head = reinterpret_cast<uint32_t*>(base + lay.seg_head);
  const Rows R{d_rec_begin, d_rec_end, d_indices};
  const uint8_t* text = static_cast<const uint8_t*>(d_text);
  const dim3 block(kThreads);
  rj_sort_stats total{0, 0, 0, 0};
  uint64_t n_active = k >= 2 ? k : 0, n_segments = 1;
  for (bool first = true; first || n_active; first = false) {
    int rc;
    unsigned long long *scratch = nullptr, *summary = nullptr;
    if ((rc = records_begin(s, scratch_words, st, &scratch, &summary)) != RJ_OK) return rc;
    if (first) hipLaunchKernelGGL(record_sort_init_kernel, dim3(unit_grid(n_units)), block, 0, st, n, R, n_records, k, n_units, S, d_order, summary);
    if (n_active) {
      const bool skips = skip && !first;
      const uint64_t a_units = (n_active + kThreads - 1) / kThreads;
      const dim3 a_grid(unit_grid(a_units));
      hipLaunchKernelGGL(record_sort_compact_kernel, dim3(unit_grid(n_units)), block, 0, st, k, n_units, skips, S, scratch + 1, scratch, summary);
      if (skips) {
        hipLaunchKernelGGL(record_sort_skip_kernel, a_grid, block, 0, st, text, n, R, n_active, a_units, long_bytes, S, summary);
        hipLaunchKernelGGL(record_sort_skip_long_kernel, dim3(unit_grid((n_active + kWaves - 1) / kWaves)), block, 0, st, text, n, R, long_bytes, S, summary);
      }
      hipLaunchKernelGGL(record_sort_key_kernel, a_grid, block, 0, st, text, n, R, n_active, a_units, S, summary);
      const uint64_t *keys = nullptr, *seg_rows = nullptr;
      if ((rc = order_list(s, lay, base, n_active, n_segments, st, &keys, &seg_rows)) != RJ_OK) return rc;
      const SortedList list{keys, seg_rows};
      hipLaunchKernelGGL(record_sort_cut_kernel, a_grid, block, 0, st, n_active, a_units, list, S, d_order, summary);
    }
    if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
    if (s->rec_host[kSumBadWord] != 0)
      return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_sort: row %llu names no record or a record outside the text (index < n_records, begin <= end <= n)",
                     static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
    if (n_active) {
      total.rounds += 1;
      total.keyed_rows += n_active;
      if (skip && !first) total.skip_rows += n_active;
      total.long_rows += s->rec_host[kSortLongRows];
      n_active = s->rec_host[kSortOpenRows];
      n_segments = s->rec_host[kSortOpenSegments];
    }
  }
  if (stats) *stats = total;
  return static_cast<int64_t>(k);
}

}  // extern "C"
