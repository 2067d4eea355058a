// rejit_amd/csrc/record_lookup.hip -- rj_scan_records_lookup: the rows of one record table (the probe rows) looked up in the
// rows of another (the set rows), each table over a device text of its own: d_index[j] = the smallest set row equal to probe
// row j (Arrow's index_in; is_in, `grep -F -x -f`, a semi-join), d_set_hits[i] = the probe rows that found set row i (the
// anti-join's right side where it is 0), exactly and without a download.  record_lookup.h has the arithmetic and the argument
// why the probes need nothing but plain loads; four or five memsets and up to eight launches on one stream, one synchronise:
//
// Build: record_group_build.h's hash, hash-long, insert and insert-long kernels over the SET table -- rj_scan_records_group's own.
// Probe (lane): one probe row per lane.  The pack's checks (rows::resolve; the first bad row wins, note_bad_row, in a summary
//   word of the probe side's own); rows of at most L bytes are hashed and looked up at once -- the probe side stores no hash
//   and no length --, longer ones are appended to a list (wave_append).  One unit of 256 rows per workgroup.  The byte compare
//   covers at most L bytes and reads both texts (rows::groups_equal).  The answer is staged as a 32-bit word (record_lookup.h:
//   a refused call writes no output row).
//   With hit counts the lanes that ended at the slot of the wave's first found lane issue ONE atomic add (the peel), the
//   others their own; without them (the is_in path: neither d_set_hits nor stats) the kernel issues no atomic on the table or
//   the counts.
// Probe (wave): one wave per listed row, 64 lanes x 16 bytes = 1 KiB per iteration for the hash (wave_sum64) and for the
//   compare across the two texts, which a ballot ends at the first difference; lane 0 loads the slots, the answers are broadcast.
// Emit: d_index[j] = the staged answer, widened; n_found: one ballot per unit, one atomic add per wave.
// Hits: one lane per set row: d_set_hits[i] = hits[slot_of[i]] when slot[slot_of[i]] == i, else 0; n_set_distinct and
//   n_set_hit from ballots, one atomic add per wave.
// Every kernel behind the first check returns at once when the summary holds a bad row of either table.  Nothing here waits
// for another lane's progress.  The rows, the text, the refusal and the two wave idioms are record_frame.h's.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_group.h"
#include "record_group_build.h"
#include "record_lookup.h"
#include "record_rows.h"

namespace rejit_amd {

namespace {

// the summary words of a lookup: kSumBadWord is the SET's first bad row (the build's), the probe side has its own
enum { kSumFound = kSumKept, kSumLongRows = kSumMatching, kSumSetDistinct = kSumSelected, kSumSetHit = kSumTotal, kSumProbeBad = 7 };
static_assert(kSumProbeBad < kSumWords && kSumProbeBad != kSumTimedOut && kSumProbeBad != kSumBadWord, "a summary word of its own");

__device__ __forceinline__ bool lookup_refused(const unsigned long long* summary) { return refused(summary) || summary[kSumProbeBad] != 0; }

// the probe side's scratch (lookup::layout)
struct ProbeScratch {
  uint32_t* hits;
  uint32_t* staged;
  uint32_t* long_list;   // (its counter is summary[kSumLongRows]: the statistic itself)
};

// what a probe reads of the set's scratch, behind the build: the table, and the hash pass's keys of the set rows
struct SetTable {
  const unsigned long long* __restrict__ slots;
  const uint64_t* __restrict__ hash;
  const uint32_t* __restrict__ len;
  uint32_t slot_mask;   // T - 1 (T <= 2^32)
  __device__ __forceinline__ uint64_t slot_count() const { return static_cast<uint64_t>(slot_mask) + 1; }
};

// record_lookup.h's Mem for one lane: plain loads of a table that is final
struct ProbeLaneMem {
  SetTable S;
  __device__ __forceinline__ uint64_t slot_load(uint64_t s) const { return S.slots[s]; }
  __device__ __forceinline__ uint64_t hash(uint64_t i) const { return S.hash[i]; }
  __device__ __forceinline__ uint32_t len(uint64_t i) const { return S.len[i]; }
};
// ... for a wave: lane 0 loads the slot, every lane gets the answer
struct ProbeWaveMem {
  SetTable S;
  __device__ __forceinline__ uint64_t slot_load(uint64_t s) const {
    uint64_t v = 0;
    if (lane_id() == 0) v = S.slots[s];
    return lane_value(v, 0);
  }
  __device__ __forceinline__ uint64_t hash(uint64_t i) const { return S.hash[i]; }
  __device__ __forceinline__ uint32_t len(uint64_t i) const { return S.len[i]; }
};

// ---------------------------------------------------------------------------------------------------------------- probe
template <bool kHits, bool kPeel>
__global__ __launch_bounds__(kThreads) void record_lookup_probe_kernel(const uint8_t* __restrict__ set_text, uint64_t set_n, Rows RS,
                                                                       const uint8_t* __restrict__ text, uint64_t n, Rows R, uint64_t n_records, uint64_t kp,
                                                                       uint32_t long_bytes, uint32_t hash_bits, SetTable S, ProbeScratch P,
                                                                       unsigned long long* summary) {
  if (refused(summary)) return;   // a bad set row: the set table is checked first, and its row is the one the call names
  const DeviceText set_src{set_text, set_n};
  const DeviceText src{text, n};
  ProbeLaneMem M{S};
  // one unit of 256 rows per workgroup (no persistent loop: what the checks and the hash need is dead when the walk begins)
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  bool bad = false, is_long = false, found = false;
  uint64_t s = 0;
  if (j < kp) {
    const rows::Row row = rows::resolve(R.rec_begin, R.rec_end, R.indices, n_records, n, j);
    bad = row.bad;
    if (!bad) {
      const uint64_t rb = row.rb, len = row.len();
      is_long = len > long_bytes;
      if (!is_long) {
        const uint64_t h = group::keep_bits(group::hash_row(src, n, rb, len), hash_bits);
        const uint64_t groups = rows::n_groups(len);
        s = lookup::probe_slot(M, h, static_cast<uint32_t>(len), S.slot_count(), [&](uint64_t i) {
          return rows::groups_equal(set_src, set_n, RS.rec_begin[RS.record(i)], src, n, rb, len, 0, 1, groups);
        });
        found = s != lookup::kAbsent;
        P.staged[j] = found ? static_cast<uint32_t>(M.slot_load(s)) : lookup::kStagedNone;
      }
    }
  }
  note_bad_row(bad, j, &summary[kSumProbeBad]);
  wave_append(is_long, static_cast<uint32_t>(j), &summary[kSumLongRows], P.long_list);
  if (kHits) {
    const uint64_t found_lanes = __ballot(found);
    if (!found_lanes) return;
    const int first_found = __builtin_ctzll(found_lanes);
    bool own = found;
    if (kPeel) {
      const uint64_t s0 = lane_value(s, first_found);
      const bool with_first = found && s == s0;
      const uint64_t same = __ballot(with_first);
      if (lane_id() == first_found) atomicAdd(&P.hits[s0], static_cast<uint32_t>(__popcll(same)));
      own = found && !with_first;
    }
    if (own) atomicAdd(&P.hits[s], 1u);
  }
}

template <bool kHits>
__global__ __launch_bounds__(kThreads) void record_lookup_probe_long_kernel(const uint8_t* __restrict__ set_text, uint64_t set_n, Rows RS,
                                                                            const uint8_t* __restrict__ text, uint64_t n, Rows R, uint32_t hash_bits, SetTable S,
                                                                            ProbeScratch P, const unsigned long long* summary) {
  if (lookup_refused(summary)) return;
  const DeviceText set_src{set_text, set_n};
  const DeviceText src{text, n};
  ProbeWaveMem M{S};
  const uint32_t n_long = static_cast<uint32_t>(summary[kSumLongRows]);   // (at most kp < 2^31; the grid has at most 1024 x 4 waves)
  const int lane = lane_id();
  uint32_t waves = gridDim.x * kWaves;
  asm volatile("" : "+v"(waves));   // (the stride in a vector register: the loop nest below has a use for every scalar one)
  for (uint32_t i = blockIdx.x * kWaves + (threadIdx.x >> 6); i < n_long; i += waves) {
    const uint64_t j = P.long_list[i];
    const uint64_t r = R.record(j);
    const uint64_t rb = R.rec_begin[r], len = R.rec_end[r] - rb;
    const uint64_t groups = rows::n_groups(len);
    const uint64_t part = group::hash_groups(src, n, rb, len, static_cast<uint64_t>(lane), kWave, groups);
    const uint64_t h = group::keep_bits(group::finalize(len, wave_sum64(part)), hash_bits);
    // (the stored length saturates: the tables have the length of a row of 4 GiB)
    const auto equal = [&](uint64_t c) {
      const uint64_t rc = RS.record(c);
      const uint64_t cb = RS.rec_begin[rc];
      if (RS.rec_end[rc] - cb != len) return false;
      for (uint64_t g0 = 0; g0 < groups; g0 += kWave) {
        const uint64_t g = g0 + static_cast<uint64_t>(lane);
        const bool differs = g < groups && !rows::group_equal(set_src, set_n, cb, src, n, rb, len, g);
        if (__ballot(differs)) return false;
      }
      return true;
    };
    const uint64_t s = lookup::probe_slot(M, h, group::stored_len(len), S.slot_count(), equal);
    if (lane == 0) {
      const bool found = s != lookup::kAbsent;
      P.staged[j] = found ? static_cast<uint32_t>(S.slots[s]) : lookup::kStagedNone;
      if (kHits && found) atomicAdd(&P.hits[s], 1u);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- emit, hits
__global__ __launch_bounds__(kThreads) void record_lookup_emit_kernel(uint64_t kp, uint64_t n_units, ProbeScratch P, uint64_t* __restrict__ index,
                                                                      unsigned long long* summary) {
  if (lookup_refused(summary)) return;
  uint32_t found_rows = 0;   // (wave-uniform)
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    uint32_t staged = lookup::kStagedNone;
    if (j < kp) {
      staged = P.staged[j];
      index[j] = lookup::widen(staged);
    }
    found_rows += static_cast<uint32_t>(__popcll(__ballot(staged != lookup::kStagedNone)));
  }
  if (found_rows && lane_id() == 0) atomicAdd(&summary[kSumFound], static_cast<unsigned long long>(found_rows));
}

__global__ __launch_bounds__(kThreads) void record_lookup_hits_kernel(uint64_t ks, uint64_t n_units, SetTable S, const uint32_t* __restrict__ slot_of,
                                                                      const uint32_t* __restrict__ hits, uint64_t* __restrict__ set_hits,
                                                                      unsigned long long* summary) {
  if (lookup_refused(summary)) return;
  ProbeLaneMem M{S};
  uint32_t distinct = 0, hit = 0;   // (wave-uniform)
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t i = unit * kThreads + threadIdx.x;
    bool first = false;
    uint32_t h = 0;
    if (i < ks) {
      const uint64_t s = slot_of[i];
      first = lookup::is_first(M, i, s);
      if (first) h = hits[s];
      if (set_hits) set_hits[i] = h;
    }
    distinct += static_cast<uint32_t>(__popcll(__ballot(first)));
    hit += static_cast<uint32_t>(__popcll(__ballot(h != 0)));
  }
  if (lane_id() == 0) {
    if (distinct) atomicAdd(&summary[kSumSetDistinct], static_cast<unsigned long long>(distinct));
    if (hit) atomicAdd(&summary[kSumSetHit], static_cast<unsigned long long>(hit));
  }
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_lookup(rj_scan* s, const void* d_set_text, uint64_t set_n, const uint64_t* d_set_begin, const uint64_t* d_set_end,
                               uint64_t n_set_records, const uint64_t* d_set_indices, uint64_t n_set_indices, const void* d_text, uint64_t n,
                               const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records, const uint64_t* d_indices, uint64_t n_indices,
                               uint64_t* d_index, uint64_t* d_set_hits, rj_lookup_stats* stats, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_lookup";
  const uint64_t ks = d_set_indices ? n_set_indices : n_set_records;
  const uint64_t kp = d_indices ? n_indices : n_records;
  if (!s || (!d_set_text && set_n) || (n_set_records && (!d_set_begin || !d_set_end)) || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) ||
      (kp && !d_index))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_lookup: null argument");
  if (!aligned8(d_set_begin, d_set_end, d_set_indices, d_rec_begin, d_rec_end, d_indices, d_index, d_set_hits))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_lookup: a table is not 8-byte aligned");
  if (!lookup::rows_fit(ks, kp))
    return rj_fail(RJ_TOO_LARGE,
                   "rj_scan_records_lookup: %llu set rows, %llu rows: hit counts and the long list are 32-bit words in the scratch (fewer than 2^31 rows each)",
                   static_cast<unsigned long long>(ks), static_cast<unsigned long long>(kp));
  if (stats) *stats = rj_lookup_stats{0, 0, 0, 0};
  if (ks == 0 && kp == 0) return 0;
  const GroupKnobs knobs = group_knobs();
  const bool want_hits = d_set_hits != nullptr || stats != nullptr;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t set_units = (ks + kThreads - 1) / kThreads, units = (kp + kThreads - 1) / kThreads;
  const lookup::Layout lay = lookup::layout(ks, kp);
  RJ_HIP(s->rec_repl_table.reserve(lay.bytes));
  int rc;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: (the group call's ticket), the set's long list's counter
  if ((rc = records_begin(s, 2, st, &scratch, &summary)) != RJ_OK) return rc;
  uint8_t* base = s->rec_repl_table.as<uint8_t>();
  const Scratch S = group_scratch(base, ks, scratch + 1);
  const SetTable table{S.slots, S.hash, S.len, static_cast<uint32_t>(S.T - 1)};
  ProbeScratch P;
  P.hits = reinterpret_cast<uint32_t*>(base + lay.hits);
  P.staged = reinterpret_cast<uint32_t*>(base + lay.staged);
  P.long_list = reinterpret_cast<uint32_t*>(base + lay.long_list);
  const Rows RS{d_set_begin, d_set_end, d_set_indices};
  const Rows R{d_rec_begin, d_rec_end, d_indices};
  const uint8_t* set_text = static_cast<const uint8_t*>(d_set_text);
  const uint8_t* text = static_cast<const uint8_t*>(d_text);
  if ((rc = group_build(set_text, set_n, RS, n_set_records, ks, knobs, S, summary, st)) != RJ_OK) return rc;
  if (want_hits) RJ_HIP(hipMemsetAsync(P.hits, 0, 4 * S.T, st));
  const dim3 grid(unit_grid(units)), block(kThreads);
#define RJ_LOOKUP_PROBE(HITS, PEEL)                                                                                                           \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(record_lookup_probe_kernel<HITS, PEEL>), dim3(static_cast<unsigned>(units ? units : 1)), block, 0, st, set_text, \
                     set_n, RS, text, n, R, n_records, kp, knobs.long_bytes, knobs.hash_bits, table, P, summary)
  if (!want_hits) RJ_LOOKUP_PROBE(false, false);
  else if (knobs.peel) RJ_LOOKUP_PROBE(true, true);
  else RJ_LOOKUP_PROBE(true, false);
#undef RJ_LOOKUP_PROBE
  if (want_hits) hipLaunchKernelGGL(record_lookup_probe_long_kernel<true>, grid, block, 0, st, set_text, set_n, RS, text, n, R, knobs.hash_bits, table, P, summary);
  else hipLaunchKernelGGL(record_lookup_probe_long_kernel<false>, grid, block, 0, st, set_text, set_n, RS, text, n, R, knobs.hash_bits, table, P, summary);
  if (kp) hipLaunchKernelGGL(record_lookup_emit_kernel, grid, block, 0, st, kp, units, P, d_index, summary);
  if (want_hits && ks)
    hipLaunchKernelGGL(record_lookup_hits_kernel, dim3(unit_grid(set_units)), block, 0, st, ks, set_units, table, S.slot_of, P.hits, d_set_hits, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0)
    return rj_fail(RJ_BAD_ARGUMENT,
                   "rj_scan_records_lookup: set row %llu names no record or a record outside the set text (index < n_set_records, begin <= end <= set_n)",
                   static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
  if (s->rec_host[kSumProbeBad] != 0)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_lookup: row %llu names no record or a record outside the text (index < n_records, begin <= end <= n)",
                   static_cast<unsigned long long>(~s->rec_host[kSumProbeBad]));
  if (stats) {
    stats->n_found = s->rec_host[kSumFound];
    stats->n_set_distinct = s->rec_host[kSumSetDistinct];
    stats->n_set_hit = s->rec_host[kSumSetHit];
    stats->long_rows = s->rec_host[kSumLongRows];
  }
  return static_cast<int64_t>(s->rec_host[kSumFound]);
}

}  // extern "C"
