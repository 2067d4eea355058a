// rejit_amd/csrc/record_group.hip -- rj_scan_records_group: the rows of a record table over a device text -- the pieces of
// rj_scan_records_split, lines, the strings of a column; every row, or the rows an index list names -- grouped by their bytes:
// d_group[j] (Arrow's dictionary_encode), d_rep[g] (the first row of every distinct string, in order of first appearance) and
// d_group_count[g] (value_counts, `uniq -c`), exactly and without a download.  record_group.h has the arithmetic and the two
// invariants that make the table exact under any interleaving; six launches on one stream, one synchronise:
//
// Hash (lane): one row per lane.  The pack's checks (the first bad row wins by one atomic max); rows of at most L bytes get
//   their 64-bit key and a 32-bit length, longer ones are appended to a list (one ballot, one atomic add per wave).
// Hash (wave): one wave per listed row, 64 lanes x 16 bytes = 1 KiB per iteration, the lanes' partial sums added by wave_sum64.
// Insert (lane): one row per lane into the open-addressing table; the byte compare covers at most L bytes.  The lanes of a
//   wave that ended at the slot of the wave's first active lane issue ONE atomic add and ONE atomic min (the peel: a column
//   with few distinct values sends most of a wave to one slot); the others issue their own.
// Insert (wave): one wave per listed row; lane 0 does the atomics, the answers are broadcast; 1 KiB per compare iteration,
//   a ballot ends it at the first difference.
// Number: record_frame.h's unit scan over the representative flags -> d_rep, d_group_count, slot_group, G.
// Emit: d_group[j] = slot_group[slot_of[j]].
// Every kernel behind the first returns at once when the summary holds a bad row.  Nothing here waits for another lane's
// progress (record_group.h); the only bounded wait is the unit scan's look-back, as in every plan of the family.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_group.h"
#include "record_pack.h"

namespace rejit_amd {

namespace {

// record_group.h's Text over record_frame.h's DeviceText
struct GroupText {
  DeviceText t;
  __device__ __forceinline__ void load16(uint64_t s, uint32_t w[4]) const { t.load16(s, w); }
  __device__ __forceinline__ void load16_guarded(uint64_t s, uint32_t w[4]) const {
    uint32_t d[6];
    load_guarded(t.text, t.n, s, d);
    w[0] = d[0], w[1] = d[1], w[2] = d[2], w[3] = d[3];
  }
};

struct Rows {
  const uint64_t* __restrict__ rec_begin;
  const uint64_t* __restrict__ rec_end;
  const uint64_t* __restrict__ indices;
  __device__ __forceinline__ uint64_t record(uint64_t j) const { return indices ? indices[j] : j; }
};

// the scratch of a call (group::layout)
struct Scratch {
  unsigned long long* slots;
  uint32_t* slot_count;
  uint32_t* slot_group;
  uint64_t* hash;
  uint32_t* len;
  uint32_t* slot_of;
  uint32_t* long_list;
  unsigned long long* long_count;
  uint64_t T;
};

__device__ __forceinline__ bool refused(const unsigned long long* summary) { return summary[kSumBadWord] != 0 || summary[kSumTimedOut] != 0; }

// ---------------------------------------------------------------------------------------------------------------- hash
__global__ __launch_bounds__(kThreads) void record_group_hash_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint64_t n_records, uint64_t k,
                                                                     uint64_t n_units, uint32_t long_bytes, uint32_t hash_bits, Scratch S,
                                                                     unsigned long long* summary) {
  const GroupText src{DeviceText{text, n}};
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    bool bad = false, is_long = false;
    if (j < k) {
      const uint64_t r = R.record(j);
      bad = pack::bad_index(r, n_records);
      uint64_t rb = 0, re = 0;
      if (!bad) {
        rb = R.rec_begin[r], re = R.rec_end[r];
        bad = pack::bad_row(rb, re, n);
      }
      if (!bad) {
        const uint64_t len = re - rb;
        S.len[j] = group::stored_len(len);
        is_long = len > long_bytes;
        if (!is_long) S.hash[j] = group::keep_bits(group::hash_row(src, n, rb, len), hash_bits);
      }
    }
    const uint64_t bad_lanes = __ballot(bad);
    if (bad_lanes && lane_id() == __builtin_ctzll(bad_lanes)) atomicMax(&summary[kSumBadWord], static_cast<unsigned long long>(~j));
    const uint64_t long_lanes = __ballot(is_long);
    if (long_lanes) {
      const int leader = __builtin_ctzll(long_lanes);
      unsigned long long base = 0;
      if (lane_id() == leader) base = atomicAdd(S.long_count, static_cast<unsigned long long>(__popcll(long_lanes)));
      base = lane_value(base, leader);
      if (is_long) S.long_list[base + lanes_below(long_lanes)] = static_cast<uint32_t>(j);
    }
  }
}

__global__ __launch_bounds__(kThreads) void record_group_hash_long_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint32_t hash_bits, Scratch S,
                                                                          const unsigned long long* summary) {
  if (refused(summary)) return;
  const GroupText src{DeviceText{text, n}};
  const uint64_t n_long = *S.long_count;
  const int lane = lane_id();
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); i < n_long; i += waves) {
    const uint64_t j = S.long_list[i];
    const uint64_t r = R.record(j);
    const uint64_t rb = R.rec_begin[r], len = R.rec_end[r] - rb;
    const uint64_t part = group::hash_groups(src, n, rb, len, static_cast<uint64_t>(lane), kWave, group::n_groups(len));
    const uint64_t sum = wave_sum64(part);
    if (lane == 0) S.hash[j] = group::keep_bits(group::finalize(len, sum), hash_bits);
  }
}

// ---------------------------------------------------------------------------------------------------------------- insert
// record_group.h's Mem for one lane: agent-scope atomics on the table, plain reads of what the hash kernels stored
struct LaneMem {
  Scratch S;
  __device__ __forceinline__ uint64_t slot_load(uint64_t s) const { return __hip_atomic_load(&S.slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ uint64_t slot_cas(uint64_t s, uint64_t j) const { return atomicCAS(&S.slots[s], group::kEmpty, static_cast<unsigned long long>(j)); }
  __device__ __forceinline__ void slot_min(uint64_t s, uint64_t j) const { atomicMin(&S.slots[s], static_cast<unsigned long long>(j)); }
  __device__ __forceinline__ void count_add(uint64_t s, uint32_t c) const { atomicAdd(&S.slot_count[s], c); }
  __device__ __forceinline__ uint64_t hash(uint64_t i) const { return S.hash[i]; }
  __device__ __forceinline__ uint32_t len(uint64_t i) const { return S.len[i]; }
};

template <bool kPeel>
__global__ __launch_bounds__(kThreads) void record_group_insert_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint64_t k, uint64_t n_units,
                                                                       uint32_t long_bytes, Scratch S, const unsigned long long* summary) {
  if (refused(summary)) return;
  const GroupText src{DeviceText{text, n}};
  LaneMem M{S};
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    uint32_t len = 0;
    bool active = false;
    if (j < k) {
      len = S.len[j];
      active = len <= long_bytes;
    }
    uint64_t s = 0;
    if (active) {
      const uint64_t rb = R.rec_begin[R.record(j)];
      const uint64_t groups = group::n_groups(len);
      s = group::find_slot(M, j, S.hash[j], len, S.T,
                           [&](uint64_t i) { return group::groups_equal(src, n, R.rec_begin[R.record(i)], rb, len, 0, 1, groups); });
      S.slot_of[j] = static_cast<uint32_t>(s);
    }
    bool own = active;
    if (kPeel) {
      const uint64_t act = __ballot(active);
      if (act) {
        const uint64_t s0 = lane_value(s, __builtin_ctzll(act));
        const bool with_first = active && s == s0;
        const uint64_t same = __ballot(with_first);
        // a wave's rows ascend with its lanes: the lowest of these lanes holds the least row
        if (with_first && lane_id() == __builtin_ctzll(same)) group::join_slot(M, s0, j, static_cast<uint32_t>(__popcll(same)));
        own = active && !with_first;
      }
    }
    if (own) group::join_slot(M, s, j, 1);
  }
}

// record_group.h's Mem for a wave: lane 0 asks, every lane gets the answer
struct WaveMem {
  Scratch S;
  __device__ __forceinline__ uint64_t slot_load(uint64_t s) const {
    uint64_t v = 0;
    if (lane_id() == 0) v = __hip_atomic_load(&S.slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return lane_value(v, 0);
  }
  __device__ __forceinline__ uint64_t slot_cas(uint64_t s, uint64_t j) const {
    uint64_t v = 0;
    if (lane_id() == 0) v = atomicCAS(&S.slots[s], group::kEmpty, static_cast<unsigned long long>(j));
    return lane_value(v, 0);
  }
  __device__ __forceinline__ void slot_min(uint64_t s, uint64_t j) const {
    if (lane_id() == 0) atomicMin(&S.slots[s], static_cast<unsigned long long>(j));
  }
  __device__ __forceinline__ void count_add(uint64_t s, uint32_t c) const {
    if (lane_id() == 0) atomicAdd(&S.slot_count[s], c);
  }
  __device__ __forceinline__ uint64_t hash(uint64_t i) const { return S.hash[i]; }
  __device__ __forceinline__ uint32_t len(uint64_t i) const { return S.len[i]; }
};

__global__ __launch_bounds__(kThreads) void record_group_insert_long_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, Scratch S,
                                                                            const unsigned long long* summary) {
  if (refused(summary)) return;
  const GroupText src{DeviceText{text, n}};
  WaveMem M{S};
  const uint64_t n_long = *S.long_count;
  const int lane = lane_id();
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); i < n_long; i += waves) {
    const uint64_t j = S.long_list[i];
    const uint64_t r = R.record(j);
    const uint64_t rb = R.rec_begin[r], len = R.rec_end[r] - rb;
    const uint64_t groups = group::n_groups(len);
    // (the stored length saturates: the tables have the length of a row of 4 GiB)
    const auto equal = [&](uint64_t c) {
      const uint64_t rc = R.record(c);
      const uint64_t cb = R.rec_begin[rc];
      if (R.rec_end[rc] - cb != len) return false;
      if (cb == rb) return true;
      for (uint64_t g0 = 0; g0 < groups; g0 += kWave) {
        const uint64_t g = g0 + static_cast<uint64_t>(lane);
        const bool differs = g < groups && !group::group_equal(src, n, cb, rb, len, g);
        if (__ballot(differs)) return false;
      }
      return true;
    };
    const uint64_t s = group::find_slot(M, j, S.hash[j], group::stored_len(len), S.T, equal);
    group::join_slot(M, s, j, 1);
    if (lane == 0) S.slot_of[j] = static_cast<uint32_t>(s);
  }
}

// ---------------------------------------------------------------------------------------------------------------- number, emit
__global__ __launch_bounds__(kThreads) void record_group_number_kernel(uint64_t k, uint64_t n_units, Scratch S, unsigned long long* granules,
                                                                       unsigned long long* ticket, uint64_t* __restrict__ rep,
                                                                       uint64_t* __restrict__ group_count, uint64_t group_cap, unsigned long long* summary) {
  __shared__ UnitSum s_unit;
  if (summary[kSumBadWord] != 0) return;
  LaneMem M{S};
  unit_init(s_unit.place);
  for (uint64_t tk; unit_take(s_unit.place, ticket, n_units, &tk);) {
    const uint64_t j = tk * kThreads + threadIdx.x;
    uint64_t s = 0;
    bool is_rep = false;
    if (j < k) {
      s = S.slot_of[j];
      is_rep = group::is_representative(M, j, s);
    }
    uint64_t g, unit_end;
    const bool ok = unit_exclusive_sum(s_unit, is_rep ? 1 : 0, tk, n_units, granules, summary, &g, &unit_end);
    if (ok && tk == n_units - 1 && threadIdx.x == 0) summary[kSumTotal] = unit_end;
    if (ok && is_rep) {
      const uint32_t rows = S.slot_count[s];        // (slot_group takes slot_count's place: the count is read first)
      S.slot_group[s] = static_cast<uint32_t>(g);
      if (g < group_cap) {
        rep[g] = j;
        group_count[g] = rows;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void record_group_emit_kernel(uint64_t k, uint64_t n_units, Scratch S, uint64_t* __restrict__ group_of,
                                                                     const unsigned long long* summary) {
  if (refused(summary)) return;
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    if (j < k) group_of[j] = S.slot_group[S.slot_of[j]];
  }
}

// the test knobs, read at every call: RJ_GROUP_HASH_BITS (0..64), RJ_GROUP_LONG_BYTES; RJ_GROUP_PEEL=0 is the probe's
uint32_t env_number(const char* name, uint32_t otherwise, uint32_t most) {
  const char* v = getenv(name);
  if (!v || !*v) return otherwise;
  char* end = nullptr;
  const unsigned long long x = strtoull(v, &end, 10);
  if (!end || *end) return otherwise;
  return x > most ? most : static_cast<uint32_t>(x);
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_group(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                              const uint64_t* d_indices, uint64_t n_indices, uint64_t* d_group, uint64_t* d_rep, uint64_t* d_group_count,
                              uint64_t group_cap, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_group";
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) || (group_cap && (!d_rep || !d_group_count)))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_group: null argument");
  if (!aligned8(d_rec_begin, d_rec_end, d_indices, d_group, d_rep, d_group_count))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_group: a table is not 8-byte aligned");
  const uint64_t k = d_indices ? n_indices : n_records;
  if (!group::rows_fit(k))
    return rj_fail(RJ_TOO_LARGE, "rj_scan_records_group: %llu rows: rows and slots share 32-bit words in the scratch (fewer than 2^31 rows)",
                   static_cast<unsigned long long>(k));
  if (k == 0) return 0;
  const uint32_t long_bytes = env_number("RJ_GROUP_LONG_BYTES", group::kLongBytes, group::kMaxLongBytes);
  const uint32_t hash_bits = env_number("RJ_GROUP_HASH_BITS", 64, 64);
  const bool peel = env_number("RJ_GROUP_PEEL", 1, 1) != 0;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  const group::Layout lay = group::layout(k);
  RJ_HIP(s->rec_repl_table.reserve(lay.bytes));
  int rc;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, the long list's counter, the look-back's words
  if ((rc = records_begin(s, 2 + lookback::granule_words(n_units), st, &scratch, &summary)) != RJ_OK) return rc;
  uint8_t* base = s->rec_repl_table.as<uint8_t>();
  Scratch S;
  S.slots = reinterpret_cast<unsigned long long*>(base + lay.table);
  S.slot_count = reinterpret_cast<uint32_t*>(base + lay.slot_count);
  S.slot_group = reinterpret_cast<uint32_t*>(base + lay.slot_group);
  S.hash = reinterpret_cast<uint64_t*>(base + lay.hash);
  S.len = reinterpret_cast<uint32_t*>(base + lay.len);
  S.slot_of = reinterpret_cast<uint32_t*>(base + lay.slot_of);
  S.long_list = reinterpret_cast<uint32_t*>(base + lay.long_list);
  S.long_count = scratch + 1;
  S.T = group::table_slots(k);
  RJ_HIP(hipMemsetAsync(S.slots, 0xFF, 8 * S.T, st));
  RJ_HIP(hipMemsetAsync(S.slot_count, 0, 4 * S.T, st));
  const Rows R{d_rec_begin, d_rec_end, d_indices};
  const uint8_t* text = static_cast<const uint8_t*>(d_text);
  const dim3 grid(unit_grid(n_units)), block(kThreads);
  hipLaunchKernelGGL(record_group_hash_kernel, grid, block, 0, st, text, n, R, n_records, k, n_units, long_bytes, hash_bits, S, summary);
  hipLaunchKernelGGL(record_group_hash_long_kernel, grid, block, 0, st, text, n, R, hash_bits, S, summary);
  if (peel) hipLaunchKernelGGL(record_group_insert_kernel<true>, grid, block, 0, st, text, n, R, k, n_units, long_bytes, S, summary);
  else hipLaunchKernelGGL(record_group_insert_kernel<false>, grid, block, 0, st, text, n, R, k, n_units, long_bytes, S, summary);
  hipLaunchKernelGGL(record_group_insert_long_kernel, grid, block, 0, st, text, n, R, S, summary);
  hipLaunchKernelGGL(record_group_number_kernel, grid, block, 0, st, k, n_units, S, scratch + 2, scratch, d_rep, d_group_count, group_cap, summary);
  if (d_group) hipLaunchKernelGGL(record_group_emit_kernel, grid, block, 0, st, k, n_units, S, d_group, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_group: row %llu names no record or a record outside the text (index < n_records, begin <= end <= n)",
                   static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
