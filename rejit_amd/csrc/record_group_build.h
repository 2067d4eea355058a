// rejit_amd/csrc/record_group_build.h -- the BUILD of record_group.h's table over one record table, shared by the two calls that
// need it: rj_scan_records_group (record_group.hip) numbers the table's strings, rj_scan_records_lookup (record_lookup.hip)
// probes it with the rows of another table.  Two memsets and four launches on one stream (group_build):
//
// Hash (lane): one row per lane.  The pack's checks (rows::resolve; the first bad row wins, note_bad_row); rows of at most L
//   bytes get their 64-bit key and a 32-bit length, longer ones are appended to a list (wave_append).
// Hash (wave): one wave per listed row, 64 lanes x 16 bytes = 1 KiB per iteration, the lanes' partial sums added by wave_sum64.
// Insert (lane): one row per lane into the open-addressing table; the byte compare covers at most L bytes.  The lanes of a
//   wave that ended at the slot of the wave's first active lane issue ONE atomic add and ONE atomic min (the peel: a column
//   with few distinct values sends most of a wave to one slot); the others issue their own.
// Insert (wave): one wave per listed row; lane 0 does the atomics, the answers are broadcast; 1 KiB per compare iteration,
//   a ballot ends it at the first difference.
// Every kernel behind the first returns at once when the summary holds a bad row.  Nothing here waits for another lane's
// progress (record_group.h).  The rows, the text, the refusal, the two wave idioms and the knobs' parser are record_frame.h's;
// like it everything here lives in an anonymous namespace: every unit gets its own copy.
#ifndef REJIT_AMD_RECORD_GROUP_BUILD_H_
#define REJIT_AMD_RECORD_GROUP_BUILD_H_

#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_group.h"
#include "record_rows.h"

namespace rejit_amd {

namespace {

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

// ---------------------------------------------------------------------------------------------------------------- hash
__global__ __launch_bounds__(kThreads) void record_group_hash_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint64_t n_records, uint64_t k,
                                                                     uint64_t n_units, uint32_t long_bytes, uint32_t hash_bits, Scratch S,
                                                                     unsigned long long* summary) {
  const DeviceText src{text, n};
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    bool bad = false, is_long = false;
    if (j < k) {
      const rows::Row row = rows::resolve(R.rec_begin, R.rec_end, R.indices, n_records, n, j);
      bad = row.bad;
      if (!bad) {
        const uint64_t len = row.len();
        S.len[j] = group::stored_len(len);
        is_long = len > long_bytes;
        if (!is_long) S.hash[j] = group::keep_bits(group::hash_row(src, n, row.rb, len), hash_bits);
      }
    }
    note_bad_row(bad, j, &summary[kSumBadWord]);
    wave_append(is_long, static_cast<uint32_t>(j), S.long_count, S.long_list);
  }
}

__global__ __launch_bounds__(kThreads) void record_group_hash_long_kernel(const uint8_t* __restrict__ text, uint64_t n, Rows R, uint32_t hash_bits, Scratch S,
                                                                          const unsigned long long* summary) {
  if (refused(summary)) return;
  const DeviceText src{text, n};
  const uint64_t n_long = *S.long_count;
  const int lane = lane_id();
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); i < n_long; i += waves) {
    const uint64_t j = S.long_list[i];
    const uint64_t r = R.record(j);
    const uint64_t rb = R.rec_begin[r], len = R.rec_end[r] - rb;
    const uint64_t part = group::hash_groups(src, n, rb, len, static_cast<uint64_t>(lane), kWave, rows::n_groups(len));
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
  const DeviceText src{text, n};
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
      const uint64_t groups = rows::n_groups(len);
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
  const DeviceText src{text, n};
  WaveMem M{S};
  const uint64_t n_long = *S.long_count;
  const int lane = lane_id();
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); i < n_long; i += waves) {
    const uint64_t j = S.long_list[i];
    const uint64_t r = R.record(j);
    const uint64_t rb = R.rec_begin[r], len = R.rec_end[r] - rb;
    const uint64_t groups = rows::n_groups(len);
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

// ---------------------------------------------------------------------------------------------------------------- host
// the test knobs, read at every call: RJ_GROUP_HASH_BITS (0..64), RJ_GROUP_LONG_BYTES; RJ_GROUP_PEEL=0 is the probe's
struct GroupKnobs {
  uint32_t long_bytes, hash_bits;
  bool peel;
};
inline GroupKnobs group_knobs() {
  GroupKnobs kn;
  kn.long_bytes = env_number("RJ_GROUP_LONG_BYTES", group::kLongBytes, rows::kMaxLongBytes);
  kn.hash_bits = env_number("RJ_GROUP_HASH_BITS", 64, 64);
  kn.peel = env_number("RJ_GROUP_PEEL", 1, 1) != 0;
  return kn;
}

// the parts of group::layout(k) at `base`; long_count: a zeroed word of the call's scratch
inline Scratch group_scratch(uint8_t* base, uint64_t k, unsigned long long* long_count) {
  const group::Layout lay = group::layout(k);
  Scratch S;
  S.slots = reinterpret_cast<unsigned long long*>(base + lay.table);
  S.slot_count = reinterpret_cast<uint32_t*>(base + lay.slot_count);
  S.slot_group = reinterpret_cast<uint32_t*>(base + lay.slot_group);
  S.hash = reinterpret_cast<uint64_t*>(base + lay.hash);
  S.len = reinterpret_cast<uint32_t*>(base + lay.len);
  S.slot_of = reinterpret_cast<uint32_t*>(base + lay.slot_of);
  S.long_list = reinterpret_cast<uint32_t*>(base + lay.long_list);
  S.long_count = long_count;
  S.T = group::table_slots(k);
  return S;
}

// the table of the k rows R names, built behind what the stream holds: every slot kEmpty or the smallest row of its string,
// slot_count their number, slot_of[j] row j's slot -- or, for a bad row, its word in summary[kSumBadWord] and a table nobody reads
inline int group_build(const uint8_t* text, uint64_t n, const Rows& R, uint64_t n_records, uint64_t k, const GroupKnobs& kn, const Scratch& S,
                       unsigned long long* summary, hipStream_t st) {
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  RJ_HIP(hipMemsetAsync(S.slots, 0xFF, 8 * S.T, st));
  RJ_HIP(hipMemsetAsync(S.slot_count, 0, 4 * S.T, st));
  const dim3 grid(unit_grid(n_units)), block(kThreads);
  hipLaunchKernelGGL(record_group_hash_kernel, grid, block, 0, st, text, n, R, n_records, k, n_units, kn.long_bytes, kn.hash_bits, S, summary);
  hipLaunchKernelGGL(record_group_hash_long_kernel, grid, block, 0, st, text, n, R, kn.hash_bits, S, summary);
  if (kn.peel) hipLaunchKernelGGL(record_group_insert_kernel<true>, grid, block, 0, st, text, n, R, k, n_units, kn.long_bytes, S, summary);
  else hipLaunchKernelGGL(record_group_insert_kernel<false>, grid, block, 0, st, text, n, R, k, n_units, kn.long_bytes, S, summary);
  hipLaunchKernelGGL(record_group_insert_long_kernel, grid, block, 0, st, text, n, R, S, summary);
  return RJ_OK;
}

}  // namespace

}  // namespace rejit_amd
#endif
