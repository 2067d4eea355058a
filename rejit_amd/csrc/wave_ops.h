// rejit_amd/csrc/wave_ops.h -- the pure wave-level primitives every kernel unit shares: lane index, ranks from a lane mask,
// DPP moves, prefix scans over the 64 lanes, reads of one lane.  Nothing here knows about texts, chunks or programs (a unit's
// geometry constants stay with the unit).  Everything lives in an anonymous namespace: every unit gets its own copy.
#ifndef REJIT_AMD_WAVE_OPS_H_
#define REJIT_AMD_WAVE_OPS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rejit_amd {

namespace {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return static_cast<int>(threadIdx.x) & (kWave - 1); }

// the number of set bits of `mask` (a ballot) in the lanes below this one: v_mbcnt_lo + v_mbcnt_hi
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// Cross-lane moves through DPP (data-parallel primitives: the operand of a VALU
// instruction comes from another lane of the wave, no LDS crossbar round trip as with ds_bpermute, which
// is what __shfl_up / __shfl_down compile to).  gfx9 family: row_shr within rows of 16 lanes, row_bcast:15 /
// row_bcast:31 to carry a row's total into the next rows, wave_shl / wave_shr by one lane.
// bound_ctrl = true: a lane whose source lies outside the wave (or its row) reads 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t x) {
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), CTRL, ROW_MASK, 0xF, true));
}
// Inclusive prefix sum / prefix maximum (unsigned) over the 64 lanes, in six steps.  0 is the neutral element of both: it is
// what a lane without a source reads, and what the rows a row_bcast does not write (ROW_MASK) add.
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x) {
  x += dpp_or_zero<0x111, 0xF>(x);  // row_shr:1
  x += dpp_or_zero<0x112, 0xF>(x);  // row_shr:2
  x += dpp_or_zero<0x114, 0xF>(x);  // row_shr:4
  x += dpp_or_zero<0x118, 0xF>(x);  // row_shr:8
  x += dpp_or_zero<0x142, 0xA>(x);  // row_bcast:15 into rows 1 and 3
  x += dpp_or_zero<0x143, 0xC>(x);  // row_bcast:31 into rows 2 and 3
  return x;
}
__device__ __forceinline__ uint32_t umax(uint32_t x, uint32_t y) { return x > y ? x : y; }
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t x) {
  x = umax(x, dpp_or_zero<0x111, 0xF>(x));
  x = umax(x, dpp_or_zero<0x112, 0xF>(x));
  x = umax(x, dpp_or_zero<0x114, 0xF>(x));
  x = umax(x, dpp_or_zero<0x118, 0xF>(x));
  x = umax(x, dpp_or_zero<0x142, 0xA>(x));
  x = umax(x, dpp_or_zero<0x143, 0xC>(x));
  return x;
}

// lane i <- lane i - 1 / lane i + 1.  One argument: the lane at the wave's end gets 0 ...
__device__ __forceinline__ uint32_t wave_from_lane_below(uint32_t x) { return dpp_or_zero<0x138, 0xF>(x); }  // wave_shr:1, lane 0 gets 0
__device__ __forceinline__ uint32_t wave_from_lane_above(uint32_t x) { return dpp_or_zero<0x130, 0xF>(x); }  // wave_shl:1, lane 63 gets 0
// ... two arguments: it keeps its own `fill` (bound_ctrl = false: the move leaves the destination as it was; another instruction
// sequence than the zero-filling form, which needs no copy of a fill value first)
__device__ __forceinline__ uint32_t wave_from_lane_below(uint32_t x, uint32_t fill) {
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(fill), static_cast<int>(x), 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ uint32_t wave_from_lane_above(uint32_t x, uint32_t fill) {
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(fill), static_cast<int>(x), 0x130, 0xF, 0xF, false));
}

// lane l's value as a wave-uniform scalar (v_readlane; l must be wave-uniform)
__device__ __forceinline__ uint32_t wave_last_lane(uint32_t x) { return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(x), kWave - 1)); }
__device__ __forceinline__ uint32_t wave_total(uint32_t x) { return wave_last_lane(wave_inclusive_sum(x)); }
__device__ __forceinline__ uint64_t lane_value(uint64_t x, int l) {
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(x)), l));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(x >> 32)), l));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

}  // namespace

}  // namespace rejit_amd
#endif
