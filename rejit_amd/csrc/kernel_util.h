// rejit_amd/csrc/kernel_util.h -- what the kernel translation units that grew out of kernels.hip share (round 6: kernels.hip was
// 3264 lines and a minute of compile time on its own): the hit regions a scanning wave appends to, the span of 1-KiB chunks a
// wave owns, guarded chunk loads.  The wave-level helpers (lane_id, DPP moves, prefix scans) are in wave_ops.h, which every
// kernel unit includes, with or without this header.  Everything lives in an anonymous namespace: every unit gets its own copy.
#ifndef REJIT_AMD_KERNEL_UTIL_H_
#define REJIT_AMD_KERNEL_UTIL_H_

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>

#include "device_program.h"
#include "kernels.h"
#include "wave_ops.h"

namespace rejit_amd {

namespace {

constexpr int kChunk = 1024;  // bytes per wave iteration: 64 lanes x 16 B

// Hit offsets of one wave go to the wave's own REGION of the hit list: region w = wave w,
// `cap` entries, filled in position order, no atomics.  Every wave owns a contiguous span of
// the text, so the regions concatenated in wave order are globally sorted by offset -- which
// is what lets the rest of the pipeline run without a sort.
//
// History (all measured, tools/ab_probe.py): appending chunk by chunk to one global counter ran
// into the ~90 atomics/us limit of a single address (11 ns per chunk-with-hits); staging 256
// hits per wave in LDS fixed that but cost one returning atomic per wave, whose latency under
// a saturated memory pipeline (~20 us) made the kernel slower the more waves it had; 16 sharded
// counters helped little.  Regions need no atomic at all.
struct RegionHits {
  uint64_t* slots;   // this wave's region
  uint32_t cap;
  uint32_t count;    // wave-uniform; keeps counting past cap so the host can size a retry

  // bit j of mask16 <-> offset at + j - bias; appended in position order
  __device__ __forceinline__ void push_bits(uint32_t mask16, uint64_t at, uint64_t bias) {
    const int lane = lane_id();
    const uint32_t cnt = __popc(mask16);
    uint32_t inc, total;
    uint64_t hitters = __ballot(cnt != 0);
    if (__popcll(hitters) <= 4) {
      // the usual case in window scans: a handful of lanes hold hits -- walk them (scalar loop,
      // v_readlane) instead of a 6-step wave scan
      uint32_t before = 0;
      total = 0;
      while (hitters) {
        const int l = __builtin_ctzll(hitters);
        hitters &= hitters - 1;
        const uint32_t c = __builtin_amdgcn_readlane(cnt, l);
        before += lane > l ? c : 0u;
        total += c;
      }
      inc = before + cnt;
    } else {
      inc = cnt;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
      }
      total = __shfl(inc, kWave - 1);
    }
    uint32_t idx = count + inc - cnt;
    while (mask16) {
      const int j = __ffs(static_cast<int>(mask16)) - 1;
      mask16 &= mask16 - 1;
      if (idx < cap) slots[idx] = at + j - bias;
      idx++;
    }
    count += total;
  }
};

// geometry shared by the scan kernels: wave w owns chunks [c0, c1)
struct WaveSpan {
  uint64_t c0, c1;
};

__device__ __forceinline__ uint64_t scalar_wave_index() {
  // as a scalar, so that chunk addresses and loop branches are wave-uniform
  return __builtin_amdgcn_readfirstlane(
      static_cast<uint32_t>((static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6));
}

__device__ __forceinline__ WaveSpan wave_span(const ScanParams& a, uint64_t wave, uint64_t first_chunk,
                                              uint64_t end_chunk) {
  WaveSpan w;
  w.c0 = first_chunk + wave * a.span_chunks;
  w.c1 = w.c0 + a.span_chunks;
  if (w.c0 > end_chunk) w.c0 = end_chunk;
  if (w.c1 > end_chunk) w.c1 = end_chunk;
  return w;
}

// 16 B of the lane + the 8 B that follow, guarded against the end of the text (tail chunk).
__device__ __forceinline__ void load_guarded(const uint8_t* text, uint64_t n, uint64_t at, uint32_t d[6]) {
#pragma unroll
  for (int q = 0; q < 6; q++) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t p = at + 4 * q + k;
      if (p < n) v |= static_cast<uint32_t>(text[p]) << (8 * k);
    }
    d[q] = v;
  }
}

}  // namespace

}  // namespace rejit_amd
#endif
