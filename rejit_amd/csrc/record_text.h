// rejit_amd/csrc/record_text.h -- device helpers the record kernels share (record_pack.hip, record_replace.hip): the 64-bit
// wave scan of their plans and the 16-byte read of a device text at any alignment.  Device code only; everything lives in an
// anonymous namespace: every unit gets its own copy.
#ifndef REJIT_AMD_RECORD_TEXT_H_
#define REJIT_AMD_RECORD_TEXT_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_util.h"
#include "stream_load.h"
#include "wave_ops.h"

namespace rejit_amd {

namespace {

// 64-bit inclusive prefix sum over the wave from wave_ops.h's 32-bit one: three pieces of at most 22 bits (64 x 2^22 fits)
__device__ __forceinline__ uint64_t wave_inclusive_sum64(uint64_t x) {
  const uint64_t a = wave_inclusive_sum(static_cast<uint32_t>(x) & 0x3FFFFFu);
  const uint64_t b = wave_inclusive_sum(static_cast<uint32_t>(x >> 22) & 0x3FFFFFu);
  const uint64_t c = wave_inclusive_sum(static_cast<uint32_t>(x >> 44));
  return a + (b << 22) + (c << 44);
}

// text[s, s + 16), all of it inside [0, n): two aligned 16-byte loads around it and a funnel shift by the source's
// misalignment, or ONE load when source and destination are aligned alike.  That one is a streaming read (stream_load.h:
// every cache line is asked for by one instruction); the two loads of the misaligned case ask for a line twice -- a lane's
// second block is its neighbour's first -- and keep the default policy.  At the text's two ends, where an aligned block
// would reach outside [0, n), kernel_util.h's guarded load reads the 16 bytes one by one.
struct DeviceText {
  const uint8_t* text;
  uint64_t n;
  __device__ __forceinline__ void load16(uint64_t s, uint32_t w[4]) const {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(text) + s;
    const uint32_t mis = static_cast<uint32_t>(addr & 15u);
    if (mis == 0) {
      const uint4 v = stream_load16(text + s);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      return;
    }
    if (s < mis || s - mis + 32 > n) {   // an aligned block would begin before the text or end behind it
      uint32_t d[6];
      load_guarded(text, n, s, d);
      w[0] = d[0], w[1] = d[1], w[2] = d[2], w[3] = d[3];
      return;
    }
    const uint4* a = reinterpret_cast<const uint4*>(text + (s - mis));
    const uint4 lo = a[0], hi = a[1];
    const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    // whole words first (a select over wave-divergent `mis`, no indexed registers), then the bytes
    uint32_t y[5];
    const uint32_t ws = mis >> 2;
#pragma unroll
    for (int i = 0; i < 5; i++) y[i] = ws == 0 ? x[i] : ws == 1 ? x[i + 1] : ws == 2 ? x[i + 2] : x[i + 3];
    const uint32_t bs = mis & 3u;
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = __builtin_amdgcn_alignbyte(y[i + 1], y[i], bs);
  }
  __device__ __forceinline__ uint32_t byte(uint64_t s) const { return s < n ? text[s] : 0u; }
};

}  // namespace

}  // namespace rejit_amd
#endif
