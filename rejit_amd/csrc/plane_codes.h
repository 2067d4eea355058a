// rejit_amd/csrc/plane_codes.h -- the 2-bit symbol codes the plane kernels (plane_scan.hip, plane_count.hip) compare
// instead of bytes: which two bits of a byte are its code is a launch constant of the pattern set.
#ifndef REJIT_AMD_PLANE_CODES_H_
#define REJIT_AMD_PLANE_CODES_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rejit_amd {

namespace {

struct PlaneCodes {
  uint32_t cmask;   // 0x03030303 << code_shift
  uint32_t shift;   // code_shift
};

// the 2-bit codes of a dword's four bytes as one byte (times 2^shift)
__device__ __forceinline__ uint32_t codes4(uint32_t d, const PlaneCodes& k) {
  return __builtin_amdgcn_udot4(d & k.cmask, 0x40100401u, 0u, false);
}

}  // namespace

}  // namespace rejit_amd
#endif
