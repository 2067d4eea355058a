// rejit_amd/csrc/plane_network.h -- two small pieces of the plane kernels' per-block arithmetic (plane_count.hip) that are
// written as fixed sequences of three-input operations, not as expressions: left to the optimiser, both come out longer.
//   at_most_one_miss   "at most one of the eight window bytes does not fit": nine v_bitop3_b32, four deep (the recurrence
//                      Z' = Z & e, O' = Z | (O & e) it replaces compiled to 12-14 operations in a chain eight deep)
//   join_codes16       the codes of four dwords joined into one word: a shift and three v_lshl_or_b32
// On the device the operations are the instructions themselves; off the device (a host compile of the same header: the
// stand-alone test program under tests/support) every three-input operation is evaluated bit by bit from the SAME truth-table
// constant, so that a host test checks the immediates the kernels execute and not a second formula.
// Plain C++ apart from the two attributes: no HIP header is needed to include it.
#ifndef REJIT_AMD_PLANE_NETWORK_H_
#define REJIT_AMD_PLANE_NETWORK_H_

#include <cstdint>

#if defined(__HIPCC__)
#define RJ_PLANE_NET_FN __host__ __device__ __forceinline__
#else
#define RJ_PLANE_NET_FN inline
#endif

namespace rejit_amd {

// One three-input bitwise operation.  T is its truth table in v_bitop3_b32's convention: bit (4 x + 2 y + z) of T is the result
// for the input bits x, y, z (as masks: x = 0xF0, y = 0xCC, z = 0xAA -- `x & y & z` is 0x80, the majority 0xE8).
template <unsigned T>
RJ_PLANE_NET_FN uint32_t bitop3(uint32_t x, uint32_t y, uint32_t z) {
  static_assert(T < 256, "eight table entries");
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
  return static_cast<uint32_t>(__builtin_amdgcn_bitop3_b32(x, y, z, T));
#else
  uint32_t r = 0;
  for (int bit = 0; bit < 32; bit++) {
    const uint32_t row = (((x >> bit) & 1u) << 2) | (((y >> bit) & 1u) << 1) | ((z >> bit) & 1u);
    r |= ((T >> row) & 1u) << bit;
  }
  return r;
#endif
}

// e0..e7: bit p set = window byte i fits at position p.  -> bit p set = at most one of the eight is clear at p.
// Three groups (e0 e1 e2), (e3 e4 e5), (e6 e7): a group's "all fit" (a) and "at most one misses" (t: the majority of three).
// The whole has at most one miss when one group has at most one and the other two have none.
RJ_PLANE_NET_FN uint32_t at_most_one_miss(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, uint32_t e4, uint32_t e5, uint32_t e6, uint32_t e7) {
  const uint32_t a1 = bitop3<0x80>(e0, e1, e2), t1 = bitop3<0xE8>(e0, e1, e2);
  const uint32_t a2 = bitop3<0x80>(e3, e4, e5), t2 = bitop3<0xE8>(e3, e4, e5);
  const uint32_t p = bitop3<0x80>(a2, e6, e7);   // groups two and three without a miss
  const uint32_t u = bitop3<0x80>(t2, e6, e7);   // at most one in group two, none in three
  const uint32_t w = bitop3<0xE0>(a2, e6, e7);   // a2 & (e6 | e7): none in group two, at most one in three
  const uint32_t s = bitop3<0xE0>(a1, u, w);     // a1 & (u | w): none in group one, at most one behind it
  return bitop3<0xEA>(t1, p, s);                 // (t1 & p) | s
}

// r0..r3: the codes of a piece's four dwords, each one byte times 2^s (codes4 of plane_codes.h).  -> bits 2k, 2k + 1 = byte k.
// (s is wave-uniform, 0..6: the three left shifts' amounts are scalars the compiler keeps across the streaming loop)
RJ_PLANE_NET_FN uint32_t join_codes16(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t s) {
  const uint32_t up8 = 8 - s, up16 = 16 - s, up24 = 24 - s;
  uint32_t c = r0 >> s;
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
  // (the empty statements keep the chain a chain: without them the compiler shifts the parts separately and joins them with a
  // three-input OR, five operations)
  c |= r1 << up8;
  asm("" : "+v"(c));
  c |= r2 << up16;
  asm("" : "+v"(c));
  c |= r3 << up24;
#else
  c |= r1 << up8;
  c |= r2 << up16;
  c |= r3 << up24;
#endif
  return c;
}

}  // namespace rejit_amd
#endif
