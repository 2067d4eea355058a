// tests/support/plane_network_exec.cc -- stand-alone host check of rejit_amd/csrc/plane_network.h (tests/test_plane_network.py).
// Off the device the header evaluates every three-input operation bit by bit from the truth-table constant the kernels hand to
// v_bitop3_b32, so what is checked here are the immediates themselves:
//   1. at_most_one_miss against "at most one of e0..e7 is 0", all 256 inputs, (a) one input in all 32 bit positions of a word,
//      (b) 32 DIFFERENT inputs in the 32 bit positions -- in order and in shuffled orders --, so that a wrong immediate cannot
//      hide behind uniform bits;
//   2. the five truth tables against what their comments say they are;
//   3. join_codes16 over codes4 (v_dot4_u32_u8 restated) against the per-byte definition -- bits 2k, 2k + 1 of the word = bits
//      shift, shift + 1 of byte k -- for every code_shift 0..6 on random 16-byte pieces.
// Prints `checked N cases` and exits 0, or the first failures and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../rejit_amd/csrc/plane_network.h"

using rejit_amd::at_most_one_miss;
using rejit_amd::bitop3;
using rejit_amd::join_codes16;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return static_cast<uint32_t>((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int failures = 0;
static long checked = 0;
static void fail(const char* what, unsigned a, unsigned b, unsigned got, unsigned want) {
  if (failures++ < 10) std::printf("FAIL %s (%u, %u): got %08x want %08x\n", what, a, b, got, want);
}

// bit i of `input` = window byte i fits
static bool at_most_one_zero(unsigned input) { return __builtin_popcount(~input & 0xFFu) <= 1; }

// 32 inputs, one per bit position -> the network's word against the definition's
static void check_word(const unsigned inputs[32], const char* what, unsigned tag) {
  uint32_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0}, want = 0;
  for (int p = 0; p < 32; p++) {
    for (int i = 0; i < 8; i++) e[i] |= ((inputs[p] >> i) & 1u) << p;
    want |= (at_most_one_zero(inputs[p]) ? 1u : 0u) << p;
  }
  const uint32_t got = at_most_one_miss(e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]);
  if (got != want) fail(what, tag, inputs[0], got, want);
  checked++;
}

// the dword's four 2-bit codes as one byte, times 2^shift (plane_codes.h: codes4 -- v_dot4_u32_u8 of the masked dword and
// 0x40100401, the sum of the four byte products)
static uint32_t codes4_host(uint32_t d, uint32_t shift) {
  const uint32_t m = d & (0x03030303u << shift), w = 0x40100401u;
  uint32_t sum = 0;
  for (int k = 0; k < 4; k++) sum += ((m >> (8 * k)) & 0xFFu) * ((w >> (8 * k)) & 0xFFu);
  return sum;
}

int main() {
  // 1a: uniform words
  for (unsigned v = 0; v < 256; v++) {
    unsigned inputs[32];
    for (int p = 0; p < 32; p++) inputs[p] = v;
    check_word(inputs, "uniform", v);
  }
  // 1b: 32 different inputs per word, in order ...
  for (unsigned r = 0; r < 8; r++) {
    unsigned inputs[32];
    for (unsigned p = 0; p < 32; p++) inputs[p] = 32 * r + p;
    check_word(inputs, "in order", r);
  }
  // ... and shuffled: every round permutes all 256 inputs over eight words
  for (unsigned round = 0; round < 64; round++) {
    unsigned perm[256];
    for (unsigned i = 0; i < 256; i++) perm[i] = i;
    for (unsigned i = 255; i > 0; i--) {
      const unsigned j = rnd() % (i + 1), t = perm[i];
      perm[i] = perm[j];
      perm[j] = t;
    }
    for (unsigned r = 0; r < 8; r++) check_word(perm + 32 * r, "shuffled", round);
  }
  // 2: the tables
  for (unsigned round = 0; round < 64; round++) {
    const uint32_t x = rnd(), y = rnd(), z = rnd();
    if (bitop3<0x80>(x, y, z) != (x & y & z)) fail("0x80", round, 0, bitop3<0x80>(x, y, z), x & y & z);
    if (bitop3<0xE8>(x, y, z) != ((x & y) | (x & z) | (y & z))) fail("0xE8", round, 0, bitop3<0xE8>(x, y, z), (x & y) | (x & z) | (y & z));
    if (bitop3<0xE0>(x, y, z) != (x & (y | z))) fail("0xE0", round, 0, bitop3<0xE0>(x, y, z), x & (y | z));
    if (bitop3<0xEA>(x, y, z) != ((x & y) | z)) fail("0xEA", round, 0, bitop3<0xEA>(x, y, z), (x & y) | z);
    if (bitop3<0xCA>(x, y, z) != ((x & y) | (~x & z))) fail("0xCA", round, 0, bitop3<0xCA>(x, y, z), (x & y) | (~x & z));
    checked += 5;
  }
  // 3: the codes of 16 bytes
  for (uint32_t shift = 0; shift <= 6; shift++) {
    for (unsigned round = 0; round < 2000; round++) {
      uint8_t piece[16];
      for (int k = 0; k < 16; k++) piece[k] = round < 16 ? (k == static_cast<int>(round) ? 0xFFu : 0u) : static_cast<uint8_t>(rnd());
      uint32_t d[4];
      std::memcpy(d, piece, 16);   // (little-endian, as the device: byte k of the piece = bits 8 (k & 3) of dword k >> 2)
      const uint32_t got = join_codes16(codes4_host(d[0], shift), codes4_host(d[1], shift), codes4_host(d[2], shift), codes4_host(d[3], shift), shift);
      uint32_t want = 0;
      for (int k = 0; k < 16; k++) want |= ((piece[k] >> shift) & 3u) << (2 * k);
      if (got != want) fail("codes16", shift, round, got, want);
      checked++;
    }
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("checked %ld cases\n", checked);
  return 0;
}
