// tests/support/checked_text.h -- TEST-ONLY: what the drivers of the record headers share: the text they read (the Text policy
// of record_pack.h's copy and of record_rows.h: pack_exec.cc, replace_exec.cc, group_exec.cc, sort_exec.cc, lookup_exec.cc),
// every access checked against its range, and the store of a 16-byte group of the pack and the replace, checked against the
// output's capacity.
#ifndef REJIT_AMD_TESTS_CHECKED_TEXT_H_
#define REJIT_AMD_TESTS_CHECKED_TEXT_H_

#include <stdint.h>

#include "../../rejit_amd/csrc/record_pack.h"

namespace {

// the byte at offset s of a text that exists as numbers only (CheckedText with text == nullptr)
inline uint8_t synth(uint64_t s) { return static_cast<uint8_t>((s * 131u + (s >> 8) * 7u + (s >> 32)) & 0xFFu); }

struct CheckedText {
  const uint8_t* text;
  uint64_t n;
  mutable bool left_range = false;
  mutable uint64_t loads16 = 0, byte_reads = 0, guarded = 0;
  uint32_t at(uint64_t s) const {
    if (s >= n) {
      left_range = true;
      return 0;
    }
    return text ? text[s] : synth(s);
  }
  // (all 16 bytes inside the text: that is the contract of the device's load16)
  void load16(uint64_t s, uint32_t w[4]) const {
    loads16++;
    for (int i = 0; i < 4; i++) w[i] = 0;
    for (uint32_t b = 0; b < 16; b++) w[b >> 2] |= at(s + b) << (8 * (b & 3));
  }
  // the bytes below n, zero behind them
  void load16_guarded(uint64_t s, uint32_t w[4]) const {
    guarded++;
    for (int i = 0; i < 4; i++) w[i] = 0;
    for (uint32_t b = 0; b < 16; b++)
      if (s + b < n) w[b >> 2] |= at(s + b) << (8 * (b & 3));
  }
  uint32_t byte(uint64_t s) const {
    byte_reads++;
    return at(s);
  }
};

// The group w of output bytes [p, p + 16) below `limit` goes to out[p - window0, ...) (out stands for the output from window0
// on).  False: the kernel's store would have left [0, out_cap).
inline bool store_group(uint8_t* out, uint64_t window0, uint64_t p, uint64_t limit, uint64_t out_cap, const uint32_t w[4]) {
  const uint32_t bytes = rejit_amd::pack::group_store_bytes(p, limit);
  if (bytes == 0 || bytes > rejit_amd::pack::kGroupBytes || p + bytes > out_cap) return false;
  for (uint32_t b = 0; b < bytes; b++) out[p - window0 + b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
  return true;
}

}  // namespace
#endif
