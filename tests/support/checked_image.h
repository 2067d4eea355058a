// tests/support/checked_image.h -- TEST-ONLY: what the drivers of the calls that emit through record_frame.h's emit_chunks
// share (format_exec.cc, time_format_exec.cc, zip_exec.cc, csv_format_exec.cc): the chunk's image, every byte of it written
// once at the most and inside the chunk, and the walk over the chunks of an output -- a chunk's bounds, its rows from the pair
// of searches, every output byte below the limit stored exactly once and none at or beyond out_cap.
#ifndef REJIT_AMD_TESTS_CHECKED_IMAGE_H_
#define REJIT_AMD_TESTS_CHECKED_IMAGE_H_

#include <stdint.h>

#include <vector>

#include "../../rejit_amd/csrc/record_pack.h"

namespace {

// The image of the chunk [c0, c1) of the output (the kernel's LDS: `room` bytes), preset with the fill byte.
struct CheckedImage {
  uint64_t c0, c1;
  std::vector<uint8_t> bytes, once;
  bool twice = false, left_range = false;
  uint64_t streamed = 0, from_image = 0;   // groups of 16, by where their bytes came from
  CheckedImage(uint64_t room, uint32_t fill, uint64_t c0_, uint64_t c1_) : c0(c0_), c1(c1_), bytes(room, static_cast<uint8_t>(fill)), once(room, 0) {}
  // the emit's put: byte `in_image` of the chunk
  void put(uint64_t in_image, uint32_t byte) {
    if (in_image >= bytes.size() || in_image >= c1 - c0 || byte > 255) {
      left_range = true;
      return;
    }
    if (once[in_image]) twice = true;
    once[in_image] = 1;
    bytes[in_image] = static_cast<uint8_t>(byte);
  }
  // The chunk as the emit stores it, in steps of 16 bytes: got[i] = byte c0 + i.  registers(p, w) -> true: the 16 bytes at p
  // are w's, not the image's -- no byte of the image may have been written under such a group.
  template <class Registers>
  void store(const Registers& registers, std::vector<uint8_t>* got) {
    got->assign(c1 - c0, 0);
    for (uint64_t p = c0; p < c1; p += rejit_amd::pack::kGroupBytes) {
      uint32_t w[4] = {0, 0, 0, 0};
      const uint64_t in_group = c1 - p < rejit_amd::pack::kGroupBytes ? c1 - p : rejit_amd::pack::kGroupBytes;
      if (registers(p, w)) {
        streamed++;
        for (uint64_t b = 0; b < in_group; b++)
          if (once[p - c0 + b]) twice = true;
      } else {
        from_image++;
        for (uint64_t b = 0; b < in_group; b++) w[b >> 2] |= static_cast<uint32_t>(bytes[p - c0 + b]) << (8 * (b & 3));
      }
      for (uint64_t b = 0; b < in_group; b++) (*got)[p - c0 + b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
    }
  }
  void store(std::vector<uint8_t>* got) {
    store([](uint64_t, uint32_t*) { return false; }, got);
  }
};

// The walk over the chunks of `chunk` bytes of out[0, min(total, out_cap)): make(c0, c1, j0, j1, &got) makes the bytes of
// chunk [c0, c1) from the rows [j0, j1) the two searches give (j1 <= k), got[i] = byte c0 + i, and the walk stores them.
// -> the chunks; -1: a search left the table, make left a byte out, or an output byte was stored twice, at or beyond out_cap,
// or never.
template <class Make>
inline long walk_chunks(const rejit_amd::pack::View& table, uint64_t k, uint64_t total, uint64_t chunk, uint8_t* out, uint64_t out_cap, const Make& make) {
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint64_t n_chunks = (limit + chunk - 1) / chunk;
  std::vector<uint8_t> got, stored(limit, 0);
  for (uint64_t c = 0; c < n_chunks; c++) {
    const uint64_t c0 = c * chunk;
    const uint64_t c1 = c0 + chunk < limit ? c0 + chunk : limit;
    const uint64_t j0 = rejit_amd::pack::chunk_first_row(table, k, c0);
    const uint64_t e = rejit_amd::pack::chunk_end_row(table, k, 0, c1);
    const uint64_t j1 = e > j0 ? e : j0;
    if (j1 > k) return -1;
    make(c0, c1, j0, j1, &got);
    if (got.size() != c1 - c0) return -1;
    for (uint64_t p = c0; p < c1; p++) {
      if (p >= out_cap || stored[p]) return -1;
      stored[p] = 1;
      out[p] = got[p - c0];
    }
  }
  for (uint64_t p = 0; p < limit; p++)
    if (!stored[p]) return -1;
  return static_cast<long>(n_chunks);
}

}  // namespace
#endif
