// rejit_amd/csrc/plane_args.h -- the launch arguments of the plane kernels (plane_scan.hip, plane_count.hip) that are pure
// arithmetic on a plan and a range: the three encodings of a plan's base windows, the window positions and 2-KiB blocks of
// the starts [sb, se) and their split over the regions, a pattern's own window range -- and the chunk range engine.hip's
// run_range scans.  Host only, no HIP: multi_pattern.hip and engine.hip fill the kernels' structs from these,
// tests/test_plane_args.py compiles them with g++.
#pragma once

#include <algorithm>
#include <cstdint>

namespace rejit_amd {

// The 2-bit symbol code of base b's window byte i.  Kernels that take more bases than the plan has get base 0 again.
inline uint32_t plane_code(const uint8_t base[][8], uint32_t n_bases, uint32_t code_shift, uint32_t b, uint32_t i) {
  return (static_cast<uint32_t>(base[b < n_bases ? b : 0][i]) >> code_shift) & 3u;
}

// PlaneParams / PlaneGParams: lo[b][i] / hi[b][i] = 0 when the low / high bit of the code is 1, else ~0
inline void plane_masks(const uint8_t base[][8], uint32_t n_bases, uint32_t code_shift, uint32_t rows, uint32_t lo[][8], uint32_t hi[][8]) {
  for (uint32_t b = 0; b < rows; b++)
    for (uint32_t i = 0; i < 8; i++) {
      const uint32_t code = plane_code(base, n_bases, code_shift, b, i);
      lo[b][i] = (code & 1u) ? 0u : ~0u;
      hi[b][i] = (code & 2u) ? 0u : ~0u;
    }
}

// PlaneCountParams::mask_bits (two bases): bit 16 b + 2 i / + 1 is set when the low / high bit of the code is 0
inline uint32_t plane_mask_bits(const uint8_t base[][8], uint32_t n_bases, uint32_t code_shift) {
  uint32_t bits = 0;
  for (uint32_t b = 0; b < 2; b++)
    for (uint32_t i = 0; i < 8; i++) {
      const uint32_t code = plane_code(base, n_bases, code_shift, b, i);
      if (!(code & 1u)) bits |= 1u << (16 * b + 2 * i);
      if (!(code & 2u)) bits |= 1u << (16 * b + 2 * i + 1);
    }
  return bits;
}

// PlaneCountGParams::idx: the code itself, or 4 for a byte beyond the n_cmp compared ones (always fits)
inline void plane_idx(const uint8_t base[][8], uint32_t n_bases, uint32_t code_shift, uint32_t n_cmp, uint32_t rows, uint32_t idx[][8]) {
  for (uint32_t b = 0; b < rows; b++)
    for (uint32_t i = 0; i < 8; i++) idx[b][i] = i < n_cmp ? plane_code(base, n_bases, code_shift, b, i) : 4u;
}

// The window positions [wlo, whi) that can belong to a start in [sb, se), sb < se -- windows of n_cmp compared bytes at the offsets
// min_offset .. max_offset inside a match -- and the 2-KiB blocks [first_block, end_block) that hold them.
struct PlaneBlocks {
  uint64_t wlo = 0, whi = 0, first_block = 0, end_block = 0;
  uint64_t blocks() const { return end_block - first_block; }
  // the list kernels' regions can hold this many candidates at the most: every position of the longest span
  uint64_t span_pairs(uint32_t n_regions) const { return std::max<uint64_t>((blocks() + n_regions - 1) / n_regions, 1); }
};
inline PlaneBlocks plane_blocks(uint64_t n, uint64_t sb, uint64_t se, uint32_t min_offset, uint32_t max_offset, uint32_t n_cmp) {
  PlaneBlocks r;
  const uint64_t last_w = n >= n_cmp ? n - n_cmp + 1 : 0;
  r.wlo = sb + min_offset;
  r.whi = std::min<uint64_t>(se + max_offset, last_w);
  r.first_block = r.wlo / 2048;
  r.end_block = r.whi > r.wlo ? (r.whi + 2047) / 2048 : r.first_block;
  return r;
}

// Region r takes span_blocks blocks, the first span_extra regions one more, one after the other from first_block.
inline void plane_split(uint64_t blocks, uint32_t n_regions, uint64_t* span_blocks, uint32_t* span_extra) {
  *span_blocks = blocks / n_regions;
  *span_extra = static_cast<uint32_t>(blocks % n_regions);
}

// ScanParams / TrainParams: one pattern's own window positions [wlo, whi), never reversed
inline void window_range(uint64_t n, uint64_t sb, uint64_t se, uint32_t win_offset, uint32_t win_len, uint64_t* wlo, uint64_t* whi) {
  const uint64_t last_w = n >= win_len ? n - win_len + 1 : 0;
  *wlo = sb + win_offset;
  *whi = std::max(std::min<uint64_t>(se + win_offset, last_w), *wlo);
}

// engine.hip, run_range: what one pattern's scan kernel walks for the starts [sb, se) -- the window positions [wlo, whi), never
// reversed, and the 1-KiB chunks [first_chunk, end_chunk) that hold them.  A window position w belongs to the starts
// w - max_offset .. w - min_offset (fixed windows: both are the window's offset; floating ones: float_min and float_max) and
// has win_len bytes of text behind it; behind an unbounded prefix a start's hit may lie anywhere up to the last position.
// Dense mode (no windows) walks the chunks of the starts themselves and has no window positions.
struct ChunkRange {
  uint64_t wlo = 0, whi = 0, first_chunk = 0, end_chunk = 0;
  uint64_t chunks() const { return end_chunk > first_chunk ? end_chunk - first_chunk : 0; }
};
inline ChunkRange chunk_range(uint64_t n, uint64_t sb, uint64_t se, bool windows, uint32_t min_offset, uint32_t max_offset, uint32_t win_len,
                              bool behind) {
  ChunkRange r;
  if (windows) {
    const uint64_t last_w = n >= win_len ? n - win_len + 1 : 0;  // a window must fit: w + len <= n
    r.wlo = sb + min_offset;
    r.whi = std::max(behind ? last_w : std::min<uint64_t>(se + max_offset, last_w), r.wlo);
    r.first_chunk = r.wlo / 1024;
    r.end_chunk = (r.whi + 1023) / 1024;
  } else {
    r.first_chunk = sb / 1024;
    r.end_chunk = (se + 1023) / 1024;
  }
  return r;
}

}  // namespace rejit_amd
