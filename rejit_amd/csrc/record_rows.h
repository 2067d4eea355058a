// rejit_amd/csrc/record_rows.h -- what the calls that read the ROWS of a record table say about a row's bytes, in ONE place:
// rj_scan_records_group (record_group.h), rj_scan_records_sort (record_sort.h), rj_scan_records_lookup (record_lookup.h) and
// rj_scan_records_parse (record_parse.h).
// The limits their scratches share, the row a call's j names (or that it names none), 16 bytes of a row at any place of the
// text, a row as zero-padded 16-byte groups, and the equality of two rows group by group.  Host and device code: the CPU
// tests drive exactly these functions (tests/support/) through a Text policy, as the kernels do.
//
// Text: load16(s, w) reads text[s, s + 16) as four little-endian words, all of it inside [0, n); load16_guarded(s, w) reads
// the bytes below n one by one and zeroes behind them -- taken where 16 bytes would reach outside the text (load_at).
#ifndef REJIT_AMD_RECORD_ROWS_H_
#define REJIT_AMD_RECORD_ROWS_H_

#include <stdint.h>

#include "record_pack.h"

namespace rejit_amd {
namespace rows {

constexpr uint64_t kGroupBytes = 16;             // bytes a step reads of a row
constexpr uint64_t kMaxRows = 1ull << 31;        // rows share 32-bit words with slots, positions and segments in the scratches
constexpr uint32_t kMaxLongBytes = 1u << 20;     // the most a lane tier may be asked to take (RJ_GROUP_LONG_BYTES, RJ_SORT_LONG_BYTES)

RJ_PACK_HD inline bool rows_fit(uint64_t k) { return k < kMaxRows; }
RJ_PACK_HD inline uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }
RJ_PACK_HD inline uint64_t n_groups(uint64_t len) { return (len + kGroupBytes - 1) / kGroupBytes; }

// ---------------------------------------------------------------------------------------------------------------- row
// Row j of a call over n_records records of a text of n bytes: record r = indices ? indices[j] : j, the bytes text[rb, re).
// bad: the pack's checks -- r names no record (rec_begin[r] is not read then), or the record is not inside the text; rb, re
// and len() mean nothing then.
struct Row {
  bool bad;
  uint64_t rb, re;
  RJ_PACK_HD uint64_t len() const { return re - rb; }
};
RJ_PACK_HD inline Row resolve(const uint64_t* rec_begin, const uint64_t* rec_end, const uint64_t* indices, uint64_t n_records, uint64_t n, uint64_t j) {
  const uint64_t r = indices ? indices[j] : j;
  Row row{pack::bad_index(r, n_records), 0, 0};
  if (!row.bad) {
    row.rb = rec_begin[r], row.re = rec_end[r];
    row.bad = pack::bad_row(row.rb, row.re, n);
  }
  return row;
}

// ---------------------------------------------------------------------------------------------------------------- groups
// text[s, s + 16) as four little-endian words, zero behind the text's end
template <class Text>
RJ_PACK_HD inline void load_at(const Text& text, uint64_t n, uint64_t s, uint32_t w[4]) {
  if (s + kGroupBytes <= n) text.load16(s, w);
  else text.load16_guarded(s, w);
}
// the bytes at and beyond `valid` (1..16) of a group become zero
RJ_PACK_HD inline void mask_group(uint32_t w[4], uint32_t valid) {
  for (uint32_t i = 0; i < 4; i++) {
    const uint32_t lo = 4 * i;
    if (valid <= lo) w[i] = 0;
    else if (valid < lo + 4) w[i] &= (1u << (8 * (valid - lo))) - 1;
  }
}
// group g (< n_groups(len)) of the row [begin, begin + len), zero-padded beyond the row's end
template <class Text>
RJ_PACK_HD inline void load_group(const Text& text, uint64_t n, uint64_t begin, uint64_t len, uint64_t g, uint32_t w[4]) {
  const uint64_t s = begin + g * kGroupBytes;
  const uint64_t left = len - g * kGroupBytes;
  load_at(text, n, s, w);
  if (left < kGroupBytes) mask_group(w, static_cast<uint32_t>(left));
}

// group g of two rows of the same length, row a in text_a (of n_a bytes) and row b in text_b (of n_b bytes): equal?  Each
// side takes its guarded load at its OWN text's end.
template <class TextA, class TextB>
RJ_PACK_HD inline bool group_equal(const TextA& text_a, uint64_t n_a, uint64_t a, const TextB& text_b, uint64_t n_b, uint64_t b, uint64_t len, uint64_t g) {
  uint32_t x[4], y[4];
  load_group(text_a, n_a, a, len, g, x);
  load_group(text_b, n_b, b, len, g, y);
  return ((x[0] ^ y[0]) | (x[1] ^ y[1]) | (x[2] ^ y[2]) | (x[3] ^ y[3])) == 0;
}
// ... the groups g0, g0 + stride, ... below g_end (a lane walks a short row with g0 = 0, stride = 1; a lane of a wave tier
// with g0 = its number, stride = 64).  No shortcut for a == b: the offsets may belong to two texts (record_group.h's
// one-text form has it).
template <class TextA, class TextB>
RJ_PACK_HD inline bool groups_equal(const TextA& text_a, uint64_t n_a, uint64_t a, const TextB& text_b, uint64_t n_b, uint64_t b, uint64_t len, uint64_t g0,
                                    uint64_t stride, uint64_t g_end) {
  for (uint64_t g = g0; g < g_end; g += stride)
    if (!group_equal(text_a, n_a, a, text_b, n_b, b, len, g)) return false;
  return true;
}

}  // namespace rows
}  // namespace rejit_amd
#endif
