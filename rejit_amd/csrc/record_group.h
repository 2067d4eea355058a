// rejit_amd/csrc/record_group.h -- the arithmetic of rj_scan_records_group (record_group.hip): the rows of a record table grouped
// by their BYTES -- Arrow's dictionary_encode / value_counts, `sort | uniq -c` in order of first appearance -- exactly, with no
// probabilistic equality.  Host and device code: the CPU tests drive exactly these functions (tests/support/group_exec.cc)
// through a Text and a Mem policy, as the kernels do.  What a row's bytes are -- the limits, the guarded 16-byte groups, their
// equality, the Text policy -- is record_rows.h's.
//
// Row j is text[rb, re) of record r(j).  Its key:
//     hash(row) = finalize(len, sum over g of mix(words of 16-byte group g, g))       (the sum mod 2^64)
// groups counted from the row's begin, the last one zero-padded beyond the row's end.  A SUM, so that any assignment of groups
// to lanes, waves or iterations gives the same value; the bytes beyond the row's end are masked, so the value depends neither
// on the row's alignment in the text nor on what follows it.  Correctness never depends on the quality of mix: rows are equal
// when their lengths, their stored hashes AND their bytes are equal.
//
// The table: open addressing, linear probing, T = table_slots(k) >= 2k slots of one 64-bit word -- kEmpty or a row index.
// Insert row j with hash h from slot h & (T - 1) on (find_slot):
//     empty            compare-and-swap to j; on failure re-read the SAME slot (it is occupied now)
//     held by row i    equal(i, j): min(slot, j), count[slot] += 1, slot_of[j] = slot, done;  else the next slot
// Two invariants make this exact under ANY interleaving of the rows' steps:
//     (1) a slot is never emptied: kEmpty -> a row is the only transition out of kEmpty, and nothing writes kEmpty;
//     (2) the STRING a slot stands for never changes: the only other write is min(slot, j) with a row j equal to the row the
//         slot names, so only which of its equal rows is named changes.
// By (1) and (2) a probe that passed a slot would pass it at any later time too, and an empty slot ends every chain (at most k
// of the T >= 2k slots are ever taken), so every string ends in exactly one slot, whoever came first.  No step waits for
// another row's progress -- a failed compare-and-swap is followed by a read of a slot that is now occupied -- so there is no
// lock, no spin and no time-out.  Behind all inserts slot[s] is the SMALLEST row of its string and count[s] their number.
//
// Numbering: row j is a representative when slot[slot_of[j]] == j; an exclusive prefix sum of that flag over the rows numbers
// the groups in order of first appearance: rep[g] = j, group_count[g] = count[s], slot_group[s] = g; group[j] =
// slot_group[slot_of[j]] in a last pass.
#ifndef REJIT_AMD_RECORD_GROUP_H_
#define REJIT_AMD_RECORD_GROUP_H_

#include <stdint.h>

#include "record_pack.h"
#include "record_rows.h"

namespace rejit_amd {
namespace group {

constexpr uint64_t kEmpty = ~0ull;
constexpr uint64_t kMinSlots = 64;
constexpr uint32_t kLongBytes = 64;              // rows longer than this are walked by a wave, not a lane (RJ_GROUP_LONG_BYTES)
constexpr uint32_t kLenSaturated = 0xFFFFFFFFu;  // the stored length of a row of 2^32 - 1 bytes or more: its table has the length

// ---------------------------------------------------------------------------------------------------------------- limits
// A call takes rows_fit(k) rows: rows and slots share 32-bit words in the scratch (slot_of, slot_group, counts).  (record_rows.h's
// rows_fit and n_groups under this header's names: one definition, the names its callers have always used.)
using rows::n_groups;
using rows::rows_fit;
// max(64, the next power of two >= 2k); k < 2^31, so at most 2^32 slots and a slot's index fits 32 bits
RJ_PACK_HD inline uint64_t table_slots(uint64_t k) {
  uint64_t t = kMinSlots;
  while (t < 2 * k) t <<= 1;
  return t;
}
// the scratch of a call, in bytes from the buffer's begin (every part 16-byte aligned): the table and slot_count (T words
// each), h, len, slot_of, the list of long rows (k words each).  slot_group takes slot_count's place: a slot's count is read
// once, by its representative, which then writes the slot's group there.  12 bytes per slot, 20 per row: 44 .. 68 per row.
struct Layout {
  uint64_t table, slot_count, slot_group, hash, len, slot_of, long_list, bytes;
};
RJ_PACK_HD inline Layout layout(uint64_t k) {
  using rows::align16;
  const uint64_t T = table_slots(k);
  Layout l;
  l.table = 0;
  l.slot_count = l.table + 8 * T;
  l.slot_group = l.slot_count;
  l.hash = l.slot_count + 4 * T;
  l.len = l.hash + align16(8 * k);
  l.slot_of = l.len + align16(4 * k);
  l.long_list = l.slot_of + align16(4 * k);
  l.bytes = l.long_list + align16(4 * k);
  return l;
}
RJ_PACK_HD inline uint32_t stored_len(uint64_t len) { return len >= kLenSaturated ? kLenSaturated : static_cast<uint32_t>(len); }

// ---------------------------------------------------------------------------------------------------------------- hash
// multiply / xor-shift over the four little-endian words of group g
RJ_PACK_HD inline uint64_t mix(const uint32_t w[4], uint64_t g) {
  const uint64_t a = static_cast<uint64_t>(w[0]) | (static_cast<uint64_t>(w[1]) << 32);
  const uint64_t b = static_cast<uint64_t>(w[2]) | (static_cast<uint64_t>(w[3]) << 32);
  uint64_t x = (a ^ (0x9E3779B97F4A7C15ull + g * 0xD6E8FEB86659FD93ull)) * 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  uint64_t y = (b ^ (0xC2B2AE3D27D4EB4Full + g * 0xA0761D6478BD642Full)) * 0x94D049BB133111EBull;
  y ^= y >> 29;
  uint64_t z = (x + (y << 23 | y >> 41)) * 0xFF51AFD7ED558CCDull;
  return z ^ (z >> 31);
}
RJ_PACK_HD inline uint64_t finalize(uint64_t len, uint64_t sum) {
  uint64_t z = sum ^ (len * 0xE7037ED1A0B428DBull + 0x8EBC6AF09C88C6E3ull);
  z ^= z >> 33;
  z *= 0xC4CEB9FE1A85EC53ull;
  z ^= z >> 29;
  z *= 0x589965CC75374CC3ull;
  return z ^ (z >> 32);
}
// RJ_GROUP_HASH_BITS: only the low `bits` bits of every hash are kept (and stored: the equality check sees the same value)
RJ_PACK_HD inline uint64_t keep_bits(uint64_t h, uint32_t bits) { return bits >= 64 ? h : h & ((1ull << bits) - 1); }

// the sum of mix over the groups g0, g0 + stride, ... below g_end: a lane's, a wave iteration's or the whole row's share
template <class Text>
RJ_PACK_HD inline uint64_t hash_groups(const Text& text, uint64_t n, uint64_t begin, uint64_t len, uint64_t g0, uint64_t stride, uint64_t g_end) {
  uint64_t sum = 0;
  for (uint64_t g = g0; g < g_end; g += stride) {
    uint32_t w[4];
    rows::load_group(text, n, begin, len, g, w);
    sum += mix(w, g);
  }
  return sum;
}
template <class Text>
RJ_PACK_HD inline uint64_t hash_row(const Text& text, uint64_t n, uint64_t begin, uint64_t len) {
  return finalize(len, hash_groups(text, n, begin, len, 0, 1, rows::n_groups(len)));
}

// group g of two rows of ONE text, of the same length: equal?  (rows::group_equal with both sides in the same text)
template <class Text>
RJ_PACK_HD inline bool group_equal(const Text& text, uint64_t n, uint64_t a, uint64_t b, uint64_t len, uint64_t g) {
  return rows::group_equal(text, n, a, text, n, b, len, g);
}
// ... the groups g0, g0 + stride, ... below g_end (a lane walks a short row with g0 = 0, stride = 1); a row is equal to itself
template <class Text>
RJ_PACK_HD inline bool groups_equal(const Text& text, uint64_t n, uint64_t a, uint64_t b, uint64_t len, uint64_t g0, uint64_t stride, uint64_t g_end) {
  if (a == b) return true;
  return rows::groups_equal(text, n, a, text, n, b, len, g0, stride, g_end);
}

// ---------------------------------------------------------------------------------------------------------------- insert
// Mem is the scratch as a step sees it:
//     slot_load(s)         the slot's word now
//     slot_cas(s, j)       kEmpty -> j; returns what the slot held (kEmpty: the row has taken it)
//     slot_min(s, j), count_add(s, c), set_slot_of(j, s)
//     hash(i), len(i)      what the hash pass stored for row i
// equal(i): rows i and j have equal bytes -- asked only when their stored lengths and hashes are equal.
// find_slot returns the slot of row j's string: one the row has just taken, or one held by an equal row.  In the wave tier
// every lane calls it with wave-uniform answers from Mem, so its branches are wave-uniform.
template <class Mem, class Equal>
RJ_PACK_HD inline uint64_t find_slot(Mem& M, uint64_t j, uint64_t h, uint32_t len32, uint64_t T, const Equal& equal) {
  uint64_t s = h & (T - 1);
  for (;;) {
    const uint64_t cur = M.slot_load(s);
    if (cur == kEmpty) {
      if (M.slot_cas(s, j) == kEmpty) return s;
      continue;   // somebody took it meanwhile: the same slot again, occupied now
    }
    if (M.len(cur) == len32 && M.hash(cur) == h && equal(cur)) return s;
    s = (s + 1) & (T - 1);
  }
}
// `c` rows with the string of slot s, the least of them j, have ended there (c = 1: one row; the wave peel hands in more)
template <class Mem>
RJ_PACK_HD inline void join_slot(Mem& M, uint64_t s, uint64_t j, uint32_t c) {
  M.slot_min(s, j);
  M.count_add(s, c);
}

// ---------------------------------------------------------------------------------------------------------------- numbering
template <class Mem>
RJ_PACK_HD inline bool is_representative(Mem& M, uint64_t j, uint64_t s) { return M.slot_load(s) == j; }

}  // namespace group
}  // namespace rejit_amd
#endif
