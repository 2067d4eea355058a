// rejit_amd/csrc/record_sort.h -- the arithmetic of rj_scan_records_sort (record_sort.hip): the rows of a record table put in
// the order of their BYTES -- memcmp's order, a proper prefix first, equal rows in ascending j: `LC_ALL=C sort -s`.  Host and
// device code: the CPU tests drive exactly these functions (tests/support/sort_exec.cc) through a Text and a Mem policy, as
// the kernels do.  The limits, the guarded 16-byte load and the Text policy are record_rows.h's.
//
// Row j is text[rb, re) of record r(j).  Its key at depth d, with c = min(len - d, 7) bytes left there:
//     key(row, d) = the c bytes row[d ..] big-endian in the upper 56 bits, zero-padded | c in the low 8 bits
// Unsigned order of the keys is byte order of the windows; the count in the low byte puts "ab" before "ab\0", which a padded
// window alone cannot tell apart -- hence 7 bytes and not 8.  Two rows of one segment share a key only when their windows are
// equal; they then share c, and c < 7 means they END there: equal rows, finished.
//
// State: perm[p], the rows in their current order (the identity at first), cut into SEGMENTS -- maximal runs of positions
// whose rows agree on everything read so far.  A segment has a depth D in bytes (any offset) and is OPEN when it has at
// least two rows whose last key had c == 7; rows of closed segments are final where they are.  A round, over the open
// positions only:
//     compact   the open positions become a dense list of (position, row, dense segment number)          (place)
//     skip      D[s] <- min over the rows of s of the length they share with the segment's FIRST row, from D[s] on;
//               any value between D[s] and the true common prefix is correct (the rows agree on all of it), so a lane
//               stops after L bytes and hands a row that agreed on all L and has more to a wave          (skip_row, wave_group)
//     key       key(row, D[seg])                                                                         (key)
//     order     a STABLE sort of the list by (segment, key): entries stay inside their segment's range of the list, so
//               writing them back through the stored positions puts them in place                        (seg_bits)
//     cut       position p heads a new segment when it headed the old one or its key differs from p - 1's; the new
//               segment is open when it has at least two rows and c == 7, at depth D[s] + 7               (cut)
// Properties (the CPU driver asserts each inside its loop):
//     (P1) the result is the unique stable order, whatever L, with or without the skip;
//     (P2) without the skip, rounds <= max_len / 7 + 1;
//     (P3) with the skip every open segment splits or closes in its round: rounds <= G + 1 for G distinct strings;
//     (P4) within a segment equal rows are in ascending j before and after every round (the sort is stable, and rows of
//          one segment were in ascending j whenever they had compared equal so far).
#ifndef REJIT_AMD_RECORD_SORT_H_
#define REJIT_AMD_RECORD_SORT_H_

#include <stdint.h>

#include "record_pack.h"
#include "record_rows.h"

namespace rejit_amd {
namespace sort {

constexpr uint64_t kWindow = 7;                  // bytes of a row a key holds
using rows::kGroupBytes;                         // bytes a compare step reads of either row
constexpr uint32_t kLongBytes = 64;              // the prefix skip's lane tier stops after this many bytes (RJ_SORT_LONG_BYTES)
constexpr uint64_t kNoDepth = ~0ull;
constexpr uint8_t kHead = 1, kOpen = 2;          // a position's flags

// ---------------------------------------------------------------------------------------------------------------- limits
// A call takes rows_fit(k) rows: rows, positions and segments share 32-bit words in the scratch.
using rows::rows_fit;
// An open segment has at least two rows: at most k / 2 of them, and one in the first round
RJ_PACK_HD inline uint64_t max_segments(uint64_t k) { return k / 2 > 1 ? k / 2 : 1; }
// The scratch of a call, in bytes from the buffer's begin (every part 16-byte aligned).  Per row: the flags (1), perm (4),
// the depth a position's segment has when it heads one (8), the active list's positions (4), keys and (segment, row) words
// twice over -- the radix passes go from one copy to the other (32) -- and the skip's list (4); per segment, at most k / 2:
// its depth before and behind the skip (16) and its head's place in the list (4).  63 bytes per row (rocPRIM's own temporary
// storage is not part of it).
struct Layout {
  uint64_t flags, perm, pos_depth, act_pos, key_a, key_b, segrow_a, segrow_b, long_list, seg_depth, seg_cur, seg_head, bytes;
};
RJ_PACK_HD inline Layout layout(uint64_t k) {
  using rows::align16;
  const uint64_t S = max_segments(k);
  Layout l;
  l.flags = 0;
  l.perm = l.flags + align16(k);
  l.pos_depth = l.perm + align16(4 * k);
  l.act_pos = l.pos_depth + align16(8 * k);
  l.key_a = l.act_pos + align16(4 * k);
  l.key_b = l.key_a + align16(8 * k);
  l.segrow_a = l.key_b + align16(8 * k);
  l.segrow_b = l.segrow_a + align16(8 * k);
  l.long_list = l.segrow_b + align16(8 * k);
  l.seg_depth = l.long_list + align16(4 * k);
  l.seg_cur = l.seg_depth + align16(8 * S);
  l.seg_head = l.seg_cur + align16(8 * S);
  l.bytes = l.seg_head + align16(4 * S);
  return l;
}
// the bits of a dense segment number below n_segments: what the second radix pass sorts by (0: one segment, no pass)
RJ_PACK_HD inline unsigned seg_bits(uint64_t n_segments) {
  if (n_segments < 2) return 0;
  unsigned bits = 1;
  while (bits < 32 && (n_segments - 1) >> bits) bits++;
  return bits;
}

// ---------------------------------------------------------------------------------------------------------------- key
RJ_PACK_HD inline uint64_t byte_swap(uint64_t v) {
  v = ((v & 0x00FF00FF00FF00FFull) << 8) | ((v >> 8) & 0x00FF00FF00FF00FFull);
  v = ((v & 0x0000FFFF0000FFFFull) << 16) | ((v >> 16) & 0x0000FFFF0000FFFFull);
  return (v << 32) | (v >> 32);
}
RJ_PACK_HD inline uint64_t window_bytes(uint64_t len, uint64_t d) { return len - d < kWindow ? len - d : kWindow; }
RJ_PACK_HD inline uint32_t key_count(uint64_t key) { return static_cast<uint32_t>(key & 0xFF); }
// d <= len
template <class Text>
RJ_PACK_HD inline uint64_t key(const Text& text, uint64_t n, uint64_t begin, uint64_t len, uint64_t d) {
  const uint64_t c = window_bytes(len, d);
  if (c == 0) return 0;
  uint32_t w[4];
  rows::load_at(text, n, begin + d, w);
  const uint64_t be = byte_swap(static_cast<uint64_t>(w[0]) | (static_cast<uint64_t>(w[1]) << 32));   // the first byte on top
  return (be & (~0ull << (8 * (8 - c)))) | c;
}

// ---------------------------------------------------------------------------------------------------------------- skip
// The first byte at which 16-byte groups of two rows differ, counted from the group's begin, at most `valid` (1..16: the
// bytes of the group both rows have) -- `valid` when they agree on all of those.  `a` and `b` are text offsets.
template <class Text>
RJ_PACK_HD inline uint32_t group_agree(const Text& text, uint64_t n, uint64_t a, uint64_t b, uint32_t valid) {
  uint32_t x[4], y[4];
  rows::load_at(text, n, a, x);
  rows::load_at(text, n, b, y);
  uint32_t at = 16;
  for (int i = 3; i >= 0; i--) {
    const uint32_t d = x[i] ^ y[i];
    if (d) at = 4 * i + ((d & 0xFF) ? 0 : (d & 0xFF00) ? 1 : (d & 0xFF0000) ? 2 : 3);
  }
  return at < valid ? at : valid;
}
// The lane tier for one row against its segment's head (rows [hb, hb + hl) and [rb, rb + rl), both at least D long): the
// depth up to which they are known to agree, D <= depth <= their common prefix, having compared at most L bytes.  *more: they
// agreed on all L bytes and both have bytes left -- the wave tier goes on from depth and gives the row's word to the minimum,
// so that the segment's new depth is its rows' exact common prefix (P3 needs that; any smaller value would still sort right).
template <class Text>
RJ_PACK_HD inline uint64_t skip_row(const Text& text, uint64_t n, uint64_t hb, uint64_t hl, uint64_t rb, uint64_t rl, uint64_t D, uint32_t L, bool* more) {
  const uint64_t both = hl < rl ? hl : rl;
  *more = false;
  if (hb == rb) return both;                     // the head itself, or the same record named again
  const uint64_t stop = both - D < L ? both : D + L;
  uint64_t d = D;
  while (d < stop) {
    const uint32_t valid = stop - d < kGroupBytes ? static_cast<uint32_t>(stop - d) : static_cast<uint32_t>(kGroupBytes);
    const uint32_t same = group_agree(text, n, hb + d, rb + d, valid);
    d += same;
    if (same < valid) return d;
  }
  *more = stop < both;
  return d;
}
// The wave tier's step: lane `lane` of an iteration that begins at depth d0 takes the group at d0 + 16 * lane.  Returns the
// depth of the first difference inside that group, or kNoDepth when the group agrees or lies behind `both`; the least over
// the lanes -- `both` when every lane of every iteration says kNoDepth -- is the common prefix.
template <class Text>
RJ_PACK_HD inline uint64_t wave_group(const Text& text, uint64_t n, uint64_t hb, uint64_t rb, uint64_t both, uint64_t d0, uint64_t lane) {
  const uint64_t d = d0 + kGroupBytes * lane;
  if (d >= both) return kNoDepth;
  const uint32_t valid = both - d < kGroupBytes ? static_cast<uint32_t>(both - d) : static_cast<uint32_t>(kGroupBytes);
  const uint32_t same = group_agree(text, n, hb + d, rb + d, valid);
  return same < valid ? d + same : kNoDepth;
}

// ---------------------------------------------------------------------------------------------------------------- compact
// What an open position adds to the running sums of the compaction: open rows in the low half, open heads in the high one.
RJ_PACK_HD inline uint64_t place_add(uint8_t flags) {
  return (flags & kOpen) ? 1ull | (static_cast<uint64_t>(flags & kHead ? 1 : 0) << 32) : 0;
}
// ... and where the sums BEFORE an open position put it: its place in the list and its dense segment number
struct Place {
  uint32_t at, seg;
};
RJ_PACK_HD inline Place place(uint64_t before, uint8_t flags) {
  const uint32_t heads = static_cast<uint32_t>(before >> 32);
  return Place{static_cast<uint32_t>(before), (flags & kHead) ? heads : heads - 1};
}
RJ_PACK_HD inline uint64_t seg_row(uint32_t seg, uint32_t row) { return (static_cast<uint64_t>(seg) << 32) | row; }
RJ_PACK_HD inline uint32_t seg_of(uint64_t sr) { return static_cast<uint32_t>(sr >> 32); }
RJ_PACK_HD inline uint32_t row_of(uint64_t sr) { return static_cast<uint32_t>(sr); }

// ---------------------------------------------------------------------------------------------------------------- cut
// The flags of the position that entry `a` of the sorted list (n_active entries) lands on.  List: seg(i), key(i).
template <class List>
RJ_PACK_HD inline uint8_t cut(const List& list, uint64_t a, uint64_t n_active) {
  const uint32_t s = list.seg(a);
  const uint64_t key = list.key(a);
  const bool head = a == 0 || list.seg(a - 1) != s || list.key(a - 1) != key;
  const bool next_same = a + 1 < n_active && list.seg(a + 1) == s && list.key(a + 1) == key;
  const bool open = key_count(key) == kWindow && (!head || next_same);
  return static_cast<uint8_t>((head ? kHead : 0) | (open ? kOpen : 0));
}
// ... and what the cut writes for position p, which `row` lands on with those flags, in a segment that was keyed at `depth`.
// Mem is the scratch and the output as a step sees them: set_flags(p, f), set_perm(p, row), set_depth(p, d), set_order(p, row).
// An open position stays in perm (its segment's head carries the next depth); a closed one is final: its output row is
// written here, once -- it is never listed again.
template <class Mem>
RJ_PACK_HD inline void settle(Mem& M, uint64_t p, uint8_t flags, uint32_t row, uint64_t depth) {
  M.set_flags(p, flags);
  if (flags & kOpen) {
    M.set_perm(p, row);
    if (flags & kHead) M.set_depth(p, depth + kWindow);
  } else {
    M.set_order(p, row);
  }
}

}  // namespace sort
}  // namespace rejit_amd
#endif
