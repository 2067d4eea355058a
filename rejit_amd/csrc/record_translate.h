// rejit_amd/csrc/record_translate.h -- the arithmetic of rj_scan_records_translate (record_translate.hip): the rows of a record
// table through a 256-byte map and a 256-bit drop set -- Python's bytes.translate(table, delete), `tr A-Z a-z`, `tr -d` --
// into a new packed text laid out as rj_scan_records_pack lays records out.  Host and device code: the CPU tests drive exactly
// these functions (tests/support/translate_exec.cc), unit by unit, slab by slab and turn by turn as the kernels do.
//
// The work is SOURCE-major over a virtual stream V: row j owns the positions [sb(j), sb(j) + len(j)] -- its bytes, then one
// terminator that stands for its gap -- so sb(j + 1) = sb(j) + len(j) + 1, S = sb(k), and sb is strictly increasing: the row of
// a position is ONE search, and an empty row still owns a position (a run of empty rows spreads over slabs like bytes do).
// V is cut into slabs of kSlab positions; a lane takes 16 positions of a slab at a time (a Group).  With
//     kept_before(q) = the bytes of V before q that are not dropped,   rows_before(q) = the terminators before q
// position q stands in the output at lead + kept_before(q) + rows_before(q) * gap, a terminator's gap right there, and
//     ob(0) = lead,   oe(j) = place of row j's terminator,   ob(j + 1) = oe(j) + gap,   total = place of S.
// A slab's output range is [place(c0), place(c1)) (slab 0: from 0, it owns the lead): the ranges partition [0, total).
//
// S is not known on the host when the launches are made (one synchronise per call), but the look-back's words are: the host
// gives a cap on the number of units (unit_cap: enough for one slab per unit whenever the rows do not overlap or repeat),
// and a unit is r = slabs_per_unit consecutive slabs -- the same r for every unit, so the units stay alike whatever the rows.
#ifndef REJIT_AMD_RECORD_TRANSLATE_H_
#define REJIT_AMD_RECORD_TRANSLATE_H_

#include <stdint.h>

#include "record_pack.h"

namespace rejit_amd {
namespace translate {

constexpr uint64_t kSlab = 4096;       // positions of V per slab: one pass of 256 lanes x 16 positions
constexpr uint64_t kImage = 4096;      // output bytes per turn of the emit: the slab's image in LDS
constexpr uint32_t kGroup = 16;        // positions a lane takes at a time

// the map and the drop set as the kernels get them: an argument of 288 bytes
struct Tables {
  uint8_t map[256];
  uint32_t drop[8];   // bit (b & 31) of word b >> 5 = bit (b & 7) of the caller's byte b >> 3
};
// -> tables from the caller's arrays (null: identity / nothing dropped); *identity: map[b] == b for all b, *drops: a bit is set
inline void make_tables(const uint8_t* map, const uint8_t* drop, Tables* t, bool* identity, bool* drops) {
  *identity = true, *drops = false;
  for (uint32_t b = 0; b < 256; b++) {
    t->map[b] = map ? map[b] : static_cast<uint8_t>(b);
    if (t->map[b] != b) *identity = false;
  }
  for (uint32_t i = 0; i < 8; i++) {
    t->drop[i] = 0;
    for (uint32_t b = 0; drop && b < 4; b++) t->drop[i] |= static_cast<uint32_t>(drop[4 * i + b]) << (8 * b);
    if (t->drop[i]) *drops = true;
  }
}
// the tables as a kernel reads them (its LDS copies) or a test does: T.mapped(b), T.dropped(b)
struct TableView {
  const uint8_t* map;
  const uint32_t* drop;
  RJ_PACK_HD uint32_t mapped(uint32_t b) const { return map[b]; }
  RJ_PACK_HD bool dropped(uint32_t b) const { return (drop[b >> 5] >> (b & 31)) & 1u; }
};

// ---------------------------------------------------------------------------------------------------------------- call
// what the call refuses before any launch -- the pack's refusals, in the pack's order
enum Refusal { kFine = 0, kNull, kFill, kOutAlign, kTableAlign, kSums };
inline Refusal check_call(const void* scan, const void* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records,
                          const uint64_t* indices, uint64_t n_indices, int fill, uint64_t lead, uint64_t gap, const void* out, uint64_t out_cap,
                          const uint64_t* out_begin, const uint64_t* out_end) {
  if (!scan || (!text && n) || (n_records && (!rec_begin || !rec_end)) || (!out && out_cap)) return kNull;
  if (fill < 0 || fill > 255) return kFill;
  if (reinterpret_cast<uintptr_t>(out) & 15u) return kOutAlign;
  const uintptr_t tables = reinterpret_cast<uintptr_t>(rec_begin) | reinterpret_cast<uintptr_t>(rec_end) | reinterpret_cast<uintptr_t>(indices) |
                           reinterpret_cast<uintptr_t>(out_begin) | reinterpret_cast<uintptr_t>(out_end);
  if (tables & 7u) return kTableAlign;
  const uint64_t k = indices ? n_indices : n_records;
  // the output's sums with the call's lead and gap, and V's with lead 0 and gap 1
  if (!pack::sums_fit(k, n, lead, gap) || !pack::sums_fit(k, n, 0, 1)) return kSums;
  return kFine;
}

// ---------------------------------------------------------------------------------------------------------------- geometry
RJ_PACK_HD inline uint64_t n_slabs(uint64_t S, uint64_t slab) { return (S + slab - 1) / slab; }
// units the host provides look-back words for: one slab per unit as long as S <= n + k (no two rows share a byte)
RJ_PACK_HD inline uint64_t unit_cap(uint64_t n, uint64_t k, uint64_t slab) { return (n + k) / slab + 1; }
RJ_PACK_HD inline uint64_t slabs_per_unit(uint64_t slabs, uint64_t cap) { return slabs <= cap ? 1 : (slabs + cap - 1) / cap; }
RJ_PACK_HD inline uint64_t n_units(uint64_t slabs, uint64_t per_unit) { return (slabs + per_unit - 1) / per_unit; }
RJ_PACK_HD inline uint64_t place(uint64_t lead, uint64_t gap, uint64_t kept_before, uint64_t rows_before) { return lead + kept_before + rows_before * gap; }

// ---------------------------------------------------------------------------------------------------------------- group
RJ_PACK_HD inline uint32_t popcount16(uint32_t m) { return static_cast<uint32_t>(__builtin_popcount(m & 0xFFFFu)); }
// byte b (0..15) of the four words, without an indexed register
RJ_PACK_HD inline uint32_t get_byte(const uint32_t w[4], uint32_t b) { return ((b < 4 ? w[0] : b < 8 ? w[1] : b < 12 ? w[2] : w[3]) >> (8 * (b & 3))) & 0xFFu; }
RJ_PACK_HD inline void set_byte(uint32_t w[4], uint32_t b, uint32_t c) {
  const uint32_t v = c << (8 * (b & 3));
  if (b < 4) w[0] |= v;
  else if (b < 8) w[1] |= v;
  else if (b < 12) w[2] |= v;
  else w[3] |= v;
}

// The positions [q0, q0 + 16) of V below S: bit b of `data`: position q0 + b is a byte of a row, and w holds it; bit b of
// `term`: it is a row's terminator; j: the row q0 lies in = the rows that ended before q0.
struct Group {
  uint32_t w[4];
  uint32_t data, term;
  uint64_t j;
};
// sb: the view of the rows' places in V (ob_at(j) = sb(j), ob_at(k) = S, src_at(j) = the row's first byte in the text);
// [j_lo, j_hi): the rows of the slab -- j_lo the row its first position lies in, j_hi the first row that begins behind it.
// Text: load16(s, w) reads 16 bytes that all lie inside one row, byte(s) one byte of a row.
template <class Text>
RJ_PACK_HD inline Group load_group(const pack::View& sb, uint64_t j_lo, uint64_t j_hi, uint64_t q0, uint64_t S, const Text& text) {
  Group g;
  g.w[0] = g.w[1] = g.w[2] = g.w[3] = 0;
  g.data = g.term = 0;
  g.j = 0;
  if (q0 >= S) return g;
  const uint64_t end = S - q0 < kGroup ? S : q0 + kGroup;
  uint64_t j = pack::upper_bound(sb, j_lo, j_hi, q0) - 1;   // (sb(j_lo) <= q0: the search ends behind j_lo)
  g.j = j;
  uint64_t q = q0;
  while (q < end) {
    const uint64_t begin = sb.ob_at(j), term_at = sb.ob_at(j + 1) - 1;
    if (q == q0 && q0 + kGroup <= term_at) {   // the common case: 16 bytes of one row
      text.load16(sb.src_at(j) + (q0 - begin), g.w);
      g.data = 0xFFFFu;
      return g;
    }
    if (q < term_at) {
      uint64_t s = sb.src_at(j) + (q - begin);
      for (; q < end && q < term_at; q++, s++) {
        const uint32_t b = static_cast<uint32_t>(q - q0);
        set_byte(g.w, b, text.byte(s));
        g.data |= 1u << b;
      }
    }
    if (q < end) {   // q == term_at
      g.term |= 1u << static_cast<uint32_t>(q - q0);
      q++, j++;
    }
  }
  return g;
}

// the group's bytes that stay (the drop set is judged on the SOURCE byte) / of those, the ones the map changes
template <class Tab>
RJ_PACK_HD inline uint32_t kept_mask(const Group& g, const Tab& tab) {
  uint32_t kept = 0;
  for (uint32_t b = 0; b < kGroup; b++)
    if (((g.data >> b) & 1u) && !tab.dropped(get_byte(g.w, b))) kept |= 1u << b;
  return kept;
}
template <class Tab>
RJ_PACK_HD inline uint32_t changed_mask(const Group& g, uint32_t kept, const Tab& tab) {
  uint32_t changed = 0;
  for (uint32_t b = 0; b < kGroup; b++) {
    const uint32_t c = get_byte(g.w, b);
    if (((kept >> b) & 1u) && tab.mapped(c) != c) changed |= 1u << b;
  }
  return changed;
}
// what a lane adds to the slab's sums, in one word: its kept bytes, and its terminators << 16 (a slab: at most 4096 of each)
RJ_PACK_HD inline uint32_t lane_sums(const Group& g, uint32_t kept) { return popcount16(kept) | (popcount16(g.term) << 16); }
RJ_PACK_HD inline uint32_t sums_kept(uint32_t sums) { return sums & 0xFFFFu; }
RJ_PACK_HD inline uint32_t sums_rows(uint32_t sums) { return sums >> 16; }

// ---------------------------------------------------------------------------------------------------------------- tables
// The rows that END in the group: end(j, oe) for each with oe = the terminator's place; kept_before: the kept bytes of V before
// the group's first position.  (Row j + 1 begins at oe + gap; row 0 at lead.)
template <class EndFn>
RJ_PACK_HD inline void row_ends(const Group& g, uint32_t kept, uint64_t kept_before, uint64_t lead, uint64_t gap, const EndFn& end) {
  uint64_t j = g.j, kb = kept_before;
  for (uint32_t b = 0; b < kGroup; b++) {
    if ((kept >> b) & 1u) kb++;
    else if ((g.term >> b) & 1u) {
      end(j, place(lead, gap, kb, j));
      j++;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- emit
// the output range of the slab [c0, ...): kept_before / j_lo as of c0, `sums` the slab's; slab 0 owns the lead
struct Range {
  uint64_t o0, o1;
};
RJ_PACK_HD inline Range slab_range(uint64_t c0, uint64_t lead, uint64_t gap, uint64_t kept_before, uint64_t j_lo, uint32_t sums) {
  Range r;
  r.o0 = c0 == 0 ? 0 : place(lead, gap, kept_before, j_lo);
  r.o1 = place(lead, gap, kept_before + sums_kept(sums), j_lo + sums_rows(sums));
  return r;
}
// the first turn's window begins at the 16-byte boundary at or before the range
RJ_PACK_HD inline uint64_t first_window(const Range& r) { return r.o0 & ~15ull; }

// One turn: the group's kept bytes whose places lie in the window [w0, w0 + image) go mapped into the image: put(offset in
// the image, byte).  at: the place of the group's first position.  A group whose places miss the window is left at once.
template <class Tab, class PutFn>
RJ_PACK_HD inline void place_group(const Group& g, uint32_t kept, uint64_t at, uint64_t gap, uint64_t w0, uint64_t image, const Tab& tab, const PutFn& put) {
  if (kept == 0) return;
  const uint64_t span_end = at + popcount16(kept) + popcount16(g.term) * gap;
  if (span_end <= w0 || at >= w0 + image) return;
  uint64_t o = at;
  for (uint32_t b = 0; b < kGroup; b++) {
    if ((kept >> b) & 1u) {
      if (o - w0 < image) put(o - w0, tab.mapped(get_byte(g.w, b)));   // (o < w0 wraps to a large number)
      o++;
    } else if ((g.term >> b) & 1u) {
      o += gap;
    }
  }
}

// The bytes [lo, hi) of the 16 at p = w0 + 16 * lane that the slab stores in this turn: those inside its range and below the
// limit (= min(total, out_cap)).  hi - lo == 16: one vector store; else byte by byte (an edge a neighbouring slab shares).
struct Store {
  uint32_t lo, hi;
};
RJ_PACK_HD inline Store group_store(uint64_t p, const Range& r, uint64_t limit) {
  const uint64_t a = r.o0 > p ? r.o0 : p;
  const uint64_t e = r.o1 < limit ? r.o1 : limit;
  const uint64_t b = e < p + kGroup ? e : p + kGroup;
  Store s{0, 0};
  if (a < b) s.lo = static_cast<uint32_t>(a - p), s.hi = static_cast<uint32_t>(b - p);
  return s;
}

}  // namespace translate
}  // namespace rejit_amd
#endif
