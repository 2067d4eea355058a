// rejit_amd/csrc/record_csv.h -- the arithmetic of rj_scan_records_csv (record_csv.hip): the rows and fields of a CSV text with
// quoted fields (RFC 4180: a quote byte around a field, doubled inside it) as record tables.  Host and device code: the CPU
// tests drive exactly these functions (tests/support/csv_exec.cc), span by span, step by step and lane by lane as the kernels do.
//
// ins(p) = the parity of the quote bytes in text[0, p).  Byte p is STRUCTURAL when ins(p) == 0 and it is the delimiter or \n;
// fields are the stretches between structural bytes, a \n also ends a row.  Which bytes are structural is a bit per byte and a
// parity, so a stretch of text is summarised under BOTH entry parities (its quote parity, its structural bytes and row ends
// outside quotes under each), two summaries compose associatively, and nothing waits for the text in front of it:
//   summarise  every wave of the grid owns one contiguous SPAN of the text (whole units; a unit only sets the grain of the
//              cut) and walks it in steps of 64 lanes x 16 bytes, carrying one Summary
//   resolve    the spans' summaries composed in order: every span's Entry (parity, fields and rows in front of it), the counts
//   emit       the same walk with the entry known: every byte's field and row number is a popcount away, and the lane that
//              owns a structural byte writes the tables' entries around it (emit_group)
// Every decision looks at most one byte back and two bytes ahead (the halo of a group), so nothing depends on where the text
// is cut.
#ifndef REJIT_AMD_RECORD_CSV_H_
#define REJIT_AMD_RECORD_CSV_H_

#include <stdint.h>

#include "record_pack.h"

namespace rejit_amd {
namespace csv {

constexpr uint32_t kGroup = 16;               // bytes a lane takes at a time
constexpr uint32_t kLanes = 64;               // lanes of a wave
constexpr uint64_t kStep = kLanes * kGroup;   // bytes a wave takes at a time
constexpr uint64_t kUnit = 4096;              // the grain of the spans (RJ_CSV_UNIT), a multiple of kStep
constexpr uint32_t kGrid = 2048;              // workgroups (RJ_CSV_GRID): eight for each of the 256 CUs
constexpr uint32_t kWavesPerGroup = 4;
constexpr uint64_t kMaxText = 1ull << 42;

// rejit_hip.h's RJ_CSV_* flags
enum : uint32_t { kEscaped = 1, kBadQuote = 2, kBadClose = 4, kBareCr = 8, kOpen = 16, kMalformed = kBadQuote | kBadClose | kBareCr | kOpen };

// ---------------------------------------------------------------------------------------------------------------- call
// what the call refuses before any launch.  Every table may be null: it is not written then.
enum Refusal { kFine = 0, kNull, kStats, kTableAlign, kFlagsAlign, kDelimiter, kQuote, kLineBreak, kSame, kTooLong };
inline Refusal check_call(const void* scan, const void* text, uint64_t n, int delimiter, int quote, const uint64_t* row_first, const uint64_t* row_begin,
                          const uint64_t* row_end, const uint64_t* field_begin, const uint64_t* field_end, const uint32_t* field_flags, const void* stats) {
  if (!scan || (!text && n)) return kNull;
  if (!stats) return kStats;
  const uintptr_t tables = reinterpret_cast<uintptr_t>(row_first) | reinterpret_cast<uintptr_t>(row_begin) | reinterpret_cast<uintptr_t>(row_end) |
                           reinterpret_cast<uintptr_t>(field_begin) | reinterpret_cast<uintptr_t>(field_end);
  if (tables & 7u) return kTableAlign;
  if (reinterpret_cast<uintptr_t>(field_flags) & 3u) return kFlagsAlign;
  if (delimiter < 0 || delimiter > 255) return kDelimiter;
  if (quote < -1 || quote > 255) return kQuote;
  if (delimiter == '\n' || delimiter == '\r' || quote == '\n' || quote == '\r') return kLineBreak;
  if (delimiter == quote) return kSame;
  if (n >= kMaxText) return kTooLong;
  return kFine;
}

// ---------------------------------------------------------------------------------------------------------------- geometry
// The text is cut into units of `unit` bytes; the first `waves` waves own `per_wave` consecutive units each (the last one the
// rest).  wave_cap: the waves the grid has.
struct Geometry {
  uint64_t units, per_wave, waves;
};
RJ_PACK_HD inline Geometry geometry(uint64_t n, uint64_t unit, uint64_t wave_cap) {
  Geometry g;
  g.units = (n + unit - 1) / unit;
  g.per_wave = g.units ? (g.units + wave_cap - 1) / wave_cap : 0;
  g.waves = g.units ? (g.units + g.per_wave - 1) / g.per_wave : 0;
  return g;
}
RJ_PACK_HD inline uint64_t span_begin(const Geometry& g, uint64_t unit, uint64_t n, uint64_t wave) {
  const uint64_t at = wave * g.per_wave * unit;
  return at < n ? at : n;
}

// ---------------------------------------------------------------------------------------------------------------- summaries
// a stretch of text under both entry parities: fields[h] / rows[h] = its structural bytes / its row ends when ins(its first
// byte) == h; parity: of its quote bytes
struct Summary {
  uint64_t parity, fields[2], rows[2];
};
RJ_PACK_HD inline Summary nothing() { return Summary{0, {0, 0}, {0, 0}}; }
// a, then b
RJ_PACK_HD inline Summary compose(const Summary& a, const Summary& b) {
  const bool swap = a.parity != 0;   // (selects, no indexed registers)
  Summary c;
  c.parity = a.parity ^ b.parity;
  c.fields[0] = a.fields[0] + (swap ? b.fields[1] : b.fields[0]);
  c.fields[1] = a.fields[1] + (swap ? b.fields[0] : b.fields[1]);
  c.rows[0] = a.rows[0] + (swap ? b.rows[1] : b.rows[0]);
  c.rows[1] = a.rows[1] + (swap ? b.rows[0] : b.rows[1]);
  return c;
}
// what lies in front of a stretch: ins(its first byte), the structural bytes and the row ends before it
struct Entry {
  uint64_t parity, fields, rows;
};
RJ_PACK_HD inline Entry advance(const Entry& e, const Summary& s) {
  return Entry{e.parity ^ s.parity, e.fields + (e.parity ? s.fields[1] : s.fields[0]), e.rows + (e.parity ? s.rows[1] : s.rows[0])};
}
// the text's counts from the state at its end: a text that does not end in a structural \n has one more field and row
RJ_PACK_HD inline uint64_t tail_row(uint64_t n, uint32_t last_byte, const Entry& end) { return n != 0 && !(last_byte == '\n' && end.parity == 0) ? 1 : 0; }

// ---------------------------------------------------------------------------------------------------------------- group
RJ_PACK_HD inline uint32_t popcount(uint32_t m) { return static_cast<uint32_t>(__builtin_popcount(m)); }
// the four bytes of x that equal c, as four bits: a zero byte of x ^ cccc leaves 0x80, and a multiplication gathers the four
// (the partial products land on different bits: no carries)
RJ_PACK_HD inline uint32_t equal4(uint32_t x, uint32_t c) {
  const uint32_t y = x ^ (c * 0x01010101u);
  const uint32_t zero = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
  return (((zero >> 7) * 0x01020408u) >> 24) & 0xFu;
}
RJ_PACK_HD inline uint32_t equal16(const uint32_t w[4], uint32_t c) { return equal4(w[0], c) | (equal4(w[1], c) << 4) | (equal4(w[2], c) << 8) | (equal4(w[3], c) << 12); }

// 16 bytes at p0 and their halo: `valid` of them lie in the text (fewer than 16: the text ends here); prev = text[p0 - 1],
// next1 = text[p0 + 16], next2 = text[p0 + 17], each -1 when outside the text
struct Group {
  uint32_t w[4];
  uint32_t valid;
  int32_t prev, next1, next2;
};
// bit b + 1 of a mask stands for position p0 + b, b = -1 .. 17; in: the position lies in the text
struct Masks {
  uint32_t q, d, nl, cr, in;
};
RJ_PACK_HD inline uint32_t halo_bits(const Group& g, int32_t c) { return (g.prev == c ? 1u : 0u) | (g.next1 == c ? 1u << 17 : 0u) | (g.next2 == c ? 1u << 18 : 0u); }
RJ_PACK_HD inline Masks make_masks(const Group& g, int delimiter, int quote) {
  const uint32_t core = (1u << g.valid) - 1u;
  Masks m;
  m.q = quote < 0 ? 0u : ((equal16(g.w, static_cast<uint32_t>(quote)) & core) << 1) | halo_bits(g, quote);
  m.d = ((equal16(g.w, static_cast<uint32_t>(delimiter)) & core) << 1) | halo_bits(g, delimiter);
  m.nl = ((equal16(g.w, '\n') & core) << 1) | halo_bits(g, '\n');
  m.cr = ((equal16(g.w, '\r') & core) << 1) | halo_bits(g, '\r');
  m.in = (core << 1) | (g.prev >= 0 ? 1u : 0u) | (g.next1 >= 0 ? 1u << 17 : 0u) | (g.next2 >= 0 ? 1u << 18 : 0u);
  return m;
}
constexpr uint32_t kCore = 0x1FFFEu;
// bit k of the result: the XOR of x's bits 0 .. k
RJ_PACK_HD inline uint32_t prefix_xor(uint32_t x) {
  x ^= x << 1;
  x ^= x << 2;
  x ^= x << 4;
  x ^= x << 8;
  x ^= x << 16;
  return x;
}

// a lane's 16 bytes under both entry parities, in words a wave can add up: c[h] = structural bytes | row ends << 16
struct LaneSummary {
  uint32_t parity, c[2];
};
RJ_PACK_HD inline LaneSummary lane_summary(const Masks& m) {
  const uint32_t qc = m.q & m.in & kCore;
  const uint32_t inside = prefix_xor(qc) << 1;   // under entry parity 0
  const uint32_t s = (m.d | m.nl) & m.in & kCore, r = m.nl & m.in & kCore;
  LaneSummary l;
  l.parity = popcount(qc) & 1u;
  l.c[0] = popcount(s & ~inside) | (popcount(r & ~inside) << 16);
  l.c[1] = popcount(s & inside) | (popcount(r & inside) << 16);
  return l;
}
RJ_PACK_HD inline Summary widen(uint32_t parity, uint32_t c0, uint32_t c1) { return Summary{parity, {c0 & 0xFFFFu, c1 & 0xFFFFu}, {c0 >> 16, c1 >> 16}}; }

// what the 16 bytes are, with the entry parity known; bit b stands for position p0 + b
struct Marks {
  uint32_t structural, row_end;                     // outside quotes: delimiter or \n / \n
  uint32_t quote, quoted;                           // a quote byte / one that is a field's first byte
  uint32_t escaped, bad_quote, bad_close, bare_cr;  // the events of rejit_hip.h
  uint32_t cr_end;                                  // a \r outside quotes directly before a \n: the field ends HERE
  uint32_t prev_quote, next_quote, prev_cr;         // text[p - 1] / text[p + 1] is the quote, text[p - 1] is \r
  uint32_t has_next;                                // p + 1 < n
  uint32_t parity, inside_end;                      // of the quotes here / ins(p0 + valid)
};
// entry = ins(p0); first: p0 == 0
RJ_PACK_HD inline Marks make_marks(const Masks& m, uint32_t entry, bool first) {
  const uint32_t core = m.in & kCore;
  const uint32_t qc = m.q & core;
  // bit of position p: ins(p).  (Bit 0, the byte before the group, reads ins(p0): right whenever that byte is no quote, and
  // a quote is not structural.)
  const uint32_t inside = (prefix_xor(qc) << 1) ^ (entry ? ~0u : 0u);
  const uint32_t s = (m.d | m.nl) & ~inside;
  const uint32_t begins = (s << 1) | (first ? 2u : 0u);   // p is a field's first position
  const uint32_t q0 = qc & ~inside, q1 = qc & inside;
  const uint32_t closes = (~m.in >> 1) | (m.d >> 1) | (m.nl >> 1) | (m.q >> 1) | ((m.cr >> 1) & (m.nl >> 2));
  const uint32_t cr0 = m.cr & core & ~inside;
  Marks k;
  k.structural = ((s & core) >> 1) & 0xFFFFu;
  k.row_end = ((m.nl & ~inside & core) >> 1) & 0xFFFFu;
  k.quote = (qc >> 1) & 0xFFFFu;
  k.quoted = ((q0 & begins) >> 1) & 0xFFFFu;
  k.escaped = ((q0 & ~begins & (m.q << 1)) >> 1) & 0xFFFFu;
  k.bad_quote = ((q0 & ~begins & ~(m.q << 1)) >> 1) & 0xFFFFu;
  k.bad_close = ((q1 & ~closes) >> 1) & 0xFFFFu;
  k.bare_cr = ((cr0 & ~(m.nl >> 1)) >> 1) & 0xFFFFu;
  k.cr_end = ((cr0 & (m.nl >> 1)) >> 1) & 0xFFFFu;
  k.prev_quote = m.q & 0xFFFFu;
  k.next_quote = (m.q >> 2) & 0xFFFFu;
  k.prev_cr = m.cr & 0xFFFFu;
  k.has_next = (m.in >> 2) & 0xFFFFu;
  k.parity = popcount(qc) & 1u;
  k.inside_end = entry ^ k.parity;
  return k;
}
RJ_PACK_HD inline uint32_t lane_counts(const Marks& k) { return popcount(k.structural) | (popcount(k.row_end) << 16); }

// ---------------------------------------------------------------------------------------------------------------- stats
// the events of a lane's walk: [0] quoted fields, [1] escapes, [2] bad quotes, [3] bad closes, [4] bare \r
struct Tally {
  uint32_t n[5];
  uint64_t first_bad;   // ~0: none
};
RJ_PACK_HD inline void tally_init(Tally* t) {
  for (uint32_t i = 0; i < 5; i++) t->n[i] = 0;
  t->first_bad = ~0ull;
}
RJ_PACK_HD inline void tally_add(Tally* t, const Marks& k, uint64_t p0) {
  t->n[0] += popcount(k.quoted);
  t->n[1] += popcount(k.escaped);
  t->n[2] += popcount(k.bad_quote);
  t->n[3] += popcount(k.bad_close);
  t->n[4] += popcount(k.bare_cr);
  const uint32_t bad = k.bad_quote | k.bad_close | k.bare_cr;
  if (bad) {
    const uint64_t at = p0 + static_cast<uint32_t>(__builtin_ctz(bad));
    if (at < t->first_bad) t->first_bad = at;
  }
}

// ---------------------------------------------------------------------------------------------------------------- emit
// The table entries the lane with the group at p0 owns.  fields_before / rows_before: the structural bytes / row ends of the
// text before p0.  The lane that owns structural byte p writes field_end[f] and field_begin[f + 1], for a \n also row_end[r],
// row_first[r + 1] and row_begin[r + 1]; where a \r stands before that \n (and so belongs to neither) the \r's lane writes
// field_end[f] instead: it sees the byte before it.  The lane with byte 0 writes field_begin[0] and row_begin[0] (row_first[0]
// is the resolve's), the lane with byte n - 1 the end of a last row without a line break.  Every event ORs its flag into
// its field.  Sink: field_begin(f, v), field_end(f, v), flag(f, bits), row_begin(r, v), row_end(r, v), row_first(r, v) --
// the caps are the sink's.
template <class Sink>
RJ_PACK_HD inline void emit_group(const Marks& k, uint64_t p0, uint32_t valid, uint64_t n, uint64_t fields_before, uint64_t rows_before, Sink& out) {
  if (valid == 0) return;
  if (p0 == 0) {
    out.field_begin(0, k.quoted & 1u);
    out.row_begin(0, 0);
  }
  uint32_t todo = k.structural | k.cr_end | k.escaped | k.bad_quote | k.bad_close | k.bare_cr;
  while (todo) {
    const uint32_t b = static_cast<uint32_t>(__builtin_ctz(todo));
    const uint32_t bit = 1u << b;
    todo &= todo - 1;
    const uint64_t p = p0 + b;
    const uint64_t f = fields_before + popcount(k.structural & (bit - 1));
    const uint64_t behind_quote = (k.prev_quote & bit) ? 1 : 0, behind_cr = (k.prev_cr & bit) ? 1 : 0;
    if (k.structural & bit) {
      const bool line = (k.row_end & bit) != 0, more = (k.has_next & bit) != 0;
      if (!(line && behind_cr)) out.field_end(f, p - behind_quote);
      if (!line || more) out.field_begin(f + 1, p + 1 + ((k.next_quote & bit) ? 1 : 0));
      if (line) {
        const uint64_t r = rows_before + popcount(k.row_end & (bit - 1));
        out.row_end(r, p - behind_cr);
        out.row_first(r + 1, f + 1);
        if (more) out.row_begin(r + 1, p + 1);
      }
    }
    if (k.cr_end & bit) out.field_end(f, p - behind_quote);
    const uint32_t flags = ((k.escaped & bit) ? kEscaped : 0u) | ((k.bad_quote & bit) ? kBadQuote : 0u) | ((k.bad_close & bit) ? kBadClose : 0u) |
                           ((k.bare_cr & bit) ? kBareCr : 0u);
    if (flags) out.flag(f, flags);
  }
  if (p0 + valid == n) {   // the text ends here
    const uint32_t last = 1u << (valid - 1);
    if (!(k.row_end & last)) {
      const uint64_t f = fields_before + popcount(k.structural), r = rows_before + popcount(k.row_end);
      out.field_end(f, k.inside_end ? n : n - ((k.quote & last) ? 1 : 0));
      if (k.inside_end) out.flag(f, kOpen);
      out.row_end(r, n);
      out.row_first(r + 1, f + 1);
    }
  }
}

}  // namespace csv
}  // namespace rejit_amd
#endif
