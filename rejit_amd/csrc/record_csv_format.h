// rejit_amd/csrc/record_csv_format.h -- the arithmetic of rj_scan_records_format_csv (record_csv_format.hip): the rows of C
// record tables put side by side into the lines of a new contiguous text, every field QUOTED exactly where Python's csv.writer
// quotes it -- the inverse of rj_scan_records_csv, and rj_scan_records_zip with a one-byte separator that knows about quoting.
// Host and device code: the CPU tests drive exactly these functions (tests/support/csv_format_exec.cc), unit by unit, chunk by
// chunk and lane by lane as the kernels do.
//
// C columns, 1 <= C <= 16, each an rj_zip_column (record_zip.h's Column; width and reserved must be 0): rows as
// rj_scan_records_pack takes them, the same row count k in every column.  With P the bytes of column c's row j, d the
// delimiter and q the quote:
//     special(P)  P holds d, q, \r or \n
//     need(c, j)  bit c of always_mask, or special(P), or C == 1 and P is empty (csv.writer's lone empty field, `""`)
//     F(c, j)     value column (bit c of raw_mask clear): need ? q + P with every q doubled + q : P
//                 raw column   (bit c of raw_mask set):   need ? q + P + q : P -- P is the interior of a field as
//                 rj_scan_records_csv delimits it, its "" still in place: nothing is doubled
//     T(j)        F(0, j) d F(1, j) d ... F(C-1, j)
// and the layout is the pack's (record_pack.h) with len(j) = |T(j)|.
//
// OUT OF SCOPE: no quoting at all (quote == -1) and escape characters -- rj_scan_records_zip joins without quoting;
// QUOTE_NONNUMERIC as a mode -- a caller who knows which columns hold strings sets their always_mask bits; delimiters of more
// than one byte; a line terminator other than what fill and gap give; per-row nulls; header lines.
//
// A piece is CLASSIFIED once, 16 bytes at a time (group_class: special, and its quote bytes counted), and staged as 16 bytes
// (Staged: source, length, quote count, need).  A row is a sequence of segments -- per column: the delimiter (not in front of
// column 0), the opening quote, the content, the closing quote -- whose places follow from the staged pieces alone (field_at).
// Three tiers by the content (tier_of):
//     bytes   a piece shorter than kStreamBytes: byte by byte into the chunk's image, doubling inline (fewer than 32 steps)
//     stream  a longer piece that doubles nothing (not quoted, quoted without a quote byte inside, or raw): output byte i of
//             the content is source byte i, so the 16-byte output groups it covers whole come from the group's own offset
//             (group_streamed) and only the partial groups at its two ends are bytes -- record_zip.h's tiers
//     expand  a longer value piece with quote bytes inside: a wave walks the source 64 lanes x 16 bytes a step, a lane's output
//             offset is its source offset plus the quote bytes in front of it (expand_group).  A chunk that begins inside
//             such a piece needs the quote bytes in front of its first byte: a piece of kCheckpointBytes or more is walked
//             ONCE between the plan and the emit, and leaves a Checkpoint for every chunk that begins inside it; a shorter
//             one (at most 8 steps) is walked from its begin by the chunk itself
#ifndef REJIT_AMD_RECORD_CSV_FORMAT_H_
#define REJIT_AMD_RECORD_CSV_FORMAT_H_

#include <stdint.h>
#include <stdio.h>

#include "record_csv.h"
#include "record_pack.h"
#include "record_rows.h"
#include "record_zip.h"

namespace rejit_amd {
namespace csvf {

using zip::Column;
using zip::Columns;
constexpr int kMaxColumns = zip::kMaxColumns;
constexpr uint64_t kStreamBytes = zip::kStreamBytes;   // the tier threshold of the content, the zip's
constexpr uint64_t kEmitChunk = zip::kEmitChunk;       // output bytes per chunk of the emit
constexpr uint64_t kWaveStep = csv::kStep;             // source bytes a wave takes at a time: 64 lanes x 16
constexpr uint64_t kWaveBytes = 1024;                  // a piece this long is classified by its wave, a shorter one by its lane
constexpr uint64_t kCheckpointBytes = 8192;            // an expanding piece this long leaves checkpoints (it spans a chunk's begin)
constexpr uint32_t kMaxExpand = 128;                   // expanding pieces a chunk can touch (each puts 35 bytes at least: 119)
static_assert(kEmitChunk / (kStreamBytes + 3) + 2 <= kMaxExpand, "the chunk's list holds every expanding piece that touches it");

// ---------------------------------------------------------------------------------------------------------------- a piece
struct Piece {
  uint64_t src, len, quotes;   // where it begins in its column's text, its length, the quote bytes in it (all below 2^42)
  bool need;
};
// ... as the 16 bytes the classify stages: x = src | low 22 bits of quotes << 42, y = len | high 20 bits of quotes << 42 | need << 63
struct Staged {
  uint64_t x, y;
};
constexpr uint64_t kLow42 = (1ull << 42) - 1;
RJ_PACK_HD inline Staged stage_piece(const Piece& p) {
  return Staged{p.src | ((p.quotes & 0x3FFFFFull) << 42), p.len | ((p.quotes >> 22) << 42) | (p.need ? 1ull << 63 : 0)};
}
RJ_PACK_HD inline Piece staged_piece(const Staged& s) {
  return Piece{s.x & kLow42, s.y & kLow42, (s.x >> 42) | (((s.y >> 42) & 0xFFFFFull) << 22), (s.y >> 63) != 0};
}

// ---------------------------------------------------------------------------------------------------------------- the call
// R = sum_c (2 n_c + 2) + (C - 1) + gap is the most a row adds (< pack::kMaxRow), and lead + k R stays below pack::kMaxTotal
inline bool sums_fit(uint64_t k, const Column* cols, int n_cols, uint64_t lead, uint64_t gap) {
  uint64_t per = 0;
  for (int c = 0; c < n_cols; c++) {
    if (cols[c].n >= pack::kMaxRow) return false;
    per += 2 * cols[c].n + 2;   // (16 x 2^43 at the most)
  }
  per += static_cast<uint64_t>(n_cols - 1);
  if (gap >= pack::kMaxRow || per + gap >= pack::kMaxRow || lead >= pack::kMaxTotal) return false;
  per += gap;
  if (k != 0 && per > (pack::kMaxTotal - 1 - lead) / k) return false;
  return true;
}
// ... that bound, lead + k R, for a call sums_fit has passed (below pack::kMaxTotal): the output is never longer, whatever
// out_cap says -- what is sized by the output's chunks is sized by min(out_cap, most_total)
inline uint64_t most_total(uint64_t k, const Column* cols, int n_cols, uint64_t lead, uint64_t gap) {
  uint64_t per = static_cast<uint64_t>(n_cols - 1) + gap;
  for (int c = 0; c < n_cols; c++) per += 2 * cols[c].n + 2;
  return lead + k * per;
}

enum Code {
  kFine = 0,
  kNullArgument,
  kColumnCount,
  kRowCounts,
  kWidth,
  kReserved,
  kFlags,
  kFill,
  kDelimiter,
  kQuote,
  kLineBreak,
  kSame,
  kMask,
  kTableAlign,
  kOutAlign,
  kBadSums,
  kTooManyRows
};
// a: the column (kRowCounts: the first of the two, b the second; kWidth, kReserved, kTableAlign), or the value refused
struct Refusal {
  Code code;
  long long a, b;
};
inline Refusal check_call(const Column* cols, int n_cols, int delimiter, int quote, uint32_t always_mask, uint32_t raw_mask, unsigned flags, int fill,
                          uint64_t lead, uint64_t gap, const void* d_out, uint64_t out_cap, const uint64_t* d_out_begin, const uint64_t* d_out_end) {
  if (n_cols < 1 || n_cols > kMaxColumns) return Refusal{kColumnCount, n_cols, 0};
  if (!cols || (!d_out && out_cap)) return Refusal{kNullArgument, 0, 0};
  const uint64_t k = zip::rows_of(cols[0]);
  for (int c = 0; c < n_cols; c++) {
    const Column& col = cols[c];
    if (col.reserved != 0) return Refusal{kReserved, c, col.reserved};
    if (col.width != 0) return Refusal{kWidth, c, col.width};
    if (zip::rows_of(col) != k) return Refusal{kRowCounts, 0, c};
    if ((!col.text && col.n) || (k && (!col.rec_begin || !col.rec_end))) return Refusal{kNullArgument, c, 0};
    if ((reinterpret_cast<uintptr_t>(col.rec_begin) | reinterpret_cast<uintptr_t>(col.rec_end) | reinterpret_cast<uintptr_t>(col.indices)) & 7u)
      return Refusal{kTableAlign, c, 0};
  }
  if ((reinterpret_cast<uintptr_t>(d_out_begin) | reinterpret_cast<uintptr_t>(d_out_end)) & 7u) return Refusal{kTableAlign, -1, 0};
  if (flags != 0) return Refusal{kFlags, static_cast<long long>(flags), 0};
  if (fill < 0 || fill > 255) return Refusal{kFill, fill, 0};
  if (delimiter < 0 || delimiter > 255) return Refusal{kDelimiter, delimiter, 0};
  if (quote < 0 || quote > 255) return Refusal{kQuote, quote, 0};
  if (delimiter == '\n' || delimiter == '\r' || quote == '\n' || quote == '\r') return Refusal{kLineBreak, delimiter, quote};
  if (delimiter == quote) return Refusal{kSame, delimiter, 0};
  const uint32_t known = (1u << n_cols) - 1u;   // (n_cols <= 16)
  if (always_mask & ~known) return Refusal{kMask, 0, static_cast<long long>(always_mask)};
  if (raw_mask & ~known) return Refusal{kMask, 1, static_cast<long long>(raw_mask)};
  if (reinterpret_cast<uintptr_t>(d_out) & 15u) return Refusal{kOutAlign, 0, 0};
  if (!rows::rows_fit(k)) return Refusal{kTooManyRows, 0, 0};
  if (!sums_fit(k, cols, n_cols, lead, gap)) return Refusal{kBadSums, 0, 0};
  return Refusal{kFine, 0, 0};
}
// the message of a refusal (the library's and the CPU tests')
inline void refusal_message(char* buf, size_t room, const char* call, const Refusal& r, uint64_t k, int n_cols) {
  switch (r.code) {
    case kFine: snprintf(buf, room, "%s: fine", call); break;
    case kNullArgument: snprintf(buf, room, "%s: null argument", call); break;
    case kColumnCount: snprintf(buf, room, "%s: %lld columns: a call takes 1 to %d", call, r.a, kMaxColumns); break;
    case kRowCounts: snprintf(buf, room, "%s: column %lld and column %lld differ in their row counts", call, r.a, r.b); break;
    case kWidth: snprintf(buf, room, "%s: column %lld: width is %lld, it must be 0 (fields are not padded)", call, r.a, r.b); break;
    case kReserved: snprintf(buf, room, "%s: column %lld: reserved is %lld, it must be 0", call, r.a, r.b); break;
    case kFlags: snprintf(buf, room, "%s: flags %#llx: no flag is defined, flags must be 0", call, static_cast<unsigned long long>(r.a)); break;
    case kFill: snprintf(buf, room, "%s: fill %lld is not a byte (0..255)", call, r.a); break;
    case kDelimiter: snprintf(buf, room, "%s: delimiter %lld is not a byte (0..255)", call, r.a); break;
    case kQuote: snprintf(buf, room, "%s: quote %lld is not a byte (0..255)", call, r.a); break;
    case kLineBreak: snprintf(buf, room, "%s: delimiter %lld or quote %lld is a line break (\\n or \\r)", call, r.a, r.b); break;
    case kSame: snprintf(buf, room, "%s: delimiter and quote are the same byte %lld", call, r.a); break;
    case kMask:
      snprintf(buf, room, "%s: %s %#llx has a bit at or above n_cols = %d", call, r.a ? "raw_mask" : "always_mask", static_cast<unsigned long long>(r.b), n_cols);
      break;
    case kTableAlign:
      if (r.a < 0) snprintf(buf, room, "%s: d_out_begin or d_out_end is not 8-byte aligned", call);
      else snprintf(buf, room, "%s: column %lld: a table or d_indices is not 8-byte aligned", call, r.a);
      break;
    case kOutAlign: snprintf(buf, room, "%s: d_out is not 16-byte aligned", call); break;
    case kBadSums:
      snprintf(buf, room, "%s: %llu rows can exceed 2^62 output bytes (lead + k * R), or R = sum of (2 n + 2) + (C - 1) + gap reaches 2^42", call,
               static_cast<unsigned long long>(k));
      break;
    case kTooManyRows:
      snprintf(buf, room, "%s: %llu rows: the record calls that read rows take fewer than 2^31 of them", call, static_cast<unsigned long long>(k));
      break;
  }
}
inline void bad_row_message(char* buf, size_t room, const char* call, unsigned long long word) { zip::bad_row_message(buf, room, call, word); }

// ---------------------------------------------------------------------------------------------------------------- classify
RJ_PACK_HD inline uint32_t valid_bits(uint32_t valid) { return valid >= 16 ? 0xFFFFu : (1u << valid) - 1u; }
// of the first `valid` (1..16) bytes of a group: the quote bytes as bits / is one of them d, q, \r or \n
RJ_PACK_HD inline uint32_t quote_bits(const uint32_t w[4], uint32_t valid, uint32_t quote) { return csv::equal16(w, quote) & valid_bits(valid); }
RJ_PACK_HD inline bool group_special(const uint32_t w[4], uint32_t valid, uint32_t delimiter, uint32_t quote) {
  return ((csv::equal16(w, delimiter) | csv::equal16(w, quote) | csv::equal16(w, '\n') | csv::equal16(w, '\r')) & valid_bits(valid)) != 0;
}
// The groups g0, g0 + stride, ... of the piece text[src, src + len): a lane walks a short piece with g0 = 0, stride = 1, a
// lane of the wave tier with g0 = its number, stride = 64.  A group may read behind the piece's end, never behind the text's
// (rows::load_at); the bytes behind the piece do not count.
template <class Text>
RJ_PACK_HD inline void classify_groups(const Text& text, uint64_t n, uint64_t src, uint64_t len, uint64_t g0, uint64_t stride, uint32_t delimiter,
                                       uint32_t quote, bool* special, uint64_t* quotes) {
  const uint64_t g_end = rows::n_groups(len);
  for (uint64_t g = g0; g < g_end; g += stride) {
    uint32_t w[4];
    rows::load_at(text, n, src + g * rows::kGroupBytes, w);
    const uint64_t left = len - g * rows::kGroupBytes;
    const uint32_t valid = left < rows::kGroupBytes ? static_cast<uint32_t>(left) : 16u;
    *special |= group_special(w, valid, delimiter, quote);
    *quotes += csv::popcount(quote_bits(w, valid, quote));
  }
}
RJ_PACK_HD inline bool need_quotes(uint32_t n_cols, uint32_t always_mask, uint32_t c, uint64_t len, bool special) {
  return ((always_mask >> c) & 1u) != 0 || special || (n_cols == 1 && len == 0);
}

// ---------------------------------------------------------------------------------------------------------------- a row
RJ_PACK_HD inline bool is_raw(uint32_t raw_mask, uint32_t c) { return ((raw_mask >> c) & 1u) != 0; }
RJ_PACK_HD inline bool doubles(const Piece& p, bool raw) { return p.need && !raw && p.quotes != 0; }
// Column c of a row, its delimiter first: [sep0, open0) the delimiter (empty for column 0), [open0, data0) the opening quote
// (empty without need), [data0, data1) the content, [data1, end) the closing quote.  `at`: where the column begins.
struct Field {
  uint64_t sep0, open0, data0, data1, end;
};
RJ_PACK_HD inline Field field_at(uint64_t at, uint32_t c, const Piece& p, bool raw) {
  Field f;
  f.sep0 = at;
  f.open0 = at + (c ? 1 : 0);
  f.data0 = f.open0 + (p.need ? 1 : 0);
  f.data1 = f.data0 + p.len + (doubles(p, raw) ? p.quotes : 0);
  f.end = f.data1 + (p.need ? 1 : 0);
  return f;
}
RJ_PACK_HD inline uint64_t field_length(uint32_t c, const Piece& p, bool raw) { return field_at(0, c, p, raw).end; }

// Source: piece(j, c) -> Piece (the staged one), text_byte(c, s), load16(c, s, w) (16 bytes of column c's text at s, all
// inside its piece).
template <class Source>
RJ_PACK_HD inline uint64_t row_length(const Source& src, uint32_t n_cols, uint32_t raw_mask, uint64_t j) {
  uint64_t len = 0;
  for (uint32_t c = 0; c < n_cols; c++) len += field_length(c, src.piece(j, c), is_raw(raw_mask, c));
  return len;
}

enum Tier { kBytes = 0, kStream, kExpand };
RJ_PACK_HD inline Tier tier_of(const Piece& p, bool raw) { return p.len < kStreamBytes ? kBytes : doubles(p, raw) ? kExpand : kStream; }

// Row j at ob (its begin in the output), inside the chunk [c0, c1): every byte of it that the bytes tier writes goes to
// put(offset in the chunk, byte), once: the delimiters, the quotes around a field, the short pieces (doubled where they must
// be), the partial groups at the two ends of a piece that streams.  A piece that expands and touches the chunk goes to
// expand(j, c, data0): its content is expand_group's.  True: a piece that streams touches the chunk.
template <class Source, class Put, class Expand>
RJ_PACK_HD inline bool row_edges(const Source& src, uint32_t n_cols, uint32_t delimiter, uint32_t quote, uint32_t raw_mask, uint64_t j, uint64_t ob,
                                 uint64_t c0, uint64_t c1, const Put& put, const Expand& expand) {
  bool any_streamed = false;
  uint64_t at = ob;
  for (uint32_t c = 0; c < n_cols && at < c1; c++) {
    const Piece pc = src.piece(j, c);
    const bool raw = is_raw(raw_mask, c);
    const Field f = field_at(at, c, pc, raw);
    at = f.end;
    if (f.end <= c0) continue;
    if (f.sep0 < f.open0 && f.sep0 >= c0 && f.sep0 < c1) put(f.sep0 - c0, delimiter);
    if (f.open0 < f.data0 && f.open0 >= c0 && f.open0 < c1) put(f.open0 - c0, quote);
    if (f.data1 < f.end && f.data1 >= c0 && f.data1 < c1) put(f.data1 - c0, quote);
    const Tier tier = tier_of(pc, raw);
    if (tier == kExpand) {
      if (zip::touches(f.data0, f.data1, c0, c1)) expand(j, c, f.data0);
    } else if (tier == kBytes && doubles(pc, raw)) {
      uint64_t o = f.data0;
      for (uint64_t i = 0; i < pc.len && o < c1; i++, o++) {   // fewer than kStreamBytes steps
        const uint32_t b = static_cast<uint32_t>(src.text_byte(c, pc.src + i));
        if (o >= c0) put(o - c0, b);
        if (b == quote) {
          o++;
          if (o >= c0 && o < c1) put(o - c0, quote);
        }
      }
    } else {
      const bool streamed = tier == kStream;
      any_streamed |= streamed && zip::touches(f.data0, f.data1, c0, c1);
      const zip::Edges e = zip::edges(f.data0, f.data1, streamed, c0, c1);
      for (uint64_t p = e.h0; p < e.h1; p++) put(p - c0, static_cast<uint32_t>(src.text_byte(c, pc.src + (p - f.data0))));
      for (uint64_t p = e.t0; p < e.t1; p++) put(p - c0, static_cast<uint32_t>(src.text_byte(c, pc.src + (p - f.data0))));
    }
  }
  return any_streamed;
}

// The aligned 16-byte group [p, p + 16) of the output, p inside or behind row j at ob: true when the content of a piece that
// streams covers it whole -- then w has its 16 bytes from the piece's text: the zip's map with data0 behind the opening quote --,
// false when row_edges or expand_group wrote its bytes (or the fill did).
template <class Source>
RJ_PACK_HD inline bool group_streamed(const Source& src, uint32_t n_cols, uint32_t raw_mask, uint64_t j, uint64_t ob, uint64_t p, uint32_t w[4]) {
  uint64_t at = ob;
  for (uint32_t c = 0; c < n_cols && at <= p; c++) {
    const Piece pc = src.piece(j, c);
    const bool raw = is_raw(raw_mask, c);
    const Field f = field_at(at, c, pc, raw);
    at = f.end;
    if (p >= f.end) continue;
    if (p < f.data0 || p + pack::kGroupBytes > f.data1 || tier_of(pc, raw) != kStream) return false;
    src.load16(c, pc.src + (p - f.data0), w);
    return true;
  }
  return false;
}

// One lane's group of the expand walk: the `valid` (1..16) source bytes in w, qbits their quote bytes, out0 the output place
// of the first one (the content's begin + its source offset + the quote bytes in front of it in the piece).  Every byte, and
// behind a quote byte its double, goes to put(offset in the chunk, byte) when it lies in [c0, c1).
template <class Put>
RJ_PACK_HD inline void expand_group(const uint32_t w[4], uint32_t valid, uint32_t qbits, uint32_t quote, uint64_t out0, uint64_t c0, uint64_t c1,
                                    const Put& put) {
  if (out0 >= c1 || out0 + valid + csv::popcount(qbits) <= c0) return;
  uint64_t o = out0;
  for (uint32_t b = 0; b < valid; b++, o++) {
    if (o >= c0 && o < c1) put(o - c0, (w[b >> 2] >> (8 * (b & 3))) & 0xFFu);
    if ((qbits >> b) & 1u) {
      o++;
      if (o >= c0 && o < c1) put(o - c0, quote);
    }
  }
}

// The expand walk takes a piece in steps of kWaveStep source bytes; step s, with `before` quote bytes in front of it, makes the
// output bytes [data0 + s + before, ... + the step's bytes + its quote bytes).  A chunk that begins inside a checkpointed piece
// starts its walk at the step that makes the chunk's first byte.
struct Checkpoint {
  uint64_t s, before;
};
RJ_PACK_HD inline bool checkpointed(const Piece& p, bool raw) { return tier_of(p, raw) == kExpand && p.len >= kCheckpointBytes; }
// the first multiple of `chunk` at or behind `at`
RJ_PACK_HD inline uint64_t boundary_from(uint64_t at, uint64_t chunk) { return (at + chunk - 1) / chunk * chunk; }
// The walk of the chunk [c0, ...) over the piece whose content begins at data0 starts at the chunk's checkpoint when the chunk
// begins inside a checkpointed piece (the walk between plan and emit has written that entry), else at the piece's begin.
RJ_PACK_HD inline bool resumes(const Piece& p, bool raw, uint64_t data0, uint64_t c0) { return checkpointed(p, raw) && c0 >= data0; }

// byte i of T(j), i < len(j): the meaning of a row one byte at a time (the tests' cut-anywhere check; the kernels do not use
// it: it loops over a piece's length)
template <class Source>
RJ_PACK_HD inline uint32_t byte_at(const Source& src, uint32_t n_cols, uint32_t delimiter, uint32_t quote, uint32_t raw_mask, uint64_t j, uint64_t i) {
  uint64_t at = 0;
  for (uint32_t c = 0; c < n_cols; c++) {
    const Piece pc = src.piece(j, c);
    const bool raw = is_raw(raw_mask, c);
    const Field f = field_at(at, c, pc, raw);
    at = f.end;
    if (i >= f.end) continue;
    if (i < f.open0) return delimiter;
    if (i < f.data0 || i >= f.data1) return quote;
    if (!doubles(pc, raw)) return src.text_byte(c, pc.src + (i - f.data0));
    uint64_t o = f.data0;
    for (uint64_t s = 0; s < pc.len; s++, o++) {
      const uint32_t b = src.text_byte(c, pc.src + s);
      if (o == i) return b;
      if (b == quote && ++o == i) return quote;
    }
  }
  return quote;
}

}  // namespace csvf
}  // namespace rejit_amd
#endif
