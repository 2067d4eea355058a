// rejit_amd/csrc/record_zip.h -- the arithmetic of rj_scan_records_zip (record_zip.hip): the rows of C record tables put side
// by side into the lines of a new contiguous text -- Arrow's binary_join_element_wise, `paste -d`, awk's `print $3, $1`, the
// `%7d %s %s` of `uniq -c` -- the inverse of rj_scan_records_split.  Host and device code: the CPU tests drive exactly these
// functions (tests/support/zip_exec.cc), unit by unit and chunk by chunk as the kernels do.
//
// C columns, 1 <= C <= 16.  Column c is a record table over a device text of its own (d_text, n, d_rec_begin, d_rec_end,
// n_records), an optional index list (d_indices, n_indices) and a width; its rows are rj_scan_records_pack's: any order,
// repeats, a non-NULL list with count 0 is no rows, every row keeps begin <= end <= n and every index is < n_records.  Columns
// may share a text and a table.  Every column has the same row count k = d_indices ? n_indices : n_records.  With P(c, j) the
// bytes of column c's row j:
//     F(c, j) = P(c, j) padded to |width_c| bytes with the byte `pad`: on the LEFT for a positive width (%7d), on the RIGHT
//               for a negative one (%-7s); width 0, or a piece already that long, adds nothing.  Nothing is ever truncated.
//     T(j)    = F(0, j) sep F(1, j) sep ... F(C-1, j)            sep: 0..64 bytes, the same between every pair of columns
// The layout is the pack's (record_pack.h) with len(j) = |T(j)|:
//     ob(0) = lead,   ob(j + 1) = ob(j) + len(j) + gap,   total = ob(k)
//     out[ob(j), ob(j) + len(j)) = T(j), every other byte of out[0, total) = fill
// With C = 1 and width 0 this IS the pack, byte for byte and table row for table row, whatever sep is.
//
// A row is a sequence of SEGMENTS -- per column: the separator (not in front of column 0), the left padding, the piece, the
// right padding -- whose places follow from the C piece lengths alone (field_at): the bytes of T(j) in any range [a, b) are
// made without the bytes in front of a, so a row cut anywhere by an output chunk is made piecewise.  Two tiers by a
// segment's length: a piece or a padding of kStreamBytes or more STREAMS -- the 16-byte output groups it covers whole are
// made 16 bytes at a time from the group's own offset (group_streamed), only the partial groups at its two ends are bytes;
// every shorter segment, and every separator, is bytes (row_edges).  No loop here runs over a long segment's length.
#ifndef REJIT_AMD_RECORD_ZIP_H_
#define REJIT_AMD_RECORD_ZIP_H_

#include <stdint.h>
#include <stdio.h>

#include "record_pack.h"
#include "record_rows.h"

namespace rejit_amd {
namespace zip {

constexpr int kMaxColumns = 16;
constexpr uint64_t kMaxSep = 64;
constexpr int64_t kMaxWidth = 4096;
constexpr uint64_t kStreamBytes = 32;   // the tier threshold T: a segment this long covers at least one aligned 16-byte group whole
constexpr uint64_t kEmitChunk = 4096;   // output bytes per chunk of the emit: one pass of 256 lanes x 16 bytes

// rj_zip_column (include/rejit_hip.h), field for field: the kernels take the caller's array as it is
struct Column {
  const uint8_t* text;
  uint64_t n;
  const uint64_t* rec_begin;
  const uint64_t* rec_end;
  uint64_t n_records;
  const uint64_t* indices;
  uint64_t n_indices;
  int32_t width, reserved;
};
static_assert(sizeof(Column) == 64, "rj_zip_column has 64 bytes");
// the kernels' arguments: 16 x 64 + 64 bytes, no upload
struct Columns {
  Column col[kMaxColumns];
};
struct Sep {
  uint8_t byte[kMaxSep];
};
// what the plan stages per piece for the emit: where the piece begins in its column's text, and its length
struct Piece {
  uint64_t src, len;
};

RJ_PACK_HD inline uint64_t rows_of(const Column& c) { return c.indices ? c.n_indices : c.n_records; }
RJ_PACK_HD inline uint64_t abs_width(int32_t width) { return static_cast<uint64_t>(width < 0 ? -static_cast<int64_t>(width) : static_cast<int64_t>(width)); }

// ---------------------------------------------------------------------------------------------------------------- the call
// The first bad (row, column) of a call: the smallest j, and at that j the smallest c, is the LARGEST word (one atomic max
// per wave, record_frame.h); 0: none (j < 2^31, so a word is never 0).
RJ_PACK_HD inline unsigned long long bad_word(uint64_t j, uint32_t c) { return ~static_cast<unsigned long long>(j * kMaxColumns + c); }
RJ_PACK_HD inline uint64_t bad_row_of(unsigned long long word) { return static_cast<uint64_t>(~word) / kMaxColumns; }
RJ_PACK_HD inline uint32_t bad_column_of(unsigned long long word) { return static_cast<uint32_t>(static_cast<uint64_t>(~word) % kMaxColumns); }

// R = sum_c max(n_c, |width_c|) + (C - 1) sep_len + gap is the most a row adds (< pack::kMaxRow: the look-back's limit), and
// lead + k * R -- the most k good rows can add up to (rows may repeat) -- stays below pack::kMaxTotal
inline bool sums_fit(uint64_t k, const Column* cols, int n_cols, uint64_t sep_len, uint64_t lead, uint64_t gap) {
  uint64_t per = 0;
  for (int c = 0; c < n_cols; c++) {
    const uint64_t w = abs_width(cols[c].width), most = cols[c].n > w ? cols[c].n : w;
    if (most >= pack::kMaxRow) return false;
    per += most;   // (16 x 2^42 at the most)
  }
  per += static_cast<uint64_t>(n_cols - 1) * sep_len;
  if (gap >= pack::kMaxRow || per + gap >= pack::kMaxRow || lead >= pack::kMaxTotal) return false;
  per += gap;
  if (k != 0 && per > (pack::kMaxTotal - 1 - lead) / k) return false;
  return true;
}

enum Code {
  kFine = 0,
  kNullArgument,
  kColumnCount,
  kRowCounts,
  kSepLength,
  kWidth,
  kReserved,
  kFlags,
  kPad,
  kFill,
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
inline Refusal check_call(const Column* cols, int n_cols, const char* sep, uint64_t sep_len, int pad, unsigned flags, int fill, uint64_t lead, uint64_t gap,
                          const void* d_out, uint64_t out_cap, const uint64_t* d_out_begin, const uint64_t* d_out_end) {
  if (n_cols < 1 || n_cols > kMaxColumns) return Refusal{kColumnCount, n_cols, 0};
  if (!cols || (!sep && sep_len) || (!d_out && out_cap)) return Refusal{kNullArgument, 0, 0};
  if (sep_len > kMaxSep) return Refusal{kSepLength, static_cast<long long>(sep_len < (1ull << 62) ? sep_len : (1ull << 62)), 0};
  const uint64_t k = rows_of(cols[0]);
  for (int c = 0; c < n_cols; c++) {
    const Column& col = cols[c];
    if (col.reserved != 0) return Refusal{kReserved, c, col.reserved};
    if (abs_width(col.width) > static_cast<uint64_t>(kMaxWidth)) return Refusal{kWidth, c, col.width};
    if (rows_of(col) != k) return Refusal{kRowCounts, 0, c};
    if ((!col.text && col.n) || (k && (!col.rec_begin || !col.rec_end))) return Refusal{kNullArgument, c, 0};
    if ((reinterpret_cast<uintptr_t>(col.rec_begin) | reinterpret_cast<uintptr_t>(col.rec_end) | reinterpret_cast<uintptr_t>(col.indices)) & 7u)
      return Refusal{kTableAlign, c, 0};
  }
  if ((reinterpret_cast<uintptr_t>(d_out_begin) | reinterpret_cast<uintptr_t>(d_out_end)) & 7u) return Refusal{kTableAlign, -1, 0};
  if (flags != 0) return Refusal{kFlags, static_cast<long long>(flags), 0};
  if (pad < 0 || pad > 255) return Refusal{kPad, pad, 0};
  if (fill < 0 || fill > 255) return Refusal{kFill, fill, 0};
  if (reinterpret_cast<uintptr_t>(d_out) & 15u) return Refusal{kOutAlign, 0, 0};
  if (!rows::rows_fit(k)) return Refusal{kTooManyRows, 0, 0};
  if (!sums_fit(k, cols, n_cols, sep_len, lead, gap)) return Refusal{kBadSums, 0, 0};
  return Refusal{kFine, 0, 0};
}
// the message of a refusal (the library's and the CPU tests')
inline void refusal_message(char* buf, size_t room, const char* call, const Refusal& r, uint64_t k) {
  switch (r.code) {
    case kFine: snprintf(buf, room, "%s: fine", call); break;
    case kNullArgument: snprintf(buf, room, "%s: null argument", call); break;
    case kColumnCount: snprintf(buf, room, "%s: %lld columns: a call takes 1 to %d", call, r.a, kMaxColumns); break;
    case kRowCounts: snprintf(buf, room, "%s: column %lld and column %lld differ in their row counts", call, r.a, r.b); break;
    case kSepLength: snprintf(buf, room, "%s: sep_len %lld: a separator has at most %llu bytes", call, r.a, static_cast<unsigned long long>(kMaxSep)); break;
    case kWidth: snprintf(buf, room, "%s: column %lld: width %lld is outside -%lld..%lld", call, r.a, r.b, static_cast<long long>(kMaxWidth), static_cast<long long>(kMaxWidth)); break;
    case kReserved: snprintf(buf, room, "%s: column %lld: reserved is %lld, it must be 0", call, r.a, r.b); break;
    case kFlags: snprintf(buf, room, "%s: flags %#llx: no flag is defined, flags must be 0", call, static_cast<unsigned long long>(r.a)); break;
    case kPad: snprintf(buf, room, "%s: pad %lld is not a byte (0..255)", call, r.a); break;
    case kFill: snprintf(buf, room, "%s: fill %lld is not a byte (0..255)", call, r.a); break;
    case kTableAlign:
      if (r.a < 0) snprintf(buf, room, "%s: d_out_begin or d_out_end is not 8-byte aligned", call);
      else snprintf(buf, room, "%s: column %lld: a table or d_indices is not 8-byte aligned", call, r.a);
      break;
    case kOutAlign: snprintf(buf, room, "%s: d_out is not 16-byte aligned", call); break;
    case kBadSums:
      snprintf(buf, room, "%s: %llu rows can exceed 2^62 output bytes (lead + k * R), or R = sum of max(n, |width|) + (C - 1) * sep_len + gap reaches 2^42", call,
               static_cast<unsigned long long>(k));
      break;
    case kTooManyRows:
      snprintf(buf, room, "%s: %llu rows: the record calls that read rows take fewer than 2^31 of them", call, static_cast<unsigned long long>(k));
      break;
  }
}
inline void bad_row_message(char* buf, size_t room, const char* call, unsigned long long word) {
  snprintf(buf, room, "%s: row %llu column %u names no record or a record outside its text (index < n_records, begin <= end <= n)", call,
           static_cast<unsigned long long>(bad_row_of(word)), bad_column_of(word));
}

// ---------------------------------------------------------------------------------------------------------------- a row
// Column c of a row, c's separator first: [sep0, pad0) the separator (empty for column 0), [pad0, data0) the left padding,
// [data0, data1) the piece, [data1, end) the right padding.  `at`: where the column begins (the end of column c - 1), in
// any coordinate -- the row's own, or the output's.
struct Field {
  uint64_t sep0, pad0, data0, data1, end;
};
RJ_PACK_HD inline Field field_at(uint64_t at, uint32_t c, uint64_t piece_len, int32_t width, uint64_t sep_len) {
  const uint64_t w = abs_width(width), padding = w > piece_len ? w - piece_len : 0;
  Field f;
  f.sep0 = at;
  f.pad0 = at + (c ? sep_len : 0);
  f.data0 = f.pad0 + (width > 0 ? padding : 0);
  f.data1 = f.data0 + piece_len;
  f.end = f.data1 + (width < 0 ? padding : 0);
  return f;
}
// what column c adds to len(j)
RJ_PACK_HD inline uint64_t field_length(uint32_t c, uint64_t piece_len, int32_t width, uint64_t sep_len) { return field_at(0, c, piece_len, width, sep_len).end; }

// Source: piece(j, c) -> Piece (the staged one), width(c), sep_byte(i), text_byte(c, s), load16(c, s, w) (16 bytes of column
// c's text at s, all inside its piece: record_frame.h's DeviceText on the device).
// len(j)
template <class Source>
RJ_PACK_HD inline uint64_t row_length(const Source& src, uint32_t n_cols, uint64_t sep_len, uint64_t j) {
  uint64_t len = 0;
  for (uint32_t c = 0; c < n_cols; c++) len += field_length(c, src.piece(j, c).len, src.width(c), sep_len);
  return len;
}

RJ_PACK_HD inline bool streams(uint64_t len) { return len >= kStreamBytes; }
// Of the segment [s0, s1) of the output, the bytes inside the chunk [c0, c1) that are written as BYTES: all of it, or -- when it
// streams -- the head [s0, up16(s0)) and the tail [down16(s1), s1), the partial 16-byte groups at its ends (up16(s0) <=
// down16(s1): it has kStreamBytes at least).  Both ranges are clipped to the chunk and may be empty (h0 >= h1, t0 >= t1).
struct Edges {
  uint64_t h0, h1, t0, t1;
};
RJ_PACK_HD inline Edges edges(uint64_t s0, uint64_t s1, bool streamed, uint64_t c0, uint64_t c1) {
  const uint64_t head_end = streamed ? (s0 + 15) & ~15ull : s1, tail_begin = streamed ? s1 & ~15ull : s1;
  Edges e;
  e.h0 = s0 > c0 ? s0 : c0;
  e.h1 = head_end < c1 ? head_end : c1;
  e.t0 = tail_begin > c0 ? tail_begin : c0;
  e.t1 = s1 < c1 ? s1 : c1;
  return e;
}
RJ_PACK_HD inline bool touches(uint64_t s0, uint64_t s1, uint64_t c0, uint64_t c1) { return (s0 > c0 ? s0 : c0) < (s1 < c1 ? s1 : c1); }

// Row j at ob (its begin in the output), inside the chunk [c0, c1): every byte of it that is written as a byte goes to
// put(offset in the chunk, byte), once.  True: a segment that streams touches the chunk (its whole groups are group_streamed's).
// The loops run over a column count, a separator, a short segment or a partial group: 64 steps at the most.
template <class Source, class Put>
RJ_PACK_HD inline bool row_edges(const Source& src, uint32_t n_cols, uint64_t sep_len, uint32_t pad, uint64_t j, uint64_t ob, uint64_t c0, uint64_t c1,
                                 const Put& put) {
  bool any_streamed = false;
  uint64_t at = ob;
  for (uint32_t c = 0; c < n_cols && at < c1; c++) {
    const Piece pc = src.piece(j, c);
    const Field f = field_at(at, c, pc.len, src.width(c), sep_len);
    at = f.end;
    if (f.end <= c0) continue;
    {
      const Edges e = edges(f.sep0, f.pad0, false, c0, c1);
      for (uint64_t q = e.h0; q < e.h1; q++) put(q - c0, static_cast<uint32_t>(src.sep_byte(static_cast<uint32_t>(q - f.sep0))));
    }
    for (int side = 0; side < 2; side++) {   // the left and the right padding (one of them is empty)
      const uint64_t s0 = side ? f.data1 : f.pad0, s1 = side ? f.end : f.data0;
      const bool streamed = streams(s1 - s0);
      any_streamed |= streamed && touches(s0, s1, c0, c1);
      const Edges e = edges(s0, s1, streamed, c0, c1);
      for (uint64_t q = e.h0; q < e.h1; q++) put(q - c0, pad);
      for (uint64_t q = e.t0; q < e.t1; q++) put(q - c0, pad);
    }
    {
      const bool streamed = streams(pc.len);
      any_streamed |= streamed && touches(f.data0, f.data1, c0, c1);
      const Edges e = edges(f.data0, f.data1, streamed, c0, c1);
      for (uint64_t q = e.h0; q < e.h1; q++) put(q - c0, static_cast<uint32_t>(src.text_byte(c, pc.src + (q - f.data0))));
      for (uint64_t q = e.t0; q < e.t1; q++) put(q - c0, static_cast<uint32_t>(src.text_byte(c, pc.src + (q - f.data0))));
    }
  }
  return any_streamed;
}

// The aligned 16-byte group [p, p + 16) of the output, p inside or behind row j at ob: true when a segment that streams covers
// it whole -- then w has its 16 bytes: 16 bytes of a piece from its text, or the padding byte --, false when row_edges wrote
// its bytes (or the fill did).
template <class Source>
RJ_PACK_HD inline bool group_streamed(const Source& src, uint32_t n_cols, uint64_t sep_len, uint32_t pad, uint64_t j, uint64_t ob, uint64_t p, uint32_t w[4]) {
  uint64_t at = ob;
  for (uint32_t c = 0; c < n_cols && at <= p; c++) {
    const Piece pc = src.piece(j, c);
    const Field f = field_at(at, c, pc.len, src.width(c), sep_len);
    at = f.end;
    if (p >= f.end) continue;
    if (p >= f.data0 && p + pack::kGroupBytes <= f.data1) {
      if (!streams(pc.len)) return false;
      src.load16(c, pc.src + (p - f.data0), w);
      return true;
    }
    const bool left = p >= f.pad0 && p + pack::kGroupBytes <= f.data0 && streams(f.data0 - f.pad0);
    const bool right = p >= f.data1 && p + pack::kGroupBytes <= f.end && streams(f.end - f.data1);
    if (!left && !right) return false;
    w[0] = w[1] = w[2] = w[3] = pack::fill_word(pad);
    return true;
  }
  return false;
}

// byte i of T(j), i < len(j): the meaning of a row one byte at a time (the tests' cut-anywhere check; the kernels do not use it)
template <class Source>
RJ_PACK_HD inline uint32_t byte_at(const Source& src, uint32_t n_cols, uint64_t sep_len, uint32_t pad, uint64_t j, uint64_t i) {
  uint64_t at = 0;
  for (uint32_t c = 0; c < n_cols; c++) {
    const Piece pc = src.piece(j, c);
    const Field f = field_at(at, c, pc.len, src.width(c), sep_len);
    at = f.end;
    if (i >= f.end) continue;
    if (i < f.pad0) return src.sep_byte(static_cast<uint32_t>(i - f.sep0));
    if (i >= f.data0 && i < f.data1) return src.text_byte(c, pc.src + (i - f.data0));
    return pad;
  }
  return pad;
}

}  // namespace zip
}  // namespace rejit_amd
#endif
