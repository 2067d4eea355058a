// rejit_amd/csrc/record_replace.h -- the arithmetic of rj_scan_records_replace (record_replace.hip): the pack of record_pack.h
// in which every packed record has its OWN matches (spans[first[r], first[r] + count[r]) of the scan's list, as rj_scan_records
// wrote them) replaced by `with`.  Host and device code: the CPU tests drive exactly these functions
// (tests/support/replace_exec.cc), unit by unit and chunk by chunk as the kernels do.
//
// ONE table over the match list, m + 1 entries (begin_m := n, W = with_len):
//     D[g] = begin_g - removed[g] + g * W,        removed[g] = the lengths of the matches before g
// -- where match g's replacement begins in the whole-text replace.  D never decreases (D[g + 1] - D[g] = the text between the
// two matches + W), and in wrapping 64-bit arithmetic everything about a row with record [rb, re), first match f and c matches
// follows from it and the spans:
//     len'  = (re - rb) - (begin_{f+c} - begin_f) + (D[f + c] - D[f])                  the replaced record's length
//     u(t)  = D[f + t] - base,   base = D[f] - (begin_f - rb)                           where match t's replacement begins in it
// The output is the pack's: ob(0) = lead, ob(j + 1) = ob(j) + len'(j) + gap.  An output byte p is found by two binary searches
// -- the pack's on ob for the row, one on D[f, f + c) for the last t with u(t) <= p - ob -- and is one of: text before the first
// match, with[q - u(t)], text at end_{f+t} + (q - u(t) - W), or fill.  Nothing here loops over a record's length, over a run of
// empty records or over a record's matches.
//
// A length that is no length (begin > end, or end > n: a list of another text) counts as 0 in `removed`; no accepted row holds
// such a match (the plan checks the row's first begin and last end against the record, the list is an ordered selection), and
// only differences inside a row are ever used.
#ifndef REJIT_AMD_RECORD_REPLACE_H_
#define REJIT_AMD_RECORD_REPLACE_H_

#include <stdint.h>

#include "record_pack.h"

namespace rejit_amd {
namespace replace {

using pack::kGroupBytes;
using pack::kMaxRow;
using pack::kMaxTotal;
// the first bad row and its kind travel in one word, (kMaxRows - 1 - j) << 3 | kind, so that one atomic max keeps the first
constexpr uint64_t kMaxRows = 1ull << 60;
constexpr uint64_t kTableUnit = 256;   // matches per unit of the table kernel

// why row j is refused (the first check that fails)
enum Kind : uint32_t {
  kOk = 0,
  kBadIndex,       // the index names no record
  kBadRow,         // the record is not inside the text
  kSaturated,      // count == UINT32_MAX: the range is unknown
  kBadRange,       // first + count reaches beyond the list
  kBeginsBefore,   // the row's first match begins before the record
  kCrosses         // the row's last match ends beyond the record
};

RJ_PACK_HD inline uint64_t bad_word(uint64_t j, uint32_t kind) { return ((kMaxRows - 1 - j) << 3) | kind; }
RJ_PACK_HD inline uint64_t bad_word_row(uint64_t w) { return kMaxRows - 1 - (w >> 3); }
RJ_PACK_HD inline uint32_t bad_word_kind(uint64_t w) { return static_cast<uint32_t>(w & 7u); }

// a row adds at most n + m * W + gap; per = n + (m + 1) * W + gap stays below kMaxRow, lead + k * per below kMaxTotal
RJ_PACK_HD inline bool sums_fit(uint64_t k, uint64_t n, uint64_t m, uint64_t with_len, uint64_t lead, uint64_t gap) {
  if (k >= kMaxRows || n >= kMaxRow || gap >= kMaxRow || with_len >= kMaxRow || m >= kMaxRow || lead >= kMaxTotal) return false;
  if (with_len != 0 && m + 1 > (kMaxRow - 1) / with_len) return false;
  const uint64_t per = n + (m + 1) * with_len + gap;   // (three terms below 2^42 each)
  if (per >= kMaxRow) return false;
  if (k != 0 && per > (kMaxTotal - 1 - lead) / k) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- table
RJ_PACK_HD inline uint64_t match_length(uint64_t begin, uint64_t end, uint64_t n) { return begin <= end && end <= n ? end - begin : 0; }
RJ_PACK_HD inline uint64_t table_entry(uint64_t begin, uint64_t removed_before, uint64_t g, uint64_t with_len) {
  return begin - removed_before + g * with_len;
}

// ---------------------------------------------------------------------------------------------------------------- plan
// Mem is what the plan and the copy read: rec_begin(r), rec_end(r), first(r), count(r), index(j), span_begin(g), span_end(g),
// table(g) (= D[g]) and with_byte(i).  The kernels hand in plain pointers, the CPU driver a checked copy.
struct RowPlan {
  uint32_t kind;
  uint64_t len;   // len'
};
template <class Mem>
RJ_PACK_HD inline RowPlan plan_row(const Mem& M, uint64_t j, bool have_indices, uint64_t n_records, uint64_t n, uint64_t m) {
  RowPlan p{kOk, 0};
  const uint64_t r = have_indices ? M.index(j) : j;
  if (pack::bad_index(r, n_records)) return RowPlan{kBadIndex, 0};
  const uint64_t rb = M.rec_begin(r), re = M.rec_end(r);
  if (pack::bad_row(rb, re, n)) return RowPlan{kBadRow, 0};
  const uint64_t f = M.first(r);
  const uint64_t c = M.count(r);
  if (c == 0xFFFFFFFFull) return RowPlan{kSaturated, 0};   // (before the range: a saturated count is no count to add to first)
  if (f > m || c > m - f) return RowPlan{kBadRange, 0};
  p.len = re - rb;
  if (c == 0) return p;
  const uint64_t bf = M.span_begin(f);
  if (bf < rb) return RowPlan{kBeginsBefore, 0};
  if (M.span_end(f + c - 1) > re) return RowPlan{kCrosses, 0};
  const uint64_t bn = f + c < m ? M.span_begin(f + c) : n;
  p.len = (re - rb) - (bn - bf) + (M.table(f + c) - M.table(f));
  return p;
}

// ---------------------------------------------------------------------------------------------------------------- copy
// what a chunk stages per row besides the pack's ob and source begin (null: read through Mem)
struct Stage {
  const uint64_t* first;
  const uint64_t* base;
  const uint32_t* count;
};

struct RowInfo {
  uint64_t rb, f, base;
  uint32_t c;
};
template <class Mem>
RJ_PACK_HD inline RowInfo row_info(const Mem& M, uint64_t j, bool have_indices) {
  const uint64_t r = have_indices ? M.index(j) : j;
  RowInfo x;
  x.rb = M.rec_begin(r);
  x.c = M.count(r);
  x.f = x.c ? M.first(r) : 0;
  x.base = x.c ? M.table(x.f) - (M.span_begin(x.f) - x.rb) : 0;
  return x;
}

// the row around output byte p: out[ob, data_end) = the replaced record, out[data_end, next) = fill
struct Row {
  uint64_t ob, data_end, next;
  RowInfo x;
};
template <class Mem>
RJ_PACK_HD inline Row locate_row(const pack::View& v, const Stage& st, const Mem& M, bool have_indices, const pack::Rows& r, uint64_t p, uint64_t gap) {
  RowInfo x{0, 0, 0, 0};
  const pack::RowAt at = pack::locate_row(v, r, p, gap, [&](uint64_t j) {
    if (st.first) {
      x = RowInfo{v.src[j - v.base], st.first[j - v.base], st.base[j - v.base], st.count[j - v.base]};
    } else {
      x = row_info(M, j, have_indices);
    }
  });
  return Row{at.ob, at.data_end, at.next, x};
}

// The piece of the row around output byte p (ob <= p < next): out[begin, end) is text[src, ...), with[0, W) or fill.
enum { kText = 0, kWith = 1, kFill = 2 };
struct Piece {
  int kind;
  uint64_t begin, end, src;
};
template <class Mem>
RJ_PACK_HD inline Piece locate_piece(const Mem& M, const Row& row, uint64_t p, uint64_t with_len) {
  if (p >= row.data_end) return Piece{kFill, row.data_end, row.next, 0};
  const RowInfo& x = row.x;
  if (x.c == 0) return Piece{kText, row.ob, row.data_end, x.rb};
  const uint64_t q = p - row.ob;
  uint64_t lo = 0, hi = x.c;   // the matches t below lo have u(t) <= q
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (M.table(x.f + mid) - x.base <= q) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return Piece{kText, row.ob, row.ob + (M.table(x.f) - x.base), x.rb};
  const uint64_t t = lo - 1;
  const uint64_t u = M.table(x.f + t) - x.base;
  if (q - u < with_len) return Piece{kWith, row.ob + u, row.ob + u + with_len, 0};
  const uint64_t end = t + 1 < x.c ? row.ob + (M.table(x.f + t + 1) - x.base) : row.data_end;
  return Piece{kText, row.ob + u + with_len, end, M.span_end(x.f + t)};
}

// The 16 output bytes [p, p + 16), p a multiple of 16, of which those below `limit` (= min(total, out_cap)) matter: four
// little-endian words, as pack::group16.  All 16 inside one text piece is one load16; all 16 inside a gap or the lead reads
// nothing; anything else goes byte by byte and searches again only when it has crossed into the next piece (the row again
// only when it has left the row).  Returns 0: one load16, 1: fill only, 2: byte by byte.
template <class Mem, class Text>
RJ_PACK_HD inline int group16(const pack::View& v, const Stage& st, const Mem& M, bool have_indices, const pack::Rows& r, uint64_t p, uint64_t limit,
                              uint64_t gap, uint32_t fill, uint64_t with_len, const Text& text, uint32_t w[4]) {
  Row row = locate_row(v, st, M, have_indices, r, p, gap);
  Piece pc = locate_piece(M, row, p, with_len);
  if (pc.kind == kText && p + kGroupBytes <= pc.end) {
    text.load16(pc.src + (p - pc.begin), w);
    return 0;
  }
  const uint32_t fw = pack::fill_word(fill);
  w[0] = w[1] = w[2] = w[3] = fw;
  if (pc.kind == kFill && p + kGroupBytes <= pc.end) return 1;
  for (uint32_t b = 0; b < kGroupBytes; b++) {
    const uint64_t q = p + b;
    if (q >= limit) break;
    if (q >= pc.end) {
      if (q >= row.next) row = locate_row(v, st, M, have_indices, r, q, gap);
      pc = locate_piece(M, row, q, with_len);
    }
    if (pc.kind != kFill) pack::put_byte(w, b, pc.kind == kText ? text.byte(pc.src + (q - pc.begin)) : M.with_byte(q - pc.begin));
  }
  return 2;
}

}  // namespace replace
}  // namespace rejit_amd
#endif
