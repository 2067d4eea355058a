// rejit_amd/csrc/record_split.h -- the arithmetic of rj_scan_records_split (record_split.hip): the fields or the matches of the
// chosen records as a PIECE TABLE -- a record table over the same device text whose rows are the pieces, plus Arrow-style
// offsets (piece_first) that say which pieces belong to which row.  Host and device code: the CPU tests drive exactly these
// functions (tests/support/split_exec.cc), unit by unit and chunk by chunk as the kernels do.
//
// Row j takes record r(j) = [rb, re) with its own matches (b_t, e_t) = spans[f + t], t < c (f = first[r], c = count[r]):
//     kBetween: c + 1 pieces, piece t = [t == 0 ? rb : e_{t-1}, t == c ? re : b_t)     -- what the replace copies as text
//     kMatches: c pieces,     piece t = [b_t, e_t)
//     piece_first[0] = 0, piece_first[j + 1] = piece_first[j] + (pieces of row j), P = piece_first[k]
// piece_first is an `ob` table in record_pack.h's sense (lead 0, gap 0, a row's length = its pieces): piece p belongs to the
// LAST j with piece_first[j] <= p -- rows without a piece (kMatches, c == 0) share their offset with the row behind them, as
// empty records do at gap 0 -- so a piece is found by one binary search and t = p - piece_first[j].  Nothing here loops over a
// row's matches or over a run of rows without any.
#ifndef REJIT_AMD_RECORD_SPLIT_H_
#define REJIT_AMD_RECORD_SPLIT_H_

#include <stdint.h>

#include "record_pack.h"
#include "record_replace.h"

namespace rejit_amd {
namespace split {

enum What : int { kBetween = 0, kMatches = 1 };

// The plan's look-back (tile_lookback.h) sums 64 units of 256 rows in a 56-bit group word: a row adds at most m + 1 pieces and
// a count below UINT32_MAX, so fewer than 2^32 -- 2^14 rows of them stay below 2^46.  A prefix has 62 bits: k * (m + 1), the
// most k rows can add up to (rows may repeat), stays below kMaxTotal.  k < kMaxRows: the row shares a word with its kind.
static_assert((64ull * 256) << 32 < (1ull << 56), "a group of the look-back carries 64 units of 256 rows of fewer than 2^32 pieces");
RJ_PACK_HD inline bool sums_fit(uint64_t k, uint64_t m) {
  if (k >= replace::kMaxRows || m >= pack::kMaxTotal) return false;
  if (k != 0 && m + 1 > (pack::kMaxTotal - 1) / k) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- plan
// Mem is what the plan and the emit read: rec_begin(r), rec_end(r), first(r), count(r), index(j), span_begin(g), span_end(g)
// -- and table(g), which replace::plan_row asks for where it works out the replaced length: the split has no such table, its
// Mem answers 0 and the length is not looked at.  The row's CHECKS are that function's, for both values of `what`.
struct RowPlan {
  uint32_t kind;     // replace::Kind
  uint64_t pieces;
};
template <class Mem>
RJ_PACK_HD inline RowPlan plan_row(const Mem& M, int what, uint64_t j, bool have_indices, uint64_t n_records, uint64_t n, uint64_t m) {
  const replace::RowPlan p = replace::plan_row(M, j, have_indices, n_records, n, m);
  if (p.kind != replace::kOk) return RowPlan{p.kind, 0};
  const uint64_t c = M.count(have_indices ? M.index(j) : j);
  return RowPlan{replace::kOk, what == kBetween ? c + 1 : c};
}

// ---------------------------------------------------------------------------------------------------------------- emit
// what a chunk stages per row besides its piece_first (null: read through Mem)
struct Stage {
  const uint64_t* rb;
  const uint64_t* re;
  const uint64_t* first;
  const uint32_t* count;
};
struct RowInfo {
  uint64_t rb, re, f;
  uint32_t c;
};
template <class Mem>
RJ_PACK_HD inline RowInfo row_info(const Mem& M, uint64_t j, bool have_indices) {
  const uint64_t r = have_indices ? M.index(j) : j;
  return RowInfo{M.rec_begin(r), M.rec_end(r), M.first(r), M.count(r)};
}

// the pieces [c0, c1) of a chunk and the rows r = [j0, j1) that touch it (pack::chunk_first_row / chunk_end_row): piece p's
// row -- the last j in r with piece_first[j] <= p; piece_first[j0] <= c0 <= p, so there is one -- and its place t in it
struct PieceAt {
  uint64_t j, t;
};
RJ_PACK_HD inline PieceAt locate_piece(const pack::View& v, const pack::Rows& r, uint64_t p) {
  const uint64_t j = pack::upper_bound(v, r.j0, r.j1, p) - 1;
  return PieceAt{j, p - v.ob_at(j)};
}

struct Piece {
  uint64_t begin, end;
};
// piece t of a row: one (kMatches, and kBetween at either end of the row) or two 8-byte reads of the list
template <class Mem>
RJ_PACK_HD inline Piece piece_of(const Mem& M, int what, const RowInfo& x, uint64_t t) {
  if (what == kMatches) return Piece{M.span_begin(x.f + t), M.span_end(x.f + t)};
  return Piece{t == 0 ? x.rb : M.span_end(x.f + t - 1), t == x.c ? x.re : M.span_begin(x.f + t)};
}

template <class Mem>
RJ_PACK_HD inline Piece piece(const pack::View& v, const Stage& st, const Mem& M, int what, bool have_indices, const pack::Rows& r, uint64_t p) {
  const PieceAt at = locate_piece(v, r, p);
  const uint64_t i = at.j - v.base;
  const RowInfo x = st.first ? RowInfo{st.rb[i], st.re[i], st.first[i], st.count[i]} : row_info(M, at.j, have_indices);
  return piece_of(M, what, x, at.t);
}

}  // namespace split
}  // namespace rejit_amd
#endif
