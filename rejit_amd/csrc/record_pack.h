// rejit_amd/csrc/record_pack.h -- the arithmetic of rj_scan_records_pack (record_pack.hip): a list of records of one device
// text gathered into a new contiguous text, `gap` fill bytes behind each, `lead` in front.  Host and device code: the CPU
// tests drive exactly these functions (tests/support/pack_exec.cc), unit by unit and chunk by chunk as the kernels do.
//
// With k output records, r(j) the text record output record j takes and len(j) its length:
//     ob(0) = lead,   ob(j + 1) = ob(j) + len(j) + gap,   total = ob(k)
//     out[ob(j), ob(j) + len(j))        = text[rec_begin[r(j)], rec_end[r(j)])
//     out[ob(j) + len(j), ob(j + 1))    = fill      (and out[0, lead) = fill)
// The copy needs ONE table, ob, and the total: len(j) = ob(j + 1) - ob(j) - gap.  An output byte p belongs to the LAST j with
// ob(j) <= p (empty records with gap 0 share their ob with the record behind them: the last one is the one with bytes), so
// a piece of the output is found by one binary search, whatever the records' sizes -- nothing here loops over a record's
// length or over a run of empty records.
#ifndef REJIT_AMD_RECORD_PACK_H_
#define REJIT_AMD_RECORD_PACK_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define RJ_PACK_HD __host__ __device__
#else
#define RJ_PACK_HD
#endif

namespace rejit_amd {
namespace pack {

constexpr uint64_t kGroupBytes = 16;          // a lane produces 16 aligned output bytes at a time
// what the plan's look-back (tile_lookback.h) can carry: a group word sums 64 units of 256 rows in 56 bits, so a row adds less
// than 2^42; a prefix has 62 bits
constexpr uint64_t kMaxRow = 1ull << 42;
constexpr uint64_t kMaxTotal = 1ull << 62;

// ---------------------------------------------------------------------------------------------------------------- plan
// row j of the pack breaks the contract: its index names no record, or the record is not inside the text
RJ_PACK_HD inline bool bad_index(uint64_t r, uint64_t n_records) { return r >= n_records; }
RJ_PACK_HD inline bool bad_row(uint64_t rec_begin, uint64_t rec_end, uint64_t n) { return rec_begin > rec_end || rec_end > n; }
// what row j adds to the running output offset (a bad row adds nothing: the sums of a refused call still cannot overflow)
RJ_PACK_HD inline uint64_t row_advance(bool bad, uint64_t rec_begin, uint64_t rec_end, uint64_t gap) { return bad ? 0 : rec_end - rec_begin + gap; }

// a row adds at most n + gap (< kMaxRow), and lead + k * (n + gap) -- the most k good rows can add up to (rows may repeat) --
// stays below kMaxTotal
RJ_PACK_HD inline bool sums_fit(uint64_t k, uint64_t n, uint64_t lead, uint64_t gap) {
  if (n >= kMaxRow || gap >= kMaxRow || n + gap >= kMaxRow || lead >= kMaxTotal) return false;
  const uint64_t per = n + gap;
  if (k != 0 && per > (kMaxTotal - 1 - lead) / k) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- copy
// The ob table and the source begins as the searches see them: the tables in memory (src == nullptr: the source begin of j
// is rec_begin[indices ? indices[j] : j]) or a chunk's staged copy of rows [base, ...) including ob's row behind the last one.
struct View {
  const uint64_t* ob;          // ob[j - base]
  const uint64_t* src;         // staged: src[j - base]
  const uint64_t* rec_begin;   // not staged
  const uint64_t* indices;     // not staged; may be null
  uint64_t base;
  uint64_t k;                  // rows the ob array holds from `base` on are below this; ob(k) = total
  uint64_t total;
  RJ_PACK_HD uint64_t ob_at(uint64_t j) const { return j < k ? ob[j - base] : total; }
  RJ_PACK_HD uint64_t src_at(uint64_t j) const { return src ? src[j - base] : rec_begin[indices ? indices[j] : j]; }
};

// the first j in [lo, hi) with ob(j) > x (hi when none) / with ob(j) >= x
RJ_PACK_HD inline uint64_t upper_bound(const View& v, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (v.ob_at(mid) <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
RJ_PACK_HD inline uint64_t lower_bound(const View& v, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (v.ob_at(mid) < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The rows the output chunk [c0, c1) can touch: j0 = the last row that begins at or before c0 -- the record that reaches into
// the chunk -- or row 0 when the chunk begins inside the lead; j1 = the first row that begins at or behind c1.  The rows that
// begin inside the chunk lie between.  One search each in the whole table (the counterpart of records::tile_range).
struct Rows {
  uint64_t j0, j1;
};
RJ_PACK_HD inline uint64_t chunk_first_row(const View& table, uint64_t k, uint64_t c0) {
  const uint64_t u = upper_bound(table, 0, k, c0);
  return u ? u - 1 : 0;
}
RJ_PACK_HD inline uint64_t chunk_end_row(const View& table, uint64_t k, uint64_t j0, uint64_t c1) { return lower_bound(table, j0, k, c1); }
// rows a chunk stages: ob of [j0, j1] (the row behind the last one bounds it), the source begins of [j0, j1)
RJ_PACK_HD inline bool chunk_fits_stage(const Rows& r, uint64_t stage_cap) { return r.j1 - r.j0 < stage_cap; }

// The row around output byte p: out[ob, data_end) = the row's bytes, out[data_end, next) = fill.  Before the first row -- the
// lead, or an output without rows -- everything is fill and `row` is not called; else row(j) fetches what the caller keeps of
// row j besides its place (replace::locate_row builds on this one too).
struct RowAt {
  uint64_t ob, data_end, next;
};
template <class RowFn>
RJ_PACK_HD inline RowAt locate_row(const View& v, const Rows& r, uint64_t p, uint64_t gap, const RowFn& row) {
  const uint64_t u = upper_bound(v, r.j0, r.j1, p);
  RowAt at;
  if (u == r.j0) {
    at.ob = at.data_end = p;
    at.next = v.ob_at(r.j0);
    return at;
  }
  const uint64_t j = u - 1;
  at.ob = v.ob_at(j);
  at.next = v.ob_at(j + 1);
  at.data_end = at.next - gap;
  row(j);
  return at;
}

// The piece of the output around byte p: out[ob, data_end) = text[src + (p - ob)], out[data_end, next) = fill.
struct Piece {
  uint64_t ob, data_end, next, src;
};
RJ_PACK_HD inline Piece locate(const View& v, const Rows& r, uint64_t p, uint64_t gap) {
  uint64_t src = 0;
  const RowAt at = locate_row(v, r, p, gap, [&](uint64_t j) { src = v.src_at(j); });
  return Piece{at.ob, at.data_end, at.next, src};
}

RJ_PACK_HD inline uint32_t fill_word(uint32_t fill) { return fill * 0x01010101u; }
// byte b of the 16 in w becomes c
RJ_PACK_HD inline void put_byte(uint32_t w[4], uint32_t b, uint32_t c) {
  const uint32_t sh = 8 * (b & 3);
  w[b >> 2] = (w[b >> 2] & ~(0xFFu << sh)) | (c << sh);
}

// The 16 output bytes [p, p + 16), p a multiple of 16, of which those below `limit` (= min(total, out_cap)) matter: four
// little-endian words.  Text::load16(s, w) reads text[s, s + 16) -- all of it inside one record --, Text::byte(s) one byte.
// The common case -- all 16 inside one record -- is one load16; a group inside a gap or the lead reads nothing; a group with a
// seam in it goes byte by byte, and searches again only when it has crossed into the next piece.
// Returns 0: one load16, 1: fill only, 2: byte by byte.
template <class Text>
RJ_PACK_HD inline int group16(const View& v, const Rows& r, uint64_t p, uint64_t limit, uint64_t gap, uint32_t fill, const Text& text, uint32_t w[4]) {
  Piece pc = locate(v, r, p, gap);
  if (p + kGroupBytes <= pc.data_end) {
    text.load16(pc.src + (p - pc.ob), w);
    return 0;
  }
  const uint32_t fw = fill_word(fill);
  w[0] = w[1] = w[2] = w[3] = fw;
  if (p >= pc.data_end && p + kGroupBytes <= pc.next) return 1;
  for (uint32_t b = 0; b < kGroupBytes; b++) {
    const uint64_t q = p + b;
    if (q >= limit) break;
    if (q >= pc.next) pc = locate(v, r, q, gap);
    if (q < pc.data_end) put_byte(w, b, text.byte(pc.src + (q - pc.ob)));
  }
  return 2;
}

// An emit that makes its rows' bytes works chunk by chunk of the output: the part of the row at [ob, ob + len) that lies
// inside the chunk [c0, c1) is the row's bytes [*lo, *hi); false: none of it does.
RJ_PACK_HD inline bool chunk_part(uint64_t ob, uint32_t len, uint64_t c0, uint64_t c1, uint32_t* lo, uint32_t* hi) {
  if (ob >= c1 || ob + len <= c0) return false;
  *lo = ob < c0 ? static_cast<uint32_t>(c0 - ob) : 0u;
  *hi = ob + len > c1 ? static_cast<uint32_t>(c1 - ob) : len;
  return *lo < *hi;
}

// bytes of the group at p a lane stores: all 16 with one vector store, or the few below the limit one by one
RJ_PACK_HD inline uint32_t group_store_bytes(uint64_t p, uint64_t limit) { return limit - p >= kGroupBytes ? static_cast<uint32_t>(kGroupBytes) : static_cast<uint32_t>(limit - p); }

}  // namespace pack
}  // namespace rejit_amd
#endif
