// rejit_amd/csrc/record_join.h -- the rule that hands the matches of ONE whole-text run to the caller's records, and the
// searches the join kernel (record_join.hip) makes for it.  Host and device code: the CPU tests drive exactly these
// functions (tests/support/record_exec.cc), tile by tile as the kernel does.
//
// Records are text[rec_begin[i], rec_end[i]), ascending and not overlapping (rec_begin[i] <= rec_end[i] <= rec_begin[i+1],
// rec_end[last] <= n; gaps allowed).  A match belongs to the record of its BEGIN b: the last i with rec_begin[i] <= b, and
// only if b <= rec_end[i] (else it lies in a gap) -- finish_packed's rule (host_api.hip).  With lb(x) = the number of
// matches whose begin is below x (the list is ascending by begin):
//     first[i] = lb(rec_begin[i])
//     count[i] = lb(min(rec_end[i] + 1, rec_begin[i + 1])) - first[i]          (rec_begin[n_records] = infinity)
// so an empty match at a record's end is the record's own when a gap follows, the next record's when the two touch.
// The list is a non-overlapping selection (end[k] <= begin[k + 1]): a kept match that ends beyond rec_end[i] is followed
// by matches that begin beyond it, so only the LAST kept match of a record can cross its end.
#ifndef REJIT_AMD_RECORD_JOIN_H_
#define REJIT_AMD_RECORD_JOIN_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define RJ_RECORD_HD __host__ __device__
#else
#define RJ_RECORD_HD
#endif

namespace rejit_amd {
namespace records {

// The begins [base, base + ...) of the match list as the searches see them: the scan's own list of (begin, end) pairs
// (stride 2, base 0) or a tile's staged copy of a range of begins (stride 1, base = the range's first match).
struct Begins {
  const uint64_t* p;
  uint64_t stride;
  uint64_t base;
  RJ_RECORD_HD uint64_t operator[](uint64_t k) const { return p[(k - base) * stride]; }
};

// the number of matches in [lo, hi) whose begin is below x, plus lo
RJ_RECORD_HD inline uint64_t lower_bound(const Begins& b, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (b[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the begins of record i's matches are below this bound (and at or above rec_begin[i])
RJ_RECORD_HD inline uint64_t upper_key(uint64_t rec_end, bool has_next, uint64_t next_begin) {
  const uint64_t own = rec_end == ~0ull ? ~0ull : rec_end + 1;
  return has_next && next_begin < own ? next_begin : own;
}

// row i breaks the table's contract
RJ_RECORD_HD inline bool bad_row(uint64_t rec_begin, uint64_t rec_end, bool has_next, uint64_t next_begin, uint64_t n) {
  return rec_begin > rec_end || rec_end > n || (has_next && rec_end > next_begin);
}

// The matches a tile of records [r0, r1) can touch: one pair of searches in the whole list, for the tile's first and last
// bound.  hi >= lo whatever the table holds (a bad table is reported, never followed out of the list).
struct Range {
  uint64_t lo, hi;
};
RJ_RECORD_HD inline Range tile_range(const Begins& list, uint64_t m, uint64_t first_begin, uint64_t last_key) {
  Range r;
  r.lo = lower_bound(list, 0, m, first_begin);
  r.hi = lower_bound(list, r.lo, m, last_key);
  return r;
}

// One record inside its tile's range [lo, hi): the first of its matches and their number.  `b` is the staged range or the
// list itself; both give the same answer for a table that keeps the contract.
RJ_RECORD_HD inline void join_row(const Begins& b, uint64_t lo, uint64_t hi, uint64_t rec_begin, uint64_t key, uint64_t* first,
                                  uint64_t* count) {
  const uint64_t f = lower_bound(b, lo, hi, rec_begin);
  const uint64_t u = lower_bound(b, f, hi, key);   // (>= f whatever the key: a count never goes below zero)
  *first = f;
  *count = u - f;
}

// does the record's last kept match (its end is `last_end`) reach beyond the record
RJ_RECORD_HD inline bool crosses(uint64_t last_end, uint64_t rec_end) { return last_end > rec_end; }

RJ_RECORD_HD inline uint32_t saturate32(uint64_t c) { return c > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(c); }

}  // namespace records
}  // namespace rejit_amd
#endif
