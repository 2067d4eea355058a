// tests/support/record_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_join.h, compiled with g++ (tests/test_record_join.py).
// It walks the record table the way record_join.hip's join kernel does -- tile by tile: the tile's range of the list from one
// pair of searches, the begins of that range staged in a buffer of `stage_cap` entries when they fit (the kernel's LDS), one
// join_row per record in the staged copy or in the list itself -- with the tile size and the capacity chosen by the test.
#include <stdint.h>

#include <vector>

#include "../../rejit_amd/csrc/record_join.h"

using namespace rejit_amd::records;

// summary: kept, matching, crossing, first bad row (~0: none), tiles that searched the staged copy, tiles that searched the list.
// Returns 0, or -1 when a search left the staged buffer (a bug the kernel would pay for with an LDS overrun).
extern "C" long re_join(const uint64_t* spans, uint64_t m, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records, uint64_t n,
                        uint64_t tile, uint64_t stage_cap, uint32_t* counts, uint64_t* first, uint64_t* summary) {
  for (int k = 0; k < 6; k++) summary[k] = 0;
  summary[3] = ~0ull;
  const Begins list{spans, 2, 0};
  std::vector<uint64_t> stage(stage_cap + 1);   // (+1: data() of an empty vector may be null)
  for (uint64_t r0 = 0; r0 < n_records; r0 += tile) {
    const uint64_t r1 = r0 + tile < n_records ? r0 + tile : n_records;
    const uint64_t last = r1 - 1;
    const bool last_has_next = last + 1 < n_records;
    const Range r = tile_range(list, m, rec_begin[r0], upper_key(rec_end[last], last_has_next, last_has_next ? rec_begin[last + 1] : 0));
    if (r.hi < r.lo || r.hi > m) return -1;
    const bool staged = r.hi - r.lo <= stage_cap;
    if (staged)
      for (uint64_t k = 0; k < r.hi - r.lo; k++) stage[k] = spans[2 * (r.lo + k)];
    summary[staged ? 4 : 5]++;
    for (uint64_t i = r0; i < r1; i++) {
      const bool has_next = i + 1 < n_records;
      const uint64_t nb = has_next ? rec_begin[i + 1] : 0;
      if (bad_row(rec_begin[i], rec_end[i], has_next, nb, n) && summary[3] == ~0ull) summary[3] = i;
      uint64_t f = 0, c = 0;
      const uint64_t key = upper_key(rec_end[i], has_next, nb);
      if (staged) join_row(Begins{stage.data(), 1, r.lo}, r.lo, r.hi, rec_begin[i], key, &f, &c);
      else join_row(list, r.lo, r.hi, rec_begin[i], key, &f, &c);
      if (f < r.lo || f + c > r.hi) return -1;
      if (c && crosses(spans[2 * (f + c - 1) + 1], rec_end[i])) summary[2]++;
      counts[i] = saturate32(c);
      first[i] = f;
      summary[0] += c;
      summary[1] += c != 0;
    }
  }
  return 0;
}

extern "C" uint32_t re_saturate32(uint64_t c) { return saturate32(c); }
