// tests/support/pack_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_pack.h, compiled with g++ (tests/test_record_pack.py).
// It walks the pack the way record_pack.hip's kernels do -- the plan unit by unit (a unit's rows, the running sum carried from
// unit to unit where the kernel looks back), the copy chunk by chunk: the chunk's rows from one pair of searches, their ob and
// source begins staged in a buffer of `stage_cap` rows when they fit (the kernel's LDS), 16 aligned output bytes per step --
// with the unit size, the chunk size and the capacity chosen by the test.  Every access is checked against its range.
//
// text == NULL: numbers only -- the byte at source offset s is synth(s), and only the output chunks [chunk_first, chunk_first
// + chunk_count) are produced, into out[0, ...) (out then stands for the output from chunk_first * chunk on): offsets above
// 2^32 and 2^40 without the memory.
#include <stdint.h>

#include <vector>

#include "../../rejit_amd/csrc/record_pack.h"
#include "checked_text.h"

using namespace rejit_amd::pack;

// summary: [0] total, [1] first bad row (~0: none), [2] chunks that used the stage, [3] chunks that searched the table,
// [4] groups that were one load16, [5] groups of fill only, [6] groups that went byte by byte, [7] single bytes read.
// Returns 0, or -1 when an access left its range (text, output, stage, tables): a bug the kernel would pay for with a fault.
extern "C" long pe_pack(const uint8_t* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records,
                        const uint64_t* indices, uint64_t n_indices, uint32_t fill, uint64_t lead, uint64_t gap, uint64_t unit, uint64_t chunk,
                        uint64_t stage_cap, uint8_t* out, uint64_t out_cap, uint64_t chunk_first, uint64_t chunk_count, uint64_t* out_begin,
                        uint64_t* out_end, uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[1] = ~0ull;
  const uint64_t k = indices ? n_indices : n_records;
  if (!sums_fit(k, n, lead, gap) || unit == 0 || chunk == 0 || chunk % kGroupBytes != 0) return -2;
  // ---- plan
  std::vector<uint64_t> own_begin(k + 1);
  uint64_t* ob = out_begin ? out_begin : own_begin.data();
  uint64_t before = 0;   // (what the look-back resolves: the sum of the units before this one)
  for (uint64_t u0 = 0; u0 < k; u0 += unit) {
    const uint64_t u1 = u0 + unit < k ? u0 + unit : k;
    uint64_t in_unit = 0;
    for (uint64_t j = u0; j < u1; j++) {
      const uint64_t r = indices ? indices[j] : j;
      bool bad = bad_index(r, n_records);
      uint64_t rb = 0, re = 0;
      if (!bad) {
        rb = rec_begin[r];
        re = rec_end[r];
        bad = bad_row(rb, re, n);
      }
      if (bad && summary[1] == ~0ull) summary[1] = j;
      const uint64_t add = row_advance(bad, rb, re, gap);
      ob[j] = lead + before + in_unit;
      if (out_end) out_end[j] = ob[j] + (bad ? 0 : re - rb);
      in_unit += add;
    }
    before += in_unit;
  }
  const uint64_t total = lead + before;
  summary[0] = total;
  if (summary[1] != ~0ull) return 0;   // a refused plan: the copy kernel returns at once
  // ---- copy
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint64_t n_chunks = (limit + chunk - 1) / chunk;
  const uint64_t window0 = text ? 0 : chunk_first * chunk;
  const View table{ob, nullptr, rec_begin, indices, 0, k, total};
  CheckedText src{text, n};
  std::vector<uint64_t> s_ob(stage_cap + 1), s_src(stage_cap + 1);
  for (uint64_t c = text ? 0 : chunk_first; c < n_chunks && (text || c < chunk_first + chunk_count); c++) {
    const uint64_t c0 = c * chunk;
    const uint64_t c1 = c0 + chunk < limit ? c0 + chunk : limit;
    Rows rows;
    rows.j0 = chunk_first_row(table, k, c0);
    const uint64_t e = chunk_end_row(table, k, 0, c1);
    rows.j1 = e > rows.j0 ? e : rows.j0;
    if (rows.j1 > k) return -1;
    const bool staged = chunk_fits_stage(rows, stage_cap);
    View view = table;
    if (staged) {
      for (uint64_t i = 0; i <= rows.j1 - rows.j0; i++) {
        if (i > stage_cap) return -1;
        s_ob[i] = table.ob_at(rows.j0 + i);
        if (rows.j0 + i < rows.j1) s_src[i] = table.src_at(rows.j0 + i);
      }
      view = View{s_ob.data(), s_src.data(), nullptr, nullptr, rows.j0, ~0ull, total};
    }
    summary[staged ? 2 : 3]++;
    for (uint64_t p = c0; p < c1; p += kGroupBytes) {
      uint32_t w[4];
      const int how = group16(view, rows, p, limit, gap, fill, src, w);
      summary[4 + how]++;
      if (!store_group(out, window0, p, limit, out_cap, w)) return -1;
    }
  }
  summary[7] = src.byte_reads;
  return src.left_range ? -1 : 0;
}

extern "C" uint8_t pe_synth(uint64_t s) { return synth(s); }
extern "C" int pe_sums_fit(uint64_t k, uint64_t n, uint64_t lead, uint64_t gap) { return sums_fit(k, n, lead, gap) ? 1 : 0; }
