// tests/support/split_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_split.h, compiled with g++
// (tests/test_record_split.py).  It walks the call the way record_split.hip's kernels do -- the plan unit by unit over k + 1
// rows (the closing row has no pieces; the running sum is carried from unit to unit where the kernel looks back), the emit
// chunk by chunk of pieces: the chunk's rows from one pair of searches, their piece_first / begin / end / first / count staged
// in buffers of `stage_cap` rows when they fit (the kernel's LDS), one piece per step -- with the unit size, the chunk size and
// the capacity chosen by the test.  Every access is checked against its range, and every table row may be written only once.
//
// With -DSPLIT_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): a fixed
// set of cases against the meaning written out in plain C++.
#include <stdint.h>

#include <vector>

#include "../../rejit_amd/csrc/record_split.h"
#include "checked_table.h"

using namespace rejit_amd;

namespace {

struct CheckedSpans {
  const uint64_t *rb, *re, *first_;
  const uint32_t* counts;
  uint64_t n_records;
  const uint64_t* indices;
  uint64_t n_indices;
  const uint64_t* spans;
  uint64_t m;
  mutable bool left_range = false;
  template <class T>
  T get(const T* p, uint64_t i, uint64_t size) const {
    if (i >= size) {
      left_range = true;
      return 0;
    }
    return p[i];
  }
  uint64_t rec_begin(uint64_t r) const { return get(rb, r, n_records); }
  uint64_t rec_end(uint64_t r) const { return get(re, r, n_records); }
  uint64_t first(uint64_t r) const { return get(first_, r, n_records); }
  uint32_t count(uint64_t r) const { return get(counts, r, n_records); }
  uint64_t index(uint64_t j) const { return get(indices, j, n_indices); }
  uint64_t span_begin(uint64_t g) const { return g < m ? spans[2 * g] : get(spans, 1, 0); }
  uint64_t span_end(uint64_t g) const { return g < m ? spans[2 * g + 1] : get(spans, 1, 0); }
  uint64_t table(uint64_t) const { return 0; }   // (record_split.h: the split has no table D)
};

}  // namespace

// summary: [0] P, [1] first bad row (~0: none), [2] its kind (replace::Kind), [3] chunks that used the stage, [4] chunks that
// searched the table.  Returns 0, -1 when an access left its range (list, tables, stage, output) or a row was written twice:
// a bug the kernel would pay for with a fault or a race, -2 for arguments the call refuses up front.
extern "C" long sp_split(uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records, const uint32_t* counts, const uint64_t* first,
                         const uint64_t* spans, uint64_t m, const uint64_t* indices, int have_indices, uint64_t n_indices, int what, uint64_t unit,
                         uint64_t chunk, uint64_t stage_cap, uint64_t* piece_first, uint64_t* piece_begin, uint64_t* piece_end, uint64_t piece_cap,
                         uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[1] = ~0ull;
  const uint64_t k = have_indices ? n_indices : n_records;
  if (!split::sums_fit(k, m) || (what != split::kBetween && what != split::kMatches) || unit == 0 || chunk == 0) return -2;
  const CheckedSpans M{rec_begin, rec_end, first, counts, n_records, indices, n_indices, spans, m};
  // ---- plan: k + 1 rows, row k the closing one
  std::vector<uint64_t> own_first(k + 1);
  uint64_t* pf = piece_first ? piece_first : own_first.data();
  uint64_t before = 0;
  for (uint64_t u0 = 0; u0 <= k; u0 += unit) {
    uint64_t in_unit = 0;
    for (uint64_t j = u0; j < u0 + unit && j <= k; j++) {
      split::RowPlan row{replace::kOk, 0};
      if (j < k) row = split::plan_row(M, what, j, have_indices != 0, n_records, n, m);
      if (row.kind != replace::kOk && summary[1] == ~0ull) {
        summary[1] = j;
        summary[2] = row.kind;
        if (replace::bad_word_row(replace::bad_word(j, row.kind)) != j || replace::bad_word_kind(replace::bad_word(j, row.kind)) != row.kind) return -1;
      }
      pf[j] = before + in_unit;
      in_unit += row.kind == replace::kOk ? row.pieces : 0;
    }
    before += in_unit;
  }
  const uint64_t total = before;
  summary[0] = total;
  if (M.left_range) return -1;
  if (summary[1] != ~0ull) return 0;   // a refused plan: the emit kernel returns at once
  // ---- emit
  const uint64_t limit = total < piece_cap ? total : piece_cap;
  const uint64_t n_chunks = (limit + chunk - 1) / chunk;
  const pack::View whole{pf, nullptr, nullptr, nullptr, 0, k, total};
  std::vector<uint64_t> s_pf(stage_cap + 1), s_rb(stage_cap + 1), s_re(stage_cap + 1), s_first(stage_cap + 1);
  std::vector<uint32_t> s_count(stage_cap + 1);
  std::vector<uint8_t> written(limit, 0);
  for (uint64_t c = 0; c < n_chunks; c++) {
    const uint64_t c0 = c * chunk;
    const uint64_t c1 = c0 + chunk < limit ? c0 + chunk : limit;
    pack::Rows rows;
    rows.j0 = pack::chunk_first_row(whole, k, c0);
    const uint64_t e = pack::chunk_end_row(whole, k, 0, c1);
    rows.j1 = e > rows.j0 ? e : rows.j0;
    if (rows.j1 > k) return -1;
    const bool staged = pack::chunk_fits_stage(rows, stage_cap);
    pack::View view = whole;
    split::Stage stage{nullptr, nullptr, nullptr, nullptr};
    if (staged) {
      for (uint64_t i = 0; i <= rows.j1 - rows.j0; i++) {
        if (i > stage_cap) return -1;
        s_pf[i] = whole.ob_at(rows.j0 + i);
        if (rows.j0 + i < rows.j1) {
          const split::RowInfo x = split::row_info(M, rows.j0 + i, have_indices != 0);
          s_rb[i] = x.rb, s_re[i] = x.re, s_first[i] = x.f, s_count[i] = x.c;
        }
      }
      view = pack::View{s_pf.data(), nullptr, nullptr, nullptr, rows.j0, ~0ull, total};
      stage = split::Stage{s_rb.data(), s_re.data(), s_first.data(), s_count.data()};
    }
    summary[staged ? 3 : 4]++;
    for (uint64_t p = c0; p < c1; p++) {
      // (the searches the lane is about to make stay inside the chunk's rows)
      const split::PieceAt at = split::locate_piece(view, rows, p);
      if (at.j < rows.j0 || at.j >= rows.j1 || at.j >= k) return -1;
      const split::Piece pc = split::piece(view, stage, M, what, have_indices != 0, rows, p);
      if (p >= piece_cap || written[p]) return -1;
      written[p] = 1;
      piece_begin[p] = pc.begin;
      piece_end[p] = pc.end;
    }
  }
  return M.left_range ? -1 : 0;
}

extern "C" int sp_sums_fit(uint64_t k, uint64_t m) { return split::sums_fit(k, m) ? 1 : 0; }

#ifdef SPLIT_EXEC_MAIN
#include <stdio.h>

namespace {

// one case: records of the given sizes (a seam of 2 text bytes between them), matches planted inside the records, the pieces
// row by row from the meaning
int one_case(int what, uint64_t unit, uint64_t chunk, uint64_t stage_cap, bool take) {
  static const uint64_t kSizes[] = {0, 1, 15, 16, 17, 40, 0, 0, 33, 300};
  static const uint64_t kLens[] = {0, 1, 1, 2, 16};
  std::vector<uint64_t> rb, re, spans, first;
  std::vector<uint32_t> counts;
  uint64_t at = 3;
  for (int i = 0; i < 60; i++) {
    const uint64_t size = kSizes[rnd(10)];
    rb.push_back(at), re.push_back(at + size);
    first.push_back(spans.size() / 2);
    uint64_t pos = at + rnd(3);
    while (pos <= at + size && rnd(8) != 0) {
      uint64_t len = kLens[rnd(5)];
      if (pos + len > at + size) len = at + size - pos;
      spans.push_back(pos), spans.push_back(pos + len);
      pos += len + (len == 0 ? 1 + rnd(4) : rnd(4) * rnd(2));
    }
    counts.push_back(static_cast<uint32_t>(spans.size() / 2 - first.back()));
    at += size + 2;
  }
  const uint64_t n = at + 5, m = spans.size() / 2, n_records = rb.size();
  std::vector<uint64_t> idx;
  if (take)
    for (int i = 0; i < 90; i++) idx.push_back(rnd(n_records));
  const uint64_t k = take ? idx.size() : n_records;
  std::vector<uint64_t> w_first, w_begin, w_end;
  for (uint64_t j = 0; j < k; j++) {
    const uint64_t r = take ? idx[j] : j;
    w_first.push_back(w_begin.size());
    uint64_t pos = rb[r];
    for (uint64_t g = first[r]; g < first[r] + counts[r]; g++) {
      if (what == split::kBetween) w_begin.push_back(pos), w_end.push_back(spans[2 * g]);
      else w_begin.push_back(spans[2 * g]), w_end.push_back(spans[2 * g + 1]);
      pos = spans[2 * g + 1];
    }
    if (what == split::kBetween) w_begin.push_back(pos), w_end.push_back(re[r]);
  }
  w_first.push_back(w_begin.size());
  const uint64_t P = w_begin.size();
  // exact allocations: the sanitizer sees any row beyond them
  std::vector<uint64_t> pf(k + 1), pb(P), pe(P);
  uint64_t summary[8];
  const long rc = sp_split(n, rb.data(), re.data(), n_records, counts.data(), first.data(), spans.data(), m, take ? idx.data() : nullptr, take, idx.size(),
                           what, unit, chunk, stage_cap, pf.data(), pb.data(), pe.data(), P, summary);
  if (rc != 0 || summary[0] != P || summary[1] != ~0ull) return 1;
  if (pf != w_first || pb != w_begin || pe != w_end) return 2;
  // a capacity inside the table: nothing at or beyond it, and the scan's own offsets
  std::vector<uint64_t> hb(P / 2), he(P / 2);
  const long rc2 = sp_split(n, rb.data(), re.data(), n_records, counts.data(), first.data(), spans.data(), m, take ? idx.data() : nullptr, take, idx.size(),
                            what, unit, chunk, stage_cap, nullptr, hb.data(), he.data(), P / 2, summary);
  if (rc2 != 0 || summary[0] != P) return 3;
  for (uint64_t p = 0; p < P / 2; p++)
    if (hb[p] != w_begin[p] || he[p] != w_end[p]) return 4;
  return 0;
}

}  // namespace

int main() {
  int cases = 0;
  for (int what : {0, 1})
    for (uint64_t unit : {1, 3, 256})
      for (uint64_t chunk : {1, 3, 16, 4096})
        for (uint64_t cap : {0, 1, 7, 1024}) {
          const int bad = one_case(what, unit, chunk, cap, cases % 4 == 1);
          if (bad) {
            fprintf(stderr, "split_exec: case %d (what %d unit %llu chunk %llu stage %llu) failed: %d\n", cases, what, static_cast<unsigned long long>(unit),
                    static_cast<unsigned long long>(chunk), static_cast<unsigned long long>(cap), bad);
            return 1;
          }
          cases++;
        }
  printf("split_exec: %d cases\n", cases);
  return 0;
}
#endif
