// tests/support/replace_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_replace.h, compiled with g++
// (tests/test_record_replace.py).  It walks the call the way record_replace.hip's kernels do -- the table unit by unit and the
// plan unit by unit (the running sum carried from unit to unit where the kernels look back), the copy chunk by chunk: the
// chunk's rows from one pair of searches, their ob / source begin / first / count / base staged in buffers of `stage_cap` rows
// when they fit (the kernel's LDS), 16 aligned output bytes per step -- with the unit sizes, the chunk size and the capacity
// chosen by the test.  Every access is checked against its range.
//
// With -DREPLACE_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): a fixed
// set of cases against a splice written out in plain C++.
#include <stdint.h>

#include <vector>

#include "../../rejit_amd/csrc/record_replace.h"
#include "checked_table.h"
#include "checked_text.h"

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
  const uint64_t* table_;   // m + 1 entries
  const uint8_t* with;
  uint64_t with_len;
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
  uint64_t table(uint64_t g) const { return get(table_, g, m + 1); }
  uint32_t with_byte(uint64_t i) const { return get(with, i, with_len); }
};

}  // namespace

// summary: [0] total, [1] first bad row (~0: none), [2] its kind (replace::Kind), [3] chunks that used the stage, [4] chunks
// that searched the tables, [5] groups that were one load16, [6] groups of fill only, [7] groups that went byte by byte.
// Returns 0, -1 when an access left its range (text, list, tables, stage, output): a bug the kernel would pay for with a fault,
// -2 for arguments the call refuses up front.
extern "C" long re_replace(const uint8_t* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records,
                           const uint32_t* counts, const uint64_t* first, const uint64_t* spans, uint64_t m, const uint64_t* indices, int have_indices,
                           uint64_t n_indices, const uint8_t* with, uint64_t with_len, uint32_t fill, uint64_t lead, uint64_t gap, uint64_t table_unit,
                           uint64_t unit, uint64_t chunk, uint64_t stage_cap, uint8_t* out, uint64_t out_cap, uint64_t* out_begin, uint64_t* out_end,
                           uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[1] = ~0ull;
  const uint64_t k = have_indices ? n_indices : n_records;
  if (!replace::sums_fit(k, n, m, with_len, lead, gap) || table_unit == 0 || unit == 0 || chunk == 0 || chunk % replace::kGroupBytes != 0) return -2;
  // ---- table
  std::vector<uint64_t> table(m + 1);
  uint64_t removed = 0;   // (what the look-back resolves: the sum of the units before this one)
  for (uint64_t u0 = 0; u0 <= m; u0 += table_unit) {
    uint64_t in_unit = 0;
    for (uint64_t g = u0; g < u0 + table_unit && g <= m; g++) {
      const uint64_t begin = g < m ? spans[2 * g] : n;
      table[g] = replace::table_entry(begin, removed + in_unit, g, with_len);
      if (g < m) in_unit += replace::match_length(begin, spans[2 * g + 1], n);
    }
    removed += in_unit;
  }
  const CheckedSpans M{rec_begin, rec_end, first, counts, n_records, indices, n_indices, spans, m, table.data(), with, with_len};
  // ---- plan
  std::vector<uint64_t> own_begin(k + 1);
  uint64_t* ob = out_begin ? out_begin : own_begin.data();
  uint64_t before = 0;
  for (uint64_t u0 = 0; u0 < k; u0 += unit) {
    const uint64_t u1 = u0 + unit < k ? u0 + unit : k;
    uint64_t in_unit = 0;
    for (uint64_t j = u0; j < u1; j++) {
      const replace::RowPlan row = replace::plan_row(M, j, have_indices != 0, n_records, n, m);
      if (row.kind != replace::kOk && summary[1] == ~0ull) {
        summary[1] = j;
        summary[2] = row.kind;
        if (replace::bad_word_row(replace::bad_word(j, row.kind)) != j || replace::bad_word_kind(replace::bad_word(j, row.kind)) != row.kind) return -1;
      }
      ob[j] = lead + before + in_unit;
      if (out_end) out_end[j] = ob[j] + row.len;
      in_unit += row.kind == replace::kOk ? row.len + gap : 0;
    }
    before += in_unit;
  }
  const uint64_t total = lead + before;
  summary[0] = total;
  if (M.left_range) return -1;
  if (summary[1] != ~0ull) return 0;   // a refused plan: the copy kernel returns at once
  // ---- copy
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint64_t n_chunks = (limit + chunk - 1) / chunk;
  const pack::View whole{ob, nullptr, nullptr, nullptr, 0, k, total};
  CheckedText src{text, n};
  std::vector<uint64_t> s_ob(stage_cap + 1), s_src(stage_cap + 1), s_first(stage_cap + 1), s_base(stage_cap + 1);
  std::vector<uint32_t> s_count(stage_cap + 1);
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
    replace::Stage stage{nullptr, nullptr, nullptr};
    if (staged) {
      for (uint64_t i = 0; i <= rows.j1 - rows.j0; i++) {
        if (i > stage_cap) return -1;
        s_ob[i] = whole.ob_at(rows.j0 + i);
        if (rows.j0 + i < rows.j1) {
          const replace::RowInfo x = replace::row_info(M, rows.j0 + i, have_indices != 0);
          s_src[i] = x.rb, s_first[i] = x.f, s_base[i] = x.base, s_count[i] = x.c;
        }
      }
      view = pack::View{s_ob.data(), s_src.data(), nullptr, nullptr, rows.j0, ~0ull, total};
      stage = replace::Stage{s_first.data(), s_base.data(), s_count.data()};
    }
    summary[staged ? 3 : 4]++;
    for (uint64_t p = c0; p < c1; p += replace::kGroupBytes) {
      uint32_t w[4];
      const int how = replace::group16(view, stage, M, have_indices != 0, rows, p, limit, gap, fill, with_len, src, w);
      summary[5 + how]++;
      if (!store_group(out, 0, p, limit, out_cap, w)) return -1;
    }
  }
  return src.left_range || M.left_range ? -1 : 0;
}

extern "C" int re_sums_fit(uint64_t k, uint64_t n, uint64_t m, uint64_t with_len, uint64_t lead, uint64_t gap) {
  return replace::sums_fit(k, n, m, with_len, lead, gap) ? 1 : 0;
}

#ifdef REPLACE_EXEC_MAIN
#include <stdio.h>

#include <string>

namespace {

// one case: records of the given sizes (a seam of 0 or 2 text bytes between them), matches planted inside the records, the
// join by record_join.h's rule, the splice row by row
int one_case(uint64_t with_len, uint64_t lead, uint64_t gap, uint64_t table_unit, uint64_t unit, uint64_t chunk, uint64_t stage_cap, bool take) {
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
    while (pos <= at + size) {
      uint64_t len = kLens[rnd(5)];
      if (pos + len > at + size) len = at + size - pos;
      if (len == 0 && pos == at + size && rnd(2)) break;   // (an empty match at the record's end, in front of the seam: half of the time)
      spans.push_back(pos), spans.push_back(pos + len);
      pos += len + (len == 0 ? 1 + rnd(4) : rnd(4) * rnd(2));
    }
    counts.push_back(static_cast<uint32_t>(spans.size() / 2 - first.back()));
    at += size + 2;   // a seam: an empty match at a record's end is the record's own
  }
  const uint64_t n = at + 5, m = spans.size() / 2, n_records = rb.size();
  std::vector<uint8_t> text(n), with(with_len + 1);
  for (auto& c : text) c = static_cast<uint8_t>(32 + rnd(90));
  for (auto& c : with) c = static_cast<uint8_t>('A' + rnd(26));
  std::vector<uint64_t> idx;
  if (take)
    for (int i = 0; i < 90; i++) idx.push_back(rnd(n_records));
  const uint64_t k = take ? idx.size() : n_records;
  std::string want(lead, static_cast<char>(0x7C));
  std::vector<uint64_t> w_ob, w_oe;
  for (uint64_t j = 0; j < k; j++) {
    const uint64_t r = take ? idx[j] : j;
    w_ob.push_back(want.size());
    uint64_t pos = rb[r];
    for (uint64_t g = first[r]; g < first[r] + counts[r]; g++) {
      want.append(reinterpret_cast<const char*>(text.data()) + pos, spans[2 * g] - pos);
      want.append(reinterpret_cast<const char*>(with.data()), with_len);
      pos = spans[2 * g + 1];
    }
    want.append(reinterpret_cast<const char*>(text.data()) + pos, re[r] - pos);
    w_oe.push_back(want.size());
    want.append(gap, static_cast<char>(0x7C));
  }
  // exact allocations: the sanitizer sees any byte beyond them
  std::vector<uint8_t> out(want.size());
  std::vector<uint64_t> ob(k), oe(k);
  uint64_t summary[8];
  const long rc = re_replace(text.data(), n, rb.data(), re.data(), n_records, counts.data(), first.data(), spans.data(), m, take ? idx.data() : nullptr, take,
                             idx.size(), with.data(), with_len, 0x7C, lead, gap, table_unit, unit, chunk, stage_cap, out.data(), out.size(), ob.data(),
                             oe.data(), summary);
  if (rc != 0 || summary[0] != want.size() || summary[1] != ~0ull) return 1;
  if (std::string(out.begin(), out.end()) != want || ob != w_ob || oe != w_oe) return 2;
  // a capacity inside the output: nothing at or beyond it
  std::vector<uint8_t> part(want.size() / 2);
  const long rc2 = re_replace(text.data(), n, rb.data(), re.data(), n_records, counts.data(), first.data(), spans.data(), m, take ? idx.data() : nullptr,
                              take, idx.size(), with.data(), with_len, 0x7C, lead, gap, table_unit, unit, chunk, stage_cap, part.data(), part.size(),
                              nullptr, nullptr, summary);
  if (rc2 != 0 || summary[0] != want.size() || std::string(part.begin(), part.end()) != want.substr(0, part.size())) return 3;
  return 0;
}

}  // namespace

int main() {
  static const uint64_t kWith[] = {0, 1, 15, 16, 17, 40};
  int cases = 0;
  for (uint64_t with_len : kWith)
    for (uint64_t unit : {1, 3, 256})
      for (uint64_t chunk : {16, 48, 4096})
        for (uint64_t cap : {0, 1, 7, 1024}) {
          const int bad = one_case(with_len, cases % 2 ? 17 : 0, cases % 3 ? 1 : 0, unit, unit, chunk, cap, cases % 4 == 1);
          if (bad) {
            fprintf(stderr, "replace_exec: case %d (with_len %llu unit %llu chunk %llu stage %llu) failed: %d\n", cases,
                    static_cast<unsigned long long>(with_len), static_cast<unsigned long long>(unit), static_cast<unsigned long long>(chunk),
                    static_cast<unsigned long long>(cap), bad);
            return 1;
          }
          cases++;
        }
  printf("replace_exec: %d cases\n", cases);
  return 0;
}
#endif
