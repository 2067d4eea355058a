// tests/support/translate_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_translate.h, compiled with g++
// (tests/test_record_translate.py).  It walks the call the way record_translate.hip's kernels do -- the rows' plan (every row
// through record_rows.h's resolver, the places in the virtual stream, the first bad row as the largest word), the count unit by
// unit and slab by slab (a lane = 16 positions, the running sum carried from unit to unit where the kernel looks back, the
// tables written by the lane that holds a row's terminator) or the layout where nothing is dropped, the emit slab by slab and
// turn by turn through an image -- with the slab size, the image size and the unit cap chosen by the test, so that seams can
// be forced on tiny texts.  Every text read is checked against its range, and every output byte, image byte and table row
// may be written only once; a complete call must have written every byte below the total and every row.
//
// With -DTRANSLATE_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): the same
// driver over seeded cases, against a translate written with std::string, over allocations exact in their last byte.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_rows.h"
#include "../../rejit_amd/csrc/record_translate.h"
#include "checked_table.h"
#include "checked_text.h"

using namespace rejit_amd;

namespace {

struct Lane {
  translate::Group g;
  uint32_t kept;
};

struct Walk {
  const pack::View& sb;
  const CheckedText& text;
  const translate::TableView& tab;
  uint64_t k, S, slab;
  // the slab's lanes as the kernels make them: the two searches, then 16 positions per lane; -> the slab's sums
  uint32_t slab_lanes(uint64_t c0, std::vector<Lane>* lanes, uint64_t* j_lo) const {
    const uint64_t c1 = c0 + slab < S ? c0 + slab : S;
    *j_lo = pack::chunk_first_row(sb, k, c0);
    const uint64_t e = pack::chunk_end_row(sb, k, 0, c1);
    const uint64_t j_hi = e > *j_lo ? e : *j_lo;
    lanes->clear();
    uint32_t sums = 0;
    for (uint64_t t = 0; t < slab / translate::kGroup; t++) {
      Lane l;
      l.g = translate::load_group(sb, *j_lo, j_hi, c0 + t * translate::kGroup, S, text);
      l.kept = translate::kept_mask(l.g, tab);
      sums += translate::lane_sums(l.g, l.kept);
      lanes->push_back(l);
    }
    return sums;
  }
};

}  // namespace

// [0] kSlab, [1] kImage, [2] kGroup, [3] sizeof(Tables)
extern "C" void te_constants(int64_t* out) {
  out[0] = translate::kSlab;
  out[1] = translate::kImage;
  out[2] = translate::kGroup;
  out[3] = sizeof(translate::Tables);
}

// summary: [0] total, [1] the first bad row (~0: none), [2] check_call's code, [3] S, [4] units, [5] slabs per unit, [6] turns,
// [7] bytes_in, [8] bytes_dropped, [9] bytes_changed, [10] groups stored whole, [11] bytes stored one by one, [12] 1: the count
// ran, 0: the layout.
// Returns 0; -1 when an access left its range, something was written twice or a complete call left a byte or a row unwritten
// (a bug the kernel would pay for with a fault, a race or a hole); -2 for a call check_call refuses or bad driver parameters.
extern "C" long te_translate(const uint8_t* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records, const uint64_t* indices,
                             uint64_t n_indices, const uint8_t* map, const uint8_t* drop, int fill, uint64_t lead, uint64_t gap, uint64_t unit_rows, uint64_t slab,
                             uint64_t image, uint64_t unit_cap, int want_stats, uint8_t* out, uint64_t out_cap, uint64_t* out_begin, uint64_t* out_end,
                             uint64_t* summary) {
  for (int i = 0; i < 13; i++) summary[i] = 0;
  summary[1] = ~0ull;
  int scan = 0;
  const translate::Refusal why = translate::check_call(&scan, text, n, rec_begin, rec_end, n_records, indices, n_indices, fill, lead, gap, out, out_cap, out_begin, out_end);
  summary[2] = why;
  if (why != translate::kFine) return -2;
  if (unit_rows == 0 || slab == 0 || slab % translate::kGroup || image == 0 || image % translate::kGroup || unit_cap == 0) return -2;
  const uint64_t k = indices ? n_indices : n_records;
  translate::Tables tables;
  bool identity, drops;
  translate::make_tables(map, drop, &tables, &identity, &drops);
  const translate::TableView tab{tables.map, tables.drop};
  // ---- rows: no table row and no byte behind a bad row
  std::vector<uint64_t> sb_table(k + 1);
  unsigned long long worst = 0;
  uint64_t before = 0;
  for (uint64_t u0 = 0; u0 < k; u0 += unit_rows) {
    uint64_t in_unit = 0;
    for (uint64_t j = u0; j < k && j < u0 + unit_rows; j++) {
      const rows::Row row = rows::resolve(rec_begin, rec_end, indices, n_records, n, j);
      if (row.bad && ~j > worst) worst = ~j;
      sb_table[j] = before + in_unit;
      in_unit += pack::row_advance(row.bad, 0, row.bad ? 0 : row.len(), 1);
    }
    before += in_unit;
  }
  if (worst != 0) {
    summary[1] = ~worst;
    return 0;
  }
  const uint64_t S = before;
  const uint64_t slabs = translate::n_slabs(S, slab), per_unit = translate::slabs_per_unit(slabs, unit_cap), units = translate::n_units(slabs, per_unit);
  summary[3] = S, summary[4] = units, summary[5] = per_unit;
  if (units > unit_cap) return -1;   // (the look-back's words are the host's)
  const pack::View sb{sb_table.data(), nullptr, rec_begin, indices, 0, k, S};
  const CheckedText src{text, n};
  const Walk walk{sb, src, tab, k, S, slab};
  bool twice = false, left_range = false;
  std::vector<uint8_t> begin_once(k, 0), end_once(k, 0);
  const auto put_begin = [&](uint64_t j, uint64_t v) {
    if (j >= k) return void(left_range = true);
    if (begin_once[j]) twice = true;
    begin_once[j] = 1;
    if (out_begin) out_begin[j] = v;
  };
  const auto put_end = [&](uint64_t j, uint64_t v) {
    if (j >= k) return void(left_range = true);
    if (end_once[j]) twice = true;
    end_once[j] = 1;
    if (out_end) out_end[j] = v;
  };
  // ---- count, or the layout
  const bool counts = drops || (want_stats && !identity);
  summary[12] = counts;
  std::vector<uint64_t> kp(units, 0);
  std::vector<Lane> lanes;
  uint64_t total = lead, kept_all = 0, changed_all = 0;
  if (!counts) {
    kept_all = S - k;
    total = translate::place(lead, gap, S - k, k);
    for (uint64_t j = 0; j < k; j++) {
      const uint64_t at = sb.ob_at(j), next = sb.ob_at(j + 1);
      put_begin(j, translate::place(lead, gap, at - j, j));
      put_end(j, translate::place(lead, gap, next - 1 - j, j));
    }
  } else {
    uint64_t carried = 0;
    for (uint64_t tk = 0; tk < units; tk++) {
      const uint64_t slab0 = tk * per_unit, slab1 = slab0 + per_unit < slabs ? slab0 + per_unit : slabs;
      uint64_t unit_kept = 0, j_lo;
      for (uint64_t c = slab0; c < slab1; c++) {
        unit_kept += translate::sums_kept(walk.slab_lanes(c * slab, &lanes, &j_lo));
        for (const Lane& l : lanes) changed_all += translate::popcount16(translate::changed_mask(l.g, l.kept, tab));
      }
      kp[tk] = carried;
      uint64_t running = carried;
      for (uint64_t c = slab0; c < slab1; c++) {
        const uint32_t sums = walk.slab_lanes(c * slab, &lanes, &j_lo);
        uint32_t lane_before = 0;
        for (size_t t = 0; t < lanes.size(); t++) {
          const Lane& l = lanes[t];
          if (c == 0 && t == 0) put_begin(0, lead);
          translate::row_ends(l.g, l.kept, running + translate::sums_kept(lane_before), lead, gap, [&](uint64_t j, uint64_t oe) {
            put_end(j, oe);
            if (j + 1 < k) put_begin(j + 1, oe + gap);
          });
          lane_before += translate::lane_sums(l.g, l.kept);
        }
        running += translate::sums_kept(sums);
      }
      carried += unit_kept;
      if (running != carried) return -1;
    }
    kept_all = carried;
    total = translate::place(lead, gap, carried, k);
  }
  summary[0] = total;
  summary[7] = S - k, summary[8] = S - k - kept_all, summary[9] = counts ? changed_all : 0;
  for (uint64_t j = 0; j < k; j++)
    if (!begin_once[j] || !end_once[j]) return -1;
  // ---- emit
  if (out_cap != 0) {
    const uint64_t limit = total < out_cap ? total : out_cap;
    std::vector<uint8_t> out_once(limit, 0);
    const auto store = [&](uint64_t p, uint8_t byte) {
      if (p >= limit) return void(left_range = true);
      if (out_once[p]) twice = true;
      out_once[p] = 1;
      out[p] = byte;
    };
    if (units == 0)
      for (uint64_t p = 0; p < limit; p++) store(p, static_cast<uint8_t>(fill));
    std::vector<uint8_t> img(image), img_once(image);
    for (uint64_t u = 0; u < units; u++) {
      const uint64_t slab0 = u * per_unit, slab1 = slab0 + per_unit < slabs ? slab0 + per_unit : slabs;
      uint64_t running = 0;
      for (uint64_t c = slab0; c < slab1; c++) {
        const uint64_t c0 = c * slab;
        uint64_t j_lo;
        const uint32_t sums = walk.slab_lanes(c0, &lanes, &j_lo);
        if (c == slab0) running = counts ? kp[u] : c0 - j_lo;
        const translate::Range range = translate::slab_range(c0, lead, gap, running, j_lo, sums);
        const uint64_t stop = range.o1 < limit ? range.o1 : limit;
        for (uint64_t w0 = translate::first_window(range); w0 < stop; w0 += image) {
          summary[6]++;
          img.assign(image, static_cast<uint8_t>(fill));
          img_once.assign(image, 0);
          uint32_t lane_before = 0;
          for (const Lane& l : lanes) {
            const uint64_t at = translate::place(lead, gap, running + translate::sums_kept(lane_before), l.g.j);
            translate::place_group(l.g, l.kept, at, gap, w0, image, tab, [&](uint64_t in_image, uint32_t byte) {
              if (in_image >= image) return void(left_range = true);
              if (img_once[in_image]) twice = true;
              img_once[in_image] = 1;
              img[in_image] = static_cast<uint8_t>(byte);
            });
            lane_before += translate::lane_sums(l.g, l.kept);
          }
          for (uint64_t t = 0; t < image / translate::kGroup; t++) {
            const uint64_t p = w0 + t * translate::kGroup;
            const translate::Store st = translate::group_store(p, range, limit);
            if (st.hi - st.lo == translate::kGroup) summary[10]++;
            else summary[11] += st.hi - st.lo;
            for (uint32_t b = st.lo; b < st.hi; b++) store(p + b, img[t * translate::kGroup + b]);
          }
          // (a byte placed outside what the turn stores would be lost)
          for (uint64_t i = 0; i < image; i++)
            if (img_once[i] && (w0 + i < range.o0 || w0 + i >= range.o1)) left_range = true;
        }
        running += translate::sums_kept(sums);
      }
    }
    for (uint64_t p = 0; p < limit; p++)
      if (!out_once[p]) return -1;
  }
  return left_range || twice || src.left_range ? -1 : 0;
}

#ifdef TRANSLATE_EXEC_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <string>

int main() {
  const std::vector<std::vector<uint64_t>> length_sets = {{0}, {0, 1, 15, 16, 17, 33}, {31, 32, 33}, {3, 8, 200}, {1, 2, 700}};
  int cases = 0;
  for (size_t ls = 0; ls < length_sets.size(); ls++)
    for (int tables_kind = 0; tables_kind < 4; tables_kind++)     // 0: identity, 1: map only, 2: drop only, 3: both
      for (int layout = 0; layout < 4; layout++) {
        const uint64_t n_records = 30 + rnd(40);
        const bool with_indices = layout & 1;
        const uint64_t lead = layout & 1 ? 5 : 0, gap = layout == 0 ? 0 : layout == 1 ? 1 : layout == 2 ? 3 : 90;
        std::vector<uint8_t> text;
        std::vector<uint64_t> begins, ends, indices;
        for (uint64_t r = 0; r < n_records; r++) {
          const uint64_t len = length_sets[ls][rnd(length_sets[ls].size())];
          begins.push_back(text.size());
          for (uint64_t i = 0; i < len; i++) text.push_back(static_cast<uint8_t>(rnd(7) == 0 ? ',' : 'A' + rnd(26) + 32 * rnd(2)));
          ends.push_back(text.size());
        }
        const uint64_t k = with_indices ? 50 : n_records;
        for (uint64_t j = 0; with_indices && j < k; j++) indices.push_back(rnd(n_records));
        uint8_t map[256], drop[32];
        memset(drop, 0, sizeof(drop));
        for (int b = 0; b < 256; b++) map[b] = static_cast<uint8_t>(tables_kind & 1 && b >= 'A' && b <= 'Z' ? b + 32 : b);
        if (tables_kind & 2) drop[',' >> 3] |= 1 << (',' & 7), drop['q' >> 3] |= 1 << ('q' & 7);
        std::string want(lead, '\n');
        std::vector<uint64_t> want_begin, want_end;
        for (uint64_t j = 0; j < k; j++) {
          const uint64_t r = with_indices ? indices[j] : j;
          want_begin.push_back(want.size());
          for (uint64_t s = begins[r]; s < ends[r]; s++)
            if (!((drop[text[s] >> 3] >> (text[s] & 7)) & 1)) want += static_cast<char>(map[text[s]]);
          want_end.push_back(want.size());
          want += std::string(gap, '\n');
        }
        // the text, exact in its last byte
        uint8_t* exact = static_cast<uint8_t*>(malloc(text.size() ? text.size() : 1));
        if (!text.empty()) memcpy(exact, text.data(), text.size());
        std::vector<uint64_t> ob(k), oe(k);
        uint64_t summary[13];
        void* room = nullptr;
        if (posix_memalign(&room, 16, want.size() ? want.size() : 1) != 0) return 1;
        uint8_t* out = static_cast<uint8_t*>(room);
        const uint64_t slab = layout == 0 ? 16 : layout == 1 ? 64 : layout == 2 ? 4096 : 32;
        const uint64_t image = layout == 0 ? 16 : layout == 1 ? 4096 : layout == 2 ? 64 : 48;
        const uint64_t cap = layout == 3 ? 3 : 1u << 20;
        const long rc = te_translate(exact, text.size(), begins.data(), ends.data(), n_records, with_indices ? indices.data() : nullptr, indices.size(),
                                     tables_kind & 1 ? map : nullptr, tables_kind & 2 ? drop : nullptr, '\n', lead, gap, 16, slab, image, cap, layout & 2, out,
                                     want.size(), ob.data(), oe.data(), summary);
        const bool same = rc == 0 && summary[0] == want.size() && memcmp(out, want.data(), want.size()) == 0 && ob == want_begin && oe == want_end;
        free(out);
        free(exact);
        if (!same) {
          fprintf(stderr, "translate_exec: lengths %zu, tables %d, layout %d: rc %ld total %llu want %zu\n", ls, tables_kind, layout, rc,
                  static_cast<unsigned long long>(summary[0]), want.size());
          return 1;
        }
        cases += static_cast<int>(k);
      }
  printf("translate_exec: %d cases\n", cases);
  return 0;
}
#endif
