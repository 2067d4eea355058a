// tests/support/sort_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_sort.h, compiled with g++
// (tests/test_record_sort.py).  It walks the call the way record_sort.hip's kernels do -- the compaction unit by unit with
// the running sums carried from unit to unit where the kernel looks back, the prefix skip's lane tier row by row and its
// wave tier 64 groups per iteration, the keys, a stable sort by key and then by the bits of the segment number (what the
// two radix passes do), the cut -- and asserts the header's properties INSIDE the loop:
//     P1  the result is the unique stable order (against std::stable_sort over memcmp);
//     P2  without the skip, rounds <= max_len / 7 + 1;
//     P3  with the skip every open segment splits into at least two parts or closes in its round; rounds <= G + 1;
//     P4  within a segment equal rows are in ascending j before and after every round;
// and that sorted entries stay inside their segment's range of the list.  Every access is checked against its range, and
// every output row may be written only once.
//
// With -DSORT_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): a fixed
// set of cases with exact allocations.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../rejit_amd/csrc/record_sort.h"
#include "checked_table.h"
#include "checked_text.h"

using namespace rejit_amd;

namespace {

// record_sort.h's Mem: the scratch a position owns and the output, every index checked, an output row written once
struct CheckedPositions {
  std::vector<uint8_t> flags, written;
  std::vector<uint32_t> perm;
  std::vector<uint64_t> pos_depth;
  uint64_t* order;
  bool left_range = false, twice = false;
  bool ok(uint64_t p) {
    if (p >= flags.size()) left_range = true;
    return p < flags.size();
  }
  void set_flags(uint64_t p, uint8_t f) {
    if (ok(p)) flags[p] = f;
  }
  void set_perm(uint64_t p, uint32_t row) {
    if (ok(p)) perm[p] = row;
  }
  void set_depth(uint64_t p, uint64_t d) {
    if (ok(p)) pos_depth[p] = d;
  }
  void set_order(uint64_t p, uint32_t row) {
    if (!ok(p)) return;
    if (written[p]) twice = true;
    written[p] = 1;
    order[p] = row;
  }
  uint32_t row_at(uint64_t p) const { return (flags[p] & sort::kOpen) ? perm[p] : static_cast<uint32_t>(order[p]); }
};

struct Entry {
  uint64_t key, seg_row;
};
struct ListView {
  const std::vector<Entry>& e;
  uint32_t seg(uint64_t i) const { return sort::seg_of(e[i].seg_row); }
  uint64_t key(uint64_t i) const { return e[i].key; }
};

struct Table {
  const uint8_t* text;
  std::vector<uint64_t> rb, ln;
  int compare(uint64_t a, uint64_t b) const {
    const uint64_t m = ln[a] < ln[b] ? ln[a] : ln[b];
    const int c = m ? memcmp(text + rb[a], text + rb[b], m) : 0;
    return c ? c : ln[a] < ln[b] ? -1 : ln[a] > ln[b] ? 1 : 0;
  }
};

// P4 over every segment (open and closed): equal rows in ascending j
bool equal_rows_ascend(const Table& T, const CheckedPositions& mem, uint64_t k) {
  std::map<std::string, uint32_t> last;
  for (uint64_t p = 0; p < k; p++) {
    if (mem.flags[p] & sort::kHead) last.clear();
    const uint32_t j = mem.row_at(p);
    if (j >= k) return false;
    const std::string s(reinterpret_cast<const char*>(T.text) + T.rb[j], T.ln[j]);
    auto it = last.find(s);
    if (it != last.end() && it->second >= j) return false;
    last[s] = j;
  }
  return true;
}

}  // namespace

// key(row, d) of the row [begin, begin + len) -> *out; [1] of out: 1 when the guarded load was taken.  0, -1 when a read left the text.
extern "C" long so_key(const uint8_t* text, uint64_t n, uint64_t begin, uint64_t len, uint64_t d, uint64_t* out) {
  if (begin > n || len > n - begin || d > len) return -2;
  const CheckedText T{text, n};
  out[0] = sort::key(T, n, begin, len, d);
  out[1] = T.guarded;
  return T.left_range ? -1 : 0;
}
extern "C" int so_rows_fit(uint64_t k) { return rows::rows_fit(k) ? 1 : 0; }
extern "C" uint64_t so_scratch_bytes(uint64_t k) { return sort::layout(k).bytes; }
extern "C" unsigned so_seg_bits(uint64_t n_segments) { return sort::seg_bits(n_segments); }
// the lane tier for one pair of rows -> the depth, *more
extern "C" long so_skip_row(const uint8_t* text, uint64_t n, uint64_t hb, uint64_t hl, uint64_t rb, uint64_t rl, uint64_t D, uint32_t L, uint64_t* out) {
  const CheckedText T{text, n};
  bool more = false;
  out[0] = sort::skip_row(T, n, hb, hl, rb, rl, D, L, &more);
  out[1] = more ? 1 : 0;
  return T.left_range ? -1 : 0;
}

// summary: [0] rounds, [1] first bad row (~0: none), [2] keyed rows, [3] skip rows, [4] long rows, [5] the most open segments
// a round had, [6] which property broke (1..4; 5: an entry left its segment's range; 6: the wave tier's lanes do not ascend),
// [7] guarded loads.  Returns 0; -1 when an access left its range or an output row was written twice or not at all; -2 for
// arguments the call refuses up front; -3 when a property broke.
extern "C" long so_sort(const uint8_t* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records, const uint64_t* indices,
                        int have_indices, uint64_t n_indices, uint64_t unit, uint32_t L, int skip, uint64_t* out_order, uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[1] = ~0ull;
  const uint64_t k = have_indices ? n_indices : n_records;
  if (!rows::rows_fit(k) || unit == 0) return -2;
  if (k == 0) return 0;
  const CheckedText T{text, n};
  // ---- init: the pack's checks, the first bad row wins
  Table table{text, std::vector<uint64_t>(k), std::vector<uint64_t>(k)};
  uint64_t max_len = 0;
  for (uint64_t j = 0; j < k; j++) {
    const rows::Row row = rows::resolve(rec_begin, rec_end, have_indices ? indices : nullptr, n_records, n, j);
    if (row.bad) {
      if (summary[1] == ~0ull) summary[1] = j;
      continue;
    }
    table.rb[j] = row.rb, table.ln[j] = row.len();
    if (table.ln[j] > max_len) max_len = table.ln[j];
  }
  if (summary[1] != ~0ull) return 0;   // a refused call: the later kernels return at once
  CheckedPositions mem;
  mem.flags.assign(k, 0), mem.written.assign(k, 0), mem.perm.assign(k, 0), mem.pos_depth.assign(k, 0);
  mem.order = out_order;
  for (uint64_t j = 0; j < k; j++) {
    mem.perm[j] = static_cast<uint32_t>(j);
    mem.flags[j] = k < 2 ? 0 : static_cast<uint8_t>(sort::kOpen | (j == 0 ? sort::kHead : 0));
  }
  if (k == 1) mem.set_order(0, 0);
  // the meaning: the unique stable order
  std::vector<uint32_t> want(k);
  for (uint64_t j = 0; j < k; j++) want[j] = static_cast<uint32_t>(j);
  std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return table.compare(a, b) < 0; });
  uint64_t distinct = 1;
  for (uint64_t i = 1; i < k; i++) distinct += table.compare(want[i - 1], want[i]) != 0;

  const uint64_t max_segments = sort::max_segments(k);
  uint64_t n_active = k >= 2 ? k : 0, n_segments = 1;
  std::vector<uint32_t> act_pos(k), seg_head(max_segments);
  std::vector<uint64_t> seg_depth(max_segments), seg_cur(max_segments);
  std::vector<Entry> list, before_sort;
  for (bool first = true; n_active; first = false) {
    if (!equal_rows_ascend(table, mem, k)) return summary[6] = 4, -3;
    const bool skips = skip && !first;
    // ---- compact, unit by unit
    list.assign(n_active, Entry{0, 0});
    uint64_t carried = 0;
    for (uint64_t u0 = 0; u0 < k; u0 += unit) {
      uint64_t in_unit = 0;
      for (uint64_t p = u0; p < u0 + unit && p < k; p++) {
        const uint8_t f = mem.flags[p];
        const uint64_t before = carried + in_unit;
        in_unit += sort::place_add(f);
        if (!(f & sort::kOpen)) continue;
        const sort::Place at = sort::place(before, f);
        if (at.at >= n_active || at.seg >= n_segments || at.seg >= max_segments) return -1;
        act_pos[at.at] = static_cast<uint32_t>(p);
        list[at.at].seg_row = sort::seg_row(at.seg, mem.perm[p]);
        if (f & sort::kHead) {
          seg_depth[at.seg] = mem.pos_depth[p];
          seg_cur[at.seg] = skips ? sort::kNoDepth : mem.pos_depth[p];
          seg_head[at.seg] = at.at;
        }
      }
      carried += in_unit;
    }
    if (static_cast<uint32_t>(carried) != n_active || carried >> 32 != n_segments) return -1;
    if (n_segments > summary[5]) summary[5] = n_segments;
    // ---- skip: the lane tier, then the wave tier over its list
    if (skips) {
      std::vector<uint32_t> long_list;
      for (uint64_t a = 0; a < n_active; a++) {
        const uint32_t s = sort::seg_of(list[a].seg_row);
        const uint32_t j = sort::row_of(list[a].seg_row), h = sort::row_of(list[seg_head[s]].seg_row);
        bool more = false;
        const uint64_t depth = sort::skip_row(T, n, table.rb[h], table.ln[h], table.rb[j], table.ln[j], seg_depth[s], L, &more);
        if (!more && depth < seg_cur[s]) seg_cur[s] = depth;
        if (more) long_list.push_back(static_cast<uint32_t>(a));
      }
      summary[3] += n_active;
      summary[4] += long_list.size();
      for (uint32_t a : long_list) {
        const uint32_t s = sort::seg_of(list[a].seg_row);
        const uint32_t j = sort::row_of(list[a].seg_row), h = sort::row_of(list[seg_head[s]].seg_row);
        const uint64_t both = table.ln[h] < table.ln[j] ? table.ln[h] : table.ln[j];
        uint64_t depth = both;
        for (uint64_t d0 = seg_depth[s] + L; d0 < both && depth == both; d0 += 64 * sort::kGroupBytes) {
          uint64_t found = sort::kNoDepth;
          for (uint64_t lane = 0; lane < 64; lane++) {
            const uint64_t at = sort::wave_group(T, n, table.rb[h], table.rb[j], both, d0, lane);
            if (at == sort::kNoDepth) continue;
            if (found == sort::kNoDepth) found = at;
            else if (at <= found) return summary[6] = 6, -3;
          }
          if (found != sort::kNoDepth) depth = found;
        }
        if (depth < seg_cur[s]) seg_cur[s] = depth;
      }
      // the skip is exact here (both tiers ran): the depth is the segment's common prefix
      for (uint64_t a = 0; a < n_active; a++) {
        const uint32_t s = sort::seg_of(list[a].seg_row);
        const uint32_t j = sort::row_of(list[a].seg_row), h = sort::row_of(list[seg_head[s]].seg_row);
        if (seg_cur[s] < seg_depth[s] || seg_cur[s] > table.ln[j] || memcmp(text + table.rb[h], text + table.rb[j], seg_cur[s]) != 0) return summary[6] = 1, -3;
      }
    }
    // ---- key
    for (uint64_t a = 0; a < n_active; a++) {
      const uint32_t j = sort::row_of(list[a].seg_row);
      const uint64_t d = seg_cur[sort::seg_of(list[a].seg_row)];
      if (d > table.ln[j]) return -1;
      list[a].key = sort::key(T, n, table.rb[j], table.ln[j], d);
    }
    summary[2] += n_active;
    // ---- order: stable by key, then stable by the bits of the segment number
    before_sort = list;
    std::stable_sort(list.begin(), list.end(), [](const Entry& x, const Entry& y) { return x.key < y.key; });
    const unsigned bits = sort::seg_bits(n_segments);
    if (bits) {
      const uint64_t mask = ((1ull << bits) - 1) << 32;
      std::stable_sort(list.begin(), list.end(), [mask](const Entry& x, const Entry& y) { return (x.seg_row & mask) < (y.seg_row & mask); });
    }
    for (uint64_t a = 0; a < n_active; a++)
      if (sort::seg_of(list[a].seg_row) != sort::seg_of(before_sort[a].seg_row)) return summary[6] = 5, -3;
    // ---- cut
    const ListView view{list};
    uint64_t open_rows = 0, open_segments = 0;
    std::vector<uint32_t> parts(n_segments, 0), still_open(n_segments, 0);
    for (uint64_t a = 0; a < n_active; a++) {
      const uint8_t f = sort::cut(view, a, n_active);
      const uint32_t s = sort::seg_of(list[a].seg_row);
      sort::settle(mem, act_pos[a], f, sort::row_of(list[a].seg_row), seg_cur[s]);
      if (f & sort::kHead) parts[s]++;
      if (f & sort::kOpen) open_rows++, still_open[s]++;
      if ((f & sort::kOpen) && (f & sort::kHead)) open_segments++;
    }
    summary[0]++;
    if (skips)
      for (uint64_t s = 0; s < n_segments; s++)
        if (parts[s] < 2 && still_open[s]) return summary[6] = 3, -3;
    if (!equal_rows_ascend(table, mem, k)) return summary[6] = 4, -3;
    if (!skip && summary[0] > max_len / sort::kWindow + 1) return summary[6] = 2, -3;
    if (skip && summary[0] > distinct + 1) return summary[6] = 3, -3;
    n_active = open_rows, n_segments = open_segments;
    if (mem.left_range || mem.twice || T.left_range) return -1;
  }
  summary[7] = T.guarded;
  for (uint64_t p = 0; p < k; p++) {
    if (!mem.written[p]) return -1;
    if (out_order[p] != want[p]) return summary[6] = 1, -3;
  }
  return (T.left_range || mem.left_range || mem.twice) ? -1 : 0;
}

#ifdef SORT_EXEC_MAIN
#include <stdio.h>

namespace {

// one case: k rows over a small alphabet behind a shared prefix, lengths around the window and the group, some rows a
// prefix of their neighbour or differing in the last byte, laid out with 0..3 bytes between them, the last one ending at n
int one_case(uint64_t k, uint64_t prefix, uint32_t L, int skip, uint64_t unit, bool take) {
  static const uint64_t kLens[] = {0, 1, 6, 7, 8, 13, 14, 15, 21, 63, 64, 65, 70, 1100};
  std::vector<std::string> pool;
  const uint64_t d = k < 4 ? k + 1 : k / 2;
  for (uint64_t i = 0; i < d; i++) {
    std::string s(prefix, 'p');
    const uint64_t len = kLens[rnd(14)];
    for (uint64_t b = 0; b < len; b++) s.push_back(static_cast<char>(rnd(2) ? 0xFF : rnd(2) ? 0 : 'a'));
    if (i % 3 == 1 && !pool.empty()) s = pool.back().substr(0, pool.back().size() / 2);
    if (i % 3 == 2 && !pool.empty() && !pool.back().empty()) s = pool.back(), s.back() = '#';
    pool.push_back(s);
  }
  std::vector<uint8_t> text;
  std::vector<uint64_t> rb, re;
  const uint64_t n_records = take ? d : k;
  for (uint64_t i = 0; i < n_records; i++) {
    const std::string& s = pool[take ? i : rnd(d)];
    for (uint64_t p = rnd(4); p > 0; p--) text.push_back('|');
    rb.push_back(text.size());
    text.insert(text.end(), s.begin(), s.end());
    re.push_back(text.size());
  }
  std::vector<uint64_t> idx;
  if (take)
    for (uint64_t i = 0; i < k; i++) idx.push_back(rnd(d));
  // exact allocations: the sanitizer sees any byte or row beyond them; the driver itself checks the order (P1)
  std::vector<uint64_t> order(k);
  uint64_t summary[8];
  const long rc = so_sort(text.data(), text.size(), rb.data(), re.data(), n_records, take ? idx.data() : nullptr, take, idx.size(), unit, L, skip, order.data(),
                          summary);
  if (rc != 0 || summary[1] != ~0ull) return 1 + static_cast<int>(summary[6]) * 10;
  std::vector<uint8_t> seen(k, 0);
  for (uint64_t p = 0; p < k; p++) {
    if (order[p] >= k || seen[order[p]]) return 2;
    seen[order[p]] = 1;
  }
  return 0;
}

}  // namespace

int main() {
  int cases = 0;
  for (uint64_t k : {1, 2, 3, 65, 257})
    for (uint64_t prefix : {0, 9, 40})
      for (uint32_t L : {1, 16, 64})
        for (int skip : {0, 1})
          for (uint64_t unit : {1, 3, 256}) {
            const int bad = one_case(k, prefix, L, skip, unit, cases % 3 == 1);
            if (bad) {
              fprintf(stderr, "sort_exec: case %d (k %llu prefix %llu L %u skip %d unit %llu) failed: %d\n", cases, static_cast<unsigned long long>(k),
                      static_cast<unsigned long long>(prefix), L, skip, static_cast<unsigned long long>(unit), bad);
              return 1;
            }
            cases++;
          }
  printf("sort_exec: %d cases\n", cases);
  return 0;
}
#endif
