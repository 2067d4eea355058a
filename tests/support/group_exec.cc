// tests/support/group_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_group.h, compiled with g++
// (tests/test_record_group.py).  It walks the call the way record_group.hip's kernels do -- the hash of every row, the inserts
// ONE ROW AT A TIME in an order the test chooses (the kernels' lanes interleave: every order must give the same tables), the
// numbering unit by unit with the running sum carried from unit to unit where the kernel looks back, the last pass over the
// rows -- with the two invariants of the table checked after every insert: no slot is ever emptied, and the string a slot
// stands for never changes.  Every access is checked against its range, and every output row may be written only once.
//
// With -DGROUP_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): a fixed
// set of cases against the meaning written out in plain C++.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_group.h"
#include "checked_table.h"
#include "checked_text.h"

using namespace rejit_amd;

// The hash of the row [begin, begin + len) with its groups dealt to `lanes` lanes -- strided (lane l: groups l, l + lanes, ...)
// or blocked (lane l: a contiguous run) -- and the lanes' sums added.  Returns 0, -1 when a read left the text.
extern "C" long gr_hash(const uint8_t* text, uint64_t n, uint64_t begin, uint64_t len, uint64_t lanes, int blocked, uint32_t bits, uint64_t* out) {
  if (lanes == 0 || begin > n || len > n - begin) return -2;
  const CheckedText T{text, n};
  const uint64_t groups = rows::n_groups(len);
  const uint64_t per = (groups + lanes - 1) / lanes;
  uint64_t sum = 0;
  for (uint64_t l = 0; l < lanes; l++) {
    if (blocked) {
      const uint64_t g0 = l * per < groups ? l * per : groups;
      const uint64_t g1 = g0 + per < groups ? g0 + per : groups;
      sum += group::hash_groups(T, n, begin, len, g0, 1, g1);
    } else {
      sum += group::hash_groups(T, n, begin, len, l, lanes, groups);
    }
  }
  *out = group::keep_bits(group::finalize(len, sum), bits);
  return T.left_range ? -1 : 0;
}

// the equality the table uses: lengths, stored hashes, bytes -> bit 0: the keys (length, hash) are equal, bit 1: the bytes are
extern "C" long gr_rows_equal(const uint8_t* text, uint64_t n, uint64_t a, uint64_t la, uint64_t b, uint64_t lb, uint32_t bits) {
  const CheckedText T{text, n};
  const uint64_t ha = group::keep_bits(group::hash_row(T, n, a, la), bits), hb = group::keep_bits(group::hash_row(T, n, b, lb), bits);
  long r = 0;
  if (group::stored_len(la) == group::stored_len(lb) && ha == hb) r |= 1;
  if (la == lb && group::groups_equal(T, n, a, b, la, 0, 1, rows::n_groups(la))) r |= 2;
  return T.left_range ? -1 : r;
}

extern "C" uint64_t gr_table_slots(uint64_t k) { return group::table_slots(k); }
extern "C" int gr_rows_fit(uint64_t k) { return rows::rows_fit(k) ? 1 : 0; }
extern "C" uint64_t gr_scratch_bytes(uint64_t k) { return group::layout(k).bytes; }

// summary: [0] G, [1] first bad row (~0: none), [2] slot reads of all probes, [3] slots of the table.  order[0 .. k): the rows
// in the order they are inserted.  Returns 0; -1 when an access left its range or an output row was written twice; -2 for
// arguments the call refuses up front; -3 when an invariant of the table broke; -4 when `order` is no permutation.
extern "C" long gr_group(const uint8_t* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records, const uint64_t* indices,
                         int have_indices, uint64_t n_indices, uint32_t bits, const uint64_t* order, uint64_t unit, uint64_t* out_group, uint64_t* out_rep,
                         uint64_t* out_count, uint64_t group_cap, uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[1] = ~0ull;
  const uint64_t k = have_indices ? n_indices : n_records;
  if (!rows::rows_fit(k) || unit == 0) return -2;
  if (k == 0) return 0;
  const CheckedText T{text, n};
  const uint64_t slots = group::table_slots(k);
  summary[3] = slots;
  CheckedMem mem(slots, k);
  MemView M{mem};
  // ---- hash: the pack's checks, the first bad row wins
  std::vector<uint64_t> rb(k), ln(k);
  for (uint64_t j = 0; j < k; j++) {
    const rows::Row row = rows::resolve(rec_begin, rec_end, have_indices ? indices : nullptr, n_records, n, j);
    if (row.bad) {
      if (summary[1] == ~0ull) summary[1] = j;
      continue;
    }
    rb[j] = row.rb, ln[j] = row.len();
    mem.len[j] = group::stored_len(ln[j]);
    mem.hash[j] = group::keep_bits(group::hash_row(T, n, rb[j], ln[j]), bits);
  }
  if (T.left_range) return -1;
  if (summary[1] != ~0ull) return 0;   // a refused call: the later kernels return at once
  // ---- insert, one row at a time, the invariants checked behind every step
  if (!permutation(order, k)) return -4;
  std::vector<uint64_t> before(slots);
  for (uint64_t step = 0; step < k; step++) {
    const uint64_t j = order[step];
    before = mem.slots;
    const auto equal = [&](uint64_t i) { return group::groups_equal(T, n, rb[i], rb[j], ln[j], 0, 1, rows::n_groups(ln[j])); };
    const uint64_t s = group::find_slot(M, j, mem.hash[j], mem.len[j], slots, equal);
    if (s >= slots) return -1;
    group::join_slot(M, s, j, 1);
    mem.slot_of[j] = static_cast<uint32_t>(s);
    for (uint64_t x = 0; x < slots; x++) {
      if (before[x] == mem.slots[x]) continue;
      if (mem.slots[x] == group::kEmpty) return -3;                       // (1) a slot is never emptied
      if (x != s || mem.slots[x] != j) return -3;                         // only the row's own slot changes, to the row
      if (before[x] != group::kEmpty) {                                   // (2) the string it stands for stays
        const uint64_t i = before[x];
        if (j > i || ln[i] != ln[j] || memcmp(text + rb[i], text + rb[j], ln[j]) != 0) return -3;
      }
    }
    if (mem.slots[s] == group::kEmpty || mem.slots[s] > j) return -3;
  }
  summary[2] = mem.probes;
  // ---- number: unit by unit, the count of representatives carried along
  std::vector<uint8_t> written(group_cap, 0);
  uint64_t carried = 0;
  for (uint64_t u0 = 0; u0 < k; u0 += unit) {
    uint64_t in_unit = 0;
    for (uint64_t j = u0; j < u0 + unit && j < k; j++) {
      const uint64_t s = mem.slot_of[j];
      if (!group::is_representative(M, j, s)) continue;
      const uint64_t g = carried + in_unit++;
      mem.slot_group[s] = static_cast<uint32_t>(g);
      if (g < group_cap) {
        if (written[g]) return -1;
        written[g] = 1;
        out_rep[g] = j;
        out_count[g] = mem.slot_count[s];
      }
    }
    carried += in_unit;
  }
  summary[0] = carried;
  // ---- emit
  if (out_group)
    for (uint64_t j = 0; j < k; j++) out_group[j] = mem.slot_group[mem.slot_of[j]];
  return (T.left_range || mem.left_range) ? -1 : 0;
}

#ifdef GROUP_EXEC_MAIN
#include <stdio.h>

#include <map>
#include <string>

namespace {

// one case: k rows drawn from a pool of d strings (prefixes of one another, a shared 16-byte prefix and another last byte),
// laid out with 0..3 bytes between them, the last one ending at n; inserted in a random order; against a std::map
int one_case(uint64_t k, uint64_t d, uint32_t bits, uint64_t unit, bool take) {
  static const uint64_t kLens[] = {0, 1, 15, 16, 17, 31, 32, 33, 40, 700};
  std::vector<std::string> pool;
  for (uint64_t i = 0; i < d; i++) {
    std::string s(kLens[rnd(10)], 'a');
    for (auto& c : s) c = static_cast<char>('a' + rnd(3));
    if (i % 3 == 1 && !pool.empty()) s = pool.back().substr(0, pool.back().size() / 2);          // a prefix of its neighbour
    if (i % 3 == 2 && !pool.empty() && !pool.back().empty()) s = pool.back(), s.back() = '#';   // ... and one that differs in the last byte
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
  const std::vector<uint64_t> order = shuffled(k);
  std::map<std::string, uint64_t> seen;
  std::vector<uint64_t> w_group, w_rep, w_count;
  for (uint64_t j = 0; j < k; j++) {
    const uint64_t r = take ? idx[j] : j;
    const std::string s(text.begin() + rb[r], text.begin() + re[r]);
    auto it = seen.find(s);
    if (it == seen.end()) {
      it = seen.emplace(s, w_rep.size()).first;
      w_rep.push_back(j), w_count.push_back(0);
    }
    w_group.push_back(it->second);
    w_count[it->second]++;
  }
  const uint64_t G = w_rep.size();
  // exact allocations: the sanitizer sees any byte or row beyond them
  std::vector<uint64_t> gg(k), rep(G), cnt(G);
  uint64_t summary[8];
  const long rc = gr_group(text.data(), text.size(), rb.data(), re.data(), n_records, take ? idx.data() : nullptr, take, idx.size(), bits, order.data(), unit,
                           gg.data(), rep.data(), cnt.data(), G, summary);
  if (rc != 0 || summary[0] != G || summary[1] != ~0ull) return 1;
  if (gg != w_group || rep != w_rep || cnt != w_count) return 2;
  // a capacity inside the table and no d_group
  std::vector<uint64_t> hr(G / 2), hc(G / 2);
  const long rc2 = gr_group(text.data(), text.size(), rb.data(), re.data(), n_records, take ? idx.data() : nullptr, take, idx.size(), bits, order.data(), unit,
                            nullptr, hr.data(), hc.data(), G / 2, summary);
  if (rc2 != 0 || summary[0] != G) return 3;
  for (uint64_t g = 0; g < G / 2; g++)
    if (hr[g] != w_rep[g] || hc[g] != w_count[g]) return 4;
  return 0;
}

}  // namespace

int main() {
  int cases = 0;
  for (uint64_t k : {1, 2, 33, 257})
    for (uint64_t d : {1, 2, 7, 40})
      for (uint32_t bits : {0, 1, 4, 64})
        for (uint64_t unit : {1, 3, 256}) {
          const int bad = one_case(k, d, bits, unit, cases % 3 == 1);
          if (bad) {
            fprintf(stderr, "group_exec: case %d (k %llu d %llu bits %u unit %llu) failed: %d\n", cases, static_cast<unsigned long long>(k),
                    static_cast<unsigned long long>(d), bits, static_cast<unsigned long long>(unit), bad);
            return 1;
          }
          cases++;
        }
  printf("group_exec: %d cases\n", cases);
  return 0;
}
#endif
