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

using namespace rejit_amd;

namespace {

struct CheckedText {
  const uint8_t* text;
  uint64_t n;
  mutable bool left_range = false;
  uint32_t at(uint64_t s) const {
    if (s >= n) {
      left_range = true;
      return 0;
    }
    return text[s];
  }
  // (all 16 bytes inside the text: that is the contract of the device's load16)
  void load16(uint64_t s, uint32_t w[4]) const {
    for (int i = 0; i < 4; i++) w[i] = 0;
    for (uint32_t b = 0; b < 16; b++) w[b >> 2] |= at(s + b) << (8 * (b & 3));
  }
  void load16_guarded(uint64_t s, uint32_t w[4]) const {
    for (int i = 0; i < 4; i++) w[i] = 0;
    for (uint32_t b = 0; b < 16; b++)
      if (s + b < n) w[b >> 2] |= at(s + b) << (8 * (b & 3));
  }
};

struct CheckedMem {
  std::vector<uint64_t> slots;
  std::vector<uint32_t> slot_count, slot_group, len, slot_of;
  std::vector<uint64_t> hash;
  bool left_range = false;
  uint64_t probes = 0;
  bool slot_ok(uint64_t s) {
    if (s >= slots.size()) left_range = true;
    return s < slots.size();
  }
  bool row_ok(uint64_t i) {
    if (i >= hash.size()) left_range = true;
    return i < hash.size();
  }
  uint64_t slot_load(uint64_t s) {
    probes++;
    return slot_ok(s) ? slots[s] : 0;
  }
  uint64_t slot_cas(uint64_t s, uint64_t j) {
    if (!slot_ok(s)) return 0;
    const uint64_t was = slots[s];
    if (was == group::kEmpty) slots[s] = j;
    return was;
  }
  void slot_min(uint64_t s, uint64_t j) {
    if (slot_ok(s) && j < slots[s]) slots[s] = j;
  }
  void count_add(uint64_t s, uint32_t c) {
    if (slot_ok(s)) slot_count[s] += c;
  }
  uint32_t len_of(uint64_t i) { return row_ok(i) ? len[i] : 0; }
};
// (record_group.h asks for M.hash(i) and M.len(i): the vectors have other names)
struct MemView {
  CheckedMem& m;
  uint64_t slot_load(uint64_t s) { return m.slot_load(s); }
  uint64_t slot_cas(uint64_t s, uint64_t j) { return m.slot_cas(s, j); }
  void slot_min(uint64_t s, uint64_t j) { m.slot_min(s, j); }
  void count_add(uint64_t s, uint32_t c) { m.count_add(s, c); }
  uint64_t hash(uint64_t i) { return m.row_ok(i) ? m.hash[i] : 0; }
  uint32_t len(uint64_t i) { return m.len_of(i); }
};

}  // namespace

// The hash of the row [begin, begin + len) with its groups dealt to `lanes` lanes -- strided (lane l: groups l, l + lanes, ...)
// or blocked (lane l: a contiguous run) -- and the lanes' sums added.  Returns 0, -1 when a read left the text.
extern "C" long gr_hash(const uint8_t* text, uint64_t n, uint64_t begin, uint64_t len, uint64_t lanes, int blocked, uint32_t bits, uint64_t* out) {
  if (lanes == 0 || begin > n || len > n - begin) return -2;
  const CheckedText T{text, n};
  const uint64_t groups = group::n_groups(len);
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
  if (la == lb && group::groups_equal(T, n, a, b, la, 0, 1, group::n_groups(la))) r |= 2;
  return T.left_range ? -1 : r;
}

extern "C" uint64_t gr_table_slots(uint64_t k) { return group::table_slots(k); }
extern "C" int gr_rows_fit(uint64_t k) { return group::rows_fit(k) ? 1 : 0; }
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
  if (!group::rows_fit(k) || unit == 0) return -2;
  if (k == 0) return 0;
  const CheckedText T{text, n};
  const uint64_t slots = group::table_slots(k);
  summary[3] = slots;
  CheckedMem mem;
  mem.slots.assign(slots, group::kEmpty);
  mem.slot_count.assign(slots, 0);
  mem.slot_group.assign(slots, 0);
  mem.hash.assign(k, 0), mem.len.assign(k, 0), mem.slot_of.assign(k, 0);
  MemView M{mem};
  // ---- hash: the pack's checks, the first bad row wins
  std::vector<uint64_t> rb(k), ln(k);
  for (uint64_t j = 0; j < k; j++) {
    const uint64_t r = have_indices ? indices[j] : j;
    if (pack::bad_index(r, n_records) || pack::bad_row(rec_begin[r], rec_end[r], n)) {
      if (summary[1] == ~0ull) summary[1] = j;
      continue;
    }
    rb[j] = rec_begin[r], ln[j] = rec_end[r] - rec_begin[r];
    mem.len[j] = group::stored_len(ln[j]);
    mem.hash[j] = group::keep_bits(group::hash_row(T, n, rb[j], ln[j]), bits);
  }
  if (T.left_range) return -1;
  if (summary[1] != ~0ull) return 0;   // a refused call: the later kernels return at once
  // ---- insert, one row at a time, the invariants checked behind every step
  std::vector<uint8_t> seen(k, 0);
  std::vector<uint64_t> before(slots);
  for (uint64_t step = 0; step < k; step++) {
    const uint64_t j = order[step];
    if (j >= k || seen[j]) return -4;
    seen[j] = 1;
    before = mem.slots;
    const auto equal = [&](uint64_t i) { return group::groups_equal(T, n, rb[i], rb[j], ln[j], 0, 1, group::n_groups(ln[j])); };
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

uint64_t g_rng = 88172645463325252ull;
uint64_t rnd(uint64_t below) {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng % below;
}

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
  std::vector<uint64_t> order(k);
  for (uint64_t i = 0; i < k; i++) order[i] = i;
  for (uint64_t i = k; i > 1; i--) {
    const uint64_t o = rnd(i);
    const uint64_t t = order[i - 1];
    order[i - 1] = order[o], order[o] = t;
  }
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
