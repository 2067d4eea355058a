// tests/support/lookup_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_lookup.h, compiled with g++
// (tests/test_record_lookup.py).  It walks the call the way record_lookup.hip's kernels do: the set side is built with
// record_group.h's functions -- the hash of every set row, the inserts ONE ROW AT A TIME in an order the test chooses --, then
// the probe rows are visited in an order and in units the test chooses: the pack's checks, the hash in the PROBE text, the
// read-only walk of the chain (probe_slot; the driver's table refuses every write once the build is over), the byte compare
// across the two texts, the answer staged as a 32-bit word; with hit counts the rows of a unit that ended at the slot of the
// unit's first found row add ONE count (the peel), the others their own.  Behind all units the staged answers are widened
// and the hits read per set row.  Every access is checked against its range, and every output row may be written only once.
//
// With -DLOOKUP_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): seeded
// random cases against the meaning written out with std::map, exact allocations.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_lookup.h"
#include "checked_table.h"
#include "checked_text.h"

using namespace rejit_amd;

extern "C" int lk_rows_fit(uint64_t ks, uint64_t kp) { return lookup::rows_fit(ks, kp) ? 1 : 0; }
// [0] bytes, [1] hits, [2] staged, [3] long_list, [4] the set side's bytes
extern "C" void lk_layout(uint64_t ks, uint64_t kp, uint64_t* out) {
  const lookup::Layout l = lookup::layout(ks, kp);
  out[0] = l.bytes, out[1] = l.hits, out[2] = l.staged, out[3] = l.long_list, out[4] = l.set.bytes;
}

// the two-text compare alone: set row [a, a + len) of set_text against probe row [b, b + len) of text, the groups dealt to
// `lanes` lanes (strided) -> 1 equal, 0 different, -1 a read left its text
extern "C" long lk_rows_equal(const uint8_t* set_text, uint64_t set_n, uint64_t a, const uint8_t* text, uint64_t n, uint64_t b, uint64_t len, uint64_t lanes) {
  if (lanes == 0 || a > set_n || len > set_n - a || b > n || len > n - b) return -2;
  const CheckedText TS{set_text, set_n}, TP{text, n};
  bool equal = true;
  for (uint64_t l = 0; l < lanes; l++) equal = rows::groups_equal(TS, set_n, a, TP, n, b, len, l, lanes, rows::n_groups(len)) && equal;
  return (TS.left_range || TP.left_range) ? -1 : equal ? 1 : 0;
}

// summary: [0] n_found, [1] first bad set row (~0: none), [2] first bad probe row (~0: none), [3] n_set_distinct, [4] n_set_hit,
// [5] slots of the table, [6] slot reads of all probes.  insert_order[0 .. ks): the set rows in the order they are inserted;
// probe_order[0 .. kp): the probe rows in the order they are visited, `unit` at a time.  Returns 0; -1 when an access left its
// range, an output row was written twice or the probe wrote the table; -2 for arguments the call refuses up front; -4 when an
// order is no permutation.
extern "C" long lk_lookup(const uint8_t* set_text, uint64_t set_n, const uint64_t* set_begin, const uint64_t* set_end, uint64_t n_set_records,
                          const uint64_t* set_indices, int have_set_indices, uint64_t n_set_indices, const uint8_t* text, uint64_t n, const uint64_t* rec_begin,
                          const uint64_t* rec_end, uint64_t n_records, const uint64_t* indices, int have_indices, uint64_t n_indices, uint32_t bits,
                          const uint64_t* insert_order, const uint64_t* probe_order, uint64_t unit, int want_hits, int peel, uint64_t* out_index,
                          uint64_t* out_hits, uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[1] = summary[2] = ~0ull;
  const uint64_t ks = have_set_indices ? n_set_indices : n_set_records;
  const uint64_t kp = have_indices ? n_indices : n_records;
  if (!lookup::rows_fit(ks, kp) || unit == 0) return -2;
  if (!permutation(insert_order, ks) || !permutation(probe_order, kp)) return -4;
  const CheckedText TS{set_text, set_n}, TP{text, n};
  const uint64_t slots = group::table_slots(ks);
  summary[5] = slots;
  CheckedMem mem(slots, ks);
  MemView M{mem};
  // ---- the set side: the group's hash pass (the pack's checks, the first bad row wins) and its inserts, one row at a time
  std::vector<uint64_t> sb(ks), sl(ks);
  for (uint64_t i = 0; i < ks; i++) {
    const rows::Row row = rows::resolve(set_begin, set_end, have_set_indices ? set_indices : nullptr, n_set_records, set_n, i);
    if (row.bad) {
      if (summary[1] == ~0ull) summary[1] = i;
      continue;
    }
    sb[i] = row.rb, sl[i] = row.len();
    mem.len[i] = group::stored_len(sl[i]);
    mem.hash[i] = group::keep_bits(group::hash_row(TS, set_n, sb[i], sl[i]), bits);
  }
  if (TS.left_range) return -1;
  if (summary[1] != ~0ull) return 0;   // a refused call: the later kernels return at once, the probe rows are not even checked
  for (uint64_t step = 0; step < ks; step++) {
    const uint64_t i = insert_order[step];
    const auto equal = [&](uint64_t c) { return group::groups_equal(TS, set_n, sb[c], sb[i], sl[i], 0, 1, rows::n_groups(sl[i])); };
    const uint64_t s = group::find_slot(M, i, mem.hash[i], mem.len[i], slots, equal);
    if (s >= slots) return -1;
    group::join_slot(M, s, i, 1);
    mem.slot_of[i] = static_cast<uint32_t>(s);
  }
  mem.final = true;   // behind all inserts: the probe kernels start here
  // ---- the probe side, unit by unit in the chosen order
  std::vector<uint32_t> staged(kp, 0);
  std::vector<uint8_t> staged_once(kp, 0);
  bool twice = false;
  uint64_t found_rows = 0, reads = 0;
  struct Counting {
    MemView& m;
    uint64_t& reads;
    uint64_t slot_load(uint64_t s) {
      reads++;
      return m.slot_load(s);
    }
    uint64_t hash(uint64_t i) { return m.hash(i); }
    uint32_t len(uint64_t i) { return m.len(i); }
  } PM{M, reads};
  for (uint64_t u0 = 0; u0 < kp; u0 += unit) {
    uint64_t first_slot = lookup::kAbsent;
    uint32_t with_first = 0;
    for (uint64_t at = u0; at < u0 + unit && at < kp; at++) {
      const uint64_t j = probe_order[at];
      const rows::Row row = rows::resolve(rec_begin, rec_end, have_indices ? indices : nullptr, n_records, n, j);
      if (row.bad) {
        if (j < summary[2]) summary[2] = j;
        continue;
      }
      const uint64_t rb = row.rb, len = row.len();
      const uint64_t h = group::keep_bits(group::hash_row(TP, n, rb, len), bits);
      const auto equal = [&](uint64_t c) { return sl[c] == len && rows::groups_equal(TS, set_n, sb[c], TP, n, rb, len, 0, 1, rows::n_groups(len)); };
      const uint64_t s = lookup::probe_slot(PM, h, group::stored_len(len), slots, equal);
      if (staged_once[j]) twice = true;
      staged_once[j] = 1;
      if (s == lookup::kAbsent) {
        staged[j] = lookup::kStagedNone;
        continue;
      }
      if (s >= slots) return -1;
      staged[j] = static_cast<uint32_t>(M.slot_load(s));
      found_rows++;
      if (!want_hits) continue;
      if (peel && first_slot == lookup::kAbsent) first_slot = s;
      if (peel && s == first_slot) with_first++;
      else mem.hits[s] += 1;
    }
    if (with_first) mem.hits[first_slot] += with_first;   // ONE add for the rows that went with the unit's first found row
  }
  summary[6] = reads;
  if (TS.left_range || TP.left_range || mem.left_range || mem.wrote_final || twice) return -1;
  if (summary[2] != ~0ull) return 0;   // a refused call: nothing is emitted
  // ---- emit, hits
  summary[0] = found_rows;
  for (uint64_t j = 0; j < kp; j++) {
    if (!staged_once[j]) return -1;
    out_index[j] = lookup::widen(staged[j]);
  }
  if (want_hits) {
    for (uint64_t i = 0; i < ks; i++) {
      const uint64_t s = mem.slot_of[i];
      const bool first = lookup::is_first(M, i, s);
      const uint32_t h = first ? mem.hits[s] : 0;
      if (out_hits) out_hits[i] = h;
      summary[3] += first ? 1 : 0;
      summary[4] += h ? 1 : 0;
    }
  }
  return (mem.left_range || mem.wrote_final) ? -1 : 0;
}

#ifdef LOOKUP_EXEC_MAIN
#include <stdio.h>

#include <map>
#include <string>

namespace {

struct Table {
  std::vector<uint8_t> text;
  std::vector<uint64_t> rb, re, idx;
  bool take = false;
  uint64_t rows() const { return take ? idx.size() : rb.size(); }
  std::string row(uint64_t j) const {
    const uint64_t r = take ? idx[j] : j;
    return std::string(text.begin() + rb[r], text.begin() + re[r]);
  }
};

// k rows drawn from `pool`, laid out with 0..3 bytes of `sep` between them, the last one ending at the text's last byte
void fill(Table& t, const std::vector<std::string>& pool, uint64_t k, bool take, char sep) {
  t.take = take;
  const uint64_t n_records = take ? pool.size() : k;
  for (uint64_t i = 0; i < n_records; i++) {
    const std::string& s = pool[take ? i : rnd(pool.size())];
    for (uint64_t p = rnd(4); p > 0; p--) t.text.push_back(static_cast<uint8_t>(sep));
    t.rb.push_back(t.text.size());
    t.text.insert(t.text.end(), s.begin(), s.end());
    t.re.push_back(t.text.size());
  }
  if (take)
    for (uint64_t i = 0; i < k; i++) t.idx.push_back(rnd(pool.size()));
}

// one case: set and probe rows drawn from one pool of d strings (prefixes of one another, another last byte), each table in
// a text of its own -- or both in one --; random insert and probe orders; against a std::map
int one_case(uint64_t ks, uint64_t kp, uint64_t d, uint32_t bits, uint64_t unit, bool take, bool one_text, bool hits) {
  static const uint64_t kLens[] = {0, 1, 15, 16, 17, 31, 32, 33, 40, 700};
  std::vector<std::string> pool;
  for (uint64_t i = 0; i < d; i++) {
    std::string s(kLens[rnd(10)], 'a');
    for (auto& c : s) c = static_cast<char>('a' + rnd(3));
    if (i % 3 == 1 && !pool.empty()) s = pool.back().substr(0, pool.back().size() / 2);
    if (i % 3 == 2 && !pool.empty() && !pool.back().empty()) s = pool.back(), s.back() = '#';
    pool.push_back(s);
  }
  // the set draws from the pool's first two thirds, the probe from all of it: some probe strings are absent
  const std::vector<std::string> set_pool(pool.begin(), pool.begin() + (2 * d + 2) / 3);
  Table S, P;
  fill(S, set_pool, ks, take, '|');
  fill(P, pool, kp, take, '~');
  if (one_text) {   // both tables over ONE buffer: the probe's offsets shifted behind the set's text
    const uint64_t shift = S.text.size();
    S.text.insert(S.text.end(), P.text.begin(), P.text.end());
    for (auto& x : P.rb) x += shift;
    for (auto& x : P.re) x += shift;
    P.text = S.text;
  }
  std::map<std::string, uint64_t> first;
  for (uint64_t i = 0; i < S.rows(); i++) first.emplace(S.row(i), i);
  std::vector<uint64_t> w_index(kp), w_hits(ks, 0);
  uint64_t w_found = 0;
  for (uint64_t j = 0; j < kp; j++) {
    const auto it = first.find(P.row(j));
    w_index[j] = it == first.end() ? lookup::kNone : it->second;
    if (it != first.end()) w_hits[it->second]++, w_found++;
  }
  const std::vector<uint64_t> io = shuffled(ks), po = shuffled(kp);
  // exact allocations: the sanitizer sees any byte or row beyond them
  std::vector<uint64_t> index(kp), got_hits(ks);
  uint64_t summary[8];
  const uint8_t* ptext = one_text ? S.text.data() : P.text.data();
  const long rc = lk_lookup(S.text.data(), S.text.size(), S.rb.data(), S.re.data(), S.rb.size(), S.take ? S.idx.data() : nullptr, S.take, S.idx.size(), ptext,
                            P.text.size(), P.rb.data(), P.re.data(), P.rb.size(), P.take ? P.idx.data() : nullptr, P.take, P.idx.size(), bits, io.data(),
                            po.data(), unit, hits, bits != 1, index.data(), hits ? got_hits.data() : nullptr, summary);
  if (rc != 0 || summary[0] != w_found || summary[1] != ~0ull || summary[2] != ~0ull) return 1;
  if (index != w_index) return 2;
  if (hits && got_hits != w_hits) return 3;
  if (hits && summary[3] != first.size()) return 4;
  return 0;
}

}  // namespace

int main() {
  int cases = 0;
  for (uint64_t ks : {0, 1, 7, 65})
    for (uint64_t kp : {0, 1, 33, 130})
      for (uint64_t d : {1, 5, 40})
        for (uint32_t bits : {0, 1, 4, 64}) {
          static const uint64_t kUnits[] = {1, 3, 64, 256};
          const int bad = one_case(ks, kp, d, bits, kUnits[cases % 4], cases % 3 == 1, cases % 5 == 2, cases % 2 == 0);
          if (bad) {
            fprintf(stderr, "lookup_exec: case %d (ks %llu kp %llu d %llu bits %u) failed: %d\n", cases, static_cast<unsigned long long>(ks),
                    static_cast<unsigned long long>(kp), static_cast<unsigned long long>(d), bits, bad);
            return 1;
          }
          cases++;
        }
  printf("lookup_exec: %d cases\n", cases);
  return 0;
}
#endif
