// tests/support/checked_table.h -- TEST-ONLY: what the drivers of the record group and the record lookup (group_exec.cc,
// lookup_exec.cc) share: record_group.h's table as its Mem policy sees it, every access checked against its range, and a
// write behind the build's end an error; and what the drivers' stand-alone programs share: their random numbers and orders.
#ifndef REJIT_AMD_TESTS_CHECKED_TABLE_H_
#define REJIT_AMD_TESTS_CHECKED_TABLE_H_

#include <stdint.h>

#include <vector>

#include "../../rejit_amd/csrc/record_group.h"

namespace {

// the scratch of group::layout as vectors (hits: the lookup's counts per slot); `final`: the build is over, and a write is
// an error; probes: the slot reads so far
struct CheckedMem {
  std::vector<uint64_t> slots, hash;
  std::vector<uint32_t> slot_count, slot_group, len, slot_of, hits;
  bool left_range = false, wrote_final = false, final = false;
  uint64_t probes = 0;
  CheckedMem(uint64_t n_slots, uint64_t k)
      : slots(n_slots, rejit_amd::group::kEmpty), hash(k, 0), slot_count(n_slots, 0), slot_group(n_slots, 0), len(k, 0), slot_of(k, 0), hits(n_slots, 0) {}
  bool slot_ok(uint64_t s) {
    if (s >= slots.size()) left_range = true;
    return s < slots.size();
  }
  bool row_ok(uint64_t i) {
    if (i >= hash.size()) left_range = true;
    return i < hash.size();
  }
  bool writable() {
    if (final) wrote_final = true;
    return !final;
  }
  uint64_t slot_load(uint64_t s) {
    probes++;
    return slot_ok(s) ? slots[s] : 0;
  }
  uint64_t slot_cas(uint64_t s, uint64_t j) {
    if (!writable() || !slot_ok(s)) return 0;
    const uint64_t was = slots[s];
    if (was == rejit_amd::group::kEmpty) slots[s] = j;
    return was;
  }
  void slot_min(uint64_t s, uint64_t j) {
    if (writable() && slot_ok(s) && j < slots[s]) slots[s] = j;
  }
  void count_add(uint64_t s, uint32_t c) {
    if (writable() && slot_ok(s)) slot_count[s] += c;
  }
};
// (record_group.h asks for M.hash(i) and M.len(i): the vectors have these names)
struct MemView {
  CheckedMem& m;
  uint64_t slot_load(uint64_t s) { return m.slot_load(s); }
  uint64_t slot_cas(uint64_t s, uint64_t j) { return m.slot_cas(s, j); }
  void slot_min(uint64_t s, uint64_t j) { m.slot_min(s, j); }
  void count_add(uint64_t s, uint32_t c) { m.count_add(s, c); }
  uint64_t hash(uint64_t i) { return m.row_ok(i) ? m.hash[i] : 0; }
  uint32_t len(uint64_t i) { return m.row_ok(i) ? m.len[i] : 0; }
};

inline bool permutation(const uint64_t* order, uint64_t k) {
  std::vector<uint8_t> seen(k, 0);
  for (uint64_t i = 0; i < k; i++) {
    if (order[i] >= k || seen[order[i]]) return false;
    seen[order[i]] = 1;
  }
  return true;
}

// the stand-alone programs' numbers: xorshift from a fixed seed, every program draws its own sequence
inline uint64_t rnd(uint64_t below) {
  static uint64_t rng = 88172645463325252ull;
  rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
  return rng % below;
}
inline std::vector<uint64_t> shuffled(uint64_t k) {
  std::vector<uint64_t> order(k);
  for (uint64_t i = 0; i < k; i++) order[i] = i;
  for (uint64_t i = k; i > 1; i--) {
    const uint64_t o = rnd(i), t = order[i - 1];
    order[i - 1] = order[o], order[o] = t;
  }
  return order;
}

}  // namespace
#endif
