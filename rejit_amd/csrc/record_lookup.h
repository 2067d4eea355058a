// rejit_amd/csrc/record_lookup.h -- the arithmetic of rj_scan_records_lookup (record_lookup.hip) on top of record_group.h: the
// rows of one record table (the PROBE rows, over one text) looked up in the rows of another (the SET rows, over a text of
// their own) -- Arrow's index_in / is_in, `grep -F -x -f`, a semi-, anti- or inner join on a string key -- exactly.  Host and
// device code: the CPU tests drive exactly these functions (tests/support/lookup_exec.cc) through two Text policies and a Mem
// policy, as the kernels do.  The byte compare across the two texts is record_rows.h's group_equal / groups_equal.
//
// The set side is record_group.h's table, built by its hash and insert passes over the set rows, unchanged.  A row's hash
// depends on its bytes and length alone -- not on its alignment, not on its text -- so a probe row hashed in ITS text starts
// at the slot an equal set row started from, and walks the chain that row walked (probe_slot).
//
// Why plain loads suffice.  The probe kernels are launched on the same stream, behind the inserts: the table is FINAL when
// they start.  Then
//     slot[s] is the smallest set row of its string                 (record_group.h, "Behind all inserts"), and
//     a chain ends at its first empty slot                          (invariant (1): no slot on an inserted row's way to its
//                                                                    slot was empty when the row passed, and none is emptied),
// so a probe row whose string is in the set meets that string's slot before any empty one, and one whose string is not meets
// an empty slot after at most ks occupied ones (T >= 2 ks).  Nothing writes the table any more: no compare-and-swap, no
// atomic load, and the answer -- the row a slot names -- does not depend on how probe rows are assigned to lanes, waves or
// launches.  The only writes of a probe are its own answer and, when hit counts are wanted, an atomic add on hits[s].
#ifndef REJIT_AMD_RECORD_LOOKUP_H_
#define REJIT_AMD_RECORD_LOOKUP_H_

#include <stdint.h>

#include "record_group.h"

namespace rejit_amd {
namespace lookup {

constexpr uint64_t kNone = ~0ull;          // RJ_LOOKUP_NONE
constexpr uint64_t kAbsent = ~0ull;        // probe_slot: the string is in no slot
constexpr uint32_t kStagedNone = ~0u;      // a staged answer: set rows are below 2^31

// ---------------------------------------------------------------------------------------------------------------- limits
RJ_PACK_HD inline bool rows_fit(uint64_t ks, uint64_t kp) { return rows::rows_fit(ks) && rows::rows_fit(kp); }

// The scratch of a call, in bytes from the buffer's begin (every part 16-byte aligned): group::layout(ks) for the set side
// (44 .. 68 bytes per set row); `hits`, one 32-bit count per slot (4 bytes per slot: 8 .. 16 per set row); and for the probe
// side `staged`, a probe row's answer as a 32-bit word, and `long_list`, the rows handed to the wave tier (4 bytes per probe
// row each).  The probe side stores no hash and no length.  (staged: the lane tier checks a row and answers it in one
// kernel, and a refused call writes no output row -- so the answers wait in the scratch until every row has been checked, and
// a last pass widens them into d_index.)
struct Layout {
  group::Layout set;
  uint64_t hits, staged, long_list, bytes;
};
RJ_PACK_HD inline Layout layout(uint64_t ks, uint64_t kp) {
  using rows::align16;
  Layout l;
  l.set = group::layout(ks);
  l.hits = align16(l.set.bytes);
  l.staged = l.hits + align16(4 * group::table_slots(ks));
  l.long_list = l.staged + align16(4 * kp);
  l.bytes = l.long_list + align16(4 * kp);
  return l;
}
RJ_PACK_HD inline uint64_t widen(uint32_t staged) { return staged == kStagedNone ? kNone : static_cast<uint64_t>(staged); }

// ---------------------------------------------------------------------------------------------------------------- probe
// The read-only walk of find_slot's chain for a row with hash h and stored length len32.  Mem:
//     slot_load(s)         the slot's word (plain: the table is final)
//     hash(i), len(i)      what the set's hash pass stored for set row i
// equal(i): set row i and the probe row have equal bytes -- asked only when their stored lengths and hashes are equal.
// Returns the slot of the row's string, or kAbsent.  In the wave tier every lane calls it with wave-uniform answers from Mem.
template <class Mem, class Equal>
RJ_PACK_HD inline uint64_t probe_slot(Mem& M, uint64_t h, uint32_t len32, uint64_t T, const Equal& equal) {
  uint64_t s = h & (T - 1);
  for (;;) {
    const uint64_t cur = M.slot_load(s);
    if (cur == group::kEmpty) return kAbsent;
    if (M.len(cur) == len32 && M.hash(cur) == h && equal(cur)) return s;
    s = (s + 1) & (T - 1);
  }
}

// The byte compare of set row a (in the set text) and probe row b (in the probe text): record_rows.h's two-text group_equal /
// groups_equal, under this header's names too.  No shortcut for a == b: the offsets belong to two texts.
using rows::group_equal;
using rows::groups_equal;

// ---------------------------------------------------------------------------------------------------------------- hits
// set row i behind all probes: its string's hit count when it is the smallest row of its string, else 0
template <class Mem>
RJ_PACK_HD inline bool is_first(Mem& M, uint64_t i, uint64_t s) { return M.slot_load(s) == i; }

}  // namespace lookup
}  // namespace rejit_amd
#endif
