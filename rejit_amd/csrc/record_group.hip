// rejit_amd/csrc/record_group.hip -- rj_scan_records_group: the rows of a record table over a device text -- the pieces of
// rj_scan_records_split, lines, the strings of a column; every row, or the rows an index list names -- grouped by their bytes:
// d_group[j] (Arrow's dictionary_encode), d_rep[g] (the first row of every distinct string, in order of first appearance) and
// d_group_count[g] (value_counts, `uniq -c`), exactly and without a download.  record_group.h has the arithmetic and the two
// invariants that make the table exact under any interleaving; six launches on one stream, one synchronise:
//
// Hash (lane), Hash (wave), Insert (lane), Insert (wave): the build of the table, record_group_build.h (rj_scan_records_lookup
//   builds its set side with the same four).
// Number: record_frame.h's unit scan over the representative flags -> d_rep, d_group_count, slot_group, G.
// Emit: d_group[j] = slot_group[slot_of[j]].
// Every kernel behind the first returns at once when the summary holds a bad row.  Nothing here waits for another lane's
// progress (record_group.h); the only bounded wait is the unit scan's look-back, as in every plan of the family.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "record_frame.h"
#include "record_group.h"
#include "record_group_build.h"
#include "record_rows.h"

namespace rejit_amd {

namespace {

// ---------------------------------------------------------------------------------------------------------------- number, emit
__global__ __launch_bounds__(kThreads) void record_group_number_kernel(uint64_t k, uint64_t n_units, Scratch S, unsigned long long* granules,
                                                                       unsigned long long* ticket, uint64_t* __restrict__ rep,
                                                                       uint64_t* __restrict__ group_count, uint64_t group_cap, unsigned long long* summary) {
  __shared__ UnitSum s_unit;
  // Only the bad word, not refused(): kSumTimedOut is written by this kernel's own unit scan and by nothing before it in the
  // call, so it can be set here only by another workgroup of this launch -- and a workgroup that starts behind a time-out
  // still takes its units and publishes them (nobody waits on words it left out); the call fails at its end either way.
  if (summary[kSumBadWord] != 0) return;
  LaneMem M{S};
  unit_init(s_unit.place);
  for (uint64_t tk; unit_take(s_unit.place, ticket, n_units, &tk);) {
    const uint64_t j = tk * kThreads + threadIdx.x;
    uint64_t s = 0;
    bool is_rep = false;
    if (j < k) {
      s = S.slot_of[j];
      is_rep = group::is_representative(M, j, s);
    }
    uint64_t g, unit_end;
    const bool ok = unit_exclusive_sum(s_unit, is_rep ? 1 : 0, tk, n_units, granules, summary, &g, &unit_end);
    if (ok && tk == n_units - 1 && threadIdx.x == 0) summary[kSumTotal] = unit_end;
    if (ok && is_rep) {
      const uint32_t rows = S.slot_count[s];        // (slot_group takes slot_count's place: the count is read first)
      S.slot_group[s] = static_cast<uint32_t>(g);
      if (g < group_cap) {
        rep[g] = j;
        group_count[g] = rows;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void record_group_emit_kernel(uint64_t k, uint64_t n_units, Scratch S, uint64_t* __restrict__ group_of,
                                                                     const unsigned long long* summary) {
  if (refused(summary)) return;
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    if (j < k) group_of[j] = S.slot_group[S.slot_of[j]];
  }
}

}  // namespace

}  // namespace rejit_amd

using namespace rejit_amd;

extern "C" {

int64_t rj_scan_records_group(rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end, uint64_t n_records,
                              const uint64_t* d_indices, uint64_t n_indices, uint64_t* d_group, uint64_t* d_rep, uint64_t* d_group_count,
                              uint64_t group_cap, void* hip_stream) {
  ErrnoGuard errno_guard;
  static const char kCall[] = "rj_scan_records_group";
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) || (group_cap && (!d_rep || !d_group_count)))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_group: null argument");
  if (!aligned8(d_rec_begin, d_rec_end, d_indices, d_group, d_rep, d_group_count))
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_group: a table is not 8-byte aligned");
  const uint64_t k = d_indices ? n_indices : n_records;
  if (!rows::rows_fit(k))
    return rj_fail(RJ_TOO_LARGE, "rj_scan_records_group: %llu rows: rows and slots share 32-bit words in the scratch (fewer than 2^31 rows)",
                   static_cast<unsigned long long>(k));
  if (k == 0) return 0;
  const GroupKnobs knobs = group_knobs();
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n_units = (k + kThreads - 1) / kThreads;
  RJ_HIP(s->rec_repl_table.reserve(group::layout(k).bytes));
  int rc;
  unsigned long long *scratch = nullptr, *summary = nullptr;   // scratch: the ticket, the long list's counter, the look-back's words
  if ((rc = records_begin(s, 2 + lookback::granule_words(n_units), st, &scratch, &summary)) != RJ_OK) return rc;
  const Scratch S = group_scratch(s->rec_repl_table.as<uint8_t>(), k, scratch + 1);
  const Rows R{d_rec_begin, d_rec_end, d_indices};
  if ((rc = group_build(static_cast<const uint8_t*>(d_text), n, R, n_records, k, knobs, S, summary, st)) != RJ_OK) return rc;
  const dim3 grid(unit_grid(n_units)), block(kThreads);
  hipLaunchKernelGGL(record_group_number_kernel, grid, block, 0, st, k, n_units, S, scratch + 2, scratch, d_rep, d_group_count, group_cap, summary);
  if (d_group) hipLaunchKernelGGL(record_group_emit_kernel, grid, block, 0, st, k, n_units, S, d_group, summary);
  if ((rc = records_finish(s, kCall, st)) != RJ_OK) return rc;
  if (s->rec_host[kSumBadWord] != 0)
    return rj_fail(RJ_BAD_ARGUMENT, "rj_scan_records_group: row %llu names no record or a record outside the text (index < n_records, begin <= end <= n)",
                   static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
  return static_cast<int64_t>(s->rec_host[kSumTotal]);
}

}  // extern "C"
