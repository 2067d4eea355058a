// rejit_amd/csrc/record_frame.h -- what the record units (record_join.hip, record_pack.hip, record_replace.hip,
// record_split.hip, record_group.hip with record_group_build.h, record_sort.hip, record_lookup.hip, record_parse.hip, record_time.hip,
// record_format.hip, record_time_format.hip, record_zip.hip, record_translate.hip, record_csv.hip, record_csv_format.hip) share, in ONE place: the
// summary words of their calls and when they refuse one, the 64-bit wave sums, the first bad row and the list of flagged
// rows as a wave leaves them, the 16-byte read of a device text at any alignment (record_rows.h's Text), the rows of a
// record table, the unit of a persistent scan in arrival order (ticket, publish, resolve, timed-out), the plan over it, the
// output-major chunk copy (record_pack.hip, record_replace.hip), the output-major chunk EMIT through an image in LDS
// (record_format.hip, record_time_format.hip, record_zip.hip, record_csv_format.hip), the index check of the value-column
// calls, and the host plumbing around the launches.  Everything lives in an anonymous namespace: every unit gets its own copy.
#ifndef REJIT_AMD_RECORD_FRAME_H_
#define REJIT_AMD_RECORD_FRAME_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "engine_internal.h"
#include "kernel_util.h"
#include "record_pack.h"
#include "stream_load.h"
#include "tile_lookback.h"
#include "wave_ops.h"

namespace rejit_amd {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr uint64_t kCopyChunk = 16384;    // output bytes per chunk: four passes of 256 lanes x 16 bytes
constexpr unsigned kCopyGrid = 256 * 8;   // persistent: eight workgroups for each of the 256 CUs
constexpr uint64_t kImageChunk = kThreads * pack::kGroupBytes;   // output bytes per chunk of an emit: ONE pass of 256 lanes x 16 bytes
static_assert(kImageChunk == 4096, "one pass of the workgroup fills or stores the chunk's image (record_zip.h's kEmitChunk is this number)");

// the summary every record call writes (device words, copied to the scan's pinned copy).  kSumBadWord: the first bad row of
// the call in the call's own encoding, 0: none -- the LARGEST word wins (one atomic max), and every encoding makes that the
// first row: ~row (join, pack), replace::bad_word (replace).
enum { kSumKept = 0, kSumMatching, kSumCrossing, kSumBadWord, kSumSelected, kSumTotal, kSumTimedOut, kSumWords = 8 };

// a refused call: a bad row, or a unit scan that timed out -- its tables are not followed anywhere, and no output row is written
__device__ __forceinline__ bool refused(const unsigned long long* summary) { return summary[kSumBadWord] != 0 || summary[kSumTimedOut] != 0; }

// ---------------------------------------------------------------------------------------------------------------- wave sums
// 64-bit sum / inclusive prefix sum over the wave from wave_ops.h's 32-bit ones: three pieces of at most 22 bits (64 x 2^22 fits)
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
  const uint64_t a = wave_total(static_cast<uint32_t>(x) & 0x3FFFFFu);
  const uint64_t b = wave_total(static_cast<uint32_t>(x >> 22) & 0x3FFFFFu);
  const uint64_t c = wave_total(static_cast<uint32_t>(x >> 44));
  return a + (b << 22) + (c << 44);
}
__device__ __forceinline__ uint64_t wave_inclusive_sum64(uint64_t x) {
  const uint64_t a = wave_inclusive_sum(static_cast<uint32_t>(x) & 0x3FFFFFu);
  const uint64_t b = wave_inclusive_sum(static_cast<uint32_t>(x >> 22) & 0x3FFFFFu);
  const uint64_t c = wave_inclusive_sum(static_cast<uint32_t>(x >> 44));
  return a + (b << 22) + (c << 44);
}

// ---------------------------------------------------------------------------------------------------------------- wave lists
// The first bad row wins: the lowest lane of the wave that has a bad row gives its row's word to *bad_word by ONE atomic max
// -- a wave's rows ascend with its lanes, and every encoding makes the first row the largest word.
__device__ __forceinline__ void note_bad_word(bool bad, unsigned long long word, unsigned long long* bad_word) {
  const uint64_t bad_lanes = __ballot(bad);
  if (bad_lanes && lane_id() == __builtin_ctzll(bad_lanes)) atomicMax(bad_word, word);
}
// ... row j in the encoding ~j
__device__ __forceinline__ void note_bad_row(bool bad, uint64_t j, unsigned long long* bad_word) {
  note_bad_word(bad, static_cast<unsigned long long>(~j), bad_word);
}
// The flagged lanes' values appended to list[*counter ...): one ballot, ONE atomic add per wave (the leader's, of the
// popcount), the base broadcast, every flagged lane stores at base + the flagged lanes below it.
__device__ __forceinline__ void wave_append(bool flag, uint32_t value, unsigned long long* counter, uint32_t* list) {
  const uint64_t lanes = __ballot(flag);
  if (!lanes) return;
  const int leader = __builtin_ctzll(lanes);
  unsigned long long base = 0;
  if (lane_id() == leader) base = atomicAdd(counter, static_cast<unsigned long long>(__popcll(lanes)));
  base = lane_value(base, leader);
  if (flag) list[base + lanes_below(lanes)] = value;
}

// ---------------------------------------------------------------------------------------------------------------- text
// text[s, s + 16), all of it inside [0, n): two aligned 16-byte loads around it and a funnel shift by the source's
// misalignment, or ONE load when source and destination are aligned alike.  That one is a streaming read (stream_load.h:
// every cache line is asked for by one instruction); the two loads of the misaligned case ask for a line twice -- a lane's
// second block is its neighbour's first -- and keep the default policy.  At the text's two ends, where an aligned block
// would reach outside [0, n), kernel_util.h's guarded load reads the 16 bytes one by one.  load16_guarded is that load for
// any s: with it DeviceText is record_rows.h's Text.
struct DeviceText {
  const uint8_t* text;
  uint64_t n;
  __device__ __forceinline__ void load16(uint64_t s, uint32_t w[4]) const {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(text) + s;
    const uint32_t mis = static_cast<uint32_t>(addr & 15u);
    if (mis == 0) {
      const uint4 v = stream_load16(text + s);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      return;
    }
    if (s < mis || s - mis + 32 > n) {   // an aligned block would begin before the text or end behind it
      uint32_t d[6];
      load_guarded(text, n, s, d);
      w[0] = d[0], w[1] = d[1], w[2] = d[2], w[3] = d[3];
      return;
    }
    const uint4* a = reinterpret_cast<const uint4*>(text + (s - mis));
    const uint4 lo = a[0], hi = a[1];
    const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    // whole words first (a select over wave-divergent `mis`, no indexed registers), then the bytes
    uint32_t y[5];
    const uint32_t ws = mis >> 2;
#pragma unroll
    for (int i = 0; i < 5; i++) y[i] = ws == 0 ? x[i] : ws == 1 ? x[i + 1] : ws == 2 ? x[i + 2] : x[i + 3];
    const uint32_t bs = mis & 3u;
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = __builtin_amdgcn_alignbyte(y[i + 1], y[i], bs);
  }
  __device__ __forceinline__ void load16_guarded(uint64_t s, uint32_t w[4]) const {
    uint32_t d[6];
    load_guarded(text, n, s, d);
    w[0] = d[0], w[1] = d[1], w[2] = d[2], w[3] = d[3];
  }
  __device__ __forceinline__ uint32_t byte(uint64_t s) const { return s < n ? text[s] : 0u; }
};

// the rows of a call: row j is record indices[j], or record j
struct Rows {
  const uint64_t* __restrict__ rec_begin;
  const uint64_t* __restrict__ rec_end;
  const uint64_t* __restrict__ indices;
  __device__ __forceinline__ uint64_t record(uint64_t j) const { return indices ? indices[j] : j; }
};

// ---------------------------------------------------------------------------------------------------------------- unit scan
// A persistent workgroup takes units of work in ARRIVAL order (a ticket), so that every word the look-back of tile_lookback.h
// waits for belongs to a workgroup that has started; a unit publishes its total BEFORE it looks back, so that workgroup
// publishes without waiting.  A unit whose look-back timed out writes nothing, and the call fails (summary[kSumTimedOut]).
// Three layers: the ticket, the unit's place, a lane's place.  UnitPlace / UnitSum are the kernel's LDS words.
struct UnitPlace {
  unsigned long long ticket, before, end;
  uint32_t timed_out;
};
struct UnitSum {
  UnitPlace place;
  unsigned long long wave[kWaves];
};

// before the first ticket (its barrier makes the word visible)
__device__ __forceinline__ void unit_init(UnitPlace& f) {
  if (threadIdx.x == 0) f.timed_out = 0;
}

// the next unit in arrival order; false: none is left (workgroup-uniform)
__device__ __forceinline__ bool unit_take(UnitPlace& f, unsigned long long* ticket, uint64_t n_units, uint64_t* tk) {
  if (threadIdx.x == 0) f.ticket = atomicAdd(ticket, 1ull);
  __syncthreads();
  *tk = f.ticket;
  return *tk < n_units;
}

// Unit tk holds `total` (read in wave 0 only, behind a barrier of the caller's): wave 0 publishes it, resolves, and leaves
// f.before = the total of all units before tk and f.end = f.before + total.  False: the look-back timed out, now or in a unit
// this workgroup took earlier (workgroup-uniform).
__device__ __forceinline__ bool unit_place(UnitPlace& f, unsigned long long total, uint64_t tk, uint64_t n_units, unsigned long long* granules,
                                           unsigned long long* summary) {
  if (threadIdx.x < kWave) {
    const int lane = lane_id();
    if (lane == 0) lookback::publish(granules, n_units, tk, total);
    unsigned long long before = 0;
    const bool ok = lookback::resolve(granules, n_units, tk, &before);
    if (lane == 0) {
      f.before = before;
      f.end = before + total;
      if (!ok) {
        f.timed_out = 1;
        summary[kSumTimedOut] = 1;
      }
    }
  }
  __syncthreads();
  return f.timed_out == 0;
}

// `add` per lane -> the sum of everything before this lane (all units before, all lanes before) and the sum up to the unit's
// end.  False: as unit_place.
__device__ __forceinline__ bool unit_exclusive_sum(UnitSum& f, uint64_t add, uint64_t tk, uint64_t n_units, unsigned long long* granules,
                                                   unsigned long long* summary, uint64_t* before_lane, uint64_t* unit_end) {
  const int wv = static_cast<int>(threadIdx.x) >> 6;
  const uint64_t inc = wave_inclusive_sum64(add);
  if (lane_id() == kWave - 1) f.wave[wv] = inc;
  __syncthreads();
  unsigned long long total = 0;
  if (wv == 0) {
#pragma unroll
    for (int w = 0; w < kWaves; w++) total += f.wave[w];
  }
  const bool ok = unit_place(f.place, total, tk, n_units, granules, summary);
  uint64_t at = f.place.before + inc - add;
#pragma unroll
  for (int w = 0; w < kWaves; w++)
    if (w < wv) at += f.wave[w];
  *before_lane = at;
  *unit_end = f.place.end;
  return ok;
}

// ---------------------------------------------------------------------------------------------------------------- plan
// The plan of a pack: row-major, one row per lane, a unit = 256 rows.  row(j) -> {bad word (0: a good row), the row's output
// length}; a good row advances the output by its length + gap, a bad one by nothing.  It writes ob / oe, leaves the first bad
// row's word (the largest) and the total in the summary.
struct PlannedRow {
  unsigned long long bad;
  uint64_t len;
};
template <class RowFn>
__device__ __forceinline__ void plan_units(const RowFn& row, uint64_t k, uint64_t lead, uint64_t gap, unsigned long long* granules,
                                           unsigned long long* ticket, uint64_t n_units, uint64_t* __restrict__ out_begin,
                                           uint64_t* __restrict__ out_end, unsigned long long* summary) {
  __shared__ UnitSum s_unit;
  const uint32_t tid = threadIdx.x;
  if (n_units == 0) {   // no rows: the output is the lead
    if (blockIdx.x == 0 && tid == 0) summary[kSumTotal] = lead;
    return;
  }
  unit_init(s_unit.place);
  for (uint64_t tk; unit_take(s_unit.place, ticket, n_units, &tk);) {
    const uint64_t j = tk * kThreads + tid;
    PlannedRow r{0, 0};
    if (j < k) r = row(j);
    const uint64_t add = j < k ? pack::row_advance(r.bad != 0, 0, r.len, gap) : 0;
    note_bad_word(r.bad != 0, r.bad, &summary[kSumBadWord]);
    uint64_t before, unit_end;
    const bool ok = unit_exclusive_sum(s_unit, add, tk, n_units, granules, summary, &before, &unit_end);
    if (ok && tk == n_units - 1 && tid == 0) summary[kSumTotal] = lead + unit_end;
    if (ok && j < k) {
      if (out_begin) out_begin[j] = lead + before;
      if (out_end) out_end[j] = lead + before + r.len;
    }
  }
}

// ... over row lengths a kernel in front of it has staged (the zip, the CSV writer); returns at once behind a bad row
__device__ __forceinline__ void plan_staged_lengths(const uint64_t* __restrict__ row_len, uint64_t k, uint64_t lead, uint64_t gap,
                                                    unsigned long long* granules, unsigned long long* ticket, uint64_t n_units,
                                                    uint64_t* __restrict__ out_begin, uint64_t* __restrict__ out_end, unsigned long long* summary) {
  if (refused(summary)) return;
  const auto row = [=](uint64_t j) { return PlannedRow{0, row_len[j]}; };
  plan_units(row, k, lead, gap, granules, ticket, n_units, out_begin, out_end, summary);
}

// The check of a call whose rows index a column of n_values values: one lane per row, index < n_values; the first bad row
// wins (note_bad_row).  It stands in front of the plan, which writes its table rows unit by unit: a refused call writes none.
__device__ __forceinline__ void check_indices(const uint64_t* __restrict__ indices, uint64_t n_values, uint64_t k, uint64_t n_units,
                                              unsigned long long* summary) {
  for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const uint64_t j = unit * kThreads + threadIdx.x;
    const bool bad = j < k && indices[j] >= n_values;
    note_bad_row(bad, j, &summary[kSumBadWord]);
  }
}

// ---------------------------------------------------------------------------------------------------------------- copy
// The copy of a pack: output-major, so a workgroup's work does not depend on the records' sizes.  The output [0, min(total,
// out_cap)) is cut into chunks; the grid is persistent and reads the total from the summary (the host has not seen it yet).
// Per chunk two lanes search the ob table for the rows that touch it, the rows are staged in LDS when they fit (else every
// lane searches the table), and every lane produces 16 aligned output bytes at a time.  The policy P supplies
//   P.kRows, P::Stage          the rows a chunk stages and their LDS: ob[kRows + 1], src[kRows] and whatever else a row needs
//   P.table(ob, k, total)      the pack::View of the tables in memory
//   P.stage_row(stage, i, table, j)   what row j stages at i besides its ob
//   P.staged(stage) / P.unstaged()    what group16 reads a row's extras from, made once per chunk
//   P.group16(view, extras, rows, p, limit, gap, fill, text, w)   the 16 output bytes at p
template <class Policy>
__device__ __forceinline__ void copy_chunks(const Policy& P, const uint8_t* __restrict__ text, uint64_t n, uint64_t k, const uint64_t* __restrict__ ob,
                                            uint64_t gap, uint32_t fill, uint64_t chunk, uint32_t stage_cap, uint8_t* __restrict__ out,
                                            uint64_t out_cap, const unsigned long long* summary) {
  __shared__ typename Policy::Stage s_stage;
  __shared__ uint64_t s_rows[2];
  if (refused(summary)) return;
  const uint64_t total = summary[kSumTotal];
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint64_t n_chunks = (limit + chunk - 1) / chunk;
  const uint32_t tid = threadIdx.x;
  const pack::View table = P.table(ob, k, total);
  const DeviceText src{text, n};
  for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t c0 = c * chunk;
    const uint64_t c1 = c0 + chunk < limit ? c0 + chunk : limit;
    // ---- the rows that touch the chunk: two searches side by side, the second one from row 0 (it does not wait for the first)
    if (tid == 0) s_rows[0] = pack::chunk_first_row(table, k, c0);
    if (tid == kWave) s_rows[1] = pack::chunk_end_row(table, k, 0, c1);
    __syncthreads();
    pack::Rows rows;
    rows.j0 = s_rows[0];
    rows.j1 = s_rows[1] > rows.j0 ? s_rows[1] : rows.j0;
    const bool staged = pack::chunk_fits_stage(rows, stage_cap);   // workgroup-uniform
    pack::View view = table;
    auto extras = P.unstaged();
    if (staged) {
      for (uint64_t i = tid; i <= rows.j1 - rows.j0; i += kThreads) {
        s_stage.ob[i] = table.ob_at(rows.j0 + i);
        if (rows.j0 + i < rows.j1) P.stage_row(s_stage, i, table, rows.j0 + i);
      }
      __syncthreads();
      view = pack::View{s_stage.ob, s_stage.src, nullptr, nullptr, rows.j0, ~0ull, total};
      extras = P.staged(s_stage);
    }
    // ---- 16 aligned output bytes per lane and pass
    for (uint64_t p = c0 + static_cast<uint64_t>(tid) * pack::kGroupBytes; p < c1; p += static_cast<uint64_t>(kThreads) * pack::kGroupBytes) {
      uint32_t w[4];
      P.group16(view, extras, rows, p, limit, gap, fill, src, w);
      const uint32_t bytes = pack::group_store_bytes(p, limit);
      if (bytes == pack::kGroupBytes) {
        *reinterpret_cast<uint4*>(out + p) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (uint32_t b = 0; b < bytes; b++) out[p + b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
      }
    }
    __syncthreads();   // (the next chunk rewrites s_rows and the stage)
  }
}

// ---------------------------------------------------------------------------------------------------------------- emit
// The emit of a call that MAKES its rows' bytes: copy_chunks' sibling -- output-major, persistent, the total read from the
// summary, the rows of a chunk from the same pair of searches -- whose chunk of kImageChunk bytes is built in LDS.  Rows can be
// a few bytes at any offset, so a chunk holds hundreds of them, and a lane that searched for the rows under its 16 bytes
// would make a row once per group it touches.  Here every row of the chunk is written ONCE, by its own lane, into the
// chunk's image (preset with the fill byte), and behind a barrier every lane stores 16 aligned bytes of it.  The rows of a
// chunk are not bounded (empty rows with gap 0): the lanes take them 256 at a time.  No byte stores to memory but the last
// group's below the limit, no atomics.  The policy P supplies (ImagePolicy has the hooks a unit need not say)
//   P.row(j, c0, c1, put) -> bool     row j's bytes inside [c0, c1) through put(offset in the image, byte); true: a part of
//                                     the row is left to group16
//   P.reset()                         lane 0, before the chunk's first barrier: the flags in the unit's own LDS
//   P.note_streamed(any)              every lane, before the rows' barrier: one of its rows left a part to group16
//   P.between(c, c0, c1, put)         workgroup-uniform, behind the rows' barrier: a phase of the whole workgroup that writes
//                                     more of the image, and ends in a barrier of its own when it ran
//   P.streams() / P.group16(j, at, p, w)   in a chunk where streams() holds: true when the 16 bytes at p, inside row j at
//                                     `at`, come from registers (w) instead of the image
// LDS of a unit's own (a layout, a list, the stream flag) is declared in the unit's kernel and reaches the policy by reference.
// put(offset in the image, byte): the one writer of the image (forced inline: a call inside the rows' loop would spill the row)
struct ImagePut {
  uint8_t* image;
  __device__ __forceinline__ bool holds(uint64_t in_image) const { return in_image < kImageChunk; }
  __device__ __forceinline__ void operator()(uint64_t in_image, uint32_t byte) const {
    if (holds(in_image)) image[in_image] = static_cast<uint8_t>(byte);   // (always: every writer clips to the chunk)
  }
};
struct ImagePolicy {
  __device__ __forceinline__ void reset() const {}
  __device__ __forceinline__ void note_streamed(bool) const {}
  __device__ __forceinline__ void between(uint64_t, uint64_t, uint64_t, const ImagePut&) const {}
  __device__ __forceinline__ bool streams() const { return false; }
  __device__ __forceinline__ bool group16(uint64_t, uint64_t, uint64_t, uint32_t[4]) const { return false; }
};
// ... of a unit with a stream tier: one LDS word says whether a row of the chunk left a part to group16
struct StreamingImagePolicy : ImagePolicy {
  uint32_t& s_streams;
  __device__ __forceinline__ explicit StreamingImagePolicy(uint32_t& flag) : s_streams(flag) {}
  __device__ __forceinline__ void reset() const { s_streams = 0; }
  __device__ __forceinline__ void note_streamed(bool any) const {
    if (any) s_streams = 1;   // (every writer writes 1)
  }
  __device__ __forceinline__ bool streams() const { return s_streams != 0; }
};
template <class Policy>
__device__ __forceinline__ void emit_chunks(const Policy& P, uint64_t k, const uint64_t* __restrict__ ob, uint32_t fill, uint8_t* __restrict__ out,
                                            uint64_t out_cap, const unsigned long long* summary) {
  __shared__ uint4 s_image[kThreads];
  __shared__ uint64_t s_rows[2];
  if (refused(summary)) return;
  const uint64_t total = summary[kSumTotal];
  const uint64_t limit = total < out_cap ? total : out_cap;
  const uint64_t n_chunks = (limit + kImageChunk - 1) / kImageChunk;   // (limit <= total < pack::kMaxTotal: no wrap)
  const uint32_t tid = threadIdx.x;
  const pack::View table{ob, nullptr, nullptr, nullptr, 0, k, total};
  const ImagePut put{reinterpret_cast<uint8_t*>(s_image)};
  const uint32_t fw = pack::fill_word(fill);
  for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t c0 = c * kImageChunk;
    const uint64_t c1 = c0 + kImageChunk < limit ? c0 + kImageChunk : limit;
    // ---- the rows that touch the chunk (two searches side by side), and the image all fill
    if (tid == 0) s_rows[0] = pack::chunk_first_row(table, k, c0), P.reset();
    if (tid == kWave) s_rows[1] = pack::chunk_end_row(table, k, 0, c1);
    s_image[tid] = make_uint4(fw, fw, fw, fw);
    __syncthreads();
    const uint64_t j0 = s_rows[0], j1 = s_rows[1] > j0 ? s_rows[1] : j0;   // (j1 <= k)
    // ---- every row once: its bytes inside the chunk
    bool any_left = false;
    for (uint64_t j = j0 + tid; j < j1; j += kThreads) any_left |= P.row(j, c0, c1, put);
    P.note_streamed(any_left);
    __syncthreads();
    P.between(c, c0, c1, put);
    // ---- 16 aligned output bytes per lane: from registers where the policy has them, else the image's
    const uint64_t p = c0 + static_cast<uint64_t>(tid) * pack::kGroupBytes;
    if (p < c1) {
      uint32_t w[4];
      bool streamed = false;
      if (P.streams()) {
        const uint64_t u = pack::upper_bound(table, j0, j1, p);   // the last row that begins at or before p has p's bytes
        if (u > j0) streamed = P.group16(u - 1, ob[u - 1], p, w);
      }
      if (!streamed) {
        const uint4 v = s_image[tid];
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      }
      const uint32_t bytes = pack::group_store_bytes(p, limit);
      if (bytes == pack::kGroupBytes) {
        *reinterpret_cast<uint4*>(out + p) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (uint32_t b = 0; b < bytes; b++) out[p + b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
      }
    }
    __syncthreads();   // (the next chunk rewrites s_rows, the unit's flags and the image)
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
inline int ensure_summary(rj_scan* s) {
  if (!s->rec_host) RJ_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->rec_host), kSumWords * sizeof(unsigned long long)));
  RJ_HIP(s->rec_summary.reserve(kSumWords * sizeof(unsigned long long)));
  return RJ_OK;
}

// Before the launches of a call: the summary zeroed, and `scratch_words` zeroed words for its tickets and look-backs.
inline int records_begin(rj_scan* s, uint64_t scratch_words, hipStream_t st, unsigned long long** scratch, unsigned long long** summary) {
  const int rc = ensure_summary(s);
  if (rc != RJ_OK) return rc;
  *summary = s->rec_summary.as<unsigned long long>();
  if (scratch_words) {
    RJ_HIP(s->rec_granules.reserve(scratch_words * sizeof(unsigned long long)));
    *scratch = s->rec_granules.as<unsigned long long>();
    RJ_HIP(hipMemsetAsync(*scratch, 0, scratch_words * sizeof(unsigned long long), st));
  }
  RJ_HIP(hipMemsetAsync(*summary, 0, kSumWords * sizeof(unsigned long long), st));
  return RJ_OK;
}

// Behind them: the summary in s->rec_host, the stream idle (the one synchronise of the call).
inline int records_finish(rj_scan* s, const char* call, hipStream_t st) {
  RJ_HIP(hipMemcpyAsync(s->rec_host, s->rec_summary.p, kSumWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  RJ_HIP(hipStreamSynchronize(st));
  RJ_HIP(hipGetLastError());
  if (s->rec_host[kSumTimedOut] != 0) return rj_fail(RJ_DEVICE_ERROR, "%s: the look-back timed out", call);
  return RJ_OK;
}

// a test knob of a call, read at every call: the number in the environment's `name`, at most `most`; `otherwise` without one
inline uint32_t env_number(const char* name, uint32_t otherwise, uint32_t most) {
  const char* v = getenv(name);
  if (!v || !*v) return otherwise;
  char* end = nullptr;
  const unsigned long long x = strtoull(v, &end, 10);
  if (!end || *end) return otherwise;
  return x > most ? most : static_cast<uint32_t>(x);
}

// the argument checks rj_scan_records_pack and rj_scan_records_replace share (each checks its own tables' alignment behind them)
inline int check_pack_call(const char* call, const rj_scan* s, const void* d_text, uint64_t n, const uint64_t* d_rec_begin, const uint64_t* d_rec_end,
                           uint64_t n_records, const void* d_out, uint64_t out_cap, int fill) {
  if (!s || (!d_text && n) || (n_records && (!d_rec_begin || !d_rec_end)) || (!d_out && out_cap)) return rj_fail(RJ_BAD_ARGUMENT, "%s: null argument", call);
  if (fill < 0 || fill > 255) return rj_fail(RJ_BAD_ARGUMENT, "%s: fill %d is not a byte (0..255)", call, fill);
  if (reinterpret_cast<uintptr_t>(d_out) & 15u) return rj_fail(RJ_BAD_ARGUMENT, "%s: d_out is not 16-byte aligned", call);
  return RJ_OK;
}
template <class... P>
inline bool aligned8(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t{0}) & 7u) == 0;
}

// the new begins of a pack that copies: the caller's, else the scan's own (the copy needs the table)
inline int pack_begin_table(rj_scan* s, uint64_t* d_out_begin, bool copies, uint64_t k, uint64_t** ob) {
  *ob = d_out_begin;
  if (!*ob && copies && k) {
    RJ_HIP(s->rec_pack_begin.reserve(k * sizeof(uint64_t)));
    *ob = s->rec_pack_begin.as<uint64_t>();
  }
  return RJ_OK;
}

// What the calls over a column of values (rj_scan_records_format, rj_scan_records_format_time) do before their launches: the
// begin table, 16 bytes of stage per row for a call that copies, the summary and the scratch -- the ticket, then the
// look-back's words.
inline int value_rows_begin(rj_scan* s, uint64_t* d_out_begin, bool copies, uint64_t k, uint64_t n_units, hipStream_t st, uint64_t** ob, ulonglong2** stage,
                            unsigned long long** scratch, unsigned long long** summary) {
  const int rc = pack_begin_table(s, d_out_begin, copies, k, ob);
  if (rc != RJ_OK) return rc;
  *stage = nullptr;
  if (copies && k) {
    RJ_HIP(s->rec_format_stage.reserve(k * sizeof(ulonglong2)));
    *stage = s->rec_format_stage.as<ulonglong2>();
  }
  return records_begin(s, 1 + lookback::granule_words(n_units), st, scratch, summary);
}
// ... and behind records_finish, when check_indices left a bad row in the summary
inline int bad_index_failure(const rj_scan* s, const char* call) {
  return rj_fail(RJ_BAD_ARGUMENT, "%s: row %llu names no value (index < n_values)", call, static_cast<unsigned long long>(~s->rec_host[kSumBadWord]));
}

// persistent grids: workgroups take units / chunks until none is left.  The chunks of at most `bytes` output bytes are
// counted without a sum that could wrap: a caller's out_cap may be any "large enough" number.
inline unsigned unit_grid(uint64_t n_units) { return static_cast<unsigned>(n_units < 1 ? 1 : n_units < 1024 ? n_units : 1024); }
inline uint64_t chunks_of(uint64_t bytes, uint64_t chunk) { return bytes / chunk + (bytes % chunk != 0); }
inline unsigned chunk_grid(uint64_t bytes, uint64_t chunk) {
  const uint64_t chunks = chunks_of(bytes, chunk);
  return static_cast<unsigned>(chunks < kCopyGrid ? chunks : kCopyGrid);
}
inline unsigned copy_grid(uint64_t out_cap) { return chunk_grid(out_cap, kCopyChunk); }
inline unsigned image_grid(uint64_t bytes) { return chunk_grid(bytes, kImageChunk); }

}  // namespace

}  // namespace rejit_amd
#endif
