// tests/support/csv_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_csv.h, compiled with g++ (tests/test_record_csv.py).
// It walks the call the way record_csv.hip's kernels do -- the summarise span by span, step by step and lane by lane (the
// lanes' parities joined as the ballot joins them, the step's counts in the 16-bit halves the wave sums carry), the resolve
// with its lanes over consecutive spans, the clear, the emit with the halo taken from the neighbouring lanes, the byte before
// the step carried and the last lane's two bytes ahead read from the text -- with the unit, the lanes of a wave, the waves
// of the grid and the lanes of the resolve chosen by the test, so that every seam can be forced on tiny texts.  Every text
// read is checked against its range, every table entry may be written only once and only below its cap, and a complete
// call must have written every entry below the counts.
//
// With -DCSV_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): the same
// driver over seeded texts, against the rule written byte by byte, over allocations exact in their last byte.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_csv.h"
#include "checked_text.h"

using namespace rejit_amd;

namespace {

csv::Group load_core(const CheckedText& src, uint64_t p0, uint64_t span_end) {
  csv::Group g;
  g.w[0] = g.w[1] = g.w[2] = g.w[3] = 0;
  g.prev = g.next1 = g.next2 = -1;
  g.valid = p0 >= span_end ? 0u : span_end - p0 < csv::kGroup ? static_cast<uint32_t>(span_end - p0) : csv::kGroup;
  if (g.valid == csv::kGroup) src.load16(p0, g.w);
  else if (g.valid != 0) src.load16_guarded(p0, g.w);
  return g;
}

// a span as the summarise kernel walks it
csv::Summary summarise_span(const CheckedText& src, uint64_t s0, uint64_t s1, uint32_t lanes, int delimiter, int quote) {
  csv::Summary run = csv::nothing();
  for (uint64_t p = s0; p < s1; p += static_cast<uint64_t>(lanes) * csv::kGroup) {
    uint32_t parity = 0, c0 = 0, c1 = 0;
    for (uint32_t lane = 0; lane < lanes; lane++) {
      const csv::Group g = load_core(src, p + static_cast<uint64_t>(lane) * csv::kGroup, s1);
      const csv::LaneSummary l = csv::lane_summary(csv::make_masks(g, delimiter, quote));
      c0 += parity ? l.c[1] : l.c[0];
      c1 += parity ? l.c[0] : l.c[1];
      parity ^= l.parity;
    }
    run = csv::compose(run, csv::widen(parity, c0, c1));
  }
  return run;
}

// the caller's tables with the kernel's caps, every entry once
struct Sink {
  uint64_t *rows_first, *rows_begin, *rows_end, row_cap, *begins, *ends;
  uint32_t* flags;
  uint64_t field_cap;
  std::vector<uint8_t> once[5];   // field begin, field end, row begin, row end, row first
  bool twice = false, beyond = false;
  uint64_t n_fields = 0, n_rows = 0;   // the resolve's counts: nothing is owned beyond them
  void put(int which, uint64_t* table, uint64_t i, uint64_t cap, uint64_t count, uint64_t v) {
    if (i >= count) beyond = true;
    if (i >= cap) return;
    if (once[which].size() <= i) once[which].resize(i + 1, 0);
    if (once[which][i]) twice = true;
    once[which][i] = 1;
    if (table) table[i] = v;
  }
  void field_begin(uint64_t f, uint64_t v) { put(0, begins, f, field_cap, n_fields, v); }
  void field_end(uint64_t f, uint64_t v) { put(1, ends, f, field_cap, n_fields, v); }
  void flag(uint64_t f, uint32_t bits) {
    if (f >= n_fields) beyond = true;
    if (flags && f < field_cap) flags[f] |= bits;
  }
  void row_begin(uint64_t r, uint64_t v) { put(2, rows_begin, r, row_cap, n_rows, v); }
  void row_end(uint64_t r, uint64_t v) { put(3, rows_end, r, row_cap, n_rows, v); }
  void row_first(uint64_t r, uint64_t v) { put(4, rows_first, r, row_cap + 1, n_rows + 1, v); }
  bool complete(int which, uint64_t count) const {
    for (uint64_t i = 0; i < count; i++)
      if (i >= once[which].size() || !once[which][i]) return false;
    return true;
  }
};

}  // namespace

// [0] kGroup, [1] kLanes, [2] kStep, [3] kUnit, [4] kGrid, [5] kWavesPerGroup, [6] sizeof(Summary), [7] sizeof(Entry)
extern "C" void ce_constants(int64_t* out) {
  out[0] = csv::kGroup, out[1] = csv::kLanes, out[2] = csv::kStep, out[3] = csv::kUnit, out[4] = csv::kGrid, out[5] = csv::kWavesPerGroup;
  out[6] = sizeof(csv::Summary), out[7] = sizeof(csv::Entry);
}

// the summary of a whole text, lane by lane: [0] parity, [1] [2] fields, [3] [4] rows
extern "C" void ce_summary(const uint8_t* text, uint64_t n, int delimiter, int quote, uint32_t lanes, uint64_t* out) {
  const CheckedText src{text, n};
  const csv::Summary s = summarise_span(src, 0, n, lanes, delimiter, quote);
  out[0] = s.parity, out[1] = s.fields[0], out[2] = s.fields[1], out[3] = s.rows[0], out[4] = s.rows[1];
}
extern "C" void ce_compose(const uint64_t* a, const uint64_t* b, uint64_t* out) {
  const csv::Summary s = csv::compose(csv::Summary{a[0], {a[1], a[2]}, {a[3], a[4]}}, csv::Summary{b[0], {b[1], b[2]}, {b[3], b[4]}});
  out[0] = s.parity, out[1] = s.fields[0], out[2] = s.fields[1], out[3] = s.rows[0], out[4] = s.rows[1];
}

// stats: rj_csv_stats' nine words.  info: [0] check_call's code, [1] units, [2] units per wave, [3] waves with a span.
// Returns n_fields; -1 when an access left its range, an entry was written twice or at or beyond the counts, or a complete
// call left an entry unwritten; -2 for a call check_call refuses or bad driver parameters.
extern "C" long ce_csv(const uint8_t* text, uint64_t n, int delimiter, int quote, uint64_t unit, uint32_t lanes, uint64_t wave_cap, uint32_t resolve_lanes,
                       uint64_t* row_first, uint64_t* row_begin, uint64_t* row_end, uint64_t row_cap, uint64_t* field_begin, uint64_t* field_end,
                       uint32_t* field_flags, uint64_t field_cap, uint64_t* stats, uint64_t* info) {
  for (int i = 0; i < 4; i++) info[i] = 0;
  int scan = 0;
  const csv::Refusal why = csv::check_call(&scan, text, n, delimiter, quote, row_first, row_begin, row_end, field_begin, field_end, field_flags, stats);
  info[0] = why;
  if (why != csv::kFine) return -2;
  const uint64_t step = static_cast<uint64_t>(lanes) * csv::kGroup;
  if (lanes == 0 || lanes > csv::kLanes || unit == 0 || unit % step || wave_cap == 0 || resolve_lanes == 0) return -2;
  const csv::Geometry geo = csv::geometry(n, unit, wave_cap);
  info[1] = geo.units, info[2] = geo.per_wave, info[3] = geo.waves;
  if (geo.waves > wave_cap) return -1;
  const CheckedText src{text, n};
  // ---- summarise
  std::vector<csv::Summary> summaries(geo.waves);
  for (uint64_t v = 0; v < geo.waves; v++)
    summaries[v] = summarise_span(src, csv::span_begin(geo, unit, n, v), csv::span_begin(geo, unit, n, v + 1), lanes, delimiter, quote);
  // ---- resolve: lane l composes its spans, the lanes' parities and counts go through prefixes, every lane walks again
  std::vector<csv::Entry> entries(geo.waves);
  const uint64_t per = (geo.waves + resolve_lanes - 1) / resolve_lanes;
  csv::Entry lane_entry{0, 0, 0}, end_state{0, 0, 0};
  for (uint32_t l = 0; l < resolve_lanes; l++) {
    const uint64_t a = l * per < geo.waves ? l * per : geo.waves, b = a + per < geo.waves ? a + per : geo.waves;
    csv::Summary mine = csv::nothing();
    for (uint64_t i = a; i < b; i++) mine = csv::compose(mine, summaries[i]);
    csv::Entry e = lane_entry;
    for (uint64_t i = a; i < b; i++) {
      entries[i] = e;
      e = csv::advance(e, summaries[i]);
    }
    lane_entry = csv::advance(lane_entry, mine);
    if (e.parity != lane_entry.parity || e.fields != lane_entry.fields || e.rows != lane_entry.rows) return -1;   // (the two walks agree)
    end_state = e;
  }
  const uint64_t tail = csv::tail_row(n, n ? src.at(n - 1) : 0u, end_state);
  for (int i = 0; i < 9; i++) stats[i] = 0;
  stats[0] = end_state.rows + tail, stats[1] = end_state.fields + tail;
  stats[7] = end_state.parity;
  stats[8] = end_state.parity ? n : ~0ull;
  Sink sink{row_first, row_begin, row_end, row_cap, field_begin, field_end, field_flags, field_cap, {}, false, false, stats[1], stats[0]};
  sink.row_first(0, 0);
  // ---- clear
  for (uint64_t f = 0; field_flags && f < stats[1] && f < field_cap; f++) field_flags[f] = 0;
  // ---- emit
  std::vector<csv::Group> groups(lanes);
  for (uint64_t v = 0; v < geo.waves; v++) {
    const uint64_t s0 = csv::span_begin(geo, unit, n, v), s1 = csv::span_begin(geo, unit, n, v + 1);
    csv::Entry at = entries[v];
    int32_t prev_tail = s0 > 0 ? static_cast<int32_t>(src.at(s0 - 1)) : -1;
    for (uint64_t p = s0; p < s1; p += step) {
      for (uint32_t lane = 0; lane < lanes; lane++) groups[lane] = load_core(src, p + static_cast<uint64_t>(lane) * csv::kGroup, s1);
      for (uint32_t lane = 0; lane < lanes; lane++) {
        csv::Group& g = groups[lane];
        const uint64_t p0 = p + static_cast<uint64_t>(lane) * csv::kGroup;
        g.prev = lane == 0 ? prev_tail : static_cast<int32_t>(groups[lane - 1].w[3] >> 24);
        if (lane == lanes - 1) {
          g.next1 = p0 + 16 < n ? static_cast<int32_t>(src.at(p0 + 16)) : -1;
          g.next2 = p0 + 17 < n ? static_cast<int32_t>(src.at(p0 + 17)) : -1;
        } else {
          const csv::Group& up = groups[lane + 1];
          g.next1 = up.valid >= 1 ? static_cast<int32_t>(up.w[0] & 0xFFu) : -1;
          g.next2 = up.valid >= 2 ? static_cast<int32_t>((up.w[0] >> 8) & 0xFFu) : -1;
        }
      }
      prev_tail = static_cast<int32_t>(groups[lanes - 1].w[3] >> 24);
      uint32_t parity = 0, before = 0;
      for (uint32_t lane = 0; lane < lanes; lane++) {
        const csv::Group& g = groups[lane];
        const uint64_t p0 = p + static_cast<uint64_t>(lane) * csv::kGroup;
        const csv::Masks m = csv::make_masks(g, delimiter, quote);
        const uint32_t entry = (static_cast<uint32_t>(at.parity) ^ parity) & 1u;
        const csv::Marks k = csv::make_marks(m, entry, p0 == 0);
        csv::emit_group(k, p0, g.valid, n, at.fields + (before & 0xFFFFu), at.rows + (before >> 16), sink);
        csv::Tally t;
        csv::tally_init(&t);
        csv::tally_add(&t, k, p0);
        for (int i = 0; i < 5; i++) stats[2 + i] += t.n[i];
        if (t.first_bad < stats[8]) stats[8] = t.first_bad;
        parity ^= csv::popcount(m.q & m.in & csv::kCore) & 1u;
        before += csv::lane_counts(k);
      }
      at.parity ^= parity;
      at.fields += before & 0xFFFFu;
      at.rows += before >> 16;
    }
  }
  if (src.left_range || sink.twice || sink.beyond) return -1;
  const uint64_t fields = stats[1] < field_cap ? stats[1] : field_cap, rows = stats[0] < row_cap ? stats[0] : row_cap;
  if (!sink.complete(0, fields) || !sink.complete(1, fields) || !sink.complete(2, rows) || !sink.complete(3, rows) ||
      !sink.complete(4, stats[0] < row_cap + 1 ? stats[0] + 1 : row_cap + 1))
    return -1;
  return static_cast<long>(stats[1]);
}

#ifdef CSV_EXEC_MAIN
#include <stdio.h>
#include <stdlib.h>

namespace {

uint64_t rnd(uint64_t below) {
  static uint64_t rng = 88172645463325252ull;
  rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
  return rng % below;
}

struct Want {
  std::vector<uint64_t> row_first{0}, row_begin, row_end, begin, end;
  std::vector<uint32_t> flags;
};
// the rule, byte by byte
Want rule(const std::vector<uint8_t>& t, int d, int q) {
  const uint64_t n = t.size();
  std::vector<uint8_t> ins(n + 1, 0);
  for (uint64_t p = 0; p < n; p++) ins[p + 1] = ins[p] ^ (q >= 0 && t[p] == q ? 1 : 0);
  Want w;
  uint64_t fb = 0, rb = 0;
  uint32_t fl = 0;
  const auto field = [&](uint64_t fe, bool at_end) {
    const uint64_t b = q >= 0 && fb < fe && t[fb] == q ? fb + 1 : fb;
    const bool open = at_end && ins[n];
    w.begin.push_back(b);
    w.end.push_back(q >= 0 && !open && fe > b && t[fe - 1] == q ? fe - 1 : fe);
    w.flags.push_back(fl | (open ? csv::kOpen : 0u));
  };
  for (uint64_t p = 0; p < n; p++) {
    const int c = t[p];
    if (q >= 0 && c == q) {
      if (!ins[p]) {
        if (p != fb) fl |= t[p - 1] == q ? csv::kEscaped : csv::kBadQuote;
      } else if (!(p + 1 == n || t[p + 1] == d || t[p + 1] == '\n' || t[p + 1] == q || (t[p + 1] == '\r' && p + 2 < n && t[p + 2] == '\n'))) {
        fl |= csv::kBadClose;
      }
    }
    if (c == '\r' && !ins[p] && !(p + 1 < n && t[p + 1] == '\n')) fl |= csv::kBareCr;
    if (!ins[p] && (c == d || c == '\n')) {
      const uint64_t fe = c == '\n' && p > fb && t[p - 1] == '\r' ? p - 1 : p;
      field(fe, false);
      fb = p + 1, fl = 0;
      if (c == '\n') w.row_begin.push_back(rb), w.row_end.push_back(fe), w.row_first.push_back(w.begin.size()), rb = p + 1;
    }
  }
  if (n && !(t[n - 1] == '\n' && !ins[n - 1])) field(n, true), w.row_begin.push_back(rb), w.row_end.push_back(n), w.row_first.push_back(w.begin.size());
  return w;
}

}  // namespace

int main() {
  static const char alphabet[] = "ab\"\",,\n\n\r\t";
  int cases = 0;
  for (int round = 0; round < 3000; round++) {
    const uint64_t n = round < 40 ? round : rnd(200);
    const int d = round % 3 == 2 ? '\t' : ',', q = round % 5 == 4 ? -1 : '"';
    std::vector<uint8_t> text(n);
    for (auto& c : text) c = static_cast<uint8_t>(alphabet[rnd(sizeof(alphabet) - 1)]);
    const Want w = rule(text, d, q);
    // everything exact in its last entry
    uint8_t* exact = static_cast<uint8_t*>(malloc(n ? n : 1));
    if (n) memcpy(exact, text.data(), n);
    const uint64_t rows = w.row_begin.size(), fields = w.begin.size();
    const uint64_t row_cap = round % 7 == 6 && rows ? rows - 1 : rows, field_cap = round % 11 == 10 && fields ? fields - 1 : fields;
    std::vector<uint64_t> rf(row_cap + 1), rb(row_cap), re(row_cap), fb(field_cap), fe(field_cap);
    std::vector<uint32_t> ff(field_cap);
    uint64_t stats[9], info[4];
    const uint32_t lanes = 1 + static_cast<uint32_t>(rnd(4));
    const uint64_t unit = lanes * 16 * (1 + rnd(2));
    const long rc = ce_csv(exact, n, d, q, unit, lanes, 1 + rnd(5), 1 + static_cast<uint32_t>(rnd(4)), rf.data(), row_cap ? rb.data() : nullptr,
                           row_cap ? re.data() : nullptr, row_cap, field_cap ? fb.data() : nullptr, field_cap ? fe.data() : nullptr,
                           field_cap ? ff.data() : nullptr, field_cap, stats, info);
    free(exact);
    bool same = rc == static_cast<long>(fields) && stats[0] == rows && stats[1] == fields;
    for (uint64_t r = 0; same && r < row_cap; r++) same = rb[r] == w.row_begin[r] && re[r] == w.row_end[r];
    for (uint64_t r = 0; same && r <= row_cap; r++) same = rf[r] == w.row_first[r];
    for (uint64_t f = 0; same && f < field_cap; f++) same = fb[f] == w.begin[f] && fe[f] == w.end[f] && ff[f] == w.flags[f];
    if (!same) {
      fprintf(stderr, "csv_exec: round %d (n %llu, lanes %u, unit %llu): rc %ld, %llu rows and %llu fields wanted\n", round, static_cast<unsigned long long>(n),
              lanes, static_cast<unsigned long long>(unit), rc, static_cast<unsigned long long>(rows), static_cast<unsigned long long>(fields));
      return 1;
    }
    cases++;
  }
  printf("csv_exec: %d cases\n", cases);
  return 0;
}
#endif
