// tests/support/time_format_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_time_format.h, compiled with g++
// (tests/test_record_time_format.py).  It walks the call the way record_time_format.hip's kernels do -- the arguments and the
// format first (a refused call writes nothing), the index check, the plan (a row's status and value, its instant split ONCE
// and staged, its length L or 0 into the running sum), the emit chunk by chunk: the chunk's rows from one pair of searches,
// every row's bytes inside the chunk written once through the layout table into the chunk's image (the kernel's LDS) -- with
// the chunk size chosen by the test, so that a chunk's end cuts rows at every position.  Every access is checked against its
// range, and every output byte and table row may be written only once.  With `round_trip` every OK row is read back by
// record_time.h's own walk and must give the value with status OK.
//
// With -DTIME_FORMAT_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): seeded
// random instants under seven formats, four units and five zones against the meaning written out over std::string, with a
// calendar that counts the days year by year, over exact allocations.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_time.h"
#include "../../rejit_amd/csrc/record_time_format.h"
#include "checked_image.h"

using namespace rejit_amd;

// [0] kMaxRowBytes, [1] sizeof(Fields), [2] sizeof(Layout), [3] kSourceBytes
extern "C" void tf_constants(int64_t* out) {
  out[0] = timeformat::kMaxRowBytes;
  out[1] = sizeof(timeformat::Fields);
  out[2] = sizeof(timeformat::Layout);
  out[3] = timeformat::kSourceBytes;
}

// -> the FormatError; *at: the offset it names; code[0, 64) and *len: the program
extern "C" int tf_compile(const uint8_t* format, uint64_t format_len, int writing, uint8_t* code, uint32_t* len, uint32_t* at) {
  timeparse::Program p{};
  const int e = timeparse::compile_mode(format, format_len, writing != 0, &p, at);
  if (e != timeparse::kFormatOk) return e;
  for (uint32_t i = 0; i < timeparse::kMaxFormat; i++) code[i] = static_cast<uint8_t>(timeparse::program_byte(p, i));
  *len = p.len;
  return 0;
}

// the layout of a format: entries[0, 80) -> L; -2: the format is refused
extern "C" int tf_layout(const uint8_t* format, uint64_t format_len, int unit, int zone_minutes, uint16_t* entries) {
  timeparse::Program p{};
  uint32_t at = 0;
  if (timeparse::compile_mode(format, format_len, true, &p, &at) != timeparse::kFormatOk) return -2;
  const timeformat::Layout l = timeformat::make_layout(p, unit, zone_minutes);
  for (uint32_t i = 0; i < 2 * timeformat::kLayoutWords; i++) entries[i] = static_cast<uint16_t>(timeformat::layout_entry(l, i));
  return static_cast<int>(l.len);
}

// civil_from_days(days_from_civil(y, m, d)) == (y, m, d) for every day of 0001..9999, the days counted one by one -> the days
// walked; -1 at the first difference
extern "C" long tf_calendar(void) {
  long walked = 0;
  int64_t expected = -static_cast<int64_t>(timeformat::kEpochDay);
  for (uint32_t y = 1; y <= 9999; y++)
    for (uint32_t m = 1; m <= 12; m++)
      for (uint32_t d = 1; d <= timeparse::days_in_month(y, m); d++) {
        const int64_t days = timeparse::days_from_civil(y, m, d);
        if (days != expected++) return -1;
        const timeformat::Civil c = timeformat::civil_from_days(static_cast<uint32_t>(days + timeformat::kEpochDay));
        if (c.year != y || c.month != m || c.day != d) return -1;
        walked++;
      }
  return walked;
}

namespace {

// the row's bytes read back by record_time.h's walk, in groups of 16
timeparse::Result read_back(const uint8_t* row, uint32_t len, const timeparse::Program& p, int unit) {
  uint8_t code[timeparse::kMaxFormat];
  for (uint32_t i = 0; i < timeparse::kMaxFormat; i++) code[i] = static_cast<uint8_t>(timeparse::program_byte(p, i));
  timeparse::State s = timeparse::start(0);
  for (uint32_t at = 0; at < len && !timeparse::done(s); at += 16) {
    const uint32_t valid = len - at < 16 ? len - at : 16;
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < valid; i++) w[i >> 2] |= static_cast<uint32_t>(row[at + i]) << (8 * (i & 3));
    timeparse::step(s, code, p.len, w, valid);
  }
  return timeparse::finish(s, p.len, unit);
}

}  // namespace

// summary: [0] n_ok, [1] n_null, [2] n_range, [3] the first bad row (~0: none), [4] the format error's offset, [5] L,
// [6] the rows read back, [7] the refusal (timeformat::Refusal; 100 + the FormatError for a refused format).
// Returns the total; -1 when an access left its range, something was written twice or a byte below the limit was not written
// (bugs the kernel would pay for with a fault or a race); -2 for a call that is refused up front; -3 when a row read back gave
// another value; -4 for a bad index (a refused call: nothing is written).
extern "C" long tf_format(const uint64_t* value, const uint8_t* status, uint64_t n_values, const uint64_t* indices, int have_indices, uint64_t n_indices,
                          const uint8_t* format, uint64_t format_len, int unit, int zone_minutes, unsigned flags, int fill, uint64_t lead, uint64_t gap,
                          uint64_t chunk, int round_trip, uint8_t* out, uint64_t out_cap, uint64_t* out_begin, uint64_t* out_end, uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[3] = ~0ull;
  static const uint64_t kNoRows[1] = {0};
  const uint64_t* idx = have_indices ? (indices ? indices : kNoRows) : nullptr;
  const uint64_t k = have_indices ? n_indices : n_values;
  timeformat::Refusal why = timeformat::check_arguments(value, n_values, idx, format, format_len, unit, zone_minutes, flags, fill, out, out_cap, out_begin, out_end);
  timeparse::Program program{};
  if (why == timeformat::kFine) {
    uint32_t at = 0;
    const int bad = timeparse::compile_mode(format, format_len, true, &program, &at);
    if (bad != timeparse::kFormatOk) {
      summary[4] = at;
      summary[7] = 100 + static_cast<uint64_t>(bad);
      return -2;
    }
    why = timeformat::check_sizes(k, lead, gap);
  }
  summary[7] = why;
  if (why != timeformat::kFine || chunk == 0) return -2;
  const timeformat::Layout layout = timeformat::make_layout(program, unit, zone_minutes);
  const uint32_t L = layout.len;
  summary[5] = L;
  if (L == 0 || L > timeformat::kMaxRowBytes) return -1;
  // ---- check: the index list only
  for (uint64_t j = 0; j < k; j++)
    if (idx && idx[j] >= n_values) {
      summary[3] = j;
      return -4;
    }
  // ---- plan
  bool twice = false, left_range = false;
  std::vector<uint64_t> own_begin(k + 1);
  uint64_t* ob = out_begin ? out_begin : own_begin.data();
  std::vector<timeformat::Fields> stage(k);
  uint64_t at = lead;
  for (uint64_t j = 0; j < k; j++) {
    const uint64_t r = idx ? idx[j] : j;
    const timeformat::Fields f =
        (status && status[r] != timeformat::kStatusOk) ? timeformat::null_row() : timeformat::split_unit(value[r], unit, zone_minutes * 60);
    const uint32_t cls = timeformat::class_of(f);
    if (cls >= timeformat::kClasses) return -1;
    summary[cls == timeformat::kOk ? 0 : cls == timeformat::kNull ? 1 : 2]++;
    stage[j] = f;
    const uint64_t len = timeformat::row_len(f, L);
    ob[j] = at;
    if (out_end) out_end[j] = at + len;
    at += pack::row_advance(false, 0, len, gap);
  }
  const uint64_t total = at;
  // ---- emit
  const pack::View table{ob, nullptr, nullptr, nullptr, 0, k, total};
  const long chunks = walk_chunks(table, k, total, chunk, out, out_cap, [&](uint64_t c0, uint64_t c1, uint64_t j0, uint64_t j1, std::vector<uint8_t>* got) {
    CheckedImage image(chunk, static_cast<uint32_t>(fill), c0, c1);
    for (uint64_t j = j0; j < j1; j++) {
      const timeformat::Fields f = stage[j];   // (j < j1 <= k)
      uint32_t lo, hi;
      if (!pack::chunk_part(ob[j], timeformat::row_len(f, L), c0, c1, &lo, &hi)) continue;
      if (hi > L) {
        left_range = true;
        continue;
      }
      const timeformat::Source src = timeformat::unfold(f);
      for (uint32_t i = lo; i < hi; i++) image.put(ob[j] + i - c0, timeformat::char_at(src, timeformat::layout_entry(layout, i)));
    }
    image.store(got);
    left_range |= image.left_range, twice |= image.twice;
  });
  if (chunks < 0 || left_range) return -1;
  // ---- the rows read back (a complete output only)
  if (round_trip && total <= out_cap) {
    timeparse::Program reading{};
    uint32_t bad_at = 0;
    if (timeparse::compile(format, format_len, &reading, &bad_at) != timeparse::kFormatOk) return -3;
    for (uint64_t j = 0; j < k; j++) {
      if (timeformat::class_of(stage[j]) != timeformat::kOk) continue;
      const timeparse::Result res = read_back(out + ob[j], L, reading, unit);
      if (res.status != timeparse::kOk || res.bits != value[idx ? idx[j] : j]) return -3;
      summary[6]++;
    }
  }
  return twice ? -1 : static_cast<long>(total);
}

#ifdef TIME_FORMAT_EXEC_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <string>

namespace {

uint64_t rnd64() {
  static uint64_t rng = 88172645463325252ull;
  rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
  return rng;
}

bool leap(long y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }
int month_days(long y, int m) {
  static const int days[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  return m == 2 && leap(y) ? 29 : days[m - 1];
}
std::string digits(long long v, int width) {
  std::string s(static_cast<size_t>(width), '0');
  for (int i = width - 1; i >= 0; i--, v /= 10) s[static_cast<size_t>(i)] = static_cast<char>('0' + v % 10);
  return s;
}

// the meaning, written out over std::string: the days counted year by year and month by month from 1970
std::string meaning(int64_t value, const std::string& format, int unit, int zone_minutes) {
  const __int128 per = unit == 0 ? 1 : unit == 1 ? 1000 : unit == 2 ? 1000000 : 1000000000;
  __int128 secs = value / per, rest = value % per;
  if (rest < 0) secs -= 1, rest += per;
  secs += static_cast<__int128>(zone_minutes) * 60;
  if (secs < -62135596800ll || secs > 253402300799ll) return std::string();
  long long days = static_cast<long long>(secs / 86400), of_day = static_cast<long long>(secs % 86400);
  if (of_day < 0) days -= 1, of_day += 86400;
  long year = 1970;
  while (days < 0) year--, days += leap(year) ? 366 : 365;
  while (days >= (leap(year) ? 366 : 365)) days -= leap(year) ? 366 : 365, year++;
  int month = 1;
  while (days >= month_days(year, month)) days -= month_days(year, month), month++;
  static const char* names[12] = {"Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"};
  const long long nanos = static_cast<long long>(rest * (1000000000 / per));
  std::string s;
  for (size_t i = 0; i < format.size(); i++) {
    if (format[i] != '%') {
      s += format[i];
      continue;
    }
    const char op = format[++i];
    if (op == 'Y') s += digits(year, 4);
    if (op == 'm') s += digits(month, 2);
    if (op == 'd') s += digits(days + 1, 2);
    if (op == 'H') s += digits(of_day / 3600, 2);
    if (op == 'M') s += digits(of_day / 60 % 60, 2);
    if (op == 'S') s += digits(of_day % 60, 2);
    if (op == 'b') s += names[month - 1];
    if (op == 'f') s += unit == 0 ? std::string("000000") : digits(nanos, 9).substr(0, static_cast<size_t>(3 * unit));
    if (op == 'z') s += std::string(1, zone_minutes < 0 ? '-' : '+') + digits(abs(zone_minutes) / 60, 2) + digits(abs(zone_minutes) % 60, 2);
    if (op == '%') s += '%';
  }
  return s;
}

int64_t random_value(int unit) {
  const int64_t per = unit == 0 ? 1 : unit == 1 ? 1000 : unit == 2 ? 1000000 : 1000000000;
  const uint64_t shape = rnd64() % 8;
  if (shape == 0) return static_cast<int64_t>(rnd64());
  if (shape == 1) return static_cast<int64_t>(rnd64() % 4) - 2 + (rnd64() % 2 ? INT64_MAX - 1 : INT64_MIN + 2);
  const int64_t span = unit == 3 ? 9223372036ll : 253402300799ll + 62135596800ll + 200000;
  const int64_t secs = static_cast<int64_t>(rnd64() % static_cast<uint64_t>(span)) - (unit == 3 ? span / 2 : 62135596800ll + 100000);
  return secs * per + static_cast<int64_t>(rnd64() % static_cast<uint64_t>(per));
}

int one_case(uint64_t n_values, const std::string& format, int unit, int zone_minutes, bool take, bool with_status, uint64_t lead, uint64_t gap, uint64_t chunk,
             uint64_t* ok_rows) {
  std::vector<uint64_t> value, idx;
  std::vector<uint8_t> status;
  for (uint64_t i = 0; i < n_values; i++) {
    value.push_back(static_cast<uint64_t>(random_value(unit)));
    status.push_back(rnd64() % 5 == 0 ? static_cast<uint8_t>(1 + rnd64() % 4) : 0);
  }
  const uint64_t k = take ? n_values + n_values / 2 : n_values;
  if (take)
    for (uint64_t j = 0; j < k; j++) idx.push_back(n_values ? rnd64() % n_values : 0);
  // the expectation
  std::string want(lead, '\n');
  std::vector<uint64_t> wb, we;
  uint64_t counts[3] = {0, 0, 0};
  for (uint64_t j = 0; j < k; j++) {
    const uint64_t r = take ? idx[j] : j;
    std::string row;
    if (with_status && status[r] != 0) {
      counts[1]++;
    } else {
      row = meaning(static_cast<int64_t>(value[r]), format, unit, zone_minutes);
      counts[row.empty() ? 2 : 0]++;
    }
    wb.push_back(want.size());
    want += row;
    we.push_back(want.size());
    want += std::string(gap, '\n');
  }
  // exact allocations: the sanitizer sees any byte or row beyond them
  std::vector<uint8_t> out(want.size()), fmt(format.begin(), format.end());
  std::vector<uint64_t> ob(k), oe(k);
  uint64_t summary[8];
  const long total = tf_format(value.data(), with_status ? status.data() : nullptr, n_values, take ? idx.data() : nullptr, take, idx.size(), fmt.data(), fmt.size(),
                               unit, zone_minutes, 0, '\n', lead, gap, chunk, 0, out.data(), out.size(), ob.data(), oe.data(), summary);
  if (total != static_cast<long>(want.size())) return 1;
  if (!want.empty() && memcmp(out.data(), want.data(), want.size()) != 0) {
    for (uint64_t j = 0; j < k; j++)
      if (std::string(out.begin() + static_cast<long>(wb[j]), out.begin() + static_cast<long>(we[j])) != want.substr(wb[j], we[j] - wb[j])) {
        fprintf(stderr, "time_format_exec: row %llu value %lld: want \"%s\"\n", static_cast<unsigned long long>(j),
                static_cast<long long>(value[take ? idx[j] : j]), want.substr(wb[j], we[j] - wb[j]).c_str());
        break;
      }
    return 2;
  }
  for (uint64_t j = 0; j < k; j++)
    if (ob[j] != wb[j] || oe[j] != we[j]) return 3;
  for (int c = 0; c < 3; c++)
    if (counts[c] != summary[c]) return 4;
  *ok_rows += counts[0];
  return 0;
}

}  // namespace

int main() {
  const std::string formats[7] = {"%Y-%m-%dT%H:%M:%SZ",   "%Y-%m-%dT%H:%M:%S.%f%z",    "%d/%b/%Y:%H:%M:%S %z", "%H:%M", "%Y-%m-%d",
                                  std::string("%%%Y\0%m-%d%%%f9", 15), "%Y-%b-%dT%H:%M:%S.%f%z|abcdefghijklmnopqrstuvwxyz0123456789ABCDE"};
  const int zones[5] = {0, 330, -420, 1439, -1439};
  int cases = 0;
  uint64_t ok_rows = 0;
  for (uint64_t n_values : {0, 1, 65, 300})
    for (const std::string& format : formats)
      for (int unit : {0, 1, 2, 3}) {
        const int zone = zones[cases % 5];
        const uint64_t chunks[4] = {4096, 16, 7, 1};
        const int bad = one_case(n_values, format, unit, zone, cases % 2 != 0, cases % 3 != 0, cases % 4 == 0 ? 17 : 0, static_cast<uint64_t>(cases % 3),
                                 chunks[cases % 4], &ok_rows);
        if (bad) {
          fprintf(stderr, "time_format_exec: case %d (n %llu unit %d zone %d) failed: %d\n", cases, static_cast<unsigned long long>(n_values), unit, zone, bad);
          return 1;
        }
        cases++;
      }
  if (tf_calendar() != 3652059) {
    fprintf(stderr, "time_format_exec: the calendar walk failed\n");
    return 1;
  }
  if (ok_rows < 5000) {
    fprintf(stderr, "time_format_exec: only %llu OK rows: the generator does not exercise the value\n", static_cast<unsigned long long>(ok_rows));
    return 1;
  }
  printf("time_format_exec: %d cases, %llu OK rows, the calendar of 3652059 days\n", cases, static_cast<unsigned long long>(ok_rows));
  return 0;
}
#endif
