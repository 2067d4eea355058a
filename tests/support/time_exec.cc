// tests/support/time_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_time.h, compiled with g++
// (tests/test_record_time.py).  It walks the call the way record_time.hip's kernels do: the format compiled first (a refused
// format writes nothing), then the pack's checks of every row (the first bad row wins; a refused call writes nothing), then
// every row in the 16-byte groups of rows::load_group over a text whose every access is checked against its range, through
// timeparse::step, and timeparse::finish for the value and the status; every output row may be written only once.  With
// `splits` every row (of at most kSplitBytes bytes) is ALSO fed again
//     in steps of c bytes, for every c in 1..16                                      (16 feeds)
//     as a row that begins at alignment a would be cut by aligned blocks: a first step of 16 - a bytes, then steps of 16,
//       for every a in 0..15                                                         (16 feeds)
//     at every split of its bytes into two runs of groups, [0, p) and [p, len)       (len - 1 feeds)
// and must give the same answer every time: the result does not depend on where a row is cut.
//
// With -DTIME_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): seeded
// random rows under six formats against the meaning written out over std::string, with a calendar that counts the days year
// by year, exact allocations.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_rows.h"
#include "../../rejit_amd/csrc/record_time.h"
#include "checked_text.h"

using namespace rejit_amd;

namespace {

constexpr uint64_t kSplitBytes = 600;

struct Code {
  uint8_t bytes[timeparse::kMaxFormat];
  uint32_t len;
};
Code code_of(const timeparse::Program& p) {
  Code c;
  for (uint32_t i = 0; i < timeparse::kMaxFormat; i++) c.bytes[i] = static_cast<uint8_t>(timeparse::program_byte(p, i));
  c.len = p.len;
  return c;
}

// the bytes [a, b) of the row at rb in steps of `chunk` bytes, the first one of `first`
void feed(timeparse::State& s, const Code& code, const CheckedText& T, uint64_t rb, uint64_t a, uint64_t b, uint64_t first, uint64_t chunk, uint64_t* steps) {
  uint64_t size = first;
  for (uint64_t at = a; at < b && !timeparse::done(s); at += size, size = chunk) {
    if (size > b - at) size = b - at;
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < size; i++) w[i >> 2] |= T.at(rb + at + i) << (8 * (i & 3));
    timeparse::step(s, code.bytes, code.len, w, static_cast<uint32_t>(size));
    ++*steps;
  }
}

}  // namespace

extern "C" int te_known(int unit, unsigned flags) { return (timeparse::unit_known(unit) ? 1 : 0) | (timeparse::flags_known(flags) ? 2 : 0); }
extern "C" int te_state_size(void) { return static_cast<int>(sizeof(timeparse::State)); }

// -> the FormatError; *at: the offset it names; code[0, 64) and *len: the program
extern "C" int te_compile(const uint8_t* format, uint64_t format_len, uint8_t* code, uint32_t* len, uint32_t* at) {
  timeparse::Program p{};
  const int e = timeparse::compile(format, format_len, &p, at);
  if (e != timeparse::kFormatOk) return e;
  const Code c = code_of(p);
  memcpy(code, c.bytes, timeparse::kMaxFormat);
  *len = c.len;
  return 0;
}

// summary: [0..4] the rows per status, [5] the first bad row (~0: none), [6] the extra feeds made, [7] the step calls.
// Returns 0; -1 when an access left its range or an output row was written twice; -2 for arguments the call refuses up
// front (the format included); -3 when another feed gave another answer than the row's groups.
extern "C" long te_parse(const uint8_t* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records, const uint64_t* indices,
                         int have_indices, uint64_t n_indices, const uint8_t* format, uint64_t format_len, int unit, unsigned flags, int splits,
                         uint64_t* out_value, uint8_t* out_status, uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[5] = ~0ull;
  const uint64_t k = have_indices ? n_indices : n_records;
  timeparse::Program program{};
  uint32_t bad_at = 0;
  if (timeparse::compile(format, format_len, &program, &bad_at) != timeparse::kFormatOk) return -2;
  if (!timeparse::unit_known(unit) || !timeparse::flags_known(flags) || !rows::rows_fit(k)) return -2;
  const Code code = code_of(program);
  const uint64_t* idx = have_indices ? indices : nullptr;
  // ---- the check pass: the tables only
  for (uint64_t j = 0; j < k; j++)
    if (rows::resolve(rec_begin, rec_end, idx, n_records, n, j).bad) {
      summary[5] = j;
      return 0;   // a refused call: the kernel returns at once
    }
  // ---- the walk
  const CheckedText T{text, n};
  std::vector<uint8_t> once(k, 0);
  for (uint64_t j = 0; j < k; j++) {
    const rows::Row row = rows::resolve(rec_begin, rec_end, idx, n_records, n, j);
    const uint64_t len = row.len(), groups = rows::n_groups(len);
    timeparse::State s = timeparse::start(flags);
    for (uint64_t g = 0; g < groups && !timeparse::done(s); g++) {
      uint32_t w[4];
      rows::load_group(T, n, row.rb, len, g, w);
      const uint64_t left = len - g * rows::kGroupBytes;
      timeparse::step(s, code.bytes, code.len, w, static_cast<uint32_t>(left < rows::kGroupBytes ? left : rows::kGroupBytes));
      summary[7]++;
    }
    const timeparse::Result res = timeparse::finish(s, code.len, unit);
    if (res.status >= timeparse::kStatuses || (res.status != timeparse::kOk && res.bits != 0)) return -3;
    if (splits && len <= kSplitBytes) {
      // (feed 0..15: steps of c = feed + 1; 16..31: alignment a = feed - 16; then the two-run splits)
      for (uint64_t f = 0; f < 32 + (len ? len - 1 : 0); f++) {
        timeparse::State t = timeparse::start(flags);
        if (f < 16) {
          feed(t, code, T, row.rb, 0, len, f + 1, f + 1, &summary[7]);
        } else if (f < 32) {
          feed(t, code, T, row.rb, 0, len, 16 - (f - 16), 16, &summary[7]);
        } else {
          const uint64_t p = f - 31;
          feed(t, code, T, row.rb, 0, p, 16, 16, &summary[7]);
          feed(t, code, T, row.rb, p, len, 16, 16, &summary[7]);
        }
        const timeparse::Result again = timeparse::finish(t, code.len, unit);
        summary[6]++;
        if (again.status != res.status || again.bits != res.bits) return -3;
      }
    }
    if (once[j]) return -1;
    once[j] = 1;
    out_value[j] = res.bits;
    if (out_status) out_status[j] = static_cast<uint8_t>(res.status);
    summary[res.status]++;
  }
  return T.left_range ? -1 : 0;
}

#ifdef TIME_EXEC_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <string>

namespace {

uint64_t rnd(uint64_t below) {
  static uint64_t rng = 88172645463325252ull;
  rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
  return rng % below;
}

struct Want {
  uint32_t status;
  uint64_t bits;
};

bool is_digit(char c) { return c >= '0' && c <= '9'; }
bool leap(long y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }
int month_days(long y, int m) {
  static const int days[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  return m == 2 && leap(y) ? 29 : days[m - 1];
}
// days since 1970-01-01, counted year by year and month by month
long long days_since_epoch(long y, int m, int d) {
  long long days = 0;
  for (long a = 1970; a < y; a++) days += leap(a) ? 366 : 365;
  for (long a = y; a < 1970; a++) days -= leap(a) ? 366 : 365;
  for (int b = 1; b < m; b++) days += month_days(y, b);
  return days + d - 1;
}
bool digits(const std::string& s, size_t& at, int count, long* out) {
  long v = 0;
  for (int i = 0; i < count; i++) {
    if (at >= s.size() || !is_digit(s[at])) return false;
    v = v * 10 + (s[at++] - '0');
  }
  *out = v;
  return true;
}

// the meaning, written out over the whole string
Want meaning(std::string s, const std::string& format, int unit, bool trim) {
  if (trim) {
    while (!s.empty() && (s.back() == ' ' || s.back() == '\t')) s.pop_back();
    size_t lead = 0;
    while (lead < s.size() && (s[lead] == ' ' || s[lead] == '\t')) lead++;
    s = s.substr(lead);
  }
  if (s.empty()) return {timeparse::kEmpty, 0};
  long year = 0, month = 0, day = 0, hour = 0, minute = 0, second = 0, off_h = 0, off_m = 0, off_sign = 1;
  std::string fraction;
  size_t at = 0;
  const Want bad{timeparse::kMalformed, 0};
  for (size_t i = 0; i < format.size(); i++) {
    if (format[i] != '%') {
      if (at >= s.size() || s[at] != format[i]) return bad;
      at++;
      continue;
    }
    const char op = format[++i];
    if (op == 'Y' && !digits(s, at, 4, &year)) return bad;
    if (op == 'm' && !digits(s, at, 2, &month)) return bad;
    if (op == 'd' && !digits(s, at, 2, &day)) return bad;
    if (op == 'H' && !digits(s, at, 2, &hour)) return bad;
    if (op == 'M' && !digits(s, at, 2, &minute)) return bad;
    if (op == 'S' && !digits(s, at, 2, &second)) return bad;
    if (op == '%') {
      if (at >= s.size() || s[at] != '%') return bad;
      at++;
    }
    if (op == 'f') {
      while (at < s.size() && is_digit(s[at]) && fraction.size() < 9) fraction += s[at++];
      if (fraction.empty()) return bad;
    }
    if (op == 'b') {
      static const char* names[12] = {"jan", "feb", "mar", "apr", "may", "jun", "jul", "aug", "sep", "oct", "nov", "dec"};
      if (at + 3 > s.size()) return bad;
      std::string low;
      for (int j = 0; j < 3; j++) {
        const char c = s[at + j];
        low += (c >= 'A' && c <= 'Z') ? static_cast<char>(c + 32) : c;
      }
      for (int j = 0; j < 12; j++)
        if (low == names[j]) month = j + 1;
      if (month == 0) return bad;
      at += 3;
    }
    if (op == 'z') {
      if (at < s.size() && s[at] == 'Z') {
        at++;
      } else {
        if (at >= s.size() || (s[at] != '+' && s[at] != '-')) return bad;
        off_sign = s[at++] == '-' ? -1 : 1;
        if (!digits(s, at, 2, &off_h)) return bad;
        if (at < s.size() && s[at] == ':') at++;
        if (!digits(s, at, 2, &off_m)) return bad;
      }
    }
  }
  if (at != s.size()) return bad;
  if (year == 0 || month < 1 || month > 12 || day < 1 || day > month_days(year, static_cast<int>(month)) || hour > 23 || minute > 59 || second > 59 ||
      off_h > 23 || off_m > 59)
    return {timeparse::kRange, 0};
  const long long secs = days_since_epoch(year, static_cast<int>(month), static_cast<int>(day)) * 86400 + hour * 3600 + minute * 60 + second -
                         off_sign * (off_h * 3600 + off_m * 60);
  while (!fraction.empty() && fraction.size() < 9) fraction += '0';
  const long long nanos = fraction.empty() ? 0 : atoll(fraction.c_str());
  const __int128 total = static_cast<__int128>(secs) * 1000000000 + nanos;
  const __int128 lowest = -(static_cast<__int128>(1) << 63), highest = (static_cast<__int128>(1) << 63) - 1;
  if (unit == timeparse::kNano && (total < lowest || total > highest)) return {timeparse::kRange, 0};
  const long long below = unit == 0 ? 1000000000 : unit == 1 ? 1000000 : unit == 2 ? 1000 : 1;
  if (nanos % below != 0) return {timeparse::kInexact, 0};
  const __int128 value = static_cast<__int128>(secs) * (1000000000 / below) + nanos / below;
  return {timeparse::kOk, static_cast<uint64_t>(value)};
}

std::string two(uint64_t v) { return std::string(1, static_cast<char>('0' + v / 10 % 10)) + static_cast<char>('0' + v % 10); }

// a row that fits the format, mostly
std::string random_row(const std::string& format) {
  static const char* names[14] = {"Jan", "FEB", "mar", "Apr", "mAy", "Jun", "JUL", "aug", "Sep", "Oct", "nOV", "Dec", "xyz", "J n"};
  static const char kAny[] = "0123456789+-:.TZz/ \t\0x%";
  std::string s;
  if (rnd(16) == 0) {
    for (uint64_t i = rnd(30); i > 0; i--) s += kAny[rnd(sizeof(kAny) - 1)];
    return s;
  }
  if (rnd(5) == 0) s += std::string(rnd(3), rnd(2) ? ' ' : '\t');
  for (size_t i = 0; i < format.size(); i++) {
    if (format[i] != '%') {
      s += format[i];
      continue;
    }
    const char op = format[++i];
    const bool wild = rnd(12) == 0;
    if (op == 'Y') {
      const uint64_t y = rnd(8) == 0 ? rnd(10000) : rnd(4) == 0 ? 1600 + rnd(700) : 1960 + rnd(80);
      s += two(y / 100) + two(y % 100);
    }
    if (op == 'm') s += two(wild ? rnd(15) : 1 + rnd(12));
    if (op == 'd') s += two(wild ? rnd(34) : 1 + rnd(rnd(3) ? 28 : 31));
    if (op == 'H') s += two(wild ? rnd(26) : rnd(24));
    if (op == 'M') s += two(wild ? rnd(62) : rnd(60));
    if (op == 'S') s += two(wild ? rnd(62) : rnd(60));
    if (op == '%') s += '%';
    if (op == 'b') s += names[wild ? rnd(14) : rnd(12)];
    if (op == 'f')
      for (uint64_t c = wild ? rnd(12) : 1 + rnd(9); c > 0; c--) s += static_cast<char>('0' + (rnd(3) ? 0 : rnd(10)));
    if (op == 'z') {
      const uint64_t shape = rnd(6);
      if (shape == 0) s += wild ? 'z' : 'Z';
      else s += std::string(1, rnd(2) ? '+' : '-') + two(wild ? rnd(30) : rnd(24)) + (shape & 1 ? ":" : "") + two(wild ? rnd(70) : rnd(60)) + (rnd(20) ? "" : ":30");
    }
  }
  if (rnd(5) == 0) s += std::string(rnd(3), ' ');
  if (rnd(10) == 0 && !s.empty()) s[rnd(s.size())] = kAny[rnd(sizeof(kAny) - 1)];
  if (rnd(14) == 0 && !s.empty()) s = s.substr(0, rnd(s.size()));
  if (rnd(20) == 0) s += kAny[rnd(sizeof(kAny) - 1)];
  return s;
}

int one_case(uint64_t k, const std::string& format, int unit, bool trim, bool take, bool with_status, uint64_t* ok_rows) {
  std::vector<uint8_t> text;
  std::vector<uint64_t> rb, re, idx;
  std::vector<std::string> strings;
  const uint64_t n_records = take ? k / 2 + 1 : k;
  for (uint64_t i = 0; i < n_records; i++) {
    const std::string s = random_row(format);
    for (uint64_t p = rnd(4); p > 0; p--) text.push_back('|');
    rb.push_back(text.size());
    text.insert(text.end(), s.begin(), s.end());
    re.push_back(text.size());
    strings.push_back(s);
  }
  if (take)
    for (uint64_t i = 0; i < k; i++) idx.push_back(rnd(n_records));
  // exact allocations: the sanitizer sees any byte or row beyond them
  std::vector<uint64_t> value(k);
  std::vector<uint8_t> status(k);
  std::vector<uint8_t> fmt(format.begin(), format.end());
  uint64_t summary[8];
  const long rc = te_parse(text.data(), text.size(), rb.data(), re.data(), n_records, take ? idx.data() : nullptr, take, idx.size(), fmt.data(), fmt.size(), unit,
                           trim ? 1u : 0u, 1, value.data(), with_status ? status.data() : nullptr, summary);
  if (rc != 0 || summary[5] != ~0ull) return 1;
  uint64_t counts[5] = {0, 0, 0, 0, 0};
  for (uint64_t j = 0; j < k; j++) {
    const std::string& row = strings[take ? idx[j] : j];
    const Want w = meaning(row, format, unit, trim);
    if (value[j] != w.bits || (with_status && status[j] != w.status)) {
      fprintf(stderr, "time_exec: row %llu \"%s\": want status %u value %lld, got status %u value %lld\n", static_cast<unsigned long long>(j), row.c_str(),
              w.status, static_cast<long long>(w.bits), with_status ? status[j] : 255u, static_cast<long long>(value[j]));
      return 2;
    }
    counts[w.status]++;
  }
  for (int c = 0; c < 5; c++)
    if (counts[c] != summary[c]) return 3;
  *ok_rows += counts[0];
  return 0;
}

}  // namespace

int main() {
  const std::string formats[6] = {"%Y-%m-%dT%H:%M:%S%z", "%Y-%m-%dT%H:%M:%S.%f%z", "%d/%b/%Y:%H:%M:%S %z", "%Y/%m/%d %H:%M:%S", "%Y-%m-%d",
                                  std::string("%%%Y\0%m-%d%%", 12)};
  int cases = 0;
  uint64_t ok_rows = 0;
  for (uint64_t k : {0, 1, 65, 400})
    for (const std::string& format : formats)
      for (int unit : {0, 1, 2, 3})
        for (int trim : {0, 1}) {
          const int take = cases % 2;
          const int bad = one_case(k, format, unit, trim != 0, take != 0, cases % 3 != 0, &ok_rows);
          if (bad) {
            fprintf(stderr, "time_exec: case %d (k %llu unit %d trim %d take %d) failed: %d\n", cases, static_cast<unsigned long long>(k), unit, trim, take, bad);
            return 1;
          }
          cases++;
        }
  if (ok_rows < 1000) {
    fprintf(stderr, "time_exec: only %llu OK rows: the generator does not exercise the value\n", static_cast<unsigned long long>(ok_rows));
    return 1;
  }
  printf("time_exec: %d cases, %llu OK rows, state %d bytes\n", cases, static_cast<unsigned long long>(ok_rows), te_state_size());
  return 0;
}
#endif
