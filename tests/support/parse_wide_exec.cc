// tests/support/parse_wide_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_parse.h under RJ_PARSE_WIDE, compiled with g++
// (tests/test_record_parse_wide.py).  parse_exec.cc's discipline with the whole flags word handed through: first the pack's
// checks of every row (the first bad row wins; a refused call writes nothing), then every row in the 16-byte groups of
// rows::load_group over a text whose every access is checked against its range, through numparse::step, and numparse::finish
// for the value and the status; every output row may be written only once.  With `splits` every row (of at most kSplitBytes
// bytes) is ALSO fed again at every split of its bytes into two runs of groups and must give the same answer: saturation and
// the count of dropped digits do not depend on where a row's groups are cut.
//
// With -DPARSE_WIDE_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): a fixed
// set of rows -- the range and subnormal edges, the old window's edges, long mantissas, seeded digits of 1 to 40 places --
// against the meaning written out over std::string with strtod (of the whole row, or of the two ends of the bracket), exact
// allocations.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_parse.h"
#include "../../rejit_amd/csrc/record_rows.h"
#include "checked_text.h"

using namespace rejit_amd;

namespace {

constexpr uint64_t kSplitBytes = 1100;

// the bytes [a, b) of the row at rb, cut into groups from a on
void feed(numparse::State& s, const CheckedText& T, uint64_t rb, uint64_t a, uint64_t b, uint64_t* steps) {
  for (uint64_t at = a; at < b && !numparse::done(s); at += rows::kGroupBytes) {
    const uint32_t valid = static_cast<uint32_t>(b - at < rows::kGroupBytes ? b - at : rows::kGroupBytes);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < valid; i++) w[i >> 2] |= T.at(rb + at + i) << (8 * (i & 3));
    numparse::step(s, w, valid);
    ++*steps;
  }
}

}  // namespace

extern "C" int pwe_known(int kind, unsigned flags) { return (numparse::kind_known(kind) ? 1 : 0) | (numparse::flags_known(flags) ? 2 : 0); }

// the two 64-bit words of the power table's entry for 10^q
extern "C" int pwe_table(uint64_t* out, int room) {
  if (room < 2 * numparse::kPow5Entries) return -1;
  for (int i = 0; i < 2 * numparse::kPow5Entries; i++) out[i] = numparse::kPow5[i];
  return numparse::kPow5Entries;
}

extern "C" uint64_t pwe_state_bytes() { return sizeof(numparse::State); }

// summary: [0..4] the rows per status, [5] the first bad row (~0: none), [6] the split feeds made, [7] the step calls.
// Returns 0; -1 when an access left its range or an output row was written twice; -2 for arguments the call refuses up
// front; -3 when a split feed gave another answer than the row's groups.
extern "C" long pwe_parse(const uint8_t* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records, const uint64_t* indices,
                          int have_indices, uint64_t n_indices, int kind, unsigned flags, int splits, uint64_t* out_value, uint8_t* out_status,
                          uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[5] = ~0ull;
  const uint64_t k = have_indices ? n_indices : n_records;
  if (!numparse::kind_known(kind) || !numparse::flags_known(flags) || !rows::rows_fit(k)) return -2;
  const uint64_t* idx = have_indices ? indices : nullptr;
  // ---- the check pass: the tables only
  for (uint64_t j = 0; j < k; j++)
    if (rows::resolve(rec_begin, rec_end, idx, n_records, n, j).bad) {
      summary[5] = j;
      return 0;   // a refused call: the parse kernel returns at once
    }
  // ---- the parse pass
  const CheckedText T{text, n};
  std::vector<uint8_t> once(k, 0);
  for (uint64_t j = 0; j < k; j++) {
    const rows::Row row = rows::resolve(rec_begin, rec_end, idx, n_records, n, j);
    const uint64_t len = row.len(), groups = rows::n_groups(len);
    numparse::State s = numparse::start(kind, flags);
    for (uint64_t g = 0; g < groups && !numparse::done(s); g++) {
      uint32_t w[4];
      rows::load_group(T, n, row.rb, len, g, w);
      const uint64_t left = len - g * rows::kGroupBytes;
      numparse::step(s, w, static_cast<uint32_t>(left < rows::kGroupBytes ? left : rows::kGroupBytes));
      summary[7]++;
    }
    const numparse::Result res = numparse::finish(s, kind);
    if (res.status >= numparse::kStatuses || (res.status != numparse::kOk && res.bits != 0)) return -3;
    if (splits && len <= kSplitBytes)
      for (uint64_t p = 1; p < len; p++) {
        numparse::State t = numparse::start(kind, flags);
        feed(t, T, row.rb, 0, p, &summary[7]);
        feed(t, T, row.rb, p, len, &summary[7]);
        const numparse::Result again = numparse::finish(t, kind);
        summary[6]++;
        if (again.status != res.status || again.bits != res.bits) return -3;
      }
    if (once[j]) return -1;
    once[j] = 1;
    out_value[j] = res.bits;
    if (out_status) out_status[j] = static_cast<uint8_t>(res.status);
    summary[res.status]++;
  }
  return T.left_range ? -1 : 0;
}

#ifdef PARSE_WIDE_EXEC_MAIN
#include <math.h>
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

// strtod's bits of the magnitude; kInfBits when infinite
uint64_t magnitude(const std::string& s) {
  const double v = fabs(strtod(s.c_str(), nullptr));
  uint64_t bits;
  memcpy(&bits, &v, 8);
  return bits;
}

// the meaning of a FLOAT64 row under WIDE, written out over the string: the grammar by hand, the digits in 128 bits, the doubles
// by strtod -- of the whole row when its digits fit 64 bits, of the two ends of the bracket otherwise
Want meaning(std::string s, bool trim) {
  if (trim) {
    while (!s.empty() && (s.back() == ' ' || s.back() == '\t')) s.pop_back();
    size_t lead = 0;
    while (lead < s.size() && (s[lead] == ' ' || s[lead] == '\t')) lead++;
    s = s.substr(lead);
  }
  if (s.empty()) return {numparse::kEmpty, 0};
  size_t at = 0;
  bool neg = false;
  if (s[at] == '+' || s[at] == '-') neg = s[at++] == '-';
  std::string digits;
  while (at < s.size() && is_digit(s[at])) digits += s[at++];
  const size_t n_int = digits.size();
  size_t n_frac = 0;
  long long exp10 = 0;
  if (at < s.size() && s[at] == '.') {
    at++;
    while (at < s.size() && is_digit(s[at])) digits += s[at++], n_frac++;
  }
  if (n_int + n_frac == 0) return {numparse::kMalformed, 0};
  if (at < s.size() && (s[at] == 'e' || s[at] == 'E')) {
    at++;
    bool eneg = false;
    if (at < s.size() && (s[at] == '+' || s[at] == '-')) eneg = s[at++] == '-';
    if (at >= s.size() || !is_digit(s[at])) return {numparse::kMalformed, 0};
    while (at < s.size() && is_digit(s[at])) {
      if (exp10 < 1000000000000ll) exp10 = exp10 * 10 + (s[at] - '0');
      at++;
    }
    if (eneg) exp10 = -exp10;
  }
  if (at != s.size()) return {numparse::kMalformed, 0};
  size_t lead = 0;
  while (lead < digits.size() && digits[lead] == '0') lead++;
  digits = digits.substr(lead);
  long long q = exp10 - static_cast<long long>(n_frac);
  while (!digits.empty() && digits.back() == '0') digits.pop_back(), q++;
  const uint64_t sign = neg ? 1ull << 63 : 0;
  if (digits.empty()) return {numparse::kOk, sign};
  const unsigned __int128 most = ~0ull;
  auto value_of = [](const std::string& d) {
    unsigned __int128 v = 0;
    for (char c : d) v = v * 10 + static_cast<unsigned>(c - '0');
    return v;
  };
  if (digits.size() <= 20 && value_of(digits) <= most) {   // decided
    const uint64_t bits = magnitude(s);
    if (bits == numparse::kInfBits) return {numparse::kRange, 0};
    return {numparse::kOk, bits | sign};
  }
  std::string prefix = digits.substr(0, 20);
  if (value_of(prefix) > most) prefix.pop_back();
  const uint64_t p = static_cast<uint64_t>(value_of(prefix));
  if (p == ~0ull) return {numparse::kInexact, 0};
  const long long at10 = q + static_cast<long long>(digits.size() - prefix.size());
  char end[64];
  snprintf(end, sizeof(end), "%llue%lld", static_cast<unsigned long long>(p), at10);
  const uint64_t low = magnitude(end);
  snprintf(end, sizeof(end), "%llue%lld", static_cast<unsigned long long>(p + 1), at10);
  const uint64_t high = magnitude(end);
  if (low != high) return {numparse::kInexact, 0};
  if (low == numparse::kInfBits) return {numparse::kRange, 0};
  if (low != magnitude(s)) abort();   // (rounding is monotone)
  return {numparse::kOk, low | sign};
}

std::string random_digits(uint64_t places) {
  std::string s(1, static_cast<char>('1' + rnd(9)));
  while (s.size() < places) s += static_cast<char>('0' + rnd(10));
  return s;
}

std::string random_row(int family) {
  std::string s;
  if (rnd(4) == 0) s += rnd(2) ? '-' : '+';
  s += std::string(rnd(4) == 0 ? rnd(20) : 0, '0');
  const uint64_t places = family == 0 ? 17 : family == 1 ? 1 + rnd(19) : 20 + rnd(21);
  std::string digits = random_digits(places);
  const long long q = static_cast<long long>(rnd(655)) - 345;
  if (rnd(2)) {
    const uint64_t at = rnd(digits.size() + 1);
    s += digits.substr(0, at) + "." + digits.substr(at);
    s += (rnd(2) ? "e" : "E") + std::to_string(q + static_cast<long long>(digits.size() - at));
  } else {
    s += digits + std::string(rnd(3) == 0 ? rnd(25) : 0, '0') + "e" + std::to_string(q);
  }
  if (rnd(8) == 0) s += " ";
  return s;
}

// the rows laid into one text, parsed with splits under `flags`, against the meaning -> the rows checked, or -1
int check_rows(const std::vector<std::string>& strings, unsigned flags, bool with_status) {
  std::vector<uint8_t> text;
  std::vector<uint64_t> rb, re;
  for (const std::string& s : strings) {
    for (uint64_t p = rnd(4); p > 0; p--) text.push_back('|');
    rb.push_back(text.size());
    text.insert(text.end(), s.begin(), s.end());
    re.push_back(text.size());
  }
  const uint64_t k = strings.size();
  // exact allocations: the sanitizer sees any byte or row beyond them
  std::vector<uint64_t> value(k);
  std::vector<uint8_t> status(k);
  uint64_t summary[8];
  const long rc = pwe_parse(text.data(), text.size(), rb.data(), re.data(), k, nullptr, 0, 0, numparse::kFloat64, flags, 1, value.data(),
                            with_status ? status.data() : nullptr, summary);
  if (rc != 0 || summary[5] != ~0ull) {
    fprintf(stderr, "parse_wide_exec: rc %ld\n", rc);
    return -1;
  }
  uint64_t counts[5] = {0, 0, 0, 0, 0};
  for (uint64_t j = 0; j < k; j++) {
    const Want w = meaning(strings[j], (flags & numparse::kTrimFlag) != 0);
    if (value[j] != w.bits || (with_status && status[j] != w.status)) {
      fprintf(stderr, "parse_wide_exec: row %llu (%.60s): want status %u bits %llx, got status %u bits %llx\n", static_cast<unsigned long long>(j),
              strings[j].c_str(), w.status, static_cast<unsigned long long>(w.bits), with_status ? status[j] : 255u,
              static_cast<unsigned long long>(value[j]));
      return -1;
    }
    counts[w.status]++;
  }
  for (int c = 0; c < 5; c++)
    if (counts[c] != summary[c]) return -1;
  return static_cast<int>(k);
}

}  // namespace

int main() {
  const std::vector<std::string> named = {
      "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "1e308", "1e309", "1e999999999999999999999",
      "2.2250738585072014e-308", "2.2250738585072011e-308", "4.9406564584124654e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
      "1e-400", "-1e-400", "5e-324", "2e-324", "3e-324", "1e23", "0.1e-22", "9007199254740993", "0.30000000000000004", "9007199254740991e-23",
      "9007199254740992e23", "9007199254740993e22", "0.1000000000000000055511151231257827021181583404541015625", "10000000000000000005",
      "18446744073709551615", "18446744073709551616", "184467440737095516155", "9007199254740993.00000000000000000001", "", " ", "x", "1e", " 1.5 ",
      "-0", "0e999", "1" + std::string(30, '0') + "1", "1" + std::string(700, '0') + "1e-650", std::string(40, '0') + "." + std::string(40, '0') + "25"};
  int cases = 0;
  for (unsigned flags : {numparse::kWideFlag, numparse::kWideFlag | numparse::kTrimFlag}) {
    std::vector<std::vector<std::string>> sets = {named};
    for (int family = 0; family < 3; family++) {
      std::vector<std::string> rows;
      for (int i = 0; i < 400; i++) rows.push_back(random_row(family));
      sets.push_back(rows);
    }
    for (size_t i = 0; i < sets.size(); i++) {
      const int checked = check_rows(sets[i], flags, (i + flags) % 3 != 0);
      if (checked < 0) {
        fprintf(stderr, "parse_wide_exec: set %zu under flags %u failed\n", i, flags);
        return 1;
      }
      cases += checked;
    }
  }
  if (numparse::kPow5Entries != 651 || sizeof(numparse::State) != 40) return 1;
  printf("parse_wide_exec: %d cases\n", cases);
  return 0;
}
#endif
