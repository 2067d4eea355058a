// tests/support/parse_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_parse.h, compiled with g++
// (tests/test_record_parse.py).  It walks the call the way record_parse.hip's kernels do: first the pack's checks of every
// row (the first bad row wins; a refused call writes nothing), then every row in the 16-byte groups of rows::load_group over a
// text whose every access is checked against its range, through numparse::step, and numparse::finish for the value and the status;
// every output row may be written only once.  With `splits` every row (of at most kSplitBytes bytes) is ALSO fed again at every
// split of its bytes into two runs of groups -- [0, p) and [p, len), each cut into groups of its own -- and must give the same
// answer: the result does not depend on where a row's groups are cut.
//
// With -DPARSE_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): seeded
// random rows against the meaning written out over std::string with strtod, exact allocations.
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

extern "C" int pe_known(int kind, unsigned flags) { return (numparse::kind_known(kind) ? 1 : 0) | (numparse::flags_known(flags) ? 2 : 0); }

// summary: [0..4] the rows per status, [5] the first bad row (~0: none), [6] the split feeds made, [7] the step calls.
// Returns 0; -1 when an access left its range or an output row was written twice; -2 for arguments the call refuses up
// front; -3 when a split feed gave another answer than the row's groups.
extern "C" long pe_parse(const uint8_t* text, uint64_t n, const uint64_t* rec_begin, const uint64_t* rec_end, uint64_t n_records, const uint64_t* indices,
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

#ifdef PARSE_EXEC_MAIN
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

// the meaning, written out over the string: the grammar by hand, the integers in 128 bits, the doubles by strtod
Want meaning(std::string s, int kind, bool trim) {
  if (trim) {
    while (!s.empty() && (s.back() == ' ' || s.back() == '\t')) s.pop_back();
    size_t lead = 0;
    while (lead < s.size() && (s[lead] == ' ' || s[lead] == '\t')) lead++;
    s = s.substr(lead);
  }
  if (s.empty()) return {numparse::kEmpty, 0};
  size_t at = 0;
  bool neg = false;
  if (s[at] == '+' || s[at] == '-') {
    neg = s[at] == '-';
    if (neg && kind == numparse::kUint64) return {numparse::kMalformed, 0};
    at++;
  }
  std::string digits;
  while (at < s.size() && is_digit(s[at])) digits += s[at++];
  const size_t n_int = digits.size();
  size_t n_frac = 0;
  long long exp10 = 0;
  if (kind == numparse::kFloat64) {
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
  } else if (n_int == 0) {
    return {numparse::kMalformed, 0};
  }
  if (at != s.size()) return {numparse::kMalformed, 0};
  size_t lead = 0;
  while (lead < digits.size() && digits[lead] == '0') lead++;
  digits = digits.substr(lead);
  if (kind != numparse::kFloat64) {
    if (digits.size() > 20) return {numparse::kRange, 0};
    unsigned __int128 v = 0;
    for (char c : digits) v = v * 10 + static_cast<unsigned>(c - '0');
    const unsigned __int128 most = kind == numparse::kUint64 ? ~0ull : neg ? (1ull << 63) : (1ull << 63) - 1;
    if (v > most) return {numparse::kRange, 0};
    const uint64_t mag = static_cast<uint64_t>(v);
    return {numparse::kOk, neg ? 0 - mag : mag};
  }
  long long q = exp10 - static_cast<long long>(n_frac);
  while (!digits.empty() && digits.back() == '0') digits.pop_back(), q++;
  if (digits.empty()) return {numparse::kOk, neg ? 1ull << 63 : 0};
  if (digits.size() > 16 || q < -22 || q > 22) return {numparse::kInexact, 0};
  uint64_t m = 0;
  for (char c : digits) m = m * 10 + static_cast<uint64_t>(c - '0');
  if (m > (1ull << 53)) return {numparse::kInexact, 0};
  const double v = strtod(s.c_str(), nullptr);   // (s is in the grammar: no NUL inside, nothing strtod reads otherwise)
  uint64_t bits;
  memcpy(&bits, &v, 8);
  return {numparse::kOk, bits};
}

std::string random_row() {
  static const char kAny[] = "0123456789+-.eE \t\0x_,";
  std::string s;
  const uint64_t shape = rnd(8);
  if (shape == 0) {   // anything
    for (uint64_t i = rnd(24); i > 0; i--) s += kAny[rnd(sizeof(kAny) - 1)];
    return s;
  }
  if (rnd(4) == 0) s += std::string(rnd(3), rnd(2) ? ' ' : '\t');
  if (rnd(3) == 0) s += rnd(2) ? '-' : '+';
  s += std::string(rnd(4) == 0 ? rnd(40) : 0, '0');
  for (uint64_t i = rnd(shape < 4 ? 8 : 22); i > 0; i--) s += static_cast<char>('0' + rnd(10));
  if (shape >= 5) {
    if (rnd(3)) {
      s += '.';
      for (uint64_t i = rnd(8); i > 0; i--) s += static_cast<char>('0' + rnd(10));
      s += std::string(rnd(3) == 0 ? rnd(20) : 0, '0');
    }
    if (rnd(3) == 0) {
      s += rnd(2) ? 'e' : 'E';
      if (rnd(2)) s += rnd(2) ? '-' : '+';
      for (uint64_t i = rnd(4) ? 1 + rnd(2) : rnd(30); i > 0; i--) s += static_cast<char>('0' + rnd(10));
    }
  }
  if (rnd(4) == 0) s += std::string(rnd(3), ' ');
  if (rnd(16) == 0 && !s.empty()) s[rnd(s.size())] = kAny[rnd(sizeof(kAny) - 1)];
  return s;
}

int one_case(uint64_t k, int kind, bool trim, bool take, bool with_status) {
  std::vector<uint8_t> text;
  std::vector<uint64_t> rb, re, idx;
  std::vector<std::string> strings;
  const uint64_t n_records = take ? k / 2 + 1 : k;
  for (uint64_t i = 0; i < n_records; i++) {
    const std::string s = random_row();
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
  uint64_t summary[8];
  const long rc = pe_parse(text.data(), text.size(), rb.data(), re.data(), n_records, take ? idx.data() : nullptr, take, idx.size(), kind, trim ? 1u : 0u, 1,
                           value.data(), with_status ? status.data() : nullptr, summary);
  if (rc != 0 || summary[5] != ~0ull) return 1;
  uint64_t counts[5] = {0, 0, 0, 0, 0};
  for (uint64_t j = 0; j < k; j++) {
    const Want w = meaning(strings[take ? idx[j] : j], kind, trim);
    if (value[j] != w.bits || (with_status && status[j] != w.status)) {
      fprintf(stderr, "parse_exec: row %llu: want status %u bits %llx, got status %u bits %llx\n", static_cast<unsigned long long>(j), w.status,
              static_cast<unsigned long long>(w.bits), with_status ? status[j] : 255u, static_cast<unsigned long long>(value[j]));
      return 2;
    }
    counts[w.status]++;
  }
  for (int c = 0; c < 5; c++)
    if (counts[c] != summary[c]) return 3;
  return 0;
}

}  // namespace

int main() {
  int cases = 0;
  for (uint64_t k : {0, 1, 65, 700})
    for (int kind : {0, 1, 2})
      for (int trim : {0, 1})
        for (int take : {0, 1}) {
          const int bad = one_case(k, kind, trim != 0, take != 0, cases % 3 != 0);
          if (bad) {
            fprintf(stderr, "parse_exec: case %d (k %llu kind %d trim %d take %d) failed: %d\n", cases, static_cast<unsigned long long>(k), kind, trim, take, bad);
            return 1;
          }
          cases++;
        }
  printf("parse_exec: %d cases\n", cases);
  return 0;
}
#endif
