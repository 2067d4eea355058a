// tests/support/format_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_format.h, compiled with g++
// (tests/test_record_format.py).  It walks the call the way record_format.hip's kernels do -- the index check, the plan unit by unit (a row's
// status and value, its Small staged, the running sum carried from unit to unit where the kernel looks back), the emit chunk
// by chunk: the chunk's rows from one pair of searches, every row's bytes inside the chunk written once into the chunk's
// image (the kernel's LDS), the image stored in 16 aligned bytes per step -- with the unit size and the chunk size chosen by
// the test.  Every access is checked against its range, and every output byte and table row may be
// written only once.  fe_row produces one row's bytes whole AND piecewise at every split, and refuses when they differ.
//
// With -DFORMAT_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): a fixed set
// of values and seeded ones against the C++ library's shortest digits (std::to_chars) and strtod, and the call over exact
// allocations.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_format.h"
#include "../../rejit_amd/csrc/record_parse.h"
#include "checked_image.h"

using namespace rejit_amd;

// [0] kMaxRowBytes, [1] the table's entries, [2] its first k (as int64), [3] sizeof(Small)
extern "C" void fe_constants(int64_t* out) {
  out[0] = numformat::kMaxRowBytes;
  out[1] = numformat::kPow10Entries;
  out[2] = numformat::kPow10MinK;
  out[3] = sizeof(numformat::Small);
}

extern "C" int fe_table(uint64_t* out, int room) {
  if (room < 2 * numformat::kPow10Entries) return -1;
  for (int i = 0; i < 2 * numformat::kPow10Entries; i++) out[i] = numformat::kPow10[i];
  return numformat::kPow10Entries;
}

// One value's row into buf (kMaxRowBytes of room) -> its length; small[0..1]: the mantissa and the meta word.  -3: a piecewise
// production (every split into two ranges, and byte by byte) differs from the whole, or the length is out of range.
extern "C" int fe_row(uint64_t value, int kind, uint8_t* buf, uint64_t* small) {
  const numformat::Small s = numformat::small_of(value, kind);
  small[0] = s.digits, small[1] = s.meta;
  const uint32_t len = numformat::small_len(s);
  if (len == 0 || len > numformat::kMaxRowBytes) return -3;
  const numformat::Row row = numformat::unfold(s);
  if (row.len != len) return -3;
  for (uint32_t i = 0; i < len; i++) buf[i] = static_cast<uint8_t>(numformat::char_at(row, i));
  for (uint32_t cut = 0; cut <= len; cut++) {
    // [0, cut) and [cut, len), each in groups of at most 16 bytes placed at a varying offset inside the 16
    uint8_t again[numformat::kMaxRowBytes];
    for (uint32_t a = 0, b = cut, turn = 0; turn < 2; a = cut, b = len, turn++)
      for (uint32_t from = a; from < b;) {
        const uint32_t at = (from + cut) & 15u;
        uint32_t count = 16 - at;
        if (count > b - from) count = b - from;
        uint32_t w[4] = {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};
        numformat::put_bytes(numformat::unfold(s), from, count, at, w);
        for (uint32_t i = 0; i < 16; i++) {
          const uint8_t c = static_cast<uint8_t>(w[i >> 2] >> (8 * (i & 3)));
          if (i >= at && i < at + count) again[from + i - at] = c;
          else if (c != 0xA5) return -3;   // a byte outside the range was touched
        }
        from += count;
      }
    if (memcmp(again, buf, len) != 0) return -3;
  }
  return static_cast<int>(len);
}

// the header's own parse of a row's bytes under `flags` -> the status; *bits: the value
extern "C" int fe_parse(const uint8_t* row, uint32_t len, int kind, unsigned flags, uint64_t* bits) {
  numparse::State st = numparse::start(kind, flags);
  for (uint32_t at = 0; at < len && !numparse::done(st); at += 16) {
    const uint32_t valid = len - at < 16 ? len - at : 16;
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < valid; i++) w[i >> 2] |= static_cast<uint32_t>(row[at + i]) << (8 * (i & 3));
    numparse::step(st, w, valid);
  }
  const numparse::Result res = numparse::finish(st, kind);
  *bits = res.bits;
  return static_cast<int>(res.status);
}

// summary: [0] total, [1] first bad row (~0: none), [2] chunks, [4] groups stored, [6] rows unfolded (a row that crosses a
// chunk's end counts twice), [7] the refusal of check_call.
// Returns 0; -1 when an access left its range or something was written twice (a bug the kernel would pay for with a fault or
// a race); -2 for a call check_call refuses.
extern "C" long fe_format(const uint64_t* value, const uint8_t* status, uint64_t n_values, const uint64_t* indices, int have_indices, uint64_t n_indices,
                          int kind, unsigned flags, int fill, uint64_t lead, uint64_t gap, uint64_t unit, uint64_t chunk, uint8_t* out,
                          uint64_t out_cap, uint64_t* out_begin, uint64_t* out_end, uint64_t* summary) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[1] = ~0ull;
  const uint64_t* idx = have_indices ? indices : nullptr;
  static const uint64_t kNoRows[1] = {0};
  const numformat::Refusal why = numformat::check_call(value, status, n_values, have_indices ? (idx ? idx : kNoRows) : nullptr, n_indices, kind, flags, fill,
                                                      lead, gap, out, out_cap, out_begin, out_end);
  summary[7] = why;
  if (why != numformat::kFine) return -2;
  if (unit == 0 || chunk == 0 || chunk % pack::kGroupBytes != 0) return -2;
  const uint64_t k = have_indices ? n_indices : n_values;
  bool left_range = false, twice = false;
  const auto value_row = [&](uint64_t j) {   // r(j), checked: the index list has k rows
    if (j >= k) left_range = true;
    return idx ? idx[j] : j;
  };
  // ---- check: the index list only; a refused call writes no table row and no byte
  for (uint64_t j = 0; j < k; j++)
    if (value_row(j) >= n_values) {
      summary[1] = j;
      return left_range ? -1 : 0;
    }
  // ---- plan
  std::vector<uint64_t> own_begin(k + 1);
  uint64_t* ob = out_begin ? out_begin : own_begin.data();
  std::vector<numformat::Small> stage(k);
  std::vector<uint8_t> row_once(k, 0);
  uint64_t before = 0;
  for (uint64_t u0 = 0; u0 < k; u0 += unit) {
    const uint64_t u1 = u0 + unit < k ? u0 + unit : k;
    uint64_t in_unit = 0;
    for (uint64_t j = u0; j < u1; j++) {
      const uint64_t r = value_row(j);
      numformat::Small s = numformat::empty_row();
      if (!status || status[r] == numformat::kStatusOk) s = numformat::small_of(value[r], kind);
      stage[j] = s;
      const uint64_t len = numformat::small_len(s);
      if (row_once[j]) twice = true;
      row_once[j] = 1;
      ob[j] = lead + before + in_unit;
      if (out_end) out_end[j] = ob[j] + len;
      in_unit += pack::row_advance(false, 0, len, gap);
    }
    before += in_unit;
  }
  const uint64_t total = lead + before;
  summary[0] = total;
  // ---- emit: the chunk's image (the kernel's LDS) filled, every row of the chunk once, the image stored in groups of 16
  const pack::View table{ob, nullptr, nullptr, nullptr, 0, k, total};
  const long chunks = walk_chunks(table, k, total, chunk, out, out_cap, [&](uint64_t c0, uint64_t c1, uint64_t j0, uint64_t j1, std::vector<uint8_t>* got) {
    CheckedImage image(chunk, static_cast<uint32_t>(fill), c0, c1);
    for (uint64_t j = j0; j < j1; j++) {
      const numformat::Small s = stage[j];   // (j < j1 <= k)
      uint32_t lo, hi;
      if (!pack::chunk_part(ob[j], numformat::small_len(s), c0, c1, &lo, &hi)) continue;
      if (hi > numformat::small_len(s)) left_range = true;
      summary[6]++;
      // (the bytes through put_bytes in groups, as the piecewise check of fe_row: the kernel's char_at loop is the same function)
      const numformat::Row row = numformat::unfold(s);
      for (uint32_t i = lo; i < hi; i++) image.put(ob[j] + i - c0, numformat::char_at(row, i));
    }
    image.store(got);
    summary[4] += image.from_image;
    left_range |= image.left_range, twice |= image.twice;
  });
  if (chunks < 0) return -1;
  summary[2] = static_cast<uint64_t>(chunks);
  return left_range || twice ? -1 : 0;
}

#ifdef FORMAT_EXEC_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <charconv>
#include <string>

namespace {

uint64_t rnd64() {
  static uint64_t rng = 88172645463325252ull;
  rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
  return rng;
}

// repr(float) over std::string from the library's shortest digits (std::to_chars, scientific)
std::string repr_of(uint64_t bits) {
  double v;
  memcpy(&v, &bits, 8);
  if (v != v) return "nan";
  const bool neg = bits >> 63;
  std::string sign = neg ? "-" : "";
  if ((bits << 1) == 0x7FF0000000000000ull << 1) return sign + "inf";
  char buf[64];
  const auto res = std::to_chars(buf, buf + sizeof(buf), neg ? -v : v, std::chars_format::scientific);
  const std::string sci(buf, res.ptr);   // d[.ddd]e+-XX
  const size_t e_at = sci.find('e');
  std::string digits;
  for (size_t i = 0; i < e_at; i++)
    if (sci[i] != '.') digits += sci[i];
  const int decpt = atoi(sci.c_str() + e_at + 1) + 1;
  const int nd = static_cast<int>(digits.size());
  if (decpt > -4 && decpt <= 16) {
    if (decpt <= 0) return sign + "0." + std::string(-decpt, '0') + digits;
    if (decpt < nd) return sign + digits.substr(0, decpt) + "." + digits.substr(decpt);
    return sign + digits + std::string(decpt - nd, '0') + ".0";
  }
  char ex[16];
  snprintf(ex, sizeof(ex), "e%c%02d", decpt - 1 < 0 ? '-' : '+', abs(decpt - 1));
  return sign + digits.substr(0, 1) + (nd > 1 ? "." + digits.substr(1) : "") + ex;
}

std::string want_of(uint64_t value, int kind) {
  if (kind == numformat::kFloat64) return repr_of(value);
  if (kind == numformat::kInt64) return std::to_string(static_cast<long long>(value));
  return std::to_string(static_cast<unsigned long long>(value));
}

}  // namespace

int main() {
  int cases = 0;
  size_t longest = 0;
  for (int kind = 0; kind < numformat::kKinds; kind++) {
    std::vector<uint64_t> values = {0, 1, ~0ull, 1ull << 63, (1ull << 63) - 1, 9, 10, 99, 100, 9999999999999999999ull, 10000000000000000000ull,
                                    0x8000000000000000ull, 0x0000000000000001ull, 0x000FFFFFFFFFFFFFull, 0x0010000000000000ull, 0x7FEFFFFFFFFFFFFFull,
                                    0x7FF0000000000000ull, 0xFFF0000000000000ull, 0x7FF8000000000000ull, 0xFFF0000000000001ull, 0x4341C37937E08000ull,
                                    0x4341C37937E07FFFull, 0x3F1A36E2EB1C432Dull, 0x3F1A36E2EB1C432Cull, 0x3FD3333333333334ull, 0x444B1AE4D6E2EF50ull,
                                    0x44B52D02C7E14AF6ull, 0x9755D4C13A902931ull};
    for (uint32_t e = 1; e < 0x7FF; e++) values.push_back(static_cast<uint64_t>(e) << 52);   // the powers of two
    for (int i = 0; i < 4000; i++) values.push_back(rnd64() >> (rnd64() % 64));
    std::vector<uint8_t> status(values.size(), 0);
    for (size_t i = 0; i < values.size(); i += 7) status[i] = static_cast<uint8_t>(1 + i % 4);
    // ---- every row alone
    for (const uint64_t v : values) {
      uint8_t buf[numformat::kMaxRowBytes];
      uint64_t small[2];
      const int len = fe_row(v, kind, buf, small);
      const std::string want = want_of(v, kind);
      if (len < 0 || std::string(reinterpret_cast<char*>(buf), len) != want) {
        fprintf(stderr, "format_exec: kind %d value %llx: want %s, got %.*s (%d)\n", kind, static_cast<unsigned long long>(v), want.c_str(), len < 0 ? 0 : len,
                reinterpret_cast<char*>(buf), len);
        return 1;
      }
      if (want.size() > longest) longest = want.size();
      cases++;
    }
    // ---- the call, over exact allocations
    for (int layout = 0; layout < 4; layout++) {
      const uint64_t lead = layout & 1 ? 5 : 0, gap = layout == 0 ? 0 : layout == 1 ? 1 : layout == 2 ? 3 : 40;
      const bool with_status = layout >= 2, with_indices = layout == 1 || layout == 3;
      std::vector<uint64_t> indices;
      for (size_t i = 0; i < values.size() / 2; i++) indices.push_back(rnd64() % values.size());
      const uint64_t k = with_indices ? indices.size() : values.size();
      std::string want(lead, '\n');
      for (uint64_t j = 0; j < k; j++) {
        const uint64_t r = with_indices ? indices[j] : j;
        if (!with_status || status[r] == 0) want += want_of(values[r], kind);
        want += std::string(gap, '\n');
      }
      std::vector<uint64_t> ob(k), oe(k);
      uint64_t summary[8];
      // 16-byte aligned, exact in its last byte: the sanitizer sees any byte behind the total
      void* room = nullptr;
      if (posix_memalign(&room, 16, want.size() ? want.size() : 1) != 0) return 1;
      uint8_t* out = static_cast<uint8_t*>(room);
      const long rc = fe_format(values.data(), with_status ? status.data() : nullptr, values.size(), with_indices ? indices.data() : nullptr, with_indices,
                                indices.size(), kind, 0, '\n', lead, gap, 256, layout == 0 ? 64 : 4096, out, want.size(), ob.data(), oe.data(), summary);
      const bool same = rc == 0 && summary[0] == want.size() && memcmp(out, want.data(), want.size()) == 0;
      free(out);
      if (!same) {
        fprintf(stderr, "format_exec: kind %d layout %d: rc %ld total %llu want %zu\n", kind, layout, rc, static_cast<unsigned long long>(summary[0]), want.size());
        return 1;
      }
      cases += static_cast<int>(k);
    }
  }
  if (longest != numformat::kMaxRowBytes || sizeof(numformat::Small) != 16) return 1;
  printf("format_exec: %d cases\n", cases);
  return 0;
}
#endif
