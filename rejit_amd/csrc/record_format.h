// rejit_amd/csrc/record_format.h -- the meaning of rj_scan_records_format (record_format.hip): a column of 64-bit values written
// as decimal TEXT, the inverse of record_parse.h -- the bytes are exactly what Python writes, str(int) for the integer kinds and
// repr(float) for the doubles.  Host and device code: the CPU tests drive exactly these functions
// (tests/support/format_exec.cc), as the kernels do.
//
// A value becomes a Small first: 16 bytes, the decimal mantissa in one word and the row's sign, class, digit count, decimal
// point and length in the other.  For an integer the mantissa is its magnitude; for a finite double it is the SHORTEST digit
// string (1 to 17 digits) that reads back as the same double, the closest to the exact value among the strings of that length:
// shortest() below, the Schubfach algorithm (Giulietti, "The Schubfach way to render doubles", 2020) in integers only -- three
// 64 x 128 bit products with pow10_table.h's g(k), rounded to odd, and a few comparisons; no fallback, no floating-point
// operation.  From a Small the row's text follows byte by byte in closed form (Row, char_at): any byte range of a row is
// produced without the bytes before it, so the answer does not depend on where the output cuts a row (put_bytes, pack::chunk_part).
//
// repr(float): with the digits d1 d2 ... dn and the value 0.d1d2...dn x 10^decpt, the form is positional for -4 < decpt <= 16
// (a `.0` behind an integer), else d1[.d2...dn]e+-XX with at least two exponent digits; -0.0 is `-0.0`; the non-finite values
// are `inf`, `-inf` and `nan` (any sign, any payload).  rj_scan_records_parse reads none of those three back: its grammar has
// digits only.
#ifndef REJIT_AMD_RECORD_FORMAT_H_
#define REJIT_AMD_RECORD_FORMAT_H_

#include <stdint.h>

#include "pow10_table.h"
#include "record_pack.h"
#include "record_rows.h"

// (forced inline on the device: a Row handed to a function that is not inlined would live in scratch memory)
#if defined(__HIPCC__)
#define RJ_FORMAT_HD __host__ __device__ __forceinline__
#else
#define RJ_FORMAT_HD inline
#endif

namespace rejit_amd {
namespace numformat {

// RJ_FORMAT_INT64 / _UINT64 / _FLOAT64 (include/rejit_hip.h): the kind numbers of RJ_PARSE_*
enum Kind : int { kInt64 = 0, kUint64 = 1, kFloat64 = 2, kKinds = 3 };
RJ_FORMAT_HD bool kind_known(int kind) { return kind >= 0 && kind < kKinds; }
RJ_FORMAT_HD bool flags_known(unsigned flags) { return flags == 0; }
constexpr uint32_t kStatusOk = 0;   // RJ_PARSE_OK: every other status makes the row empty

// the longest row: -2.9205048131065683e-196 (a sign, 17 digits, the point, e, the exponent's sign, three exponent digits)
constexpr uint32_t kMaxRowBytes = 24;
constexpr uint32_t kMaxIntBytes = 20;   // -9223372036854775808, 18446744073709551615

// rows advance the output by at most kMaxRowBytes + gap: the plan's look-back carries pack::kMaxRow per row, pack::kMaxTotal in all
RJ_FORMAT_HD bool sums_fit(uint64_t k, uint64_t lead, uint64_t gap) { return pack::sums_fit(k, kMaxRowBytes, lead, gap); }

// what rj_scan_records_format refuses before it launches anything, in this order (the first bad index is found by its check kernel)
enum Refusal : int { kFine = 0, kNullArgument, kTableAlign, kOutAlign, kBadKind, kBadFlags, kBadFill, kBadSums, kTooManyRows };
RJ_FORMAT_HD Refusal check_call(const void* value, const void* status, uint64_t n_values, const void* indices, uint64_t n_indices, int kind,
                                     unsigned flags, int fill, uint64_t lead, uint64_t gap, const void* out, uint64_t out_cap, const void* out_begin,
                                     const void* out_end) {
  (void)status;   // (bytes: any alignment, and optional)
  const uint64_t k = indices ? n_indices : n_values;
  if ((!value && n_values) || (!out && out_cap)) return kNullArgument;
  if ((reinterpret_cast<uintptr_t>(value) | reinterpret_cast<uintptr_t>(indices) | reinterpret_cast<uintptr_t>(out_begin) |
       reinterpret_cast<uintptr_t>(out_end)) & 7u)
    return kTableAlign;
  if (reinterpret_cast<uintptr_t>(out) & 15u) return kOutAlign;
  if (!kind_known(kind)) return kBadKind;
  if (!flags_known(flags)) return kBadFlags;
  if (fill < 0 || fill > 255) return kBadFill;
  if (!sums_fit(k, lead, gap)) return kBadSums;
  if (!rows::rows_fit(k)) return kTooManyRows;
  return kFine;
}

// ---------------------------------------------------------------------------------------------------------------- integers
RJ_FORMAT_HD uint64_t mul_high(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

// the decimal digits of x, 1 for 0: nine comparisons with 32-bit literals
RJ_FORMAT_HD uint32_t digit_count32(uint32_t x) {
  return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) + (x >= 100000000u) +
         (x >= 1000000000u);
}
// the decimal digits of m: 1 for 0, 20 at most (m / 10^10 < 2^31)
RJ_FORMAT_HD uint32_t digit_count(uint64_t m) {
  const uint32_t high = static_cast<uint32_t>(m / 10000000000ull);
  if (high) return 10u + digit_count32(high);
  return (m >> 32) ? 10u : digit_count32(static_cast<uint32_t>(m));
}

// ---------------------------------------------------------------------------------------------------------------- Small
enum Class : uint32_t { kEmptyRow = 0, kInteger = 1, kFinite = 2, kInf = 3, kNan = 4 };
// meta: bits 0..7 the row's length, bit 8 the sign, bits 9..11 the class, bits 12..16 the digit count, bits 20..31 decpt + 1024
struct Small {
  uint64_t digits, meta;
};
RJ_FORMAT_HD uint64_t make_meta(uint32_t len, uint32_t neg, uint32_t cls, uint32_t nd, int32_t decpt) {
  return len | neg << 8 | cls << 9 | nd << 12 | static_cast<uint32_t>(decpt + 1024) << 20;
}
RJ_FORMAT_HD uint32_t small_len(const Small& s) { return static_cast<uint32_t>(s.meta) & 0xFFu; }
RJ_FORMAT_HD Small empty_row() { return Small{0, make_meta(0, 0, kEmptyRow, 0, 0)}; }

RJ_FORMAT_HD bool positional(int32_t decpt) { return decpt > -4 && decpt <= 16; }
// the length of repr()'s form of nd digits with the point at decpt (the sign not counted)
RJ_FORMAT_HD uint32_t repr_len(uint32_t nd, int32_t decpt) {
  if (positional(decpt)) {
    if (decpt <= 0) return 2u + static_cast<uint32_t>(-decpt) + nd;     // 0.000ddd
    if (static_cast<uint32_t>(decpt) < nd) return nd + 1;                 // dd.ddd
    return static_cast<uint32_t>(decpt) + 2;                              // ddd000.0
  }
  const int32_t e = decpt - 1;
  const uint32_t ae = static_cast<uint32_t>(e < 0 ? -e : e);
  return nd + (nd > 1 ? 1u : 0u) + 2u + (ae >= 100 ? 3u : 2u);             // d[.ddd]e+-XX[X]
}

// an integer kind's value: str(int)
RJ_FORMAT_HD Small small_of_int(uint64_t value, int kind) {
  const uint32_t neg = kind == kInt64 && (value >> 63) ? 1u : 0u;
  const uint64_t mag = neg ? 0 - value : value;
  const uint32_t nd = digit_count(mag);
  return Small{mag, make_meta(nd + neg, neg, kInteger, nd, 0)};
}

// ---------------------------------------------------------------------------------------------------------------- Schubfach
// floor(log2(10^e)) for |e| <= 1233, floor(log10(2^e)) and floor(log10(3/4 x 2^e)) for |e| <= 1500 (arithmetic shifts)
RJ_FORMAT_HD int32_t floor_log2_pow10(int32_t e) { return (e * 1741647) >> 19; }
RJ_FORMAT_HD int32_t floor_log10_pow2(int32_t e) { return (e * 1262611) >> 22; }
RJ_FORMAT_HD int32_t floor_log10_three_quarters_pow2(int32_t e) { return (e * 1262611 - 524031) >> 22; }

// floor(g x cp / 2^128), with the bits dropped behind it folded into bit 0 ("round to odd"): g = (g1, g0) overshoots the
// power it stands for by at most one unit, hence the product by less than 2^64 -- a middle word of 0 or 1 counts as nothing
RJ_FORMAT_HD uint64_t round_to_odd(uint64_t g1, uint64_t g0, uint64_t cp) {
  const uint64_t x1 = mul_high(g0, cp);
  const uint64_t y0 = g1 * cp;
  uint64_t y1 = mul_high(g1, cp);
  const uint64_t z = y0 + x1;
  if (z < y0) y1++;
  return y1 | (z > 1 ? 1u : 0u);
}

struct Decimal {
  uint64_t m;    // the digits, no trailing zero (0 for +-0.0)
  int32_t e10;   // the value is m x 10^e10
};
// the shortest decimal of the finite, non-zero double with the 52 mantissa bits f and the biased exponent be
RJ_FORMAT_HD Decimal shortest(uint64_t f, uint32_t be) {
  const uint64_t c = be != 0 ? (f | 1ull << 52) : f;
  const int32_t q = be != 0 ? static_cast<int32_t>(be) - 1075 : -1074;
  const bool even = (c & 1) == 0;                  // the interval's ends round to c
  const bool lower_closer = f == 0 && be > 1;      // a power of two: the neighbour below is half as far
  const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
  const int32_t k = lower_closer ? floor_log10_three_quarters_pow2(q) : floor_log10_pow2(q);
  const int32_t h = q + floor_log2_pow10(-k) + 1;   // 1..4
  const uint64_t* g = &kPow10[2 * (-k - kPow10MinK)];
  const uint64_t g1 = g[0], g0 = g[1];
  const uint64_t vbl = round_to_odd(g1, g0, cbl << h);
  const uint64_t vb = round_to_odd(g1, g0, cb << h);
  const uint64_t vbr = round_to_odd(g1, g0, cbr << h);
  const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
  const uint64_t s = vb >> 2;
  uint64_t m;
  int32_t e10 = k;
  bool found = false;
  if (s >= 10) {   // a shorter candidate: one digit fewer
    const uint64_t sp = s / 10;
    const bool up_inside = lower <= 40 * sp, wp_inside = 40 * sp + 40 <= upper;
    if (up_inside != wp_inside) {
      m = sp + (wp_inside ? 1 : 0);
      e10 = k + 1;
      found = true;
    }
  }
  if (!found) {
    const bool u_inside = lower <= 4 * s, w_inside = 4 * s + 4 <= upper;
    if (u_inside != w_inside) {
      m = s + (w_inside ? 1 : 0);
    } else {   // both or neither: the closer one, the even one at a tie
      const uint64_t mid = 4 * s + 2;
      m = s + ((vb > mid || (vb == mid && (s & 1))) ? 1 : 0);
    }
  }
  // trailing zeros belong to the exponent (at most 17 turns; eight at a time first)
  if (m % 100000000u == 0) m /= 100000000u, e10 += 8;
  while (m % 10 == 0) m /= 10, e10++;
  return Decimal{m, e10};
}

// a double's bits: repr(float)
RJ_FORMAT_HD Small small_of_double(uint64_t bits) {
  const uint32_t neg = static_cast<uint32_t>(bits >> 63);
  const uint32_t be = static_cast<uint32_t>(bits >> 52) & 0x7FFu;
  const uint64_t f = bits & ((1ull << 52) - 1);
  if (be == 0x7FFu) {
    if (f != 0) return Small{0, make_meta(3, 0, kNan, 0, 0)};
    return Small{0, make_meta(3 + neg, neg, kInf, 0, 0)};
  }
  if (be == 0 && f == 0) return Small{0, make_meta(3 + neg, neg, kFinite, 1, 1)};   // 0.0: the digit 0 with the point behind it
  const Decimal d = shortest(f, be);
  const uint32_t nd = digit_count(d.m);
  const int32_t decpt = d.e10 + static_cast<int32_t>(nd);
  return Small{d.m, make_meta(repr_len(nd, decpt) + neg, neg, kFinite, nd, decpt)};
}

RJ_FORMAT_HD Small small_of(uint64_t value, int kind) { return kind == kFloat64 ? small_of_double(value) : small_of_int(value, kind); }

// ---------------------------------------------------------------------------------------------------------------- rows
// x < 10^8 as eight ASCII digits, the first one in the lowest byte
RJ_FORMAT_HD uint64_t ascii8(uint32_t x) {
  uint64_t r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    r = r << 8 | (0x30u + x % 10);
    x /= 10;
  }
  return r;
}

// a Small unfolded once for the bytes that follow: the mantissa as 24 ASCII digits with zeros in front (three words)
struct Row {
  uint64_t a, b, c;
  uint32_t len, neg, cls, nd;
  int32_t decpt;
};
RJ_FORMAT_HD Row unfold(const Small& s) {
  Row r;
  const uint32_t meta = static_cast<uint32_t>(s.meta);
  r.len = meta & 0xFFu;
  r.neg = meta >> 8 & 1u;
  r.cls = meta >> 9 & 7u;
  r.nd = meta >> 12 & 31u;
  r.decpt = static_cast<int32_t>(meta >> 20) - 1024;
  const uint64_t top = s.digits / 10000000000000000ull, rest = s.digits % 10000000000000000ull;   // top < 1845
  r.a = ascii8(static_cast<uint32_t>(top));
  r.b = ascii8(static_cast<uint32_t>(rest / 100000000u));
  r.c = ascii8(static_cast<uint32_t>(rest % 100000000u));
  return r;
}
// digit t of the mantissa's nd, t < nd
RJ_FORMAT_HD uint32_t digit_at(const Row& r, uint32_t t) {
  const uint32_t pos = 24 - r.nd + t;
  // (masks, not a chain of selects: the compiler turns that chain into an indexed load of {a, b, c} from scratch memory)
  const uint64_t in_a = 0 - static_cast<uint64_t>(pos < 8), in_c = 0 - static_cast<uint64_t>(pos >= 16);
  const uint64_t word = (r.a & in_a) | (r.b & ~(in_a | in_c)) | (r.c & in_c);
  return static_cast<uint32_t>(word >> (8 * (pos & 7))) & 0xFFu;
}
// byte i of the row's text, i < r.len
RJ_FORMAT_HD uint32_t char_at(const Row& r, uint32_t i) {
  if (i < r.neg) return 0x2Du;   // -
  i -= r.neg;
  if (r.cls == kInteger) return digit_at(r, i);
  if (r.cls == kInf) return 0x666E69u >> (8 * i) & 0xFFu;   // inf
  if (r.cls == kNan) return 0x6E616Eu >> (8 * i) & 0xFFu;   // nan
  const uint32_t nd = r.nd;
  const int32_t decpt = r.decpt;
  if (positional(decpt)) {
    if (decpt <= 0) {   // 0.000ddd
      const uint32_t zeros = static_cast<uint32_t>(-decpt);
      if (i == 0) return 0x30u;
      if (i == 1) return 0x2Eu;
      return i - 2 < zeros ? 0x30u : digit_at(r, i - 2 - zeros);
    }
    const uint32_t point = static_cast<uint32_t>(decpt);
    if (point < nd) return i < point ? digit_at(r, i) : i == point ? 0x2Eu : digit_at(r, i - 1);   // dd.ddd
    return i < nd ? digit_at(r, i) : i == point ? 0x2Eu : 0x30u;                                     // ddd000.0
  }
  const uint32_t mant = nd + (nd > 1 ? 1u : 0u);
  if (i < mant) return i == 0 ? digit_at(r, 0) : i == 1 ? 0x2Eu : digit_at(r, i - 1);
  i -= mant;
  const int32_t e = decpt - 1;
  if (i == 0) return 0x65u;                    // e
  if (i == 1) return e < 0 ? 0x2Du : 0x2Bu;    // - +
  const uint32_t ae = static_cast<uint32_t>(e < 0 ? -e : e);   // <= 324
  const uint32_t place = (ae >= 100 ? 3u : 2u) - (i - 2);      // 3: hundreds, 2: tens, 1: units
  return 0x30u + (place == 3 ? ae / 100 : place == 2 ? ae / 10 % 10 : ae % 10);
}

// byte b of the 16 in w becomes c -- pack::put_byte for a b that is not known at compile time: the word is chosen by four
// selects, not by an indexed register (which the device would keep in scratch memory)
RJ_FORMAT_HD void put_byte(uint32_t w[4], uint32_t b, uint32_t c) {
  const uint32_t sh = 8 * (b & 3), keep = ~(0xFFu << sh), word = b >> 2;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < 4; i++) w[i] = word == i ? ((w[i] & keep) | c << sh) : w[i];
}
// bytes [from, from + count) of the row into bytes [at, at + count) of the 16 in w
RJ_FORMAT_HD void put_bytes(const Row& r, uint32_t from, uint32_t count, uint32_t at, uint32_t w[4]) {
  for (uint32_t i = 0; i < count; i++) put_byte(w, at + i, char_at(r, from + i));
}

// (record_pack.h's chunk_part under this header's name: one definition, the name its callers have always used)
using pack::chunk_part;

}  // namespace numformat
}  // namespace rejit_amd
#endif
