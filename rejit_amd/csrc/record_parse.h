// rejit_amd/csrc/record_parse.h -- the meaning of rj_scan_records_parse (record_parse.hip): a row of a record table read as a
// NUMBER -- an int64, a uint64 or a double -- exactly, or not at all: a row's value is what Python's int() / float() (strtod,
// correctly rounded) make of its bytes, or the row carries a status that says why it has none.  Host and device code: the CPU
// tests drive exactly these functions (tests/support/parse_exec.cc), as the kernel does.
//
// A row is consumed in the 16-byte groups of record_rows.h (step), in order; the State between two groups is all that is
// kept, so the result does not depend on where a row's bytes are cut, and a row of any length costs a fixed state.
//
// Grammar (D = [0-9]; with kTrim the spaces and tabs before and behind the number are dropped first, without it they are
// ordinary bytes; nothing else is skipped, a NUL is an ordinary byte):
//     INT64    [+-]?D+          UINT64   \+?D+          FLOAT64  [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?
// Statuses, in this order: EMPTY (no bytes left), MALFORMED (not in the grammar), RANGE (integer kinds: outside the type),
// INEXACT (FLOAT64: outside the exact window, below).
//
// The value of a row's digits is kept as  m x 10^(zeros - frac + exp):
//     m       the mantissa's digits up to its last NON-ZERO one, saturating above 2^64 - 1 (kSat);
//     zeros   the zeros seen behind that digit -- they are folded into m only when another non-zero digit follows, so trailing
//             zeros never enter m, and leading zeros (m == 0) are dropped;
//     frac    the mantissa digits behind the point;  exp: the explicit exponent's magnitude, saturating at 2^62.
// So m is not divisible by 10, and (m, q = zeros - frac +- exp) is a property of the value, not of its spelling: 1.50, 15e-1
// and 0.0015e3 are (15, -1).  zeros and frac are at most the row's length; no text has 2^62 bytes, so q is exact, or so far
// outside the window that the saturation cannot matter.
//
// The exact window (Clinger's fast path): m <= 2^53 and -22 <= q <= 22.  Then double(m) is exact, 10^|q| is exact (5^22 <
// 2^53), and the value is ONE IEEE operation on two exact operands -- double(m) * 10^q or double(m) / 10^-q --, hence the
// correctly rounded value, strtod's bits.  m == 0 is +-0.0 whatever the exponent says.  Everything else is INEXACT: never a
// nearby value.
//
// RJ_PARSE_WIDE (FLOAT64; kWide in the State's flags, the *_as<true> functions below) gives every
// decimal the State can hold its correctly rounded double.  With S the significant digits (first to last non-zero mantissa
// digit) and the value int(S) x 10^q:
//     int(S) <= 2^64 - 1   the row is DECIDED: the window's one operation where it applies, else the Eisel-Lemire product
//                          (eisel_lemire below) -- OK with float()'s bits, or RANGE when that double is infinite;
//     otherwise            m holds P, the longest prefix of S that fits 64 bits, and `zeros` counts every mantissa digit
//                          dropped behind it.  The value lies strictly between P x 10^Q and (P + 1) x 10^Q, Q = zeros - frac
//                          +- exp: both ends round to one double -> OK with it (rounding is monotone); both infinite ->
//                          RANGE; else, or when P + 1 does not fit, INEXACT.
// For that the wide walk folds pending zeros into m one at a time while they fit (the `zeros >= 20` shortcut saturates without
// folding: right without WIDE, where a saturated m has no value, wrong with it), and saturation is only ever triggered by a
// non-zero digit, so the dropped tail is never all zeros and the bracket is strict.  Without WIDE nothing changes: the
// *_as<false> functions are the ones this header always had.
#ifndef REJIT_AMD_RECORD_PARSE_H_
#define REJIT_AMD_RECORD_PARSE_H_

#include <stdint.h>

#include "pow5_table.h"
#include "record_pack.h"

namespace rejit_amd {
namespace numparse {

// RJ_PARSE_INT64 / _UINT64 / _FLOAT64, RJ_PARSE_TRIM, RJ_PARSE_OK ... _INEXACT (include/rejit_hip.h)
enum Kind : int { kInt64 = 0, kUint64 = 1, kFloat64 = 2, kKinds = 3 };
constexpr unsigned kTrimFlag = 1u;
constexpr unsigned kWideFlag = 4u;   // (2u is reserved: unknown and refused)
enum Status : uint32_t { kOk = 0, kEmpty = 1, kMalformed = 2, kRange = 3, kInexact = 4, kStatuses = 5 };

RJ_PACK_HD inline bool kind_known(int kind) { return kind >= 0 && kind < kKinds; }
RJ_PACK_HD inline bool flags_known(unsigned flags) { return (flags & ~(kTrimFlag | kWideFlag)) == 0; }

// ---------------------------------------------------------------------------------------------------------------- state
// the phases of the grammar, in the order the bytes of a number pass them
enum Phase : uint32_t {
  kStart = 0,     // nothing but trimmed blanks so far
  kSign = 1,      // the mantissa's sign
  kInt = 2,       // D+                                   (accepting)
  kPoint = 3,     // a point without a digit before it: a digit must follow
  kFrac = 4,      // D+\.D*  or  \.D+                      (accepting)
  kExpMark = 5,   // e / E
  kExpSign = 6,   // the exponent's sign
  kExp = 7,       // its digits                            (accepting)
  kTrail = 8,     // trimmed blanks behind the number      (accepting)
  kBad = 9        // not in the grammar, whatever follows
};
RJ_PACK_HD inline bool accepting(uint32_t phase) { return phase == kInt || phase == kFrac || phase == kExp || phase == kTrail; }

enum : uint32_t { kNeg = 1u, kExpNeg = 2u, kSat = 4u, kTrim = 8u, kFloat = 16u, kUnsigned = 32u, kWide = 64u };

constexpr uint64_t kExpCap = 1ull << 62;                   // the explicit exponent's magnitude saturates here
constexpr uint64_t kTenth = 0xFFFFFFFFFFFFFFFFull / 10;    // m x 10 + d fits below it, and at it for d <= 5
constexpr uint64_t kMantissaMax = 1ull << 53;              // the largest m of the exact window (inclusive)
constexpr int64_t kPowerMax = 22;                          // |q| of the exact window

struct State {
  uint64_t m, zeros, frac, exp;
  uint32_t phase, flags;
};
// kWideWalk: the row is a FLOAT64 under RJ_PARSE_WIDE (the flag is inert for the integer kinds)
template <bool kWideWalk>
RJ_PACK_HD inline State start_as(int kind, unsigned flags) {
  State s{0, 0, 0, 0, kStart, 0};
  if (flags & kTrimFlag) s.flags |= kTrim;
  if (kind == kFloat64) s.flags |= kFloat;
  if (kind == kUint64) s.flags |= kUnsigned;
  if (kWideWalk) s.flags |= kWide;
  return s;
}
RJ_PACK_HD inline State start(int kind, unsigned flags) {
  return kind == kFloat64 && (flags & kWideFlag) ? start_as<true>(kind, flags) : start_as<false>(kind, flags);
}
// nothing that follows changes the row's status any more (a malformed row may stop early; a row heading for RANGE or
// INEXACT may not: MALFORMED outranks both)
RJ_PACK_HD inline bool done(const State& s) { return s.phase == kBad; }

// ---------------------------------------------------------------------------------------------------------------- digits
// m = m x 10 + d, or kSat
RJ_PACK_HD inline void times10_add(uint64_t& m, uint32_t& flags, uint32_t d) {
  if (m > kTenth || (m == kTenth && d > 5)) flags |= kSat;
  else m = m * 10 + d;
}
// m = m x 10^zeros for m != 0 (20 zeros behind any digit leave 64 bits)
RJ_PACK_HD inline void fold_zeros(uint64_t& m, uint32_t& flags, uint64_t zeros) {
  if (zeros >= 20) {
    flags |= kSat;
    return;
  }
  for (uint64_t i = 0; i < zeros && !(flags & kSat); i++) times10_add(m, flags, 0);
}
RJ_PACK_HD inline void mantissa_digit(State& s, uint32_t d) {
  if (d == 0) {
    s.zeros++;
    return;
  }
  if (!(s.flags & kSat)) {
    if (s.m != 0) fold_zeros(s.m, s.flags, s.zeros);   // (m == 0: the zeros so far were leading ones)
    if (!(s.flags & kSat)) times10_add(s.m, s.flags, d);
  }
  s.zeros = 0;
}
// the wide walk: m is the longest prefix of the significant digits that fits; once saturated, zeros counts every digit dropped
RJ_PACK_HD inline void mantissa_digit_wide(State& s, uint32_t d) {
  if ((s.flags & kSat) || d == 0) {
    s.zeros++;
    return;
  }
  uint64_t pending = s.m != 0 ? s.zeros : 0;   // (m == 0: the zeros so far were leading ones)
  for (; pending != 0 && s.m <= kTenth; pending--) s.m *= 10;   // (at most 20 turns: m >= 1)
  if (pending == 0) times10_add(s.m, s.flags, d);
  else s.flags |= kSat;
  s.zeros = (s.flags & kSat) ? pending + 1 : 0;   // the zeros that did not fit, and d
}
RJ_PACK_HD inline void exponent_digit(State& s, uint32_t d) {
  if (s.exp > kExpCap / 10) s.exp = kExpCap;
  else s.exp = s.exp * 10 + d;
  if (s.exp > kExpCap) s.exp = kExpCap;
}

// ---------------------------------------------------------------------------------------------------------------- step
template <bool kWideWalk>
RJ_PACK_HD inline void step_byte_as(State& s, uint32_t c) {
  const uint32_t d = c - 0x30u;
  const uint32_t ph = s.phase;
  if (d <= 9u) {
    if (ph <= kInt) {
      if (kWideWalk) mantissa_digit_wide(s, d);
      else mantissa_digit(s, d);
      s.phase = kInt;
    } else if (ph == kPoint || ph == kFrac) {
      s.frac++;
      if (kWideWalk) mantissa_digit_wide(s, d);
      else mantissa_digit(s, d);
      s.phase = kFrac;
    } else if (ph >= kExpMark && ph <= kExp) {
      exponent_digit(s, d);
      s.phase = kExp;
    } else {
      s.phase = kBad;   // a digit behind trailing blanks
    }
    return;
  }
  if ((c == 0x20u || c == 0x09u) && (s.flags & kTrim)) {
    if (ph != kStart && ph != kTrail) s.phase = accepting(ph) ? kTrail : kBad;
    return;
  }
  if (c == 0x2Bu || c == 0x2Du) {   // + -
    const bool minus = c == 0x2Du;
    if (ph == kStart && !(minus && (s.flags & kUnsigned))) {
      if (minus) s.flags |= kNeg;
      s.phase = kSign;
    } else if (ph == kExpMark) {
      if (minus) s.flags |= kExpNeg;
      s.phase = kExpSign;
    } else {
      s.phase = kBad;
    }
    return;
  }
  if (s.flags & kFloat) {
    if (c == 0x2Eu) {   // .
      s.phase = ph <= kSign ? kPoint : ph == kInt ? kFrac : kBad;
      return;
    }
    if ((c | 0x20u) == 0x65u) {   // e E
      s.phase = (ph == kInt || ph == kFrac) ? kExpMark : kBad;
      return;
    }
  }
  s.phase = kBad;
}

// the first `valid` (1..16) bytes of a group of rows::load_group, in order
template <bool kWideWalk>
RJ_PACK_HD inline void step_as(State& s, const uint32_t w[4], uint32_t valid) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < 4; i++) {
    uint32_t x = w[i];
    const uint32_t bytes = valid >= 4 * i + 4 ? 4u : valid > 4 * i ? valid - 4 * i : 0u;
    for (uint32_t b = 0; b < bytes && s.phase != kBad; b++) {
      step_byte_as<kWideWalk>(s, x & 0xFFu);
      x >>= 8;
    }
  }
}
RJ_PACK_HD inline void step_byte(State& s, uint32_t c) {
  if (s.flags & kWide) step_byte_as<true>(s, c);
  else step_byte_as<false>(s, c);
}
RJ_PACK_HD inline void step(State& s, const uint32_t w[4], uint32_t valid) {
  if (s.flags & kWide) step_as<true>(s, w, valid);
  else step_as<false>(s, w, valid);
}

// ---------------------------------------------------------------------------------------------------------------- finish
struct Result {
  uint32_t status;
  uint64_t bits;   // 0 unless status == kOk
};

RJ_PACK_HD inline uint64_t double_bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}
// 10^e for 0 <= e <= 22: the 23 powers a double holds exactly
RJ_PACK_HD inline double exact_power(uint32_t e) {
  const double p[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                        1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return p[e];
}

// ---------------------------------------------------------------------------------------------------------- Eisel-Lemire
// The double nearest to w x 10^q (w != 0), by integer arithmetic: its bits, kInfBits when it is infinite.  w is normalised
// to 64 bits and multiplied by the 128-bit truncated power of five (pow5_table.h); the second partial product is needed only
// when the first leaves the low nine bits of the high word all ones; for w < 2^64 and -342 <= q <= 308 that decides every
// case (Mushtak and Lemire, "Fast Number Parsing Without Fallback").  Below -342 the value is under half the smallest
// subnormal (w < 2^64 < 1.9e19) and rounds to 0; above 308 it is at least 1e309.
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;

RJ_PACK_HD inline uint32_t leading_zeros(uint64_t w) {   // w != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<uint32_t>(__clzll(static_cast<long long>(w)));
#else
  return static_cast<uint32_t>(__builtin_clzll(w));
#endif
}
RJ_PACK_HD inline uint64_t mul_high(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

RJ_PACK_HD inline uint64_t eisel_lemire(uint64_t w, int64_t q) {
  if (q < kPow5MinQ) return 0;
  if (q > kPow5MaxQ) return kInfBits;
  uint32_t lz = leading_zeros(w);
  w <<= lz;
  const uint64_t* five = &kPow5[2 * static_cast<uint32_t>(q - kPow5MinQ)];
  uint64_t lo = w * five[0], hi = mul_high(w, five[0]);
  if ((hi & 0x1FFu) == 0x1FFu) {   // 55 bits of the product are wanted: the first word may not decide them
    const uint64_t second = mul_high(w, five[1]);
    lo += second;
    if (second > lo) hi++;
  }
  const uint32_t upper = static_cast<uint32_t>(hi >> 63);
  const uint32_t shift = upper + 9;                      // 64 - 52 - 3 + upper: 54 bits of mantissa, one of them the round bit
  uint64_t mant = hi >> shift;
  // floor(log2(10^q)) + 63, the binary exponent of the table's entry; + 1023, the bias
  int32_t power2 = static_cast<int32_t>((217706 * static_cast<int32_t>(q)) >> 16) + 63 + static_cast<int32_t>(upper) - static_cast<int32_t>(lz) + 1023;
  if (power2 <= 0) {   // subnormal, or zero
    if (1 - power2 >= 64) return 0;
    mant >>= 1 - power2;
    mant += mant & 1;
    mant >>= 1;
    return mant;       // (mant == 2^52: the smallest normal; its bit 52 is the exponent's 1)
  }
  // exactly halfway -- possible only for -4 <= q <= 23, where 5^q or its reciprocal's error can vanish --: round to even
  if (lo <= 1 && q >= -4 && q <= 23 && (mant & 3) == 1 && (mant << shift) == hi) mant &= ~1ull;
  mant += mant & 1;
  mant >>= 1;
  if (mant >= (2ull << 52)) {
    mant = 1ull << 52;
    power2++;
  }
  mant &= ~(1ull << 52);
  if (power2 >= 0x7FF) return kInfBits;
  return mant | static_cast<uint64_t>(power2) << 52;
}

template <bool kWideWalk>
RJ_PACK_HD inline Result finish_as(const State& s, int kind) {
  if (s.phase == kStart) return Result{kEmpty, 0};
  if (!accepting(s.phase)) return Result{kMalformed, 0};
  const bool neg = (s.flags & kNeg) != 0;
  if (kind != kFloat64) {
    uint64_t mag = s.m;
    uint32_t flags = s.flags;
    if (mag != 0 && !(flags & kSat)) fold_zeros(mag, flags, s.zeros);
    if (flags & kSat) return Result{kRange, 0};
    if (kind == kUint64) return Result{kOk, mag};
    const uint64_t most = neg ? (1ull << 63) : (1ull << 63) - 1;
    if (mag > most) return Result{kRange, 0};
    return Result{kOk, neg ? 0 - mag : mag};
  }
  const uint64_t sign = neg ? 1ull << 63 : 0;
  const bool sat = (s.flags & kSat) != 0;
  if (!sat && s.m == 0) return Result{kOk, sign};
  if (!kWideWalk && (sat || s.m > kMantissaMax)) return Result{kInexact, 0};
  // (unsigned arithmetic: every term is below 2^62 in magnitude or saturated there, see above)
  const int64_t q = static_cast<int64_t>(s.zeros - s.frac + ((s.flags & kExpNeg) ? 0 - s.exp : s.exp));
  if (kWideWalk && (sat || s.m > kMantissaMax || q < -kPowerMax || q > kPowerMax)) {
    // decided: the double of m x 10^q.  Saturated: the value lies strictly between m x 10^q and (m + 1) x 10^q, and has the
    // double both ends round to, when they agree (one copy of the product's code: the second end is a second turn)
    if (sat && s.m == 0xFFFFFFFFFFFFFFFFull) return Result{kInexact, 0};
    uint64_t bits = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t end = 0; end <= (sat ? 1u : 0u); end++) {
      const uint64_t b = eisel_lemire(s.m + end, q);
      if (end != 0 && b != bits) return Result{kInexact, 0};
      bits = b;
    }
    if (bits == kInfBits) return Result{kRange, 0};
    return Result{kOk, bits | sign};
  }
  if (q < -kPowerMax || q > kPowerMax) return Result{kInexact, 0};
  const double mant = static_cast<double>(s.m);
  const double v = q >= 0 ? mant * exact_power(static_cast<uint32_t>(q)) : mant / exact_power(static_cast<uint32_t>(-q));
  return Result{kOk, double_bits(v) | sign};
}
RJ_PACK_HD inline Result finish(const State& s, int kind) { return (s.flags & kWide) ? finish_as<true>(s, kind) : finish_as<false>(s, kind); }

}  // namespace numparse
}  // namespace rejit_amd
#endif
