// rejit_amd/csrc/record_time_format.h -- the meaning of rj_scan_records_format_time (record_time_format.hip): a column of int64
// INSTANTS -- counts of seconds, milli-, micro- or nanoseconds since 1970-01-01T00:00:00Z -- written as TEXT under a
// strftime-style format, the inverse of record_time.h.  Host and device code: the CPU tests drive exactly these functions
// (tests/support/time_format_exec.cc), as the kernels do.
//
// The instant: floor(value / units per second) seconds -- the floor toward minus infinity, so -1 ns is
// 1969-12-31T23:59:59.999999999 -- and a non-negative rest; the seconds shifted by the call's fixed offset (zone_minutes,
// -1439..1439), then split into the civil fields by the inverse of timeparse::days_from_civil: the 400-year-era formula in
// integers, no table of years (split, civil_from_days).  The divisors are compile-time constants (split<unit>); behind the
// range check everything is 32-bit arithmetic.
//
// The format is compiled by timeparse::compile_mode in its writing mode (the parse's own directives and refusals, less the
// two that only make sense when reading), and then, still on the host, into a LAYOUT of L <= 77 entries (make_layout): every
// directive has a fixed width, so every OK row of a call has the same length L and byte i of every row comes from the same
// place -- entry i is either a literal byte or an index into the row's Source, 32 bytes of ASCII made once per row:
//
//     %Y  4 digits, zero-padded (0001..9999)      %H %M %S  2 digits each         %z  +hhmm / -hhmm of zone_minutes, +0000 for 0
//     %m %d  2 digits each                        %f  the unit's fraction digits: 3 under MILLI, 6 under MICRO, 9 under NANO,
//     %b  Jan..Dec                                    six zeros under SECOND      %%  a `%`        any other byte: itself
//
// %z, %%, the zeros of %f under SECOND and the literals are literal entries; the rest are Source entries.  char_at is one table
// read and one byte extraction: no per-lane program counter, no phase dispatch.  Fields the format does not name are dropped
// (a floor to the finest named field), as strftime drops them.
//
// An OK row is, byte for byte, what Python's datetime.strftime writes for the same instant and format -- but for %Y, which is
// isoformat()'s four digits here: on glibc datetime(1, 1, 1).strftime('%Y') is '1', not '0001' --, and %f under NANO / MILLI
// writes 9 / 3 digits where Python's datetime has microseconds only.  A row is the EMPTY row (zero bytes) when its status is
// not OK (null_row), or when the SHIFTED instant's year is outside 0001..9999 (kOutOfRange: never a nearby or wrapped value).
// Only SECOND, MILLI and MICRO can produce the latter: every int64 under NANO lies inside 1677..2262.
#ifndef REJIT_AMD_RECORD_TIME_FORMAT_H_
#define REJIT_AMD_RECORD_TIME_FORMAT_H_

#include <stdint.h>

#include "record_pack.h"
#include "record_rows.h"
#include "record_time.h"

// (forced inline on the device: a Source handed to a function that is not inlined would live in scratch memory)
#if defined(__HIPCC__)
#define RJ_TIMEFORMAT_HD __host__ __device__ __forceinline__
#else
#define RJ_TIMEFORMAT_HD inline
#endif

namespace rejit_amd {
namespace timeformat {

constexpr uint32_t kStatusOk = timeparse::kOk;   // RJ_PARSE_OK: every other status makes the row empty
constexpr int kMaxZoneMinutes = 1439;
RJ_TIMEFORMAT_HD bool zone_known(int zone_minutes) { return zone_minutes >= -kMaxZoneMinutes && zone_minutes <= kMaxZoneMinutes; }
RJ_TIMEFORMAT_HD bool flags_known(unsigned flags) { return flags == 0; }

// ---------------------------------------------------------------------------------------------------------------- widths
constexpr uint32_t kWidthYear = 4, kWidthTwo = 2, kWidthName = 3, kWidthFraction = 9, kWidthZone = 5, kWidthPercent = 1;
constexpr uint32_t kSecondFractionZeros = 6;   // %f under SECOND: Python's microseconds, all zero
// The longest row.  A directive takes two bytes of the format and can stand in it once (%% any number of times, but it
// SHRINKS: one byte for two), so a format gains width - 2 per directive, and only %Y, %b, %f (under NANO) and %z gain: the
// 64 bytes of the longest format, + 2 + 1 + 7 + 3.
constexpr uint32_t kMaxRowBytes = 77;
static_assert(kMaxRowBytes == timeparse::kMaxFormat + (kWidthYear - 2) + (kWidthName - 2) + (kWidthFraction - 2) + (kWidthZone - 2), "the longest row");
static_assert(kWidthTwo == 2 && kWidthPercent < 2 && kSecondFractionZeros <= kWidthFraction, "no other directive gains");

// rows advance the output by at most kMaxRowBytes + gap: the plan's look-back carries pack::kMaxRow per row, pack::kMaxTotal in all
RJ_TIMEFORMAT_HD bool sums_fit(uint64_t k, uint64_t lead, uint64_t gap) { return pack::sums_fit(k, kMaxRowBytes, lead, gap); }

// what rj_scan_records_format_time refuses before it launches anything, in this order (the format is compiled between kBadFill and
// kBadSums; the first bad index is found by the check kernel)
enum Refusal : int { kFine = 0, kNullArgument, kTableAlign, kOutAlign, kBadUnit, kBadZone, kBadFlags, kBadFill, kBadSums, kTooManyRows };
RJ_TIMEFORMAT_HD Refusal check_arguments(const void* value, uint64_t n_values, const void* indices, const void* format, uint64_t format_len, int unit,
                                         int zone_minutes, unsigned flags, int fill, const void* out, uint64_t out_cap, const void* out_begin,
                                         const void* out_end) {
  if ((!value && n_values) || (!out && out_cap) || (!format && format_len)) return kNullArgument;
  if ((reinterpret_cast<uintptr_t>(value) | reinterpret_cast<uintptr_t>(indices) | reinterpret_cast<uintptr_t>(out_begin) |
       reinterpret_cast<uintptr_t>(out_end)) & 7u)
    return kTableAlign;
  if (reinterpret_cast<uintptr_t>(out) & 15u) return kOutAlign;
  if (!timeparse::unit_known(unit)) return kBadUnit;
  if (!zone_known(zone_minutes)) return kBadZone;
  if (!flags_known(flags)) return kBadFlags;
  if (fill < 0 || fill > 255) return kBadFill;
  return kFine;
}
RJ_TIMEFORMAT_HD Refusal check_sizes(uint64_t k, uint64_t lead, uint64_t gap) {
  if (!sums_fit(k, lead, gap)) return kBadSums;
  if (!rows::rows_fit(k)) return kTooManyRows;
  return kFine;
}

// ---------------------------------------------------------------------------------------------------------------- layout
// The row's Source: 32 bytes of ASCII, made once per row (unfold).  A layout entry with kSource set names one of its bytes.
//     [0, 8)  YYYYMMDD      [8, 16)  00HHMMSS      [16, 19)  the month's name      [23, 32)  the nine digits of the nanoseconds
enum : uint32_t { kSrcYear = 0, kSrcMonth = 4, kSrcDay = 6, kSrcHour = 10, kSrcMinute = 12, kSrcSecond = 14, kSrcName = 16, kSrcFraction = 23, kSourceBytes = 32 };
constexpr uint32_t kSource = 0x100u;   // entry: kSource | index into the Source, or a literal byte
constexpr uint32_t kLayoutWords = 40;  // 80 entries of 16 bits
static_assert(kLayoutWords * 2 >= kMaxRowBytes, "the layout holds the longest row");

// the entries as 40 little-endian words (a kernel argument that is only ever indexed by constants), and the rows' length L
struct Layout {
  uint32_t words[kLayoutWords];
  uint32_t len;
};
RJ_TIMEFORMAT_HD uint32_t layout_entry(const Layout& l, uint32_t i) { return (l.words[i >> 1] >> (16 * (i & 1))) & 0xFFFFu; }

// the fraction digits %f writes from the Source under `unit` (under SECOND it writes zeros instead)
RJ_TIMEFORMAT_HD uint32_t fraction_digits(int unit) { return 3u * static_cast<uint32_t>(unit); }

// a program compiled in writing mode -> the layout of the rows it writes under `unit` and `zone_minutes`
inline Layout make_layout(const timeparse::Program& p, int unit, int zone_minutes) {
  Layout l{};
  const auto put = [&l](uint32_t entry) {
    if (l.len < 2 * kLayoutWords) l.words[l.len >> 1] |= entry << (16 * (l.len & 1));   // (always: kMaxRowBytes)
    l.len++;
  };
  const auto put_source = [&put](uint32_t from, uint32_t count) {
    for (uint32_t i = 0; i < count; i++) put(kSource | (from + i));
  };
  for (uint32_t i = 0; i < p.len; i++) {
    const uint32_t x = timeparse::program_byte(p, i);
    if (x != timeparse::kDirective) {
      put(x);
      continue;
    }
    switch (timeparse::program_byte(p, ++i)) {
      case timeparse::kYear: put_source(kSrcYear, kWidthYear); break;
      case timeparse::kMonth: put_source(kSrcMonth, kWidthTwo); break;
      case timeparse::kDay: put_source(kSrcDay, kWidthTwo); break;
      case timeparse::kHour: put_source(kSrcHour, kWidthTwo); break;
      case timeparse::kMinute: put_source(kSrcMinute, kWidthTwo); break;
      case timeparse::kSecondOf: put_source(kSrcSecond, kWidthTwo); break;
      case timeparse::kMonthName: put_source(kSrcName, kWidthName); break;
      case timeparse::kFraction:
        if (unit == timeparse::kSecond) {
          for (uint32_t z = 0; z < kSecondFractionZeros; z++) put(0x30u);
        } else {
          put_source(kSrcFraction, fraction_digits(unit));
        }
        break;
      case timeparse::kZone: {
        const uint32_t minutes = static_cast<uint32_t>(zone_minutes < 0 ? -zone_minutes : zone_minutes);
        put(zone_minutes < 0 ? 0x2Du : 0x2Bu);
        put(0x30u + minutes / 600);
        put(0x30u + minutes / 60 % 10);
        put(0x30u + minutes % 60 / 10);
        put(0x30u + minutes % 10);
        break;
      }
      default: put(timeparse::kDirective); break;   // kPercent
    }
  }
  return l;
}

// ---------------------------------------------------------------------------------------------------------------- the instant
constexpr int64_t kFirstSecond = -62135596800ll;   // 0001-01-01T00:00:00
constexpr int64_t kLastSecond = 253402300799ll;    // 9999-12-31T23:59:59
constexpr uint32_t kEpochDay = 719162;             // 1970-01-01, in days since 0001-01-01
static_assert(kFirstSecond == -static_cast<int64_t>(kEpochDay) * 86400, "the first second");

struct Civil {
  uint32_t year, month, day;
};
// the proleptic Gregorian date of a day counted from 0001-01-01 (day 0), up to 9999-12-31: the inverse of
// timeparse::days_from_civil -- eras of 400 March-based years (146097 days) from 0000-03-01, 306 days before day 0
RJ_TIMEFORMAT_HD Civil civil_from_days(uint32_t days) {
  const uint32_t z = days + 306;
  const uint32_t era = z / 146097, doe = z - era * 146097;
  const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const uint32_t mp = (5 * doy + 2) / 153;
  const uint32_t day = doy - (153 * mp + 2) / 5 + 1;
  const uint32_t month = mp < 10 ? mp + 3 : mp - 9;
  return Civil{yoe + era * 400 + (month <= 2 ? 1u : 0u), month, day};
}

// A row as it is staged between the plan and the emit, 16 bytes:
//   packed  year * 10000 + month * 100 + day | (hour * 10000 + minute * 100 + second) << 27 | month << 45 | class << 49
//   nanos   the nanoseconds of the second, 0..999999999
enum Class : uint32_t { kNull = 0, kOk = 1, kOutOfRange = 2, kClasses = 3 };
struct Fields {
  uint64_t packed, nanos;
};
RJ_TIMEFORMAT_HD uint32_t class_of(const Fields& f) { return static_cast<uint32_t>(f.packed >> 49) & 3u; }
RJ_TIMEFORMAT_HD Fields null_row() { return Fields{static_cast<uint64_t>(kNull) << 49, 0}; }
// the row's length under a layout of L bytes
RJ_TIMEFORMAT_HD uint32_t row_len(const Fields& f, uint32_t L) { return class_of(f) == kOk ? L : 0u; }

// value (the int64's bits, a count of kUnit) shifted by zone_seconds -> its fields, or kOutOfRange
template <int kUnit>
RJ_TIMEFORMAT_HD Fields split(uint64_t bits, int32_t zone_seconds) {
  constexpr int64_t per = kUnit == timeparse::kSecond ? 1 : kUnit == timeparse::kMilli ? 1000 : kUnit == timeparse::kMicro ? 1000000 : 1000000000;
  const int64_t value = static_cast<int64_t>(bits);
  int64_t secs = value / per, rest = value - secs * per;   // (truncated; |secs * per| <= |value|)
  if (rest < 0) secs -= 1, rest += per;                    // the floor toward minus infinity
  // the range is judged on the SHIFTED instant; the bounds move, not the value (which may sit at an end of int64)
  if (secs < kFirstSecond - zone_seconds || secs > kLastSecond - zone_seconds) return Fields{static_cast<uint64_t>(kOutOfRange) << 49, 0};
  const uint64_t since = static_cast<uint64_t>(secs + zone_seconds - kFirstSecond);   // seconds since 0001-01-01: below 2^39
  const uint32_t days = static_cast<uint32_t>(since >> 7) / 675u;                       // / 86400 = / 128 / 675, in 32 bits
  const uint32_t of_day = static_cast<uint32_t>(since - static_cast<uint64_t>(days) * 86400u);
  const Civil c = civil_from_days(days);
  const uint32_t hour = of_day / 3600, minute = of_day / 60 % 60, second = of_day % 60;
  const uint64_t ymd = c.year * 10000 + c.month * 100 + c.day, hms = hour * 10000 + minute * 100 + second;
  return Fields{ymd | hms << 27 | static_cast<uint64_t>(c.month) << 45 | static_cast<uint64_t>(kOk) << 49,
                static_cast<uint64_t>(rest) * static_cast<uint64_t>(1000000000 / per)};
}
// ... for a unit known at run time only (host code, the tests)
RJ_TIMEFORMAT_HD Fields split_unit(uint64_t bits, int unit, int32_t zone_seconds) {
  switch (unit) {
    case timeparse::kSecond: return split<timeparse::kSecond>(bits, zone_seconds);
    case timeparse::kMilli: return split<timeparse::kMilli>(bits, zone_seconds);
    case timeparse::kMicro: return split<timeparse::kMicro>(bits, zone_seconds);
    default: return split<timeparse::kNano>(bits, zone_seconds);
  }
}

// ---------------------------------------------------------------------------------------------------------------- rows
// x < 10^8 as eight ASCII digits, the first one in the lowest byte
RJ_TIMEFORMAT_HD uint64_t digits8(uint32_t x) {
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
constexpr uint32_t name3(char a, char b, char c) {
  return static_cast<uint32_t>(static_cast<uint8_t>(a)) | static_cast<uint32_t>(static_cast<uint8_t>(b)) << 8 | static_cast<uint32_t>(static_cast<uint8_t>(c)) << 16;
}
// Jan..Dec, the first letter in the lowest byte; 1 <= month <= 12
RJ_TIMEFORMAT_HD uint32_t month_name(uint32_t month) {
  switch (month) {
    case 1: return name3('J', 'a', 'n');
    case 2: return name3('F', 'e', 'b');
    case 3: return name3('M', 'a', 'r');
    case 4: return name3('A', 'p', 'r');
    case 5: return name3('M', 'a', 'y');
    case 6: return name3('J', 'u', 'n');
    case 7: return name3('J', 'u', 'l');
    case 8: return name3('A', 'u', 'g');
    case 9: return name3('S', 'e', 'p');
    case 10: return name3('O', 'c', 't');
    case 11: return name3('N', 'o', 'v');
    default: return name3('D', 'e', 'c');
  }
}

// the 32 bytes of an OK row's Source as four words
struct Source {
  uint64_t a, b, c, d;
};
RJ_TIMEFORMAT_HD Source unfold(const Fields& f) {
  const uint32_t ymd = static_cast<uint32_t>(f.packed) & 0x7FFFFFFu, hms = static_cast<uint32_t>(f.packed >> 27) & 0x3FFFFu;
  const uint32_t month = static_cast<uint32_t>(f.packed >> 45) & 15u, nanos = static_cast<uint32_t>(f.nanos);
  return Source{digits8(ymd), digits8(hms), month_name(month) | static_cast<uint64_t>(0x30u + nanos / 100000000u) << 56, digits8(nanos % 100000000u)};
}
// byte `index` of the Source, index < kSourceBytes
RJ_TIMEFORMAT_HD uint32_t source_byte(const Source& s, uint32_t index) {
  // (masks, not a chain of selects: the compiler turns that chain into an indexed load of {a, b, c, d} from scratch memory)
  const uint32_t word = index >> 3;
  const uint64_t in_a = 0 - static_cast<uint64_t>(word == 0), in_b = 0 - static_cast<uint64_t>(word == 1), in_c = 0 - static_cast<uint64_t>(word == 2),
                 in_d = 0 - static_cast<uint64_t>(word == 3);
  const uint64_t w = (s.a & in_a) | (s.b & in_b) | (s.c & in_c) | (s.d & in_d);
  return static_cast<uint32_t>(w >> (8 * (index & 7))) & 0xFFu;
}
// the row's byte whose layout entry is `entry`: one table read (the caller's) and one extraction
RJ_TIMEFORMAT_HD uint32_t char_at(const Source& s, uint32_t entry) { return (entry & kSource) ? source_byte(s, entry & (kSourceBytes - 1)) : (entry & 0xFFu); }

// (record_pack.h's chunk_part under this header's name: one definition, the name its callers have always used)
using pack::chunk_part;

}  // namespace timeformat
}  // namespace rejit_amd
#endif
