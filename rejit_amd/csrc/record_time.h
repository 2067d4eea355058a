// rejit_amd/csrc/record_time.h -- the meaning of rj_scan_records_parse_time (record_time.hip): a row of a record table read as
// a TIMESTAMP under a strptime-style format -- an int64 count of seconds, milli-, micro- or nanoseconds since
// 1970-01-01T00:00:00Z --, exactly or not at all: an OK row's value is what Python's datetime.strptime makes of the same bytes
// and format, as (dt - epoch) // unit, or the row carries a status that says why it has none.  Host and device code: the CPU
// tests drive exactly these functions (tests/support/time_exec.cc), as the kernel does.
//
// A row is consumed in the 16-byte groups of record_rows.h (step), in order; the State between two groups is all that is
// kept, so the result does not depend on where a row's bytes are cut, and a row of any length costs a fixed state.
//
// The format is compiled on the host (compile) into a Program of at most 64 bytes: a literal byte stands for itself, a
// directive is the byte '%' followed by the number of its Op -- a '%' in a program always begins a directive, the literal one
// is kPercent.  A row's State holds a program counter into it; step_byte reads the program through a pointer (the kernel's
// LDS copy), never through a register array.
//
//     %Y  exactly 4 digits, 0001..9999 (0000 is RANGE)        %H %M %S  exactly 2 digits, 00..23, 00..59, 00..59 (no leap second)
//     %m  exactly 2 digits, 01..12                            %f  1 to 9 digits, as many as there are (greedy): the fraction
//     %b  exactly 3 ASCII letters, jan..dec in any case;      %z  `Z`, or [+-]DD, an optional `:`, DD: hours 00..23, minutes
//         other letters or bytes are MALFORMED                    00..59; the offset is subtracted.  Nothing behind the minutes
//     %d  exactly 2 digits, 01..the month's last day          %%  a `%`
//         (decided in finish: year and month may follow)      any other byte, NUL and blanks included: itself, exactly
// Absent fields are 0, an absent %z is UTC.  Statuses, in this order: EMPTY (no bytes left), MALFORMED (the row ends early, a
// byte does not fit its step, or bytes remain behind the last step), RANGE (a field outside its range above, or the instant
// outside int64 in the call's unit -- NANO only), INEXACT (a non-zero %f digit below the unit: the instant is not
// representable, and is never truncated or rounded).  MALFORMED outranks RANGE, so a row heading for RANGE is walked to its
// end; only a malformed row stops early (done).
//
// With kTrim the spaces and tabs before and behind the row are dropped FIRST, as in record_parse.h; without it they are
// ordinary bytes.  In a walk from byte to byte that is: blanks before the first other byte are skipped (kStart); blanks behind
// the last step are skipped (kTrail); and a blank literal that COMPLETES the program is malformed -- everything behind it
// would have to be blank too, so the trimmed row ended before it.
//
// The value: days from the civil date by the era formula (400-year eras of 146097 days, March-based years; integers only, no
// table), x 86400 + the time of day - the offset, x the units per second + the fraction.  Under NANO the seconds are compared
// with the two ends of int64 before they are multiplied.
#ifndef REJIT_AMD_RECORD_TIME_H_
#define REJIT_AMD_RECORD_TIME_H_

#include <stdint.h>

#include "record_pack.h"

namespace rejit_amd {
namespace timeparse {

// RJ_TIME_SECOND ... _NANO, RJ_PARSE_TRIM, RJ_PARSE_OK ... _INEXACT (include/rejit_hip.h)
enum Unit : int { kSecond = 0, kMilli = 1, kMicro = 2, kNano = 3, kUnits = 4 };
constexpr unsigned kTrimFlag = 1u;
enum Status : uint32_t { kOk = 0, kEmpty = 1, kMalformed = 2, kRange = 3, kInexact = 4, kStatuses = 5 };

RJ_PACK_HD inline bool unit_known(int unit) { return unit >= 0 && unit < kUnits; }
RJ_PACK_HD inline bool flags_known(unsigned flags) { return (flags & ~kTrimFlag) == 0; }

// -------------------------------------------------------------------------------------------------------------- program
constexpr uint32_t kMaxFormat = 64;
constexpr uint32_t kDirective = 0x25;   // '%'
enum Op : uint32_t { kYear = 0, kMonth = 1, kDay = 2, kHour = 3, kMinute = 4, kSecondOf = 5, kFraction = 6, kMonthName = 7, kZone = 8, kPercent = 9, kOps = 10 };

// the program's bytes as 16 little-endian words (a kernel argument that is only ever indexed by constants), and its length
struct Program {
  uint32_t words[kMaxFormat / 4];
  uint32_t len;
};
RJ_PACK_HD inline uint32_t program_byte(const Program& p, uint32_t i) { return (p.words[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

enum FormatError : int {
  kFormatOk = 0,
  kFormatEmpty,      // no bytes
  kFormatTooLong,    // more than kMaxFormat bytes                                  (at: kMaxFormat)
  kFormatUnknown,    // an unknown directive                                        (at: its '%')
  kFormatDangling,   // a '%' as the last byte                                      (at: it)
  kFormatTwice,      // a directive given twice, or %m together with %b             (at: the second one's '%')
  kFormatGreedy,     // %f directly followed by a digit literal or a digit directive (at: that byte)
  kFormatNoDate      // no %Y, no %d, or neither %m nor %b                          (at: the format's length)
};

RJ_PACK_HD inline const char* format_error_text(int e) {
  switch (e) {
    case kFormatEmpty: return "the format is empty";
    case kFormatTooLong: return "the format has more than 64 bytes";
    case kFormatUnknown: return "an unknown directive (the directives are %Y %m %b %d %H %M %S %f %z %%)";
    case kFormatDangling: return "a % as the last byte";
    case kFormatTwice: return "a directive given twice (%m and %b count as one)";
    case kFormatGreedy: return "%f directly followed by a digit: the greedy read would be ambiguous";
    case kFormatNoDate: return "the format needs %Y, %d and one of %m / %b";
    default: return "";
  }
}

// format[0, len) -> *out; on an error *at is the byte offset the message names.  `writing`: the format is compiled for
// record_time_format.h, which writes rows -- the two refusals that only make sense when reading are lifted: a writer's %f has
// a fixed width (nothing is greedy), and `%H:%M` is a fine thing to write (host code only, in both modes)
inline int compile_mode(const uint8_t* format, uint64_t len, bool writing, Program* out, uint32_t* at) {
  Program p{};
  *at = 0;
  if (len == 0) return kFormatEmpty;
  if (len > kMaxFormat) {
    *at = kMaxFormat;
    return kFormatTooLong;
  }
  uint32_t seen = 0;
  bool after_fraction = false;
  for (uint32_t i = 0; i < len; i++) {
    const uint32_t c = format[i];
    uint32_t op = kOps;
    if (c == kDirective) {
      *at = i;
      if (i + 1 == len) return kFormatDangling;
      switch (format[i + 1]) {
        case 'Y': op = kYear; break;
        case 'm': op = kMonth; break;
        case 'd': op = kDay; break;
        case 'H': op = kHour; break;
        case 'M': op = kMinute; break;
        case 'S': op = kSecondOf; break;
        case 'f': op = kFraction; break;
        case 'b': op = kMonthName; break;
        case 'z': op = kZone; break;
        case '%': op = kPercent; break;
        default: return kFormatUnknown;
      }
      if (op != kPercent) {
        const uint32_t bit = 1u << (op == kMonthName ? static_cast<uint32_t>(kMonth) : op);
        if (seen & bit) return kFormatTwice;
        seen |= bit;
      }
    }
    if (!writing && after_fraction && (op <= kFraction || (c >= '0' && c <= '9'))) {
      *at = i;
      return kFormatGreedy;
    }
    after_fraction = op == kFraction;
    p.words[i >> 2] |= c << (8 * (i & 3));
    if (op != kOps) {
      i++;
      p.words[i >> 2] |= op << (8 * (i & 3));
    }
  }
  const uint32_t date = (1u << kYear) | (1u << kMonth) | (1u << kDay);
  if (!writing && (seen & date) != date) {
    *at = static_cast<uint32_t>(len);
    return kFormatNoDate;
  }
  p.len = static_cast<uint32_t>(len);
  *out = p;
  return kFormatOk;
}
inline int compile(const uint8_t* format, uint64_t len, Program* out, uint32_t* at) { return compile_mode(format, len, false, out, at); }

// ---------------------------------------------------------------------------------------------------------------- state
enum Phase : uint32_t {
  kStart = 0,     // nothing but trimmed blanks so far
  kRun = 1,       // between two steps: pc is the next step (pc == len: accepting)
  kDigits = 2,    // inside a field of a fixed number of digits: `left` more
  kFrac = 3,      // inside %f, behind its first digit            (accepting when pc == len)
  kLetters = 4,   // inside %b: `left` more
  kZoneHours = 5, // behind the offset's sign: `left` more digits
  kZoneSep = 6,   // behind its hours: a `:` or the minutes' first digit
  kZoneMinutes = 7,
  kTrail = 8,     // trimmed blanks behind the last step          (accepting)
  kBad = 9        // malformed, whatever follows
};
enum : uint32_t { kTrim = 1u, kOffsetNeg = 2u };

// the cold fields are packed, a byte each (two digits are at most 99): a lane carries nine words through its walk
//   date   year | month << 16 | day << 24            clock   hour | minute << 8 | second << 16 | fraction digits << 24
//   zone   offset hours | offset minutes << 8 | flags << 16 | the field being read << 24
struct State {
  uint32_t pc, left, acc, phase, nanos, letters, date, clock, zone;
};
RJ_PACK_HD inline uint32_t year_of(const State& s) { return s.date & 0xFFFFu; }
RJ_PACK_HD inline uint32_t month_of_state(const State& s) { return (s.date >> 16) & 0xFFu; }
RJ_PACK_HD inline uint32_t day_of(const State& s) { return s.date >> 24; }
RJ_PACK_HD inline uint32_t hour_of(const State& s) { return s.clock & 0xFFu; }
RJ_PACK_HD inline uint32_t minute_of(const State& s) { return (s.clock >> 8) & 0xFFu; }
RJ_PACK_HD inline uint32_t second_of(const State& s) { return (s.clock >> 16) & 0xFFu; }
RJ_PACK_HD inline uint32_t fraction_digits(const State& s) { return s.clock >> 24; }
RJ_PACK_HD inline uint32_t offset_hours(const State& s) { return s.zone & 0xFFu; }
RJ_PACK_HD inline uint32_t offset_minutes(const State& s) { return (s.zone >> 8) & 0xFFu; }
RJ_PACK_HD inline uint32_t flags_of(const State& s) { return (s.zone >> 16) & 0xFFu; }
RJ_PACK_HD inline State start(unsigned flags) {
  State s{};
  s.phase = kStart;
  if (flags & kTrimFlag) s.zone = kTrim << 16;
  return s;
}
RJ_PACK_HD inline bool done(const State& s) { return s.phase == kBad; }

// jan..dec as three lower-case letters -> 1..12; 0: no month
RJ_PACK_HD inline uint32_t month_of(uint32_t letters) {
  switch (letters) {
    case 0x6A616E: return 1;    // jan
    case 0x666562: return 2;    // feb
    case 0x6D6172: return 3;    // mar
    case 0x617072: return 4;    // apr
    case 0x6D6179: return 5;    // may
    case 0x6A756E: return 6;    // jun
    case 0x6A756C: return 7;    // jul
    case 0x617567: return 8;    // aug
    case 0x736570: return 9;    // sep
    case 0x6F6374: return 10;   // oct
    case 0x6E6F76: return 11;   // nov
    case 0x646563: return 12;   // dec
    default: return 0;
  }
}

// a fixed field's digits are complete (every field is read at most once: its bits are still zero)
RJ_PACK_HD inline void store_field(State& s) {
  const uint32_t v = s.acc, field = s.zone >> 24;
  const uint32_t placed = v << (field == kYear || field == kHour ? 0 : field == kMinute ? 8 : field == kMonth || field == kSecondOf ? 16 : 24);
  s.date |= field <= kDay ? placed : 0u;
  s.clock |= field <= kDay ? 0u : placed;
}

// ---------------------------------------------------------------------------------------------------------------- step
// one byte of the row; code[0, len) is the program
RJ_PACK_HD inline void step_byte(State& s, const uint8_t* code, uint32_t len, uint32_t c) {
  const uint32_t d = c - 0x30u;
  const bool blank = (c == 0x20u || c == 0x09u) && (flags_of(s) & kTrim);
  uint32_t ph = s.phase;
  if (ph == kStart) {
    if (blank) return;
    ph = kRun;
  }
  if (ph == kFrac) {
    if (d <= 9u && fraction_digits(s) < 9) {
      s.nanos = s.nanos * 10 + d;
      s.clock += 1u << 24;
      return;
    }
    ph = kRun;   // the fraction ends before this byte: it belongs to the next step
  }
  switch (ph) {
    case kRun: {
      if (s.pc >= len) {
        s.phase = blank ? kTrail : kBad;
        return;
      }
      const uint32_t x = code[s.pc];
      if (x != kDirective) {   // a literal; a blank one that completes the program lies behind the trimmed row's end
        s.pc++;
        s.phase = (c == x && !(blank && s.pc == len)) ? kRun : kBad;
        return;
      }
      const uint32_t op = code[s.pc + 1];
      s.pc += 2;
      if (op <= kSecondOf) {
        s.zone = (s.zone & 0x00FFFFFFu) | op << 24;
        s.left = op == kYear ? 3 : 1;
        s.acc = d;
        s.phase = d <= 9u ? kDigits : kBad;
      } else if (op == kFraction) {
        s.nanos = d;
        s.clock |= 1u << 24;
        s.phase = d <= 9u ? kFrac : kBad;
      } else if (op == kMonthName) {
        const uint32_t l = c | 0x20u;
        s.letters = l;
        s.left = 2;
        s.phase = l - 0x61u < 26u ? kLetters : kBad;
      } else if (op == kZone) {
        if (c == 0x5Au) {   // Z
          s.phase = kRun;
        } else if (c == 0x2Bu || c == 0x2Du) {
          if (c == 0x2Du) s.zone |= kOffsetNeg << 16;
          s.left = 2;
          s.acc = 0;
          s.phase = kZoneHours;
        } else {
          s.phase = kBad;
        }
      } else {
        s.phase = c == kDirective ? kRun : kBad;
      }
      return;
    }
    case kDigits:
      if (d > 9u) {
        s.phase = kBad;
        return;
      }
      s.acc = s.acc * 10 + d;
      if (--s.left == 0) {
        store_field(s);
        s.phase = kRun;
      }
      return;
    case kLetters: {
      const uint32_t l = c | 0x20u;
      if (l - 0x61u >= 26u) {
        s.phase = kBad;
        return;
      }
      s.letters = s.letters << 8 | l;
      if (--s.left == 0) {
        const uint32_t m = month_of(s.letters);
        s.date |= m << 16;
        s.phase = m ? kRun : kBad;
      }
      return;
    }
    case kZoneSep:
      if (c == 0x3Au) {   // :
        s.left = 2;
        s.acc = 0;
        s.phase = kZoneMinutes;
        return;
      }
      if (d > 9u) {
        s.phase = kBad;
        return;
      }
      s.left = 1;
      s.acc = d;
      s.phase = kZoneMinutes;
      return;
    case kZoneHours:
    case kZoneMinutes:
      if (d > 9u) {
        s.phase = kBad;
        return;
      }
      s.acc = s.acc * 10 + d;
      if (--s.left == 0) {
        if (ph == kZoneHours) s.zone |= s.acc, s.phase = kZoneSep;
        else s.zone |= s.acc << 8, s.phase = kRun;
      }
      return;
    case kTrail:
      if (!blank) s.phase = kBad;
      return;
    default:
      s.phase = kBad;
      return;
  }
}

// the first `valid` (1..16) bytes of a group of rows::load_group, in order.  ONE copy of step_byte in a loop over the bytes
// (the word is picked by selects, not by an indexed register): sixteen inlined copies cost the kernel twice the registers.
RJ_PACK_HD inline void step(State& s, const uint8_t* code, uint32_t len, const uint32_t w[4], uint32_t valid) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t b = 0; b < valid && s.phase != kBad; b++) {
    const uint32_t i = b >> 2;
    const uint32_t x = i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3];
    step_byte(s, code, len, (x >> (8 * (b & 3))) & 0xFFu);
  }
}

// ---------------------------------------------------------------------------------------------------------------- finish
struct Result {
  uint32_t status;
  uint64_t bits;   // the int64's; 0 unless status == kOk
};

RJ_PACK_HD inline bool leap_year(uint32_t y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }
RJ_PACK_HD inline uint32_t days_in_month(uint32_t y, uint32_t m) {   // 1 <= m <= 12
  return m == 2 ? (leap_year(y) ? 29u : 28u) : 30u + ((m + (m >> 3)) & 1u);
}
// days since 1970-01-01 of the proleptic Gregorian y-m-d, 1 <= y: years begin in March, eras have 400 of them
RJ_PACK_HD inline int64_t days_from_civil(uint32_t y, uint32_t m, uint32_t d) {
  y -= m <= 2 ? 1u : 0u;
  const uint32_t era = y / 400, yoe = y - era * 400;
  const uint32_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
  const uint32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return static_cast<int64_t>(era) * 146097 + static_cast<int64_t>(doe) - 719468;
}

constexpr int64_t kNanoMaxSeconds = 9223372036;    // 2^63 - 1 = kNanoMaxSeconds x 10^9 + kNanoMaxRest
constexpr uint32_t kNanoMaxRest = 854775807;
constexpr int64_t kNanoMinSeconds = -9223372037;   // -2^63 = kNanoMinSeconds x 10^9 + kNanoMinRest
constexpr uint32_t kNanoMinRest = 145224192;

RJ_PACK_HD inline Result finish(const State& s, uint32_t len, int unit) {
  if (s.phase == kStart) return Result{kEmpty, 0};
  if (!((s.phase == kRun || s.phase == kFrac || s.phase == kTrail) && s.pc == len)) return Result{kMalformed, 0};
  const uint32_t y = year_of(s), m = month_of_state(s), d = day_of(s);
  if (y == 0 || m < 1 || m > 12 || d < 1 || d > days_in_month(y, m) || hour_of(s) > 23 || minute_of(s) > 59 || second_of(s) > 59 || offset_hours(s) > 23 ||
      offset_minutes(s) > 59)
    return Result{kRange, 0};
  const int64_t offset = static_cast<int64_t>(offset_hours(s) * 3600 + offset_minutes(s) * 60);
  const int64_t secs = days_from_civil(y, m, d) * 86400 + static_cast<int64_t>(hour_of(s) * 3600 + minute_of(s) * 60 + second_of(s)) -
                       ((flags_of(s) & kOffsetNeg) ? -offset : offset);
  uint32_t nanos = s.nanos;
  for (uint32_t i = fraction_digits(s); i < 9 && nanos != 0; i++) nanos *= 10;
  if (unit == kNano) {
    if (secs > kNanoMaxSeconds || (secs == kNanoMaxSeconds && nanos > kNanoMaxRest) || secs < kNanoMinSeconds ||
        (secs == kNanoMinSeconds && nanos < kNanoMinRest))
      return Result{kRange, 0};
    return Result{kOk, static_cast<uint64_t>(secs) * 1000000000ull + nanos};   // (two's complement: the sum is inside int64)
  }
  // units per second, and the fraction in units and what lies below them (divisions by constants, one per unit)
  uint32_t per = 1, whole = 0, rest = nanos;
  if (unit == kMilli) per = 1000u, whole = nanos / 1000000u, rest = nanos % 1000000u;
  if (unit == kMicro) per = 1000000u, whole = nanos / 1000u, rest = nanos % 1000u;
  if (rest != 0) return Result{kInexact, 0};
  return Result{kOk, static_cast<uint64_t>(secs * static_cast<int64_t>(per) + static_cast<int64_t>(whole))};
}

}  // namespace timeparse
}  // namespace rejit_amd
#endif
