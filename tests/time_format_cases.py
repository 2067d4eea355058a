"""What the tests of rj_scan_records_format_time share (tests/test_record_time_format.py on the CPU,
tests/test_gpu_record_time_format.py on the GPU): the MEANING of an instant under a format, written in Python independently of
rejit_amd/csrc/record_time_format.h, and the values and formats both suites ask about.

    instant   integer divmod by the unit (the floor toward minus infinity, a non-negative rest), + zone_minutes * 60 seconds
    range     the shifted seconds against 0001-01-01T00:00:00 .. 9999-12-31T23:59:59, else the row is empty
    fields    datetime(1970, 1, 1) + timedelta(seconds=...), written by hand with %04d / %02d
    layout    ob(0) = lead, ob(j + 1) = ob(j) + len(j) + gap; every other byte is the fill

cross_check() compares the hand-written fields with isoformat(), and with strftime itself for the years from 1000 on."""
import datetime
import random

OK, NULL, RANGE = "n_ok", "n_null", "n_range"
SECOND, MILLI, MICRO, NANO = range(4)
UNITS = (SECOND, MILLI, MICRO, NANO)
UNIT_NAMES = {SECOND: "s", MILLI: "ms", MICRO: "us", NANO: "ns"}
MASK = (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
EPOCH = datetime.datetime(1970, 1, 1)
FIRST_SECOND, LAST_SECOND = -62135596800, 253402300799      # 0001-01-01T00:00:00, 9999-12-31T23:59:59
MONTHS = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")
MAX_ROW = 77

ISO = b"%Y-%m-%dT%H:%M:%SZ"                # 20 bytes a row
ISO_F = b"%Y-%m-%dT%H:%M:%S.%f%z"
CLF = b"%d/%b/%Y:%H:%M:%S %z"              # 26 bytes a row
MINUTE = b"%Y-%m-%dT%H:%M"
CLOCK = b"%H:%M"                           # no date: fine to write
ODD = b"%%%Y\0%m-%d%%%f9"                  # a %% at either end, a NUL literal, %f before a digit
LONGEST = b"%Y-%b-%dT%H:%M:%S.%f%z|" + b"abcdefghijklmnopqrstuvwxyz0123456789ABCDE"      # 64 bytes; 77 bytes a row under NANO
FORMATS = (ISO, ISO_F, CLF, MINUTE, CLOCK, ODD, LONGEST)
FORMAT_IDS = ["iso", "iso_f", "clf", "minute", "clock", "odd", "longest"]
ZONES = (0, 330, -420, 1439, -1439)
assert len(LONGEST) == 64

WIDTHS = {"Y": 4, "m": 2, "d": 2, "H": 2, "M": 2, "S": 2, "b": 3, "z": 5, "%": 1}


def tokens(fmt):
    """-> the format as a list of literal bytes objects (one byte each) and directive letters (str)"""
    out, i = [], 0
    while i < len(fmt):
        if fmt[i:i + 1] == b"%":
            out.append(fmt[i + 1:i + 2].decode())
            i += 2
        else:
            out.append(fmt[i:i + 1])
            i += 1
    return out


def has(fmt, key):
    return key in [t for t in tokens(fmt) if isinstance(t, str)]


def row_length(fmt, unit):
    """L: the length of every OK row of a call"""
    return sum(1 if isinstance(t, bytes) else (3 * unit if unit else 6) if t == "f" else WIDTHS[t] for t in tokens(fmt))


def instant(value, unit, zone_minutes=0):
    """-> None when the shifted instant is outside 0001..9999, else (the naive datetime of its whole seconds, its nanoseconds)"""
    per = 10 ** (3 * unit)
    secs, rest = divmod(value, per)
    secs += zone_minutes * 60
    if not FIRST_SECOND <= secs <= LAST_SECOND:
        return None
    return EPOCH + datetime.timedelta(seconds=secs), rest * 10 ** (9 - 3 * unit)


def text_of(value, fmt, unit, zone_minutes=0):
    """the row's bytes; b"" for an instant out of range"""
    at = instant(value, unit, zone_minutes)
    if at is None:
        return b""
    dt, nanos = at
    out = b""
    for t in tokens(fmt):
        if isinstance(t, bytes):
            out += t
        elif t == "Y":
            out += b"%04d" % dt.year
        elif t in "mdHMS":
            out += b"%02d" % {"m": dt.month, "d": dt.day, "H": dt.hour, "M": dt.minute, "S": dt.second}[t]
        elif t == "b":
            out += MONTHS[dt.month - 1].encode()
        elif t == "f":
            out += b"000000" if unit == SECOND else (b"%09d" % nanos)[:3 * unit]
        elif t == "z":
            out += b"%s%02d%02d" % (b"-" if zone_minutes < 0 else b"+", abs(zone_minutes) // 60, abs(zone_minutes) % 60)
        else:
            assert t == "%"
            out += b"%"
    assert len(out) == row_length(fmt, unit) <= MAX_ROW
    return out


def cross_check(values, fmt, unit, zone_minutes):
    """the hand-written fields against isoformat(), and the whole row against strftime where Python can write it: years from
    1000 on (glibc does not pad %Y), no NUL in the format, %f only where it has Python's six digits.  -> the rows compared
    with strftime"""
    compared = 0
    tz = datetime.timezone(datetime.timedelta(minutes=zone_minutes))
    for v in values:
        at = instant(v, unit, zone_minutes)
        if at is None:
            continue
        dt, nanos = at
        assert text_of(v, b"%Y-%m-%dT%H:%M:%S", unit, zone_minutes).decode() == dt.isoformat()
        if dt.year >= 1000 and b"\0" not in fmt and (not has(fmt, "f") or unit in (SECOND, MICRO)):
            aware = dt.replace(microsecond=nanos // 1000, tzinfo=tz)
            assert text_of(v, fmt, unit, zone_minutes).decode("latin-1") == aware.strftime(fmt.decode("latin-1")), (v, fmt, unit, zone_minutes)
            compared += 1
    return compared


def layout(values, fmt, unit, status=None, indices=None, zone_minutes=0, fill=10, lead=0, gap=1):
    """-> (text, begins, ends, {n_ok, n_null, n_range})"""
    order = range(len(values)) if indices is None else indices
    out, begins, ends, counts = bytearray(bytes([fill]) * lead), [], [], {OK: 0, NULL: 0, RANGE: 0}
    for r in order:
        if status is not None and status[r] != 0:
            row, cls = b"", NULL
        else:
            row = text_of(values[r], fmt, unit, zone_minutes)
            cls = OK if row else RANGE
        counts[cls] += 1
        begins.append(len(out))
        out += row
        ends.append(len(out))
        out += bytes([fill]) * gap
    return bytes(out), begins, ends, counts


# ------------------------------------------------------------------------------------------------ the values
def seconds_of(*civil):
    return (datetime.datetime(*civil) - EPOCH) // datetime.timedelta(seconds=1)


def edge_seconds():
    """the epoch and its neighbours, both ends of the range with their outside neighbours (also as the zones +-1439 see
    them), leap days and century rules, every month end of five years"""
    out = [0, -1, 1, 59, 60, 3599, 3600, 86399, 86400, -86400, -86401, 971211336, 1792516500]
    for end in (FIRST_SECOND, LAST_SECOND):
        out += [end + d for d in (-1439 * 60 - 1, -1439 * 60, -1, 0, 1, 1439 * 60, 1439 * 60 + 1)]
    for year in (400, 1600, 1900, 2000, 2023, 2024, 2100):
        out += [seconds_of(year, 2, 28, 23, 59, 59), seconds_of(year, 2, 28, 23, 59, 59) + 1, seconds_of(year, 3, 1) - 1, seconds_of(year, 3, 1)]
        for month in range(1, 13):
            first = seconds_of(year, month, 1)
            out += [first - 1, first]
    return out


def values_of(unit, count=300, seed=26):
    """the edge seconds in `unit` with the fractions 0, 1 and per - 1, both ends of int64 and their neighbours, and seeded
    random values: over all of int64, over 0001..9999, around today.  All inside int64."""
    per = 10 ** (3 * unit)
    out = [s * per + f for s in edge_seconds() for f in sorted({0, 1, per - 1, per // 2})]
    out += [INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1]
    rng = random.Random(seed + unit)
    out += [rng.randrange(INT64_MIN, INT64_MAX + 1) for _ in range(count // 6)]
    out += [rng.randrange(FIRST_SECOND * per, (LAST_SECOND + 1) * per) for _ in range(count)]
    out += [rng.randrange(10 ** 9, 2 * 10 ** 9) * per + rng.randrange(per) for _ in range(count)]
    return [v for v in out if INT64_MIN <= v <= INT64_MAX]


def status_column(n, seed=3):
    """a parse's status column: mostly OK, every other status among the rest"""
    rng = random.Random(seed)
    return [rng.randrange(1, 5) if rng.randrange(5) == 0 else 0 for _ in range(n)]


def to_words(values):
    return [v & MASK for v in values]


def parse_round_trips(fmt, unit, zone_minutes):
    """whether rj_scan_records_parse_time reads the value back: the format names every field down to the unit, and the zone
    unless it is UTC"""
    named = all(has(fmt, k) for k in "YdHMS") and (has(fmt, "m") or has(fmt, "b")) and (unit == SECOND or has(fmt, "f"))
    return named and (zone_minutes == 0 or has(fmt, "z"))


REFUSED_FORMATS = (      # (format, the byte offset the message names) -- in writing mode
    (b"", 0), (b"%Y-%m-%d" + b" " * 57, 64), (b"%Y-%m-%d %q", 9), (b"%Y-%m-%d %y", 9), (b"%Y-%m-%d %", 9), (b"%H%", 2), (b"%Y-%m-%d %Y", 9),
    (b"%H:%H", 3), (b"%d %b %Y %m", 9), (b"%m/%d/%Y %b", 9), (b"%z%z", 2), (b"%f.%f", 3), (b"%f%f", 2))
ACCEPTED_FORMATS = (b"%H:%M:%S", b"%Y-%m", b"%b %d", b"plain", b"%f0", b"%f%S", b"%Y-%m-%d %f9", b"%f%Y-%m-%d", b"%%", b"\0", b"%Y-%m-%d" + b" " * 56, b"%z")
