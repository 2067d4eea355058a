"""What the tests of rj_scan_records_parse_time share (tests/test_record_time.py on the CPU, tests/test_gpu_record_time.py on
the GPU): the MEANING of a row under a format, written in Python independently of rejit_amd/csrc/record_time.h, and the rows
both suites ask about.

    grammar   an `re` pattern built from the format, fullmatch over the row's bytes (trimmed of spaces and tabs first under
              TRIM): %Y [0-9]{4}, %m %d %H %M %S [0-9]{2}, %b [A-Za-z]{3} and then one of jan..dec, %f [0-9]{1,9},
              %z Z|[+-][0-9]{2}:?[0-9]{2}, every other byte itself
    ranges    calendar.monthrange for the day (not strptime), the plain bounds for the rest; the offset's hours and minutes
    instant   datetime / timedelta integer arithmetic -> whole seconds; x 10^9 + the fraction's nanoseconds, a Python int
    then      the int64 range in the call's unit, then the digits below the unit (INEXACT)

cross_check() compares this meaning with datetime.strptime itself."""
import calendar
import datetime
import random
import re

from parse_cases import lay  # noqa: F401  (the suites lay their rows with it)

OK, EMPTY, MALFORMED, RANGE, INEXACT = range(5)
SECOND, MILLI, MICRO, NANO = range(4)
UNITS = (SECOND, MILLI, MICRO, NANO)
UNIT_NAMES = {SECOND: "s", MILLI: "ms", MICRO: "us", NANO: "ns"}
MASK = (1 << 64) - 1

ISO = b"%Y-%m-%dT%H:%M:%S%z"
ISO_F = b"%Y-%m-%dT%H:%M:%S.%f%z"
CLF = b"%d/%b/%Y:%H:%M:%S %z"
PLAIN = b"%Y/%m/%d %H:%M:%S"
DATE = b"%Y-%m-%d"
ODD = b"%%%Y\0%m-%d%%"                     # a %% at either end and a NUL literal
FORMATS = (ISO, ISO_F, CLF, PLAIN, DATE, ODD)

MONTHS = ("jan", "feb", "mar", "apr", "may", "jun", "jul", "aug", "sep", "oct", "nov", "dec")
_PIECES = {b"Y": rb"(?P<Y>[0-9]{4})", b"m": rb"(?P<m>[0-9]{2})", b"d": rb"(?P<d>[0-9]{2})", b"H": rb"(?P<H>[0-9]{2})", b"M": rb"(?P<M>[0-9]{2})",
           b"S": rb"(?P<S>[0-9]{2})", b"b": rb"(?P<b>[A-Za-z]{3})", b"f": rb"(?P<f>[0-9]{1,9})", b"z": rb"(?P<z>Z|[+-][0-9]{2}:?[0-9]{2})", b"%": rb"%"}
_patterns = {}
EPOCH = datetime.datetime(1970, 1, 1)


def pattern_of(fmt):
    if fmt not in _patterns:
        out, i = b"", 0
        while i < len(fmt):
            if fmt[i:i + 1] == b"%":
                out += _PIECES[fmt[i + 1:i + 2]]
                i += 2
            else:
                out += re.escape(fmt[i:i + 1])
                i += 1
        _patterns[fmt] = re.compile(out, re.DOTALL)
    return _patterns[fmt]


def fields_of(row, fmt, trim):
    """-> None (no bytes left), False (not in the grammar), or the match's groups as a dict of bytes"""
    s = row.strip(b" \t") if trim else row
    if not s:
        return None
    mt = pattern_of(fmt).fullmatch(s)
    if not mt:
        return False
    g = {k: v for k, v in mt.groupdict().items() if v is not None}
    if "b" in g and g["b"].decode("ascii").lower() not in MONTHS:
        return False
    return g


def meaning(row, fmt, unit, trim):
    """-> (status, the 64 bits of the int64 value; 0 unless status is OK)"""
    g = fields_of(row, fmt, trim)
    if g is None:
        return EMPTY, 0
    if g is False:
        return MALFORMED, 0
    num = lambda k: int(g.get(k, b"0"))
    year, day, hour, minute, second = num("Y"), num("d"), num("H"), num("M"), num("S")
    month = MONTHS.index(g["b"].decode("ascii").lower()) + 1 if "b" in g else num("m")
    sign, off_h, off_m = 1, 0, 0
    if "z" in g and g["z"] != b"Z":
        z = g["z"].replace(b":", b"")
        sign, off_h, off_m = (-1 if z[:1] == b"-" else 1), int(z[1:3]), int(z[3:5])
    if not (1 <= year <= 9999 and 1 <= month <= 12 and 1 <= day <= calendar.monthrange(year, month)[1] and hour <= 23 and minute <= 59 and second <= 59
            and off_h <= 23 and off_m <= 59):
        return RANGE, 0
    delta = datetime.datetime(year, month, day, hour, minute, second) - EPOCH - sign * datetime.timedelta(hours=off_h, minutes=off_m)
    assert delta.microseconds == 0
    total = (delta.days * 86400 + delta.seconds) * 10 ** 9 + int(g.get("f", b"0").ljust(9, b"0"))
    if unit == NANO and not -(1 << 63) <= total < (1 << 63):
        return RANGE, 0
    below = 10 ** (9 - 3 * unit)
    if total % below:
        return INEXACT, 0
    return OK, (total // below) & MASK


def english_months():
    return [datetime.date(2001, m, 1).strftime("%b").lower() for m in range(1, 13)] == list(MONTHS)


def cross_check(rows, fmt, unit, trim):
    """Every OK row with at most 6 %f digits has datetime.strptime's value, as (dt - epoch) // unit; every row strptime
    rejects is not OK here (but for %f with 7 to 9 digits, which strptime does not read).  -> the number of rows compared by
    value; None when LC_TIME's month names are not the English ones (the caller skips)."""
    if not english_months():
        return None
    py_fmt = fmt.decode("latin-1")
    aware = b"%z" in fmt
    epoch = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc) if aware else EPOCH
    per = datetime.timedelta(microseconds=10 ** (6 - 3 * unit)) if unit != NANO else None
    compared = 0
    for row in rows:
        status, bits = meaning(row, fmt, unit, trim)
        g = fields_of(row, fmt, trim)
        long_fraction = bool(g) and len(g.get("f", b"")) > 6
        s = (row.strip(b" \t") if trim else row).decode("latin-1")
        try:
            dt = datetime.datetime.strptime(s, py_fmt)
        except ValueError:
            assert status != OK or long_fraction, (row, fmt, unit, trim)
            continue
        if status == OK and not long_fraction:
            delta = dt - epoch
            want = (delta // datetime.timedelta(microseconds=1)) * 1000 if unit == NANO else delta // per
            assert bits == want & MASK, (row, fmt, unit, trim, bits, want)
            compared += 1
    return compared


# ------------------------------------------------------------------------------------------------ the rows
PARTS = {"Y": b"2000", "m": b"10", "b": b"Oct", "d": b"10", "H": b"13", "M": b"55", "S": b"36", "f": b"123", "z": b"+05:30"}


def render(fmt, **parts):
    """the format with every directive replaced by its part (bytes; PARTS unless given)"""
    out, i = b"", 0
    while i < len(fmt):
        if fmt[i:i + 1] == b"%":
            key = fmt[i + 1:i + 2].decode()
            out += b"%" if key == "%" else parts.get(key, PARTS[key])
            i += 2
        else:
            out += fmt[i:i + 1]
            i += 1
    return out


def has(fmt, key):
    return (b"%" + key.encode()) in fmt.replace(b"%%", b"")


def of_instant(fmt, dt, fraction=b"0", zone=b"Z"):
    """the row of the civil fields of `dt` (a naive datetime) with the given fraction digits and zone text"""
    return render(fmt, Y=b"%04d" % dt.year, m=b"%02d" % dt.month, b=MONTHS[dt.month - 1].capitalize().encode(), d=b"%02d" % dt.day, H=b"%02d" % dt.hour,
                  M=b"%02d" % dt.minute, S=b"%02d" % dt.second, f=fraction, z=zone)


def status_rows(fmt):
    """rows of every status: good ones, cut short at every length, one byte too long, every digit replaced by a letter, the
    zone's wrong spellings, month names, field ranges, fractions, blanks"""
    good = render(fmt)
    rows = [good, b""]
    rows += [good[:i] for i in range(1, len(good))]                                      # cut short at every length
    rows += [good + c for c in (b"0", b"x", b" ", b"\0", b"Z", b":")]                    # one byte too long
    rows += [good[:i] + b"x" + good[i + 1:] for i in range(len(good)) if good[i:i + 1].isdigit()]      # a letter for every digit
    rows += [good[:i] + b"\xb1" + good[i + 1:] for i in range(0, len(good), 3)]
    if has(fmt, "z"):
        rows += [render(fmt, z=z) for z in (b"Z", b"z", b"+0530", b"-05:30", b"+00:00", b"-00:00", b"+05:30:15", b"+053015", b"+05", b"+05:", b"+5:30", b"05:30",
                                             b"+05:3", b"+24:00", b"+00:60", b"-23:59", b"+23:59", b"+99:99", b"UTC", b"+05-30", b" 05:30", b"", b"ZZ", b"+0530Z")]
    if has(fmt, "b"):
        rows += [render(fmt, b=b) for b in (b"oct", b"OCT", b"Oct", b"oCT", b"xyz", b"XYZ", b"o1t", b"oc", b"octo", b"Ja\0", b"\xd6ct", b"feb", b"DEC", b"JaN", b"ma ",
                                             b"may", b"Mar", b"jUL", b"Jun", b"aug", b"SEP", b"Nov", b"apr")]
    if has(fmt, "m"):
        rows += [render(fmt, m=m) for m in (b"00", b"01", b"12", b"13", b"99", b"1", b"010", b"+1", b" 1")]
    rows += [render(fmt, d=d) for d in (b"00", b"01", b"31", b"32", b"99", b"1", b" 1")]
    rows += [render(fmt, Y=y) for y in (b"0000", b"0001", b"9999", b"200", b"20000", b"-200", b"1970", b"1969")]
    for month, name, last in ((b"02", b"Feb", 29), (b"04", b"apr", 30), (b"12", b"DEC", 31)):
        rows += [render(fmt, m=month, b=name, d=b"%02d" % d) for d in (last, last + 1)]
    rows += [render(fmt, Y=b"1900", m=b"02", b=b"feb", d=b"29"), render(fmt, Y=b"2023", m=b"02", b=b"feb", d=b"29")]
    if has(fmt, "H"):
        rows += [render(fmt, H=h) for h in (b"00", b"23", b"24", b"99")] + [render(fmt, M=m) for m in (b"00", b"59", b"60")]
        rows += [render(fmt, S=s) for s in (b"00", b"59", b"60", b"61")]
    if has(fmt, "f"):
        rows += [render(fmt, f=f) for f in (b"5", b"50", b"500", b"5000", b"500000", b"500000000", b"1234", b"1234567", b"000000001", b"123456789", b"0", b"000",
                                             b"1234567890", b"", b"12x", b"000000000", b"0010", b"999999999")]
        rows += [render(fmt, m=b"13", b=b"Oct", d=b"32", f=b"1234567"), render(fmt, d=b"32", f=b"1234567") + b"x"]      # RANGE outranks INEXACT, MALFORMED both
    rows += [b" " + good, good + b" ", b" \t" + good + b"\t ", b" ", b"\t \t", good.replace(b"-", b" ").replace(b"/", b" "), b"\n" + good, good + b"\n",
             good + b" x", b"x " + good]
    return rows


def placed_rows():
    """the two seam rows: 26 bytes under CLF (one seam) and 35 bytes under ISO_F (two seams)"""
    clf, iso = b"10/Oct/2000:13:55:36 -0700", b"2000-10-10T13:55:36.123456789+05:30"
    assert len(clf) == 26 and len(iso) == 35
    return (CLF, clf), (ISO_F, iso)


def lay_at_every_alignment(row):
    """the row laid 16 times, beginning at every residue 0..15; the last copy ends at the text's last byte -> (text, records)"""
    text, records = bytearray(), []
    for mis in range(16):
        text += b"|"
        while len(text) % 16 != mis:
            text += b"|"
        records.append((len(text), len(text) + len(row)))
        text += row
    return bytes(text), records


EDGES = ((1, 1, 1, 0, 0, 0), (1600, 2, 29, 12, 0, 0), (1900, 3, 1, 0, 0, 0), (1969, 12, 31, 23, 59, 59), (1970, 1, 1, 0, 0, 0), (2000, 2, 29, 0, 0, 0),
         (2038, 1, 19, 3, 14, 7), (9999, 12, 31, 23, 59, 59))
FIRST, LAST = datetime.datetime(1, 1, 1), datetime.datetime(9999, 12, 31, 23, 59, 59)


def calendar_rows(fmt):
    """-> (rows, want) -- want[i]: the instant's seconds straight from datetime, or None where the row is RANGE"""
    rows, want = [], []

    def add(dt, zone=b"Z", minutes=0):
        rows.append(of_instant(fmt, dt, zone=zone))
        want.append((dt - EPOCH) // datetime.timedelta(seconds=1) - minutes * 60)
    one = datetime.timedelta(seconds=1)
    for e in EDGES:
        for dt in (datetime.datetime(*e) - one if datetime.datetime(*e) > FIRST else None, datetime.datetime(*e),
                   datetime.datetime(*e) + one if datetime.datetime(*e) < LAST else None):
            if dt is not None:
                add(dt)
    for year in (1900, 2000, 2023, 2024):
        for month in range(1, 13):
            last = calendar.monthrange(year, month)[1]
            add(datetime.datetime(year, month, last, 23, 59, 59))
            rows.append(render(fmt, Y=b"%04d" % year, m=b"%02d" % month, b=MONTHS[month - 1].upper().encode(), d=b"%02d" % (last + 1), f=b"0", z=b"Z"))
            want.append(None)
    if has(fmt, "z"):
        for dt in (datetime.datetime(2000, 6, 15, 23, 30, 0), datetime.datetime(2000, 6, 15, 0, 30, 0), datetime.datetime(1999, 12, 31, 23, 59, 59),
                   datetime.datetime(2000, 1, 1, 0, 0, 0), FIRST, LAST, datetime.datetime(1970, 1, 1, 0, 0, 0)):
            add(dt, b"+23:59", 23 * 60 + 59)
            add(dt, b"-23:59", -(23 * 60 + 59))
            add(dt, b"-2359", -(23 * 60 + 59))
        for zone in (b"+24:00", b"+00:60", b"-24:00"):
            rows.append(of_instant(fmt, datetime.datetime(2000, 1, 1), zone=zone))
            want.append(None)
    rng = random.Random(1970)
    span = (LAST - FIRST) // one
    for _ in range(4096):
        dt = FIRST + rng.randrange(span + 1) * one
        if has(fmt, "z") and rng.randrange(3) == 0:
            minutes = rng.randrange(-(23 * 60 + 59), 24 * 60)
            add(dt, b"%s%02d%s%02d" % (b"-" if minutes < 0 else b"+", abs(minutes) // 60, rng.choice((b"", b":")), abs(minutes) % 60), minutes)
        else:
            add(dt)
    if not has(fmt, "H"):      # a date-only format has no time of day: the rows above dropped it
        want = [None if w is None else w - w % 86400 for w in want]
    return rows, want


NANO_LOW, NANO_HIGH = b"1677-09-21T00:12:43.145224192", b"2262-04-11T23:47:16.854775807"


def nano_rows():
    """(row under ISO_F, the expected (status, bits) under NANO): the two ends of int64, their neighbours by one nanosecond,
    and the same instants spelled with a non-zero offset"""
    lo, hi = -(1 << 63), (1 << 63) - 1
    return [(NANO_LOW + b"Z", (OK, lo & MASK)), (b"1677-09-21T00:12:43.145224191Z", (RANGE, 0)), (b"1677-09-21T00:12:43.145224193Z", (OK, (lo + 1) & MASK)),
            (NANO_HIGH + b"Z", (OK, hi)), (b"2262-04-11T23:47:16.854775808Z", (RANGE, 0)), (b"2262-04-11T23:47:16.854775806Z", (OK, hi - 1)),
            (b"1677-09-21T05:42:43.145224192+05:30", (OK, lo & MASK)), (b"1677-09-21T05:42:43.145224191+05:30", (RANGE, 0)),
            (b"1677-09-20T17:12:43.145224192-07:00", (OK, lo & MASK)), (b"1677-09-20T17:12:43.145224191-0700", (RANGE, 0)),
            (b"2262-04-12T05:17:16.854775807+05:30", (OK, hi)), (b"2262-04-12T05:17:16.854775808+05:30", (RANGE, 0)),
            (b"2262-04-11T16:47:16.854775807-07:00", (OK, hi)), (b"2262-04-11T16:47:16.854775808-07:00", (RANGE, 0)),
            (b"1677-09-21T00:12:42.999999999Z", (RANGE, 0)), (b"2262-04-11T23:47:17.0Z", (RANGE, 0)), (b"0001-01-01T00:00:00.0Z", (RANGE, 0)),
            (b"9999-12-31T23:59:59.999999999Z", (RANGE, 0)), (b"1970-01-01T00:00:00.000000001Z", (OK, 1)), (b"1969-12-31T23:59:59.999999999Z", (OK, MASK))]


def inexact_rows():
    """(row under ISO_F, the status per unit SECOND..NANO)"""
    at = lambda f: b"2000-10-10T13:55:36." + f + b"Z"
    return [(at(b"5"), (INEXACT, OK, OK, OK)), (at(b"1234"), (INEXACT, INEXACT, OK, OK)), (at(b"1234567"), (INEXACT, INEXACT, INEXACT, OK)),
            (at(b"000000001"), (INEXACT, INEXACT, INEXACT, OK)), (at(b"500000000"), (INEXACT, OK, OK, OK)), (at(b"0"), (OK, OK, OK, OK)),
            (at(b"000000000"), (OK, OK, OK, OK)), (b"2000-13-10T13:55:36.1234567Z", (RANGE, RANGE, RANGE, RANGE)),
            (b"2000-10-10T13:55:36.1234567+24:00", (RANGE, RANGE, RANGE, RANGE)), (b"2000-13-10T13:55:36.1234567Zx", (MALFORMED,) * 4)]


REFUSED_FORMATS = (      # (format, the byte offset the message names)
    (b"", 0), (b"%Y-%m-%d" + b" " * 57, 64), (b"%Y-%m-%d %q", 9), (b"%Y-%m-%d %y", 9), (b"%Y-%m-%d %", 9), (b"%Y-%m-%d%", 8), (b"%Y-%m-%d %Y", 9),
    (b"%Y-%m-%d %d", 9), (b"%d %b %Y %m", 9), (b"%m/%d/%Y %b", 9), (b"%Y-%m-%dT%H:%H", 12), (b"%Y-%m-%d %z%z", 11), (b"%Y-%m-%d %f.%f", 12),
    (b"%H:%M:%S", 8), (b"%Y-%m", 5), (b"%Y-%d", 5), (b"%m-%d %H", 8), (b"%b %d", 5), (b"plain", 5), (b"%Y-%m-%d %f0", 11), (b"%Y-%m-%d %f9", 11),
    (b"%f%Y-%m-%d", 2), (b"%Y-%m-%f%d", 8), (b"%Y-%m-%d %f%S", 11), (b"%Y-%m-%d %f%f", 11))
ACCEPTED_FORMATS = (b"%Y-%m-%d" + b" " * 56, b"%Y%m%d", b"%Y%m%d%H%M%S%f", b"%Y-%m-%d %f%z", b"%f %d %b %Y", b"%Y-%m-%d %f%%", b"%d%b%Y",
                    b"%Y-%m-%d %fx")
