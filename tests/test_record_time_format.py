"""CPU tests of the timestamp writer (rejit_amd/csrc/record_time_format.h): the meaning of rj_scan_records_format_time -- a
column of int64 instants written as text under a strftime-style format, laid out as rj_scan_records_format lays its rows out.

The header is compiled with g++ into the test-only driver tests/support/time_format_exec.cc, which refuses what the call
refuses, plans the rows, and emits the output chunk by chunk through the layout table, with the chunk size chosen here, every
access checked against its range and every byte and table row written exactly once.  The expectation is
tests/time_format_cases.py's meaning, written in Python independently of the header (divmod, datetime + timedelta, %04d /
%02d by hand), which is itself compared with isoformat() and strftime.  All comparisons are exact."""
import ctypes
import datetime
import itertools
import subprocess

import pytest

import time_format_cases as tf
from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_time_format.h", "record_time.h", "record_pack.h"))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u16p = ctypes.POINTER(ctypes.c_uint16)
_u32p = ctypes.POINTER(ctypes.c_uint32)
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 3
ROOM_BYTES = 19
FINE, NULL_ARGUMENT, TABLE_ALIGN, OUT_ALIGN, BAD_UNIT, BAD_ZONE, BAD_FLAGS, BAD_FILL, BAD_SUMS, TOO_MANY_ROWS = range(10)


@pytest.fixture(scope="module")
def tx():
    lib = shared_driver("time_format_exec", DEPS)
    u64, cp, ci, cu = ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.tf_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.tf_compile.argtypes = [cp, u64, ci, _u8p, _u32p, _u32p]
    lib.tf_layout.argtypes = [cp, u64, ci, ci, _u16p]
    lib.tf_calendar.restype = ctypes.c_long
    lib.tf_format.restype = ctypes.c_long
    lib.tf_format.argtypes = [_u64p, _u8p, u64, _u64p, ci, u64, cp, u64, ci, ci, cu, ci, u64, u64, u64, ci, _u8p, u64, _u64p, _u64p, _u64p]
    return lib


def run(lib, values, fmt, unit, status=None, indices=None, zone=0, flags=0, fill=10, lead=0, gap=1, chunk=4096, round_trip=False, cap=None, with_begin=True,
        with_end=True):
    """-> (rc, summary, out bytes with the spare ones, begins, ends with the spare rows)"""
    k = len(values) if indices is None else len(indices)
    if cap is None:
        cap = lead + k * (tf.MAX_ROW + gap)
    out = (ctypes.c_uint8 * (cap + ROOM_BYTES))(*([POISON8] * (cap + ROOM_BYTES)))
    begins, ends = _arr([POISON] * (k + ROOM)), _arr([POISON] * (k + ROOM))
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.tf_format(_arr(tf.to_words(values)), None if status is None else _arr(status, ctypes.c_uint8), len(values), None if indices is None else _arr(indices),
                       int(indices is not None), 0 if indices is None else len(indices), fmt, len(fmt), unit, zone, flags, fill, lead, gap, chunk,
                       int(round_trip), out, cap, begins if with_begin else None, ends if with_end else None, summ)
    return rc, [int(x) for x in summ], bytes(out), list(begins), list(ends)


def check(lib, values, fmt, unit, status=None, indices=None, zone=0, fill=10, lead=0, gap=1, chunk=4096, round_trip=False):
    text, begins, ends, counts = tf.layout(values, fmt, unit, status, indices, zone, fill, lead, gap)
    rc, summ, out, gb, ge = run(lib, values, fmt, unit, status, indices, zone, 0, fill, lead, gap, chunk, round_trip, cap=len(text))
    ctx = (fmt, unit, zone, fill, lead, gap, chunk)
    assert rc == len(text), (ctx, rc, summ)
    k = len(begins)
    if out[:rc] != text:
        j = next(j for j in range(k) if out[begins[j]:ends[j]] != text[begins[j]:ends[j]])
        raise AssertionError((ctx, "row", j, (values if indices is None else [values[i] for i in indices])[j], out[begins[j]:ends[j]], text[begins[j]:ends[j]]))
    assert out[rc:] == bytes([POISON8]) * ROOM_BYTES, ctx
    assert gb[:k] == begins and ge[:k] == ends and gb[k:] == [POISON] * ROOM and ge[k:] == [POISON] * ROOM, ctx
    assert summ[:3] == [counts[tf.OK], counts[tf.NULL], counts[tf.RANGE]] and summ[3] == NONE and summ[5] == tf.row_length(fmt, unit), (ctx, summ, counts)
    if round_trip:
        assert summ[6] == counts[tf.OK], ctx
    return text, begins, ends, counts


# ------------------------------------------------------------------------------------------------ the meaning itself
def test_the_python_meaning_on_instants_whose_text_is_known_by_hand():
    T = tf.text_of
    assert T(0, tf.ISO, tf.SECOND) == b"1970-01-01T00:00:00Z" and T(-1, tf.ISO, tf.SECOND) == b"1969-12-31T23:59:59Z"
    assert T(-1, tf.ISO_F, tf.NANO) == b"1969-12-31T23:59:59.999999999+0000" and T(-1, tf.ISO_F, tf.MILLI) == b"1969-12-31T23:59:59.999+0000"
    assert T(-1, tf.ISO_F, tf.MICRO, 330) == b"1970-01-01T05:29:59.999999+0530" and T(0, tf.ISO_F, tf.SECOND, -420) == b"1969-12-31T17:00:00.000000-0700"
    assert T(971211336, tf.CLF, tf.SECOND, -420) == b"10/Oct/2000:13:55:36 -0700" and T(1792516500123, tf.MINUTE, tf.MILLI) == b"2026-10-20T17:15"
    assert T(tf.FIRST_SECOND, tf.ISO, 0) == b"0001-01-01T00:00:00Z" and T(tf.LAST_SECOND, tf.ISO, 0) == b"9999-12-31T23:59:59Z"
    assert T(tf.FIRST_SECOND - 1, tf.ISO, 0) == b"" and T(tf.LAST_SECOND + 1, tf.ISO, 0) == b""
    assert T(tf.INT64_MIN, b"%Y-%m-%dT%H:%M:%S.%f", tf.NANO) == b"1677-09-21T00:12:43.145224192"
    assert T(tf.INT64_MAX, b"%Y-%m-%dT%H:%M:%S.%f", tf.NANO) == b"2262-04-11T23:47:16.854775807"
    assert T(951782400009, tf.ODD, tf.MILLI) == b"%2000\x0002-29%0099" and T(3600 * 13 + 60 * 5, tf.CLOCK, 0) == b"13:05"
    assert [tf.row_length(tf.LONGEST, u) for u in tf.UNITS] == [74, 71, 74, 77] and tf.row_length(tf.ISO, 0) == 20 and tf.row_length(tf.CLF, 0) == 26


def test_the_python_meaning_agrees_with_isoformat_and_strftime():
    if [datetime.date(2001, m, 1).strftime("%b") for m in range(1, 13)] != list(tf.MONTHS):
        pytest.skip("LC_TIME's month names are not the English ones")
    compared = 0
    for fmt, unit, zone in itertools.product(tf.FORMATS, tf.UNITS, tf.ZONES):
        compared += tf.cross_check(tf.values_of(unit, 60), fmt, unit, zone)
    assert compared > 20000


# ------------------------------------------------------------------------------------------------ the header
@pytest.mark.parametrize("fmt", tf.FORMATS, ids=tf.FORMAT_IDS)
def test_every_directive_under_every_unit_and_zone(tx, fmt):
    """the edges (the epoch, -1, both ends of the range and their outside neighbours, also as the zones +-1439 see them,
    INT64_MIN and INT64_MAX, leap days, century rules, every month end) and seeded values"""
    seen = set()
    for unit in tf.UNITS:
        values = tf.values_of(unit)
        for zone in tf.ZONES:
            _, _, _, counts = check(tx, values, fmt, unit, zone=zone, round_trip=tf.parse_round_trips(fmt, unit, zone))
            assert counts[tf.OK] > 300 and (counts[tf.RANGE] > 20) == (unit != tf.NANO) and (unit != tf.NANO or counts[tf.RANGE] == 0)
            seen.add(tf.parse_round_trips(fmt, unit, zone))
    assert (True in seen) == (fmt in (tf.ISO, tf.ISO_F, tf.CLF, tf.LONGEST))


def test_the_ends_of_the_range_are_judged_on_the_shifted_instant(tx):
    for unit in (tf.SECOND, tf.MILLI, tf.MICRO):
        per = 10 ** (3 * unit)
        for zone in (0, 1, -1, 1439, -1439):
            first, last = (tf.FIRST_SECOND - zone * 60) * per, (tf.LAST_SECOND - zone * 60) * per + per - 1
            values = [first - 1, first, last, last + 1]
            text, begins, ends, counts = check(tx, values, tf.ISO_F, unit, zone=zone)
            L = tf.row_length(tf.ISO_F, unit)
            assert counts == {tf.OK: 2, tf.NULL: 0, tf.RANGE: 2} and [e - b for b, e in zip(begins, ends)] == [0, L, L, 0]
            assert text[begins[1]:begins[1] + 19] == b"0001-01-01T00:00:00" and text[begins[2]:begins[2] + 19] == b"9999-12-31T23:59:59"


def test_both_ends_of_int64_under_every_unit(tx):
    """RANGE everywhere but under NANO, where every int64 lies inside 1677..2262 -- under every zone"""
    values = [tf.INT64_MIN, tf.INT64_MAX, tf.INT64_MIN + 1, tf.INT64_MAX - 1]
    for unit in tf.UNITS:
        for zone in tf.ZONES:
            text, begins, ends, counts = check(tx, values, b"%Y-%m-%dT%H:%M:%S.%f", unit, zone=zone)
            assert counts[tf.OK] == (4 if unit == tf.NANO else 0) and counts[tf.RANGE] == (0 if unit == tf.NANO else 4)
    text, begins, ends, _ = check(tx, values, b"%Y-%m-%dT%H:%M:%S.%f", tf.NANO)
    assert text[begins[0]:ends[0]] == b"1677-09-21T00:12:43.145224192" and text[begins[1]:ends[1]] == b"2262-04-11T23:47:16.854775807"
    years = {int(tf.text_of(v, b"%Y", tf.NANO, z)) for v in values for z in (-1439, 1439)}
    assert years == {1677, 2262}


def test_the_calendar_is_the_inverse_of_the_parses_for_every_day(tx):
    assert tx.tf_calendar() == 3652059      # every day of 0001..9999, counted one by one, there and back


def test_leap_days_century_rules_and_month_ends(tx):
    days = [(1900, 2, 28), (1900, 3, 1), (2000, 2, 29), (2000, 3, 1), (2100, 2, 28), (2100, 3, 1), (400, 2, 29), (400, 3, 1), (2024, 2, 29), (2023, 2, 28)]
    days += [(y, m, d) for y in (1999, 2024) for m in range(1, 13) for d in (1, 28)]
    values = [tf.seconds_of(*d) + s for d in days for s in (0, 86399)]
    text, begins, ends, _ = check(tx, values, b"%Y-%b-%d", tf.SECOND)
    want = [("%04d-%s-%02d" % (y, tf.MONTHS[m - 1], d)).encode() for y, m, d in days for _ in (0, 1)]
    assert [text[b:e] for b, e in zip(begins, ends)] == want
    ends_of_months = [tf.seconds_of(y, m, 1) - 1 for y in (1900, 2000, 2023, 2024, 2100) for m in range(1, 13)]
    text, begins, ends, _ = check(tx, ends_of_months, b"%m-%d", tf.SECOND)
    assert {text[b:e] for b, e in zip(begins, ends)} == {b"12-31", b"01-31", b"02-28", b"02-29", b"03-31", b"04-30", b"05-31", b"06-30", b"07-31", b"08-31",
                                                           b"09-30", b"10-31", b"11-30"}


def test_the_rows_length_is_the_layouts_and_never_more_than_77(tx):
    consts = (ctypes.c_int64 * 4)()
    tx.tf_constants(consts)
    assert list(consts) == [tf.MAX_ROW, 16, 164, 32]
    entries = (ctypes.c_uint16 * 80)()
    for fmt, unit, zone in itertools.product(tf.FORMATS + tf.ACCEPTED_FORMATS, tf.UNITS, (0, -1439)):
        assert tx.tf_layout(fmt, len(fmt), unit, zone, entries) == tf.row_length(fmt, unit) <= tf.MAX_ROW
    # the bound by brute force: the formats of 64 bytes made of any subset of the directives (each once, %m or %b) and then as
    # many %% or literals as fit -- no other format can be longer, since every byte left over gives one byte at the most
    longest = 0
    for picked in itertools.product((False, True), repeat=8):
        for month in ("m", "b"):
            letters = [c for c, on in zip("YdHMSfz", picked) if on] + ([month] if picked[7] else [])
            head = b"".join(b"%" + c.encode() for c in letters)
            for filler in (b"x", b"%%"):
                fmt = head + filler * ((64 - len(head)) // len(filler))
                fmt += b"x" * (64 - len(fmt))
                for unit in tf.UNITS:
                    length = tx.tf_layout(fmt, 64, unit, 1439, entries)
                    assert length == tf.row_length(fmt, unit)
                    longest = max(longest, length)
    assert longest == tf.MAX_ROW
    assert tx.tf_layout(tf.LONGEST, 64, tf.NANO, 0, entries) == 77 and tx.tf_layout(tf.LONGEST + b"x", 65, tf.NANO, 0, entries) == -2
    # a layout entry is a literal byte or an index into the row's 32 source bytes
    assert tx.tf_layout(b"%Y\xff%%%z", 7, 0, -330, entries) == 11
    assert list(entries[:11]) == [0x100, 0x101, 0x102, 0x103, 0xFF, 0x25, 0x2D, 0x30, 0x35, 0x33, 0x30] and not any(entries[11:])


@pytest.mark.parametrize("fmt,unit,gap", [(tf.ISO, tf.SECOND, 1), (tf.LONGEST, tf.NANO, 0), (tf.CLF, tf.MICRO, 1)])
def test_every_cut_of_a_row_by_a_chunks_end(tx, fmt, unit, gap):
    """chunks of 16 bytes against an odd pitch put a seam at every phase of a row; chunks of 1 and 7 bytes likewise; the output
    is the output of one chunk"""
    values = tf.values_of(unit, 40)
    pitch = tf.row_length(fmt, unit) + gap
    assert pitch % 2 == 1
    status = tf.status_column(len(values))
    for chunk in (1, 7, 16, pitch, pitch + 1, 4096):
        check(tx, values, fmt, unit, status=status, gap=gap, chunk=chunk, lead=3)


def test_layouts_tables_fills_and_the_size_query(tx):
    values = tf.values_of(tf.MILLI, 50)
    status = tf.status_column(len(values))
    for lead, gap, fill in itertools.product((0, 1, 15, 16, 17), (0, 1, 5), (10, 0, 0x2C)):
        check(tx, values, tf.ISO_F, tf.MILLI, status=status, lead=lead, gap=gap, fill=fill, chunk=64)
    text, begins, ends, _ = tf.layout(values, tf.CLF, tf.MILLI, status, None, 330, 0x2C, 5, 2)
    for with_begin, with_end in ((True, False), (False, True), (False, False)):
        rc, _, out, gb, ge = run(tx, values, tf.CLF, tf.MILLI, status, None, 330, 0, 0x2C, 5, 2, cap=len(text), with_begin=with_begin, with_end=with_end)
        assert rc == len(text) and out[:rc] == text
        assert gb[:len(begins)] == (begins if with_begin else [POISON] * len(begins)) and ge[:len(ends)] == (ends if with_end else [POISON] * len(ends))
    # the size query writes the tables and no byte; a capacity below the total: nothing at or beyond it
    rc, _, out, gb, ge = run(tx, values, tf.CLF, tf.MILLI, status, None, 330, 0, 0x2C, 5, 2, cap=0)
    assert rc == len(text) and out == bytes([POISON8]) * ROOM_BYTES and gb[:len(begins)] == begins and ge[:len(ends)] == ends
    for cap in (1, 16, 17, len(text) - 1, len(text) - 30):
        rc, _, out, _, _ = run(tx, values, tf.CLF, tf.MILLI, status, None, 330, 0, 0x2C, 5, 2, cap=cap, chunk=32)
        assert rc == len(text) and out[:cap] == text[:cap] and out[cap:] == bytes([POISON8]) * ROOM_BYTES


def test_index_lists_and_no_rows(tx):
    values = tf.values_of(tf.SECOND, 30)
    status = tf.status_column(len(values))
    n = len(values)
    for indices in (list(reversed(range(n))), [5] * 300, [i * 7 % n for i in range(2 * n)], []):
        check(tx, values, tf.CLF, tf.SECOND, status=status, indices=indices, zone=-420, lead=2)
    check(tx, [], tf.ISO, tf.SECOND, lead=4)
    # more than 256 empty rows in a row, gap 0: null rows and rows out of range between OK rows
    mixed = [0, tf.INT64_MAX] * 300 + [1] * 3
    check(tx, mixed, tf.ISO, tf.SECOND, status=[0, 0, 2, 0] * 150 + [0, 1, 0], gap=0, chunk=64)


def test_refusals_in_their_order_write_nothing(tx):
    values = [0, 1, 2]

    def refused(why, rc_want=-2, **kw):
        rc, summ, out, gb, ge = run(tx, values, kw.pop("fmt", tf.ISO), kw.pop("unit", 0), cap=kw.pop("cap", 256), **kw)
        assert rc == rc_want and summ[7] == why, (why, rc, summ)
        assert out == bytes([POISON8]) * len(out) and gb == [POISON] * len(gb) and ge == [POISON] * len(ge)
        return summ

    for unit in (-1, 4, 99):
        refused(BAD_UNIT, unit=unit)
    for zone in (1440, -1440, 1 << 20):
        refused(BAD_ZONE, zone=zone)
    for flags in (1, 2, 0x80000000):
        refused(BAD_FLAGS, flags=flags)
    for fill in (-1, 256):
        refused(BAD_FILL, fill=fill)
    refused(BAD_UNIT, unit=7, zone=5000, flags=1, fill=-1, fmt=b"%q")      # the order: unit, zone, flags, fill, format, sums
    refused(BAD_ZONE, zone=5000, flags=1, fill=-1, fmt=b"%q")
    refused(100 + 3, fmt=b"%q", gap=1 << 42)
    refused(BAD_SUMS, gap=(1 << 42) - 77)
    refused(BAD_SUMS, lead=1 << 62)
    refused(BAD_SUMS, lead=(1 << 62) - 3 * 78 + 0)
    assert run(tx, values, tf.ISO, 0, lead=(1 << 62) - 3 * 78 - 1, cap=0)[0] == (1 << 62) - 3 * 78 - 1 + 3 * 21
    for fmt, offset in tf.REFUSED_FORMATS:
        summ = refused(summ_code(tx, fmt), fmt=fmt)
        assert summ[4] == offset, (fmt, summ)
    summ = refused(FINE, rc_want=-4, indices=[0, 1, 3, 2, 9])
    assert summ[3] == 2
    assert refused(FINE, rc_want=-4, indices=[NONE])[3] == 0


def summ_code(lib, fmt):
    code, length, at = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(), ctypes.c_uint32()
    return 100 + lib.tf_compile(fmt, len(fmt), 1, code, ctypes.byref(length), ctypes.byref(at))


def test_the_compiler_in_writing_mode_and_unchanged_in_parse_mode(tx):
    import time_cases as tc
    code, length, at = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(), ctypes.c_uint32()
    kinds = {}
    for fmt, offset in tf.REFUSED_FORMATS:
        kinds[fmt] = tx.tf_compile(fmt, len(fmt), 1, code, ctypes.byref(length), ctypes.byref(at))
        assert kinds[fmt] != 0 and at.value == offset, (fmt, at.value, offset)
    assert kinds[b""] == 1 and kinds[b"%Y-%m-%d" + b" " * 57] == 2 and kinds[b"%Y-%m-%d %q"] == 3 and kinds[b"%Y-%m-%d %"] == 4 and kinds[b"%H%"] == 4
    assert kinds[b"%H:%H"] == 5 and kinds[b"%m/%d/%Y %b"] == 5 and kinds[b"%f%f"] == 5
    for fmt in tf.FORMATS + tf.ACCEPTED_FORMATS + tc.FORMATS + tc.ACCEPTED_FORMATS:
        assert tx.tf_compile(fmt, len(fmt), 1, code, ctypes.byref(length), ctypes.byref(at)) == 0 and length.value == len(fmt), fmt
    # the program is the parse's: literals as they are, a directive as '%' and its number
    assert tx.tf_compile(b"%H:%M\0%f9%%", 11, 1, code, ctypes.byref(length), ctypes.byref(at)) == 0
    assert bytes(code[:11]) == b"%\x03:%\x04\x00%\x069%\x09" and not any(code[11:])
    # parse mode: every refusal of the parse with its offset, every acceptance
    for fmt, offset in tc.REFUSED_FORMATS:
        assert tx.tf_compile(fmt, len(fmt), 0, code, ctypes.byref(length), ctypes.byref(at)) != 0 and at.value == offset, fmt
    for fmt in tc.FORMATS + tc.ACCEPTED_FORMATS:
        assert tx.tf_compile(fmt, len(fmt), 0, code, ctypes.byref(length), ctypes.byref(at)) == 0, fmt
    assert tx.tf_compile(b"%H:%M:%S", 8, 0, code, ctypes.byref(length), ctypes.byref(at)) == 7 and tx.tf_compile(b"%Y-%m-%d %f0", 12, 0, code, ctypes.byref(length), ctypes.byref(at)) == 6


def test_round_trip_through_the_parse_for_every_unit(tx):
    """timeparse over the output returns the value with OK: every unit, the formats that name every field down to the unit"""
    for unit in tf.UNITS:
        values = tf.values_of(unit, 400)
        formats = [b"%Y-%m-%dT%H:%M:%S.%f%z", b"%d/%b/%Y:%H:%M:%S.%f %z", b"%f|%S%M%H%d%m%Y%z"] + ([tf.ISO, b"%Y-%m-%dT%H:%M:%S%z", tf.CLF] if unit == tf.SECOND else [])
        for fmt in formats:
            for zone in tf.ZONES if tf.has(fmt, "z") else (0,):
                assert tf.parse_round_trips(fmt, unit, zone)
                _, _, _, counts = check(tx, values, fmt, unit, zone=zone, round_trip=True)
                assert counts[tf.OK] > 300


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: 112 seeded random cases under seven formats, four units and five zones against a meaning written over
    std::string with a calendar that counts the days year by year, over exact allocations, and the calendar walk.  (The
    sanitizers' runtimes are linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("time_format_exec", DEPS)], capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"112 cases" in r.stdout
