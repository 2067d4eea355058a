"""CPU tests of the timestamp parse (rejit_amd/csrc/record_time.h): the meaning of rj_scan_records_parse_time -- a row of a
record table read under a strptime-style format as an int64 count of seconds, milli-, micro- or nanoseconds since the epoch,
exactly or not at all -- and of records.time_buckets.

The header is compiled with g++ into the test-only driver tests/support/time_exec.cc, which compiles the format, checks the
rows, walks every row in the 16-byte groups of record_rows.h over a text whose every access is checked against its range, and
feeds every row AGAIN in steps of 1..16 bytes, as cut at every begin alignment 0..15, and at every split into two runs of
groups: the answer must not depend on where a row is cut.  The expectation is tests/time_cases.py's meaning, written in
Python independently of the header (an `re` pattern built from the format, calendar.monthrange, datetime arithmetic), which is
itself compared with datetime.strptime.  All comparisons are exact."""
import ctypes
import datetime
import random
import subprocess

import pytest

import time_cases as tc
from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_time.h", "record_rows.h", "record_pack.h"), ("checked_text.h",))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 3
SPLIT_BYTES = 600      # the driver's kSplitBytes: longer rows are walked once


@pytest.fixture(scope="module")
def tx():
    lib = shared_driver("time_exec", DEPS)
    u64, cp, ci, cu = ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.te_known.argtypes = [ci, cu]
    lib.te_compile.argtypes = [cp, u64, _u8p, _u32p, _u32p]
    lib.te_parse.restype = ctypes.c_long
    lib.te_parse.argtypes = [cp, u64, _u64p, _u64p, u64, _u64p, ci, u64, cp, u64, ci, cu, ci, _u64p, _u8p, _u64p]
    return lib


def run(lib, text, records, indices, fmt, unit, trim, splits=True, with_status=True):
    """-> (rc, summary, values, statuses: the whole poisoned buffers)"""
    k = len(records) if indices is None else len(indices)
    values, statuses = _arr([POISON] * (k + ROOM)), _arr([POISON8] * (k + ROOM), ctypes.c_uint8)
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.te_parse(text, len(text), _arr([b for b, _ in records]), _arr([e for _, e in records]), len(records), None if indices is None else _arr(indices),
                      int(indices is not None), 0 if indices is None else len(indices), fmt, len(fmt), unit, 1 if trim else 0, int(splits), values,
                      statuses if with_status else None, summ)
    return rc, [int(x) for x in summ], list(values), list(statuses)


def check(lib, rows, fmt, units=tc.UNITS, trims=(False, True), indices=None, lead=b"", tail=b"", splits=True, laid=None):
    """the rows laid into one text, read under every unit and flag, against the meaning"""
    text, records = laid if laid is not None else tc.lay(rows, lead=lead, tail=tail)
    order = range(len(rows)) if indices is None else indices
    for unit in units:
        for trim in trims:
            want = [tc.meaning(rows[r], fmt, unit, trim) for r in order]
            for with_status in (True, False):
                rc, summ, values, statuses = run(lib, text, records, indices, fmt, unit, trim, splits, with_status)
                ctx = (fmt, unit, trim, with_status)
                assert rc == 0, ("an access left its range, a row was written twice or another feed differed", rc, ctx)
                k = len(want)
                for j, (w, v, s) in enumerate(zip(want, values, statuses)):
                    assert (w[1], w[0] if with_status else POISON8) == (v, s), (ctx, j, rows[order[j]], w, (s, hex(v)))
                assert values[k:] == [POISON] * ROOM and statuses[k:] == [POISON8] * ROOM, ctx
                assert summ[:5] == [sum(1 for w in want if w[0] == c) for c in range(5)] and summ[5] == NONE, (ctx, summ)
                if splits:
                    assert summ[6] == sum(32 + max(len(rows[r]) - 1, 0) for r in order if len(rows[r]) <= SPLIT_BYTES), ctx
    return text, records


# ------------------------------------------------------------------------------------------------ the meaning itself
def test_the_python_meaning_on_rows_whose_answer_is_known_by_hand():
    M = tc.meaning
    assert M(b"1970-01-01T00:00:00Z", tc.ISO, tc.SECOND, False) == (tc.OK, 0) and M(b"1969-12-31T23:59:59Z", tc.ISO, tc.SECOND, False) == (tc.OK, tc.MASK)
    assert M(b"10/Oct/2000:13:55:36 -0700", tc.CLF, tc.SECOND, False) == (tc.OK, 971211336)
    assert M(b"2026-10-20T17:15:00.123Z", tc.ISO_F, tc.MILLI, False) == (tc.OK, 1792516500123) and M(b"2026-10-20T17:15:00.123Z", tc.ISO_F, tc.SECOND, False)[0] == tc.INEXACT
    assert M(b"", tc.DATE, 0, False) == (tc.EMPTY, 0) and M(b" \t", tc.DATE, 0, True) == (tc.EMPTY, 0) and M(b" ", tc.DATE, 0, False) == (tc.MALFORMED, 0)
    assert M(b"2000-02-30", tc.DATE, 0, False) == (tc.RANGE, 0) and M(b"2000-02-29", tc.DATE, 0, False) == (tc.OK, 951782400) and M(b"1900-02-29", tc.DATE, 0, False)[0] == tc.RANGE
    assert M(b"2000-2-29", tc.DATE, 0, False)[0] == tc.MALFORMED and M(b"0000-01-01", tc.DATE, 0, False)[0] == tc.RANGE
    assert M(b"2000-01-01T00:00:00z", tc.ISO, 0, False)[0] == tc.MALFORMED and M(b"2000-01-01T00:00:00+01:00:00", tc.ISO, 0, False)[0] == tc.MALFORMED
    assert M(b"2000-01-01T00:00:60Z", tc.ISO, 0, False)[0] == tc.RANGE and M(b"2000-01-01T00:00:00+24:00", tc.ISO, 0, False)[0] == tc.RANGE
    assert M(b"%2000\x0010-10%", tc.ODD, 0, False) == (tc.OK, 971136000) and M(b"%2000 10-10%", tc.ODD, 0, False)[0] == tc.MALFORMED
    assert M(b" 2000-10-10 ", tc.DATE, 0, True) == (tc.OK, 971136000) and M(b" 2000-10-10 ", tc.DATE, 0, False)[0] == tc.MALFORMED
    assert M(b"0001-01-01T00:00:00+23:59", tc.ISO, 0, False) == (tc.OK, (-62135596800 - 86340) & tc.MASK)


def test_the_python_meaning_agrees_with_strptime():
    compared = 0
    for fmt in tc.FORMATS:
        rows = tc.status_rows(fmt) + tc.calendar_rows(fmt)[0][:300]
        for unit in tc.UNITS:
            for trim in (False, True):
                done = tc.cross_check(rows, fmt, unit, trim)
                if done is None:
                    pytest.skip("LC_TIME's month names are not the English ones")
                compared += done
    assert compared > 5000


def test_the_calendar_rows_have_datetimes_values():
    for fmt in tc.FORMATS:
        rows, want = tc.calendar_rows(fmt)
        for row, w in zip(rows, want):
            assert tc.meaning(row, fmt, tc.SECOND, False) == ((tc.RANGE, 0) if w is None else (tc.OK, w & tc.MASK)), (fmt, row, w)


# ------------------------------------------------------------------------------------------------ the header
@pytest.mark.parametrize("fmt", tc.FORMATS, ids=["iso", "iso_f", "clf", "plain", "date", "odd"])
def test_every_family_against_the_meaning(tx, fmt):
    rows = tc.status_rows(fmt)
    check(tx, rows, fmt)
    seen = {tc.meaning(r, fmt, unit, trim)[0] for r in rows for unit in tc.UNITS for trim in (False, True)}
    assert seen == {tc.OK, tc.EMPTY, tc.MALFORMED, tc.RANGE} | ({tc.INEXACT} if tc.has(fmt, "f") else set())


def test_the_seam_rows_at_every_begin_alignment(tx):
    for fmt, row in tc.placed_rows():
        laid = tc.lay_at_every_alignment(row)
        assert {b % 16 for b, _ in laid[1]} == set(range(16)) and laid[1][-1][1] == len(laid[0])
        check(tx, [row] * 16, fmt, laid=laid)
        assert tc.meaning(row, fmt, tc.NANO, False)[0] == tc.OK
        # every byte of the row spoilt in turn, at every alignment
        for i in range(len(row)):
            bad = row[:i] + b"?" + row[i + 1:]
            check(tx, [bad] * 16, fmt, units=(tc.NANO,), trims=(True,), laid=tc.lay_at_every_alignment(bad), splits=i % 5 == 0)


def test_the_calendar(tx):
    for fmt in (tc.ISO, tc.CLF, tc.DATE):
        rows, want = tc.calendar_rows(fmt)
        check(tx, rows, fmt, units=(tc.SECOND, tc.MICRO), trims=(False,), splits=False)
    rows, _ = tc.calendar_rows(tc.ISO)
    check(tx, rows[:400], tc.ISO, units=(tc.NANO,), trims=(True,))


def test_nanos_range_and_the_inexact_rows(tx):
    rows = [r for r, _ in tc.nano_rows()]
    for row, want in tc.nano_rows():
        assert tc.meaning(row, tc.ISO_F, tc.NANO, False) == want, row
    check(tx, rows, tc.ISO_F)
    for row, statuses in tc.inexact_rows():
        assert tuple(tc.meaning(row, tc.ISO_F, unit, False)[0] for unit in tc.UNITS) == statuses, row
    check(tx, [r for r, _ in tc.inexact_rows()], tc.ISO_F)


def test_index_lists_with_repeats_and_permutations(tx):
    rows = tc.status_rows(tc.CLF)
    rng = random.Random(5)
    perm = list(range(len(rows)))
    rng.shuffle(perm)
    for indices in (perm, [rng.randrange(len(rows)) for _ in range(150)], [3] * 70, []):
        check(tx, rows, tc.CLF, units=(tc.SECOND,), indices=indices, splits=False)


def test_rows_at_the_texts_ends_and_long_rows(tx):
    good = tc.render(tc.ISO)
    rows = [good, good + b" " * 700, b" " * 700 + good, good + b"0" * 700, good]
    text, records = check(tx, rows, tc.ISO, lead=b"")
    assert records[0][0] == 0 and records[-1][1] == len(text) and len(text) % 16 != 0
    big = [good + b" " * (1 << 20) + b"x", b"x" + good * 40000, good + b" " * (1 << 20)]
    _, records = check(tx, big, tc.ISO, units=(tc.SECOND,), splits=False)
    assert tc.meaning(big[0], tc.ISO, 0, True)[0] == tc.MALFORMED and tc.meaning(big[2], tc.ISO, 0, True)[0] == tc.OK
    # a row that is malformed at byte 0 stops there: one step, not 2^16
    rc, summ, _, _ = run(tx, *tc.lay([big[1]]), None, tc.ISO, 0, False, splits=False)
    assert rc == 0 and summ[7] == 1 and summ[2] == 1


def test_a_bad_row_refuses_the_call_and_nothing_is_written(tx):
    text, records = tc.lay([b"2000-10-10", b"2000-10-11", b"2000-10-12"])
    n = len(text)
    for bad_records, indices, first in (([(0, 1), (3, 2), (0, n + 1)], None, 1), ([(0, 1), (0, 1), (n, n + 1)], None, 2), (records, [0, 3, 1], 1),
                                        (records, [NONE], 0)):
        rc, summ, values, statuses = run(tx, text, bad_records, indices, tc.DATE, tc.SECOND, False)
        assert rc == 0 and summ[5] == first and summ[:5] == [0] * 5
        assert values == [POISON] * len(values) and statuses == [POISON8] * len(statuses)


def test_the_format_compilers_refusals_and_their_offsets(tx):
    code, length, at = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(), ctypes.c_uint32()
    for fmt, offset in tc.REFUSED_FORMATS:
        assert tx.te_compile(fmt, len(fmt), code, ctypes.byref(length), ctypes.byref(at)) != 0, fmt
        assert at.value == offset, (fmt, at.value, offset)
        text, records = tc.lay([b"2000-10-10"])
        rc, _, values, statuses = run(tx, text, records, None, fmt, 0, False)
        assert rc == -2 and values == [POISON] * len(values) and statuses == [POISON8] * len(statuses)
    for fmt in tc.FORMATS + tc.ACCEPTED_FORMATS:
        assert tx.te_compile(fmt, len(fmt), code, ctypes.byref(length), ctypes.byref(at)) == 0, fmt
        assert length.value == len(fmt) <= 64
    # the program: literals as they are, a directive as '%' and its number
    assert tx.te_compile(b"%Y-%m\0%d%%", 10, code, ctypes.byref(length), ctypes.byref(at)) == 0
    assert bytes(code[:10]) == b"%\x00-%\x01\x00%\x02%\x09" and not any(code[10:])
    # the error classes are told apart
    kinds = {fmt: tx.te_compile(fmt, len(fmt), code, ctypes.byref(length), ctypes.byref(at)) for fmt, _ in tc.REFUSED_FORMATS}
    assert kinds[b""] == 1 and kinds[b"%Y-%m-%d" + b" " * 57] == 2 and kinds[b"%Y-%m-%d %q"] == 3 and kinds[b"%Y-%m-%d %"] == 4
    assert kinds[b"%Y-%m-%d %Y"] == 5 and kinds[b"%m/%d/%Y %b"] == 5 and kinds[b"%Y-%m-%d %f0"] == 6 and kinds[b"%H:%M:%S"] == 7
    assert kinds[b"%Y-%m-%d %f%f"] == 5      # (given twice before ambiguous)


def test_unknown_units_and_flags_are_refused_up_front(tx):
    assert [tx.te_known(u, 0) & 1 for u in (-1, 0, 1, 2, 3, 4)] == [0, 1, 1, 1, 1, 0]
    assert [tx.te_known(0, f) >> 1 for f in (0, 1, 2, 3, 4, 5, 0x80000000)] == [1, 1, 0, 0, 0, 0, 0]
    text, records = tc.lay([b"2000-10-10"])
    assert run(tx, text, records, None, tc.DATE, 4, False)[0] == -2


def test_the_states_size_is_reported(tx):
    size = tx.te_state_size()
    print("timeparse::State: %d bytes" % size)
    assert 16 <= size <= 64      # "a few dozen bytes": a fixed state, whatever the row's length


# ------------------------------------------------------------------------------------------------ time_buckets
def test_time_buckets_floor_toward_minus_infinity_on_cpu_tensors():
    import torch
    from rejit_amd import records
    rng = random.Random(7)
    values = [0, 1, 59, 60, 61, -1, -59, -60, -61, 971211336, -62135596800, 253402300799] + [rng.randrange(-10 ** 11, 10 ** 11) for _ in range(200)]
    status = [rng.randrange(5) if rng.randrange(4) == 0 else 0 for _ in values]
    for width in (1, 60, 3600, 86400, 7):
        start, ok = records.time_buckets(torch.tensor(values, dtype=torch.int64), torch.tensor(status, dtype=torch.uint8), width)
        assert start.dtype == torch.int64 and start.tolist() == [v // width * width for v in values]
        assert ok.dtype == torch.bool and ok.tolist() == [s == 0 for s in status]
    start, _ = records.time_buckets(torch.tensor([-1], dtype=torch.int64), torch.tensor([0], dtype=torch.uint8), 60)
    assert start.tolist() == [-60] and datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=-60) == datetime.datetime(1969, 12, 31, 23, 59)
    for width in (0, -5):
        with pytest.raises(ValueError):
            records.time_buckets(torch.tensor([1]), torch.tensor([0], dtype=torch.uint8), width)


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: 192 seeded random cases under six formats against a meaning written over std::string with a calendar that
    counts the days year by year, every other feed included, exact allocations.  (The sanitizers' runtimes are linked
    statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("time_exec", DEPS)], capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"192 cases" in r.stdout
