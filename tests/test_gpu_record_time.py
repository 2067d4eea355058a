"""GPU tests (-m gpu) of rj_scan_records_parse_time (rejit_amd/csrc/record_time.hip; Scan.parse_time_records), of
records.time_buckets and of samples/linegrep_gpu.py -T.

The meaning is tests/time_cases.py's, written in Python independently of the library: an `re` pattern built from the format,
calendar.monthrange for the day, datetime arithmetic for the instant; the calendar rows are compared with datetime directly,
the table of more than one grid pass with numpy.datetime64.  A row that is not OK has the value 0.  Every comparison is
exact.  Outputs are poisoned first, with ROOM extra rows that must stay poisoned."""
import ctypes
import datetime
import functools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import time_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_TOO_LARGE, RJ_BAD_ARGUMENT = -2, -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON_U = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 7
STATS = ("n_ok", "n_empty", "n_malformed", "n_range", "n_inexact")      # rj_parse_stats: five uint64
IDS = ["iso", "iso_f", "clf", "plain", "date", "odd"]

meaning = functools.lru_cache(maxsize=None)(tc.meaning)


@pytest.fixture(scope="module")
def rj():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rejit_amd
    rejit_amd.build()
    rejit_amd.load_library()
    return rejit_amd


@pytest.fixture(scope="module")
def scan(rj):
    return rj.Scan(rj.Program(b" "))


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))).to("cuda:0")


def dev_text(data):
    import torch
    return torch.from_numpy(np.frombuffer(data if data else b"\0", dtype=np.uint8).copy()).to("cuda:0")[:len(data)]


class Table:
    """a table: the host bytes, the device text, the record tables on both, an optional index list"""

    def __init__(self, data, records, rows=None, d=None):
        self.data, self.records = data, list(records)
        self.rows = None if rows is None else list(rows)
        self.d = dev_text(data) if d is None else d
        self.rb_t, self.re_t = dev([b for b, _ in self.records]), dev([e for _, e in self.records])
        self.idx_t = None if rows is None else dev(self.rows)

    def k(self):
        return len(self.records) if self.rows is None else len(self.rows)

    def strings(self):
        rows = range(len(self.records)) if self.rows is None else self.rows
        return [self.data[self.records[r][0]:self.records[r][1]] for r in rows]

    def take(self, rows):
        return Table(self.data, self.records, rows, d=self.d)


def laid(rows, **kw):
    text, records = tc.lay(rows, **kw)
    return Table(text, records)


def call_poisoned(rj, scan, T, fmt, unit, flags, want_status=True, want_stats=True):
    """rj_scan_records_parse_time into poisoned tables -> (return value, values as uint64, status: the whole buffers, stats or None)"""
    import torch
    lib = rj.load_library()
    k = T.k()
    values = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    status = torch.full((k + ROOM,), POISON8, dtype=torch.uint8, device="cuda:0")
    keep = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
    idx = None if T.idx_t is None else (T.idx_t if k else keep)      # (a non-null pointer with a count of 0: no rows)
    out = (ctypes.c_uint64 * 5)(*([0xA5A5] * 5))
    total = lib.rj_scan_records_parse_time(scan._h, vp(T.d), int(T.d.numel()), vp(T.rb_t), vp(T.re_t), len(T.records),
                                           ctypes.c_void_p(idx.data_ptr()) if idx is not None else None, k if idx is not None else 0, fmt, len(fmt), unit,
                                           flags, vp(values), vp(status) if want_status else None,
                                           ctypes.cast(out, lib.rj_scan_records_parse_time.argtypes[14]) if want_stats else None,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    stats = dict(zip(STATS, (int(x) for x in out))) if want_stats else None
    return int(total), values.cpu().numpy().view(np.uint64), status.cpu().numpy(), stats


def check(rj, scan, T, fmt, units=tc.UNITS, trims=(False, True), api=False, ctx=None, want=None, variants=((True, True), (False, True), (True, False))):
    """the raw call into poisoned tables -- with d_status and stats, and each of them NULL -- against the meaning (or `want`, a
    list of (status, bits) for the one unit and flag asked for); Scan.parse_time_records"""
    import torch
    k, strings = T.k(), T.strings()
    for unit in units:
        for trim in trims:
            expect = want if want is not None else [meaning(s, fmt, unit, trim) for s in strings]
            w_status = np.array([w[0] for w in expect], dtype=np.uint8)
            w_bits = np.array([w[1] for w in expect], dtype=np.uint64)
            w_stats = dict(zip(STATS, (int((w_status == c).sum()) for c in range(5))))
            c = (ctx, fmt, unit, trim, k)
            for want_status, want_stats in variants:
                total, values, status, stats = call_poisoned(rj, scan, T, fmt, unit, 1 if trim else 0, want_status, want_stats)
                assert total == w_stats["n_ok"], (c, total, rj.load_library().rj_last_error())
                differ = np.nonzero(values[:k] != w_bits)[0]
                assert differ.size == 0, (c, int(differ[0]), strings[int(differ[0])][:80], hex(int(values[differ[0]])), hex(int(w_bits[differ[0]])))
                assert (values[k:] == POISON_U).all(), c
                if want_status:
                    differ = np.nonzero(status[:k] != w_status)[0]
                    assert differ.size == 0, (c, int(differ[0]), strings[int(differ[0])][:80], int(status[differ[0]]), int(w_status[differ[0]]))
                    assert (status[k:] == POISON8).all(), c
                else:
                    assert (status == POISON8).all(), c
                if want_stats:
                    assert stats == w_stats and sum(stats.values()) == k, (c, stats, w_stats)
            if api:
                a_values, a_status, a_stats = scan.parse_time_records(T.d, T.rb_t, T.re_t, fmt, indices=T.idx_t, unit=tc.UNIT_NAMES[unit], trim=trim, stats=True)
                assert a_values.numel() == k and a_status.numel() == k and a_status.dtype == torch.uint8 and a_values.dtype == torch.int64 and a_stats == w_stats, c
                assert (a_values.cpu().numpy().view(np.uint64) == w_bits).all() and (a_status.cpu().numpy() == w_status).all(), c
                only = scan.parse_time_records(T.d, T.rb_t, T.re_t, fmt.decode("latin-1") if max(fmt) < 128 else fmt, indices=T.idx_t, unit=tc.UNIT_NAMES[unit], trim=trim)
                assert len(only) == 2 and (only[0].cpu().numpy().view(np.uint64) == w_bits).all()


# ------------------------------------------------------------------------------------------------ every family, per format
@pytest.mark.parametrize("fmt", tc.FORMATS, ids=IDS)
def test_every_family_under_every_unit_and_flag(rj, scan, fmt):
    rows = tc.status_rows(fmt)
    check(rj, scan, laid(rows), fmt, api=True, ctx="families")
    seen = {meaning(r, fmt, unit, trim)[0] for r in rows for unit in tc.UNITS for trim in (False, True)}
    assert seen == {tc.OK, tc.EMPTY, tc.MALFORMED, tc.RANGE} | ({tc.INEXACT} if tc.has(fmt, "f") else set())
    good = tc.render(fmt)
    assert meaning(good[:-1], fmt, 0, False)[0] == tc.MALFORMED and meaning(good + b"0", fmt, 0, False)[0] == tc.MALFORMED
    assert meaning(b" " + good, fmt, 0, False)[0] == tc.MALFORMED and meaning(b" " + good + b"\t", fmt, 3, True)[0] == tc.OK


# ------------------------------------------------------------------------------------------------ seams
def test_the_seam_rows_at_every_begin_alignment_and_the_texts_end(rj, scan):
    """A 26-byte CLF row (one group seam) and a 35-byte ISO row with nine fraction digits (two), whole and with every byte
    spoilt in turn, each laid at every begin alignment 0..15: every field passes every seam.  The last row ends at the text's
    last byte (the guarded load).  Then the same texts behind one byte more."""
    for fmt, row in tc.placed_rows():
        rows, text, records = [], bytearray(), []
        for s in [row] + [row[:i] + b"?" + row[i + 1:] for i in range(len(row))]:
            part, recs = tc.lay_at_every_alignment(s)
            while len(text) % 16:
                text += b"|"
            records += [(b + len(text), e + len(text)) for b, e in recs]
            text += part
            rows += [s] * 16
        assert {b % 16 for b, _ in records[:16]} == set(range(16)) and records[-1][1] == len(text) and len(text) % 16 != 0
        T = Table(bytes(text), records)
        assert int(T.d.data_ptr()) % 16 == 0 and T.strings() == rows
        check(rj, scan, T, fmt, ctx="seams")
        assert [meaning(row, fmt, u, False)[0] for u in tc.UNITS] == ([tc.OK] * 4 if fmt == tc.CLF else [tc.INEXACT] * 3 + [tc.OK])
        check(rj, scan, Table(b"#" + bytes(text), [(b + 1, e + 1) for b, e in records]), fmt, units=(tc.NANO,), trims=(True,), ctx="shifted")


def test_rows_of_a_mebibyte(rj, scan):
    """a MiB of bytes that fit (trimmed blanks) before the garbage: one lane's whole walk, MALFORMED at its end; and a MiB row
    that is MALFORMED at byte 0, which stops there"""
    good = tc.render(tc.ISO)
    MiB = 1 << 20
    rows = [good, good + b" " * MiB + b"x", b"\t" * MiB + good + b"x", b"x" + good * (MiB // len(good)), good + b" " * MiB, b" " * MiB + good]
    want = [(tc.OK, 971166336), (tc.MALFORMED, 0), (tc.MALFORMED, 0), (tc.MALFORMED, 0), (tc.OK, 971166336), (tc.OK, 971166336)]
    assert meaning(good, tc.ISO, tc.SECOND, True) == want[0] and meaning(rows[3][:200], tc.ISO, 0, True) == want[3]
    T = laid(rows, sep_of=lambda i: b"|")
    check(rj, scan, T, tc.ISO, units=(tc.SECOND,), trims=(True,), want=want, ctx="MiB", variants=((True, True),))
    check(rj, scan, T, tc.ISO, units=(tc.SECOND,), trims=(False,), want=[want[0]] + [(tc.MALFORMED, 0)] * 5, ctx="MiB", variants=((True, True),))


# ------------------------------------------------------------------------------------------------ the calendar
@pytest.mark.parametrize("fmt", (tc.ISO, tc.CLF, tc.PLAIN, tc.DATE), ids=["iso", "clf", "plain", "date"])
def test_the_calendar_equals_datetime(rj, scan, fmt):
    """The second before, at and after the calendar's edges; the last day and the day behind it of every month of 1900, 2000,
    2023 and 2024; offsets of +-23:59 across a day, a year and year 1; +24:00 and +00:60; 4096 seeded instants over the whole
    range -- against the seconds datetime itself gives."""
    rows, secs = tc.calendar_rows(fmt)
    assert len(rows) > 4096 + 96 and sum(1 for w in secs if w is None) >= 48
    T = laid(rows)
    for unit in (tc.SECOND, tc.MICRO):
        want = [(tc.RANGE, 0) if w is None else (tc.OK, (w * 10 ** (3 * unit)) & tc.MASK) for w in secs]
        check(rj, scan, T, fmt, units=(unit,), trims=(False,), want=want, ctx="calendar", variants=((True, True),))
    if fmt == tc.ISO:
        assert (tc.OK, tc.MASK) in [(tc.OK, w & tc.MASK) for w in secs if w is not None]      # 1969-12-31T23:59:59 is -1
        assert min(w for w in secs if w is not None) == -62135596800 - 86340 and max(w for w in secs if w is not None) == 253402300799 + 86340


def test_nanos_range(rj, scan):
    pairs = tc.nano_rows()
    T = laid([r for r, _ in pairs])
    check(rj, scan, T, tc.ISO_F, units=(tc.NANO,), trims=(False,), want=[w for _, w in pairs], ctx="nano")
    assert pairs[0][1] == (tc.OK, 1 << 63) and pairs[3][1] == (tc.OK, (1 << 63) - 1)
    check(rj, scan, T, tc.ISO_F, ctx="nano rows, every unit")


def test_inexact_and_its_place_in_the_order(rj, scan):
    pairs = tc.inexact_rows()
    T = laid([r for r, _ in pairs])
    for unit in tc.UNITS:
        total, values, status, stats = call_poisoned(rj, scan, T, tc.ISO_F, unit, 0)
        assert status[:len(pairs)].tolist() == [w[unit] for _, w in pairs], unit
    check(rj, scan, T, tc.ISO_F, ctx="inexact")
    assert meaning(b"2000-10-10T13:55:36.500000000Z", tc.ISO_F, tc.MILLI, False) == (tc.OK, 971186136500)


# ------------------------------------------------------------------------------------------------ table rules
@pytest.fixture(scope="module")
def pool():
    rows = tc.status_rows(tc.CLF) + tc.calendar_rows(tc.CLF)[0][:700]
    random.Random(3).shuffle(rows)
    assert len(rows) >= 800
    return rows


def test_index_lists_null_status_and_no_rows(rj, scan, pool):
    T = laid(pool[:400])
    rng = random.Random(9)
    perm = list(range(400))
    rng.shuffle(perm)
    for name, rows in (("permutation", perm), ("repeats", [rng.randrange(400) for _ in range(1000)]), ("one row", [123] * 300), ("none", []),
                       ("reversed", list(range(399, -1, -1)))):
        check(rj, scan, T.take(rows), tc.CLF, units=(tc.SECOND, tc.NANO), api=name in ("repeats", "none"), ctx=name)
    for k in (0, 1, 63, 64, 65, 255, 256, 257):
        check(rj, scan, laid(pool[:k]), tc.CLF, units=(tc.MILLI,), trims=(True,), api=k in (0, 257), ctx="sizes")


def test_refusals_leave_the_poison_and_name_what_they_name(rj, scan, pool):
    import torch
    lib = rj.load_library()
    T = laid(pool[:700])
    n = len(T.data)

    def refused(why, T2, message):
        total, values, status, _ = call_poisoned(rj, scan, T2, tc.CLF, tc.SECOND, 1)
        msg = lib.rj_last_error().decode()
        assert total == RJ_BAD_ARGUMENT and message in msg, (why, total, msg)
        assert (values == POISON_U).all() and (status == POISON8).all(), why
        with pytest.raises(rj.RejitError) as err:
            scan.parse_time_records(T2.d, T2.rb_t, T2.re_t, tc.CLF, indices=T2.idx_t)
        assert err.value.status == RJ_BAD_ARGUMENT and message in err.value.message
        check(rj, scan, T.take(range(0, 700, 9)), tc.CLF, units=(tc.SECOND,), trims=(True,))      # the same scan answers a good call

    bad = list(range(0, 700, 2))
    bad[11], bad[340] = 700, -1
    refused("two bad indices: the smaller row is named", T.take(bad), "row 11 names no record or a record outside the text (index < n_records, begin <= end <= n)")
    bad = list(range(700))
    bad[0], bad[699] = 700, 700
    refused("a bad index at the first row", T.take(bad), "row 0 ")
    recs = list(T.records)
    recs[699] = (recs[699][0], n + 1)
    refused("the last row ends behind the text", Table(T.data, recs, d=T.d), "row 699 ")
    recs = list(T.records)
    recs[650] = (recs[650][0] + 1, recs[650][0])
    recs[651] = (n + 5, n + 6)
    refused("begin > end", Table(T.data, recs, d=T.d), "row 650 ")
    # arguments
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    f = lib.rj_scan_records_parse_time
    out = torch.full((708,), POISON, dtype=torch.int64, device="cuda:0")
    out8 = torch.full((708,), POISON8, dtype=torch.uint8, device="cuda:0")
    good = [scan._h, vp(T.d), n, vp(T.rb_t), vp(T.re_t), 700, None, 0, tc.CLF, len(tc.CLF), tc.SECOND, 0, vp(out), vp(out8), None, st]
    assert f(*good) >= 0
    out.fill_(POISON), out8.fill_(POISON8)
    for at in (0, 1, 3, 4, 8, 12):                                         # the scan, the text, either table, the format, d_value
        args = list(good)
        args[at] = None
        assert f(*args) == RJ_BAD_ARGUMENT and lib.rj_last_error().decode() == "rj_scan_records_parse_time: null argument", at
    off = lambda x: ctypes.c_void_p(x.data_ptr() + 4)
    for at, x in ((3, T.rb_t), (4, T.re_t), (6, T.rb_t), (12, out)):
        args = list(good)
        args[at] = off(x)
        if at == 6:
            args[7] = 5
        assert f(*args) == RJ_BAD_ARGUMENT and lib.rj_last_error().decode() == "rj_scan_records_parse_time: a table is not 8-byte aligned", at
    for fmt, offset in tc.REFUSED_FORMATS:
        args = list(good)
        args[8], args[9] = fmt, len(fmt)
        assert f(*args) == RJ_BAD_ARGUMENT and lib.rj_last_error().decode().startswith("rj_scan_records_parse_time: format byte %d: " % offset), (fmt, lib.rj_last_error())
    with pytest.raises(rj.RejitError) as err:
        scan.parse_time_records(T.d, T.rb_t, T.re_t, "%H:%M:%S")
    assert err.value.status == RJ_BAD_ARGUMENT and "format byte 8: " in err.value.message
    for fmt in tc.ACCEPTED_FORMATS:
        args = list(good)
        args[8], args[9] = fmt, len(fmt)
        assert f(*args) >= 0, (fmt, lib.rj_last_error())
    out.fill_(POISON), out8.fill_(POISON8)
    for unit in (-1, 4, 7):
        args = list(good)
        args[10] = unit
        assert f(*args) == RJ_BAD_ARGUMENT and "unit" in lib.rj_last_error().decode(), unit
    with pytest.raises(ValueError):
        scan.parse_time_records(T.d, T.rb_t, T.re_t, tc.CLF, unit="m")
    for flags in (2, 3, 4, 5, 0x80000000):
        args = list(good)
        args[11] = flags
        assert f(*args) == RJ_BAD_ARGUMENT and "flag" in lib.rj_last_error().decode(), flags
    args = list(good)
    args[5] = 1 << 31
    assert f(*args) == RJ_TOO_LARGE and "2^31" in lib.rj_last_error().decode()
    args = list(good)
    args[6], args[7] = vp(T.rb_t), 1 << 31
    assert f(*args) == RJ_TOO_LARGE
    assert bool((out == POISON).all()) and bool((out8 == POISON8).all())
    # no rows: nothing is needed, nothing is touched
    assert f(scan._h, None, 0, None, None, 0, None, 0, tc.DATE, len(tc.DATE), tc.NANO, 1, None, None, None, st) == 0
    args = list(good)
    args[6], args[7], args[12] = vp(T.rb_t), 0, None
    assert f(*args) == 0 and bool((out8 == POISON8).all())
    # a status byte table at any alignment is fine
    args = list(good)
    args[13] = ctypes.c_void_p(out8.data_ptr() + 1)
    assert f(*args) >= 0 and int(out8[0]) == POISON8 and int(out8[701]) == POISON8


# ------------------------------------------------------------------------------------------------ more than one pass of the grid
def library_grid():
    """kTimeGrid, read from the unit's source (profiles/time_kernel_resources.txt has the occupancy it comes from)"""
    with open(os.path.join(ROOT, "rejit_amd", "csrc", "record_time.hip")) as fh:
        found = re.search(r"constexpr unsigned kTimeGrid = (\d+) \* (\d+);", fh.read())
    return int(found.group(1)) * int(found.group(2))


def test_a_table_of_more_than_one_pass_of_the_grid_equals_numpy(rj, scan):
    """(grid x 256) + 256 + 65 rows of 19 bytes, 20 bytes apart (so their begins pass every alignment that is a multiple of 4),
    built vectorised; a known share of bad rows at fixed positions, the very last row among them.  The expected values are
    numpy.datetime64's reading of the same strings."""
    import torch
    grid = library_grid()
    assert 256 <= grid <= 256 * 8
    k = grid * 256 + 256 + 65
    rng = np.random.default_rng(1970)
    secs = rng.integers(-62135596800, 253402300800, size=k, dtype=np.int64)
    strings = np.datetime_as_string(secs.astype("datetime64[s]"), unit="s").astype("S19")
    want = strings.astype("U19").astype("datetime64[s]").astype(np.int64)      # numpy reads the text back
    assert (want == secs).all()
    lines = np.full((k, 20), 10, dtype=np.uint8)
    lines[:, :19] = strings.view(np.uint8).reshape(k, 19)
    malformed = np.zeros(k, dtype=bool)
    malformed[::1000] = True
    malformed[k - 1] = True
    lines[malformed, 11] = ord("x")                                       # the hour's first digit
    out_of_range = np.zeros(k, dtype=bool)
    out_of_range[7::1777] = True
    out_of_range &= ~malformed
    lines[out_of_range, 5:7] = (ord("1"), ord("3"))                       # month 13
    w_status = np.where(malformed, tc.MALFORMED, np.where(out_of_range, tc.RANGE, tc.OK)).astype(np.uint8)
    w_values = np.where(w_status == tc.OK, want, 0)
    text = torch.from_numpy(lines.reshape(-1)).to("cuda:0")
    begins = torch.arange(k, dtype=torch.int64, device="cuda:0") * 20
    ends = begins + 19
    values = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    status = torch.full((k + ROOM,), POISON8, dtype=torch.uint8, device="cuda:0")
    lib = rj.load_library()
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    out = (ctypes.c_uint64 * 5)()
    fmt = b"%Y-%m-%dT%H:%M:%S"
    total = lib.rj_scan_records_parse_time(scan._h, vp(text), int(text.numel()), vp(begins), vp(ends), k, None, 0, fmt, len(fmt), tc.SECOND, 0, vp(values),
                                           vp(status), ctypes.cast(out, lib.rj_scan_records_parse_time.argtypes[14]),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    n_bad, n_range = int(malformed.sum()), int(out_of_range.sum())
    assert total == k - n_bad - n_range and [int(x) for x in out] == [k - n_bad - n_range, 0, n_bad, n_range, 0]
    assert n_bad >= k // 1000 and n_range >= k // 1777 - 1 and w_status[-1] == tc.MALFORMED
    got_v, got_s = values.cpu().numpy(), status.cpu().numpy()
    assert (got_v[:k] == w_values).all() and (got_s[:k] == w_status).all()
    assert (got_v[k:] == POISON).all() and (got_s[k:] == POISON8).all()
    # a few rows against the Python meaning too
    data = lines.reshape(-1).tobytes()
    for j in (0, 7, 1000, 255, 256, grid * 256 - 1, grid * 256, k - 2, k - 1):
        assert meaning(data[j * 20:j * 20 + 19], fmt, tc.SECOND, False) == (int(w_status[j]), int(w_values[j]) & tc.MASK), j


# ------------------------------------------------------------------------------------------------ the scan's state
def test_the_scans_spans_stats_and_selection_stay(rj, pool):
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    t = W.log_like_numpy(1 << 16, 3)
    d = torch.from_numpy(t).to("cuda:0")
    s = rj.Scan(rj.Program(b"[0-9]+"))
    rb_t, re_t = R.line_records(d)
    res = s.run_records(d, rb_t, re_t)
    sel0, spans0, stats0 = s.select_records().clone(), s.spans_tensor(d.device).clone(), s.stats()
    assert res.n_matching > 20
    check(rj, s, laid(pool[:300]), tc.CLF, units=(tc.SECOND, tc.NANO), trims=(True,), api=True)
    assert torch.equal(s.spans_tensor(d.device), spans0) and torch.equal(s.select_records(), sel0) and s.stats() == stats0
    assert s.run_records(d, rb_t, re_t).n_kept == res.n_kept


# ------------------------------------------------------------------------------------------------ end to end
def log_lines(count, seed):
    """synthetic log lines whose fourth blank-separated field is an ISO timestamp, some of them spoilt or missing"""
    rng = random.Random(seed)
    base = datetime.datetime(1969, 12, 31, 23, 0, 0)
    spoilt = (b"-", b"2000-13-01T00:00:00Z", b"yesterday", b"2000-01-01T00:00:00", b"2000-01-01T00:00:00.5Z", b"")
    lines = []
    for i in range(count):
        dt = base + datetime.timedelta(seconds=rng.randrange(0, 3 * 3600))
        stamp = tc.of_instant(tc.ISO, dt, zone=rng.choice((b"Z", b"+00:00", b"-0100", b"+05:30")))
        if rng.randrange(9) == 0:
            stamp = rng.choice(spoilt)
        line = b"10.0.0.%d - u%d %s GET /p%d %d" % (rng.randrange(256), rng.randrange(9), stamp, rng.randrange(40), rng.choice((200, 404, 500)))
        lines.append(line if rng.randrange(50) else b"short line")
    return lines


def expected_buckets(lines, width, keep=lambda line: True):
    """a Python dict over datetime.strptime: the count per bucket start"""
    epoch = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
    counts = {}
    for line in lines:
        parts = line.split(b" ")
        if not keep(line) or len(parts) < 4 or tc.meaning(parts[3], tc.ISO, tc.SECOND, True)[0] != tc.OK:
            continue
        secs = (datetime.datetime.strptime(parts[3].decode(), tc.ISO.decode()) - epoch) // datetime.timedelta(seconds=1)
        start = secs // width * width
        counts[start] = counts.get(start, 0) + 1
    return counts


def test_split_parse_and_buckets_equal_a_dict_over_strptime(rj):
    import torch
    from rejit_amd import records as R
    if not tc.english_months():
        pytest.skip("LC_TIME's month names are not the English ones")
    lines = log_lines(3000, 11)
    data = b"\n".join(lines)
    d = dev_text(data)
    s = rj.Scan(rj.Program(b" "))
    rb_t, re_t = R.line_records(d)
    res = s.run_records(d, rb_t, re_t)
    pb, pe, pf = s.split_records(rb_t, re_t, res, len(data), what="between")
    tb, te, _ = R.field_records(pb, pe, pf, 3)
    values, status, stats = s.parse_time_records(d, tb, te, tc.ISO, unit="s", trim=True, stats=True)
    for width in (60, 3600):
        start, ok = R.time_buckets(values, status, width)
        buckets, counts = torch.unique(start[ok], return_counts=True)
        want = expected_buckets(lines, width)
        assert dict(zip(buckets.cpu().tolist(), counts.cpu().tolist())) == want
        assert min(want) < 0 < max(want) and sum(want.values()) == stats["n_ok"] < len(lines)
    assert stats["n_empty"] > 0 and stats["n_malformed"] > 0 and stats["n_range"] > 0


def test_linegrep_sample_counts_lines_per_time_bucket(rj, tmp_path):
    lines = log_lines(2000, 12)
    path = str(tmp_path / "access.log")
    with open(path, "wb") as fh:
        fh.write(b"\n".join(lines) + b"\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    fmt = tc.ISO.decode()
    show = lambda want: b"".join(b"%7d %d\n" % (want[b], b) for b in sorted(want))
    r = subprocess.run([sys.executable, sample, path, " ", "-f", "4", "-T", fmt, "-w", "60"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-500:])
    want = expected_buckets(lines, 60)
    assert r.stdout == show(want) and len(want) > 100 and min(want) < 0
    # with -p only the lines that have a separator are read (every line here has one)
    r = subprocess.run([sys.executable, sample, path, " ", "-p", "-f", "4", "-T", fmt, "-w", "3600"], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == show(expected_buckets(lines, 3600)), (r.returncode, r.stderr.decode()[-500:])


def test_linegrep_sample_refuses_t_without_its_companions(rj, tmp_path):
    path = str(tmp_path / "x.log")
    with open(path, "wb") as fh:
        fh.write(b"a b c 2000-10-10T13:55:36Z\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    fmt = tc.ISO.decode()
    for opts in (["-T", fmt, "-w", "60"], ["-f", "4", "-T", fmt], ["-f", "4", "-w", "60"], ["-f", "4", "-T", fmt, "-w", "0"], ["-f", "4", "-T", fmt, "-w", "x"],
                 ["-f", "4", "-T", fmt, "-w", "60", "-u"], ["-o", "-T", fmt, "-w", "60"], ["-f", "4", "-T", fmt, "-w", "60", "-b"],
                 ["-f", "4", "-T", fmt, "-w", "60", "-n"], ["-f", "4", "-T", fmt, "-w", "60", "-k", path], ["-f", "4", "-T", fmt, "-w", "60", "-s", "x"],
                 ["-f", "4", "-T", fmt, "-w", "60", "-D"], ["-f", "4", "-T", "%H:%M", "-w", "60"]):
        r = subprocess.run([sys.executable, sample, path, " "] + opts, capture_output=True, timeout=60)
        assert r.returncode == 2 and r.stdout == b"", opts
    r = subprocess.run([sys.executable, sample, path, " ", "-f", "4", "-T", fmt, "-w", "3600"], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"      1 971182800\n", (r.stdout, r.stderr.decode()[-300:])
