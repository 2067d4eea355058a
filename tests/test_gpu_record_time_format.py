"""GPU tests (-m gpu) of rj_scan_records_format_time (rejit_amd/csrc/record_time_format.hip; Scan.format_time_records): a
column of int64 instants written as text under a strftime-style format on the device, laid out as a pack.

The meaning is tests/time_format_cases.py's, written in Python independently of the library: divmod, datetime + timedelta,
the fields by hand, the layout arithmetic and the status rule.  Every comparison is exact.  Outputs are poisoned first, with
room behind the text and the tables that must stay poisoned."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import time_format_cases as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_BAD_ARGUMENT, RJ_TOO_LARGE = -4, -2
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON8 = 0xA5
ROOM = 7                          # spare table rows
ROOM_BYTES = 53                   # spare output bytes
UNIT_GRID_ROWS = 1024 * 256       # record_frame.h: unit_grid() workgroups of 256 rows, one pass of the check and of the plan
EMIT_GRID_BYTES = 256 * 8 * 4096  # record_time_format.hip: kCopyGrid workgroups, a chunk of kEmitChunk bytes each: one turn of the emit


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
    return rj.Scan(rj.Program(b"[0-9]+"))


def dev(x, dtype=np.int64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to("cuda:0")


class Column:
    """a unit's values (tests/time_format_cases.py: values_of) on the device, with a status column"""

    def __init__(self, unit):
        self.unit, self.values = unit, tf.values_of(unit)
        self.status = tf.status_column(len(self.values))
        self.d, self.d_status = dev(self.values), dev(self.status, np.uint8)


@pytest.fixture(scope="module")
def columns(rj):
    return {unit: Column(unit) for unit in tf.UNITS}


def format_poisoned(rj, scan, d_value, n_values, fmt, unit, d_status=None, idx_t=None, zone=0, fill=10, lead=0, gap=1, cap=0, flags=0, with_begin=True,
                    with_end=True, with_stats=True):
    """the raw call into poisoned buffers -> (return value, out bytes with the spare ones, begins, ends with the spare rows, stats)"""
    import torch
    lib = rj.load_library()
    k = n_values if idx_t is None else int(idx_t.numel())
    out = torch.full((cap + ROOM_BYTES,), POISON8, dtype=torch.uint8, device="cuda:0")
    begins = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    ends = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    assert out.data_ptr() % 16 == 0
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    counts = rj.api._FormatTimeStats(77, 77, 77)
    total = lib.rj_scan_records_format_time(scan._h, vp(d_value) if n_values else None, None if d_status is None else vp(d_status), n_values,
                                            None if idx_t is None else vp(idx_t), 0 if idx_t is None else k, fmt, len(fmt), unit, zone, flags, fill, lead, gap,
                                            vp(out) if cap else None, cap, vp(begins) if with_begin else None, vp(ends) if with_end else None,
                                            ctypes.byref(counts) if with_stats else None,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return int(total), out.cpu().numpy().tobytes(), begins.cpu().numpy(), ends.cpu().numpy(), [counts.n_ok, counts.n_null, counts.n_range]


def check(rj, scan, C, fmt, status=False, indices=None, zone=0, fill=10, lead=0, gap=1, ctx=None):
    """size query, then the call with an exact capacity, against time_format_cases.layout"""
    text, begins, ends, counts = tf.layout(C.values, fmt, C.unit, C.status if status else None, None if indices is None else list(indices), zone, fill, lead, gap)
    idx_t = None if indices is None else dev(indices)
    d_status = C.d_status if status else None
    k = len(begins)
    c = (ctx, fmt, C.unit, status, indices is not None, zone, fill, lead, gap)
    want_stats = [counts[tf.OK], counts[tf.NULL], counts[tf.RANGE]]
    total, out, gb, ge, stats = format_poisoned(rj, scan, C.d, len(C.values), fmt, C.unit, d_status, idx_t, zone, fill, lead, gap, cap=0)
    assert total == len(text), (c, total, rj.load_library().rj_last_error())
    assert out == bytes([POISON8]) * ROOM_BYTES and (gb[:k] == begins).all() and (ge[:k] == ends).all() and stats == want_stats, c
    total, out, gb, ge, stats = format_poisoned(rj, scan, C.d, len(C.values), fmt, C.unit, d_status, idx_t, zone, fill, lead, gap, cap=len(text))
    assert total == len(text), (c, total, rj.load_library().rj_last_error())
    if out[:total] != text:
        at = next(i for i in range(total) if out[i] != text[i])
        raise AssertionError((c, "first differing byte", at, out[max(at - 40, 0):at + 40], text[max(at - 40, 0):at + 40]))
    assert out[total:] == bytes([POISON8]) * ROOM_BYTES, c
    assert (gb[:k] == begins).all() and (ge[:k] == ends).all() and (gb[k:] == POISON).all() and (ge[k:] == POISON).all() and stats == want_stats, c
    return text, begins, ends, counts


# ------------------------------------------------------------------------------------------------ the families
@pytest.mark.parametrize("fmt", tf.FORMATS, ids=tf.FORMAT_IDS)
def test_the_families_per_format_unit_and_zone(rj, scan, columns, fmt):
    """the epoch, -1, both ends of the range with their outside neighbours (also as the zones +-1439 see them), both ends of
    int64, leap days, century rules, month ends and seeded values: bytes, both tables and the three counts"""
    for unit in tf.UNITS:
        for zone in tf.ZONES:
            _, _, _, counts = check(rj, scan, columns[unit], fmt, status=zone in (330, -1439), zone=zone)
            assert counts[tf.OK] > 300 and (counts[tf.RANGE] > 20) == (unit != tf.NANO)


def test_layouts_fills_either_table_null_and_the_size_query(rj, scan, columns):
    C = columns[tf.MILLI]
    for lead in (0, 1, 15, 16, 17):
        for gap in (0, 1, 5):
            check(rj, scan, C, tf.ISO_F, True, None, 330, (10, 0, 0x2C)[(lead + gap) % 3], lead, gap)
    text, begins, ends, _ = tf.layout(C.values, tf.CLF, C.unit, C.status, None, -420, 0x2C, 5, 2)
    k = len(begins)
    for with_begin, with_end, with_stats in ((True, False, True), (False, True, False), (False, False, True)):
        for cap in (0, len(text)):
            total, out, gb, ge, stats = format_poisoned(rj, scan, C.d, k, tf.CLF, C.unit, C.d_status, None, -420, 0x2C, 5, 2, cap=cap, with_begin=with_begin,
                                                        with_end=with_end, with_stats=with_stats)
            assert total == len(text) and out[:cap] == text[:cap] and out[cap:] == bytes([POISON8]) * ROOM_BYTES
            assert (gb[:k] == begins).all() if with_begin else (gb == POISON).all()
            assert (ge[:k] == ends).all() if with_end else (ge == POISON).all()
            assert stats[0] + stats[1] + stats[2] == k if with_stats else stats == [77, 77, 77]
    # an out_cap below the total: nothing at or beyond out_cap is touched, and what lies below it is complete
    for cap in (1, 15, 16, 17, 4096, 4097, len(text) - 1, len(text) - 17):
        total, out, _, _, _ = format_poisoned(rj, scan, C.d, k, tf.CLF, C.unit, C.d_status, None, -420, 0x2C, 5, 2, cap=cap)
        assert total == len(text) > 4200 and out[:cap] == text[:cap] and out[cap:] == bytes([POISON8]) * ROOM_BYTES, cap


@pytest.mark.parametrize("fmt,unit,gap,pitch", [(tf.ISO, tf.SECOND, 1, 21), (tf.LONGEST, tf.NANO, 0, 77)], ids=["iso_pitch_21", "longest_pitch_77"])
def test_every_cut_of_a_row_by_a_chunk_seam(rj, scan, fmt, unit, gap, pitch):
    """4097 OK rows of one length: both pitches are odd, so the seams at the multiples of 4096 fall on every phase of a row
    within the first `pitch` chunks (4096 is invertible modulo an odd pitch)"""
    k = 4097
    per = 10 ** (3 * unit)
    rng = np.random.RandomState(7)
    values = (rng.randint(0, 4 * 10 ** 9, k).astype(np.int64) * per + rng.randint(0, per, k)).tolist()
    assert tf.row_length(fmt, unit) + gap == pitch and pitch % 2 == 1 and k * pitch > pitch * 4096
    phases = {(c * 4096) % pitch for c in range(1, k * pitch // 4096 + 1)}
    assert phases == set(range(pitch))
    text, begins, ends, counts = tf.layout(values, fmt, unit, None, None, 0, 0x2C, 0, gap)
    assert counts[tf.OK] == k
    total, out, gb, ge, stats = format_poisoned(rj, scan, dev(values), k, fmt, unit, fill=0x2C, gap=gap, cap=len(text))
    assert total == len(text) == k * pitch, (total, rj.load_library().rj_last_error())
    got, want = np.frombuffer(out[:total], dtype=np.uint8).reshape(k, pitch), np.frombuffer(text, dtype=np.uint8).reshape(k, pitch)
    rows = np.nonzero((got != want).any(axis=1))[0]
    assert rows.size == 0, (rows[:5], bytes(got[rows[0]]), bytes(want[rows[0]]))
    assert out[total:] == bytes([POISON8]) * ROOM_BYTES and (gb[:k] == begins).all() and (ge[:k] == ends).all() and stats == [k, 0, 0]


def test_more_than_256_empty_rows_inside_one_chunk(rj, scan):
    """gap 0: runs of 300, 700 and 5000 empty rows (null status and out of range, mixed) between OK rows; the counts are exact"""
    values, status = [], []
    for run in (300, 1, 700, 2, 5000, 0):
        values += [tf.INT64_MAX if i % 3 else 5 for i in range(run)] + [971211336, 0]
        status += [0 if i % 3 else 2 for i in range(run)] + [0, 0]
    for gap in (0, 1):
        text, begins, ends, counts = tf.layout(values, tf.CLF, tf.SECOND, status, None, 60, 10, 3, gap)
        total, out, gb, ge, stats = format_poisoned(rj, scan, dev(values), len(values), tf.CLF, tf.SECOND, dev(status, np.uint8), zone=60, lead=3, gap=gap,
                                                    cap=len(text))
        assert total == len(text) and out[:total] == text and out[total:] == bytes([POISON8]) * ROOM_BYTES
        assert (gb[:len(begins)] == begins).all() and (ge[:len(ends)] == ends).all()
        assert stats == [counts[tf.OK], counts[tf.NULL], counts[tf.RANGE]] and counts[tf.OK] == 12 and counts[tf.NULL] > 2000 and counts[tf.RANGE] == 4000
    assert len(tf.layout(values, tf.CLF, tf.SECOND, status, None, 60, 10, 3, 0)[0]) == 3 + 12 * 26


def test_the_tail_store_under_an_out_cap_sweep(rj, scan):
    """an output of two chunks and 21 bytes: below min(out_cap, total) the reference's bytes, at and beyond it the sentinel, and
    the total returned whatever out_cap is"""
    k = 391
    values = (np.random.RandomState(11).randint(0, 4 * 10 ** 9, k).astype(np.int64)).tolist()
    text, begins, ends, counts = tf.layout(values, tf.ISO, tf.SECOND, None, None, 0, 0x2C, 2, 1)
    total = len(text)
    assert total == 2 * 4096 + 21 and counts[tf.OK] == k
    d = dev(values)
    for cap in (1, 15, 16, 17, 4095, 4096, 4097, total - 17, total - 16, total - 1, total, total + 16):
        got, out, gb, ge, stats = format_poisoned(rj, scan, d, k, tf.ISO, tf.SECOND, fill=0x2C, lead=2, gap=1, cap=cap)
        below = min(cap, total)
        assert got == total, (cap, got, rj.load_library().rj_last_error())
        assert out[:below] == text[:below] and out[below:] == bytes([POISON8]) * (cap + ROOM_BYTES - below), cap
        assert (gb[:k] == begins).all() and (ge[:k] == ends).all() and stats == [k, 0, 0], cap


def test_more_than_one_pass_of_both_grids(rj, scan):
    """262 465 rows at a pitch of 33 bytes: the check and the plan take their units round again, and the output passes the 8 MiB
    of one turn of the emit.  The ISO-shaped rows are compared in bulk with numpy.datetime_as_string over datetime64[s]; a
    sample of them, and the rows out of range, with the datetime oracle.  Then one bad index in the second pass."""
    k, gap, L = UNIT_GRID_ROWS + 256 + 65, 14, 19
    fmt = b"%Y-%m-%dT%H:%M:%S"
    assert (L + gap) >= 33 and k * (L + gap) > EMIT_GRID_BYTES
    rng = np.random.RandomState(99)
    n_values = 50000
    values = rng.randint(tf.FIRST_SECOND, tf.LAST_SECOND + 1, n_values).astype(np.int64)
    values[:4] = [tf.FIRST_SECOND, tf.LAST_SECOND, tf.FIRST_SECOND - 1, tf.LAST_SECOND + 1]      # (never NaT's bit pattern: that is INT64_MIN)
    pk = rng.randint(0, n_values, k).astype(np.int64)
    pk[-70:-66] = [0, 1, 2, 3]
    picked = values[pk]
    ok = (picked >= tf.FIRST_SECOND) & (picked <= tf.LAST_SECOND)
    lens = np.where(ok, L, 0).astype(np.int64)
    begins = 2 + np.concatenate([[0], np.cumsum(lens + gap)[:-1]])
    want_total = 2 + int((lens + gap).sum())
    total, out, gb, ge, stats = format_poisoned(rj, scan, dev(values), n_values, fmt, tf.SECOND, None, dev(pk), fill=0x7C, lead=2, gap=gap, cap=want_total)
    assert total == want_total, (total, rj.load_library().rj_last_error())
    assert (gb[:k] == begins).all() and (ge[:k] == begins + lens).all() and (gb[k:] == POISON).all() and (ge[k:] == POISON).all()
    assert stats == [int(ok.sum()), 0, int((~ok).sum())] and stats[2] >= 2
    got = np.frombuffer(out, dtype=np.uint8)
    assert (got[total:] == POISON8).all()
    want = np.full(total, 0x7C, dtype=np.uint8)
    rows = np.frombuffer(np.datetime_as_string(picked[ok].view("datetime64[s]")).astype("S19").tobytes(), dtype=np.uint8).reshape(-1, L)
    want[(begins[ok][:, None] + np.arange(L)[None, :]).reshape(-1)] = rows.reshape(-1)
    differing = np.nonzero(got[:total] != want)[0]
    assert differing.size == 0, (differing[:5], bytes(got[differing[0] - 20:differing[0] + 20]), bytes(want[differing[0] - 20:differing[0] + 20]))
    for j in list(range(0, k, 997)) + list(range(k - 70, k - 66)):
        assert bytes(got[gb[j]:ge[j]]) == tf.text_of(int(picked[j]), fmt, tf.SECOND), j
    bad = pk.copy()
    at = k - 1                                   # a row of the second pass
    assert UNIT_GRID_ROWS <= at < k
    bad[at] = n_values
    total, out, gb, ge, stats = format_poisoned(rj, scan, dev(values), n_values, fmt, tf.SECOND, None, dev(bad), gap=gap, cap=want_total)
    msg = rj.load_library().rj_last_error().decode()
    assert total == RJ_BAD_ARGUMENT and "row %d " % at in msg, (total, msg)
    assert out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all() and stats == [77, 77, 77]


@pytest.mark.parametrize("unit", tf.UNITS, ids=[tf.UNIT_NAMES[u] for u in tf.UNITS])
def test_round_trip_on_the_device(rj, scan, unit):
    """parse_time_records(format_time_records(v)) gives v with every row OK: 4096 seeded instants per unit, two formats, a zone"""
    import torch
    per = 10 ** (3 * unit)
    rng = np.random.RandomState(40 + unit)
    lo, hi = (-9223372036, 9223372036) if unit == tf.NANO else (tf.FIRST_SECOND + 86400, tf.LAST_SECOND - 86400)
    v = torch.from_numpy(rng.randint(lo, hi, 4096).astype(np.int64) * per + rng.randint(0, per, 4096)).to("cuda:0")
    for fmt, zone in ((tf.ISO_F, 0), (b"%d/%b/%Y:%H:%M:%S.%f %z", -420), (tf.LONGEST, 1439)):
        text, ob, oe, stats = scan.format_time_records(v, fmt, unit=tf.UNIT_NAMES[unit], zone_minutes=zone, stats=True)
        assert stats == {"n_ok": 4096, "n_null": 0, "n_range": 0} and int((oe - ob).min()) == int((oe - ob).max()) == tf.row_length(fmt, unit)
        back, status = scan.parse_time_records(text, ob, oe, fmt, unit=tf.UNIT_NAMES[unit])
        assert (status == rj.PARSE_OK).all() and torch.equal(back, v), (fmt, unit)
    sample = v[:64].cpu().tolist()
    text, ob, oe = scan.format_time_records(v[:64].contiguous(), tf.ISO_F, unit=tf.UNIT_NAMES[unit], zone_minutes=330)
    assert text.cpu().numpy().tobytes() == tf.layout(sample, tf.ISO_F, unit, zone_minutes=330)[0]


def test_index_lists_and_no_rows(rj, scan, columns):
    import torch
    C = columns[tf.MICRO]
    n = len(C.values)
    rng = np.random.RandomState(5)
    for indices in (rng.permutation(n), rng.randint(0, n, 3000), np.full(700, 11)):
        check(rj, scan, C, tf.CLF, True, indices.astype(np.int64), zone=-420, lead=1, ctx="index list")
    empty = torch.zeros(1, dtype=torch.int64, device="cuda:0")[:0]
    a_list = torch.zeros(1, dtype=torch.int64, device="cuda:0")      # a non-null list, handed over with count 0
    lib = rj.load_library()
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    for n_values, idx_t in ((0, None), (n, a_list)):
        out = torch.full((64,), POISON8, dtype=torch.uint8, device="cuda:0")
        tb = torch.full((ROOM,), POISON, dtype=torch.int64, device="cuda:0")
        counts = rj.api._FormatTimeStats(77, 77, 77)
        total = lib.rj_scan_records_format_time(scan._h, vp(C.d), None, n_values, None if idx_t is None else vp(idx_t), 0, tf.ISO, len(tf.ISO), tf.MICRO, 0, 0,
                                                0x2C, 5, 1, vp(out), 16, vp(tb), vp(tb), ctypes.byref(counts),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert total == 5 and out.cpu().numpy().tobytes() == b"," * 5 + bytes([POISON8]) * 59 and (tb.cpu().numpy() == POISON).all() and [counts.n_ok, counts.n_null, counts.n_range] == [0, 0, 0]
    text, ob, oe = scan.format_time_records(empty, tf.ISO)
    assert text.numel() == 0 and ob.numel() == 0 and oe.numel() == 0
    text, ob, oe, stats = scan.format_time_records(C.d, tf.ISO, unit="us", indices=empty, lead=3, stats=True)
    assert text.cpu().numpy().tobytes() == b"\n\n\n" and ob.numel() == 0 and stats == {"n_ok": 0, "n_null": 0, "n_range": 0}


def test_out_too_small_and_out_given_through_the_python_api(rj, scan, columns):
    import torch
    C = columns[tf.MILLI]
    want, begins, ends, counts = tf.layout(C.values, tf.ISO_F, tf.MILLI, C.status, None, 330, 0x2C, 2, 1)
    room = torch.full((len(want) + 64,), POISON8, dtype=torch.uint8, device="cuda:0")
    text, ob, oe, stats = scan.format_time_records(C.d, tf.ISO_F.decode(), unit="ms", status=C.d_status, zone_minutes=330, fill=0x2C, lead=2, out=room, stats=True)
    assert text.data_ptr() == room.data_ptr() and text.cpu().numpy().tobytes() == want and ob.cpu().tolist() == begins and oe.cpu().tolist() == ends
    assert (room[len(want):] == POISON8).all() and stats == counts
    small = torch.full((len(want) - 1,), POISON8, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(rj.RejitError) as err:
        scan.format_time_records(C.d, tf.ISO_F, unit="ms", status=C.d_status, zone_minutes=330, fill=0x2C, lead=2, out=small)
    assert "%d bytes" % len(want) in str(err.value)
    assert small.cpu().numpy().tobytes() == want[:-1]                     # nothing at or beyond out_cap was written, the rest is complete
    with pytest.raises(ValueError):
        scan.format_time_records(C.d, tf.ISO, unit="m")


def test_refusals_write_nothing(rj, scan, columns):
    import torch
    C = columns[tf.SECOND]
    lib = rj.load_library()
    n = len(C.values)

    def refused(word, status=RJ_BAD_ARGUMENT, d_value=C.d, **kw):
        total, out, gb, ge, stats = format_poisoned(rj, scan, d_value, n, kw.pop("fmt", tf.ISO), kw.pop("unit", tf.SECOND), cap=kw.pop("cap", 4096), **kw)
        msg = lib.rj_last_error().decode()
        assert total == status and word in msg and "rj_scan_records_format_time" in msg, (word, total, msg)
        assert out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all() and stats == [77, 77, 77], word

    for flags in (1, 2, 4, 0x80000000):
        refused("flags", flags=flags)
    for unit in (-1, 4):
        refused("unit %d " % unit, unit=unit)
    for zone in (1440, -1440):
        refused("zone_minutes %d " % zone, zone=zone)
    refused("fill", fill=256)
    refused("fill", fill=-1)
    refused("2^42", gap=(1 << 42) - 77)
    refused("2^62", lead=1 << 62)
    refused("8-byte aligned", d_value=C.d.view(torch.uint8)[4:].view(torch.int32))
    refused("row 3 ", idx_t=dev([0, 1, 2, n, 5, n + 7]))
    for fmt, offset in tf.REFUSED_FORMATS:
        refused("format byte %d: " % offset, fmt=fmt)
    refused("format byte 9: an unknown directive", fmt=b"%Y-%m-%d %q")
    refused("format byte 3: a directive given twice", fmt=b"%H:%H")
    with pytest.raises(rj.RejitError) as err:
        scan.format_time_records(C.d, b"%Y %j")
    assert "format byte 3: " in str(err.value)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    out = torch.full((4096 + 16,), POISON8, dtype=torch.uint8, device="cuda:0")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda value, fmt, fmt_len, d_out: lib.rj_scan_records_format_time(scan._h, value, None, n, None, 0, fmt, fmt_len, 0, 0, 0, 10, 0, 1, d_out, 4096, None, None,
                                                                              None, st)
    assert call(vp(C.d), tf.ISO, len(tf.ISO), ctypes.c_void_p(out.data_ptr() + 8)) == RJ_BAD_ARGUMENT and "16-byte aligned" in lib.rj_last_error().decode()
    assert call(None, tf.ISO, len(tf.ISO), vp(out)) == RJ_BAD_ARGUMENT and "null" in lib.rj_last_error().decode()
    assert call(vp(C.d), None, 5, vp(out)) == RJ_BAD_ARGUMENT and "null" in lib.rj_last_error().decode()
    assert call(vp(C.d), None, 0, vp(out)) == RJ_BAD_ARGUMENT and "format byte 0: " in lib.rj_last_error().decode()
    assert (out == POISON8).all()
    # k >= 2^31: refused before anything is read (the values' pointer is never followed)
    total = lib.rj_scan_records_format_time(scan._h, vp(C.d), None, 1 << 31, None, 0, tf.ISO, len(tf.ISO), 0, 0, 0, 10, 0, 1, None, 0, None, None, None, st)
    assert total == RJ_TOO_LARGE and "2^31" in lib.rj_last_error().decode()
    # the writing mode accepts what only the reader refuses
    for fmt in tf.ACCEPTED_FORMATS:
        text, ob, oe = scan.format_time_records(C.d[:3].contiguous(), fmt)
        assert text.cpu().numpy().tobytes() == tf.layout(C.values[:3], fmt, tf.SECOND)[0]
    check(rj, scan, C, tf.CLF, True, None, ctx="behind the refusals")


def test_the_scan_keeps_its_spans_stats_and_selection(rj, columns):
    import torch
    from rejit_amd import records
    text = torch.from_numpy(np.frombuffer(b"ab 12 cd 345 e 6\nxy\n7\n" * 40, dtype=np.uint8).copy()).to("cuda:0")
    s = rj.Scan(rj.Program(b"[0-9]+"))
    begins, ends = records.line_records(text)
    result = s.run_records(text, begins, ends)
    selected, spans, stats = s.select_records().clone(), s.spans_tensor(text.device).clone(), s.stats()
    assert result.n_matching == 80 and spans.numel() > 0
    s.format_time_records(columns[tf.NANO].d, tf.LONGEST, unit="ns", zone_minutes=-1439)
    assert torch.equal(s.spans_tensor(text.device), spans) and torch.equal(s.select_records(), selected) and s.stats() == stats
    assert s.run_records(text, begins, ends).n_kept == result.n_kept


# ------------------------------------------------------------------------------------------------ the sample
SAMPLE_LINES = [b"a 2026-10-20T17:15:01Z x", b"b 2026-10-20T17:15:59Z", b"c 2026-10-20T17:16:00Z", b"d 2026-13-20T17:16:00Z", b"e 1969-12-31T23:59:59Z y",
                b"f 1969-12-31T23:59:00Z", b"g", b"h 2026-10-20T17:15:30Z", b"i 0001-01-01T00:00:30Z", b"j 9999-12-31T23:59:59Z"]


def test_linegrep_sample_buckets_as_timestamps_from_the_device(rj, tmp_path):
    """-T ... -w 60 -F '%Y-%m-%dT%H:%M' against a dict over strptime plus hand formatting; without -F the output is what it was"""
    import datetime
    path = str(tmp_path / "access.log")
    with open(path, "wb") as fh:
        fh.write(b"\n".join(SAMPLE_LINES) + b"\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    base = [sys.executable, sample, path, " ", "-f", "2", "-T", "%Y-%m-%dT%H:%M:%SZ", "-w", "60"]
    plain = subprocess.run(base, capture_output=True, timeout=300)
    stamped = subprocess.run(base + ["-F", "%Y-%m-%dT%H:%M"], capture_output=True, timeout=300)
    assert plain.returncode == stamped.returncode == 0, (plain.stderr.decode()[-500:], stamped.stderr.decode()[-500:])
    buckets = {}
    for line in SAMPLE_LINES:
        try:
            dt = datetime.datetime.strptime(line.split(b" ")[1].decode(), "%Y-%m-%dT%H:%M:%SZ")
        except (IndexError, ValueError):
            continue
        start = (dt - datetime.datetime(1970, 1, 1)) // datetime.timedelta(seconds=60) * 60
        buckets[start] = buckets.get(start, 0) + 1
    assert len(buckets) == 5
    assert plain.stdout == "".join("%7d %d\n" % (buckets[b], b) for b in sorted(buckets)).encode()      # the parent's output, byte for byte
    want = b""
    for b in sorted(buckets):
        dt = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=b)
        want += b"%7d %04d-%02d-%02dT%02d:%02d\n" % (buckets[b], dt.year, dt.month, dt.day, dt.hour, dt.minute)
    assert stamped.stdout == want and b"      3 2026-10-20T17:15\n" in want and b"      1 0001-01-01T00:00\n" in want
    usage = subprocess.run([sys.executable, sample, path, " ", "-f", "2", "-F", "%Y"], capture_output=True, timeout=300)      # -F without -T ... -w
    assert usage.returncode == 2 and b"-F OUTFORMAT" in usage.stderr
