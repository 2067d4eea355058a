"""GPU tests (-m gpu) of rj_scan_records_translate (rejit_amd/csrc/record_translate.hip; Scan.translate_records): the rows of a
record table through a byte map and a drop set on the device, laid out as a pack.

The meaning is tests/translate_cases.py's, written in Python independently of the library: bytes.translate per row and the
layout arithmetic.  Every comparison is exact.  Outputs are poisoned first, with room behind the text and the tables that must
stay poisoned."""
import bisect
import collections
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import translate_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_BAD_ARGUMENT = -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON8 = 0xA5
ROOM = 7                          # spare table rows
ROOM_BYTES = 53                   # spare output bytes
SLAB = 4096                       # rejit_amd/csrc/record_translate.h: kSlab, positions of the virtual stream per slab
IMAGE = 4096                      # rejit_amd/csrc/record_translate.h: kImage, the output bytes of one turn of the emit
UNIT_GRID_ROWS = 1024 * 256       # record_frame.h: unit_grid() workgroups of 256 rows, one pass of the rows' plan
SLAB_GRID_BYTES = 256 * 8 * SLAB  # record_frame.h: kCopyGrid workgroups, a slab each: one pass of the count and of the emit
assert (SLAB, IMAGE) == (tc.SLAB, tc.IMAGE)


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


def dev(x, dtype=np.int64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to("cuda:0")


class Table:
    """the host's (text, begins, ends[, indices]) and the same on the device; `shift`: the text's first byte stands at that
    offset past a 16-byte boundary"""

    def __init__(self, table, indices=None, shift=0):
        import torch
        self.text, self.begins, self.ends = table
        self.indices = None if indices is None else [int(i) for i in indices]
        room = torch.full((len(self.text) + 32,), 0x7E, dtype=torch.uint8, device="cuda:0")
        assert room.data_ptr() % 16 == 0
        self.d_text = room[shift:shift + len(self.text)]
        if len(self.text):
            self.d_text.copy_(torch.from_numpy(np.frombuffer(self.text, dtype=np.uint8).copy()))
        self.d_begins, self.d_ends = dev(self.begins), dev(self.ends)
        self.d_indices = None if indices is None else dev(self.indices)

    def rows(self):
        return tc.rows_of(self.text, self.begins, self.ends, self.indices)

    @property
    def k(self):
        return len(self.begins) if self.indices is None else len(self.indices)


def translate_poisoned(rj, scan, t, table=None, delete=b"", fill=10, lead=0, gap=1, cap=0, with_begin=True, with_end=True, out_shift=0, table_shift=0,
                       want_stats=True):
    """the raw call into poisoned buffers -> (return value, out bytes with the spare ones, begins, ends with the spare rows, stats)"""
    import torch
    from rejit_amd.api import _TranslateStats as Stats
    lib = rj.load_library()
    out = torch.full((cap + ROOM_BYTES + 16,), POISON8, dtype=torch.uint8, device="cuda:0")
    begins = torch.full((t.k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    ends = torch.full((t.k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    assert out.data_ptr() % 16 == 0
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
    idx, n_idx = t.d_indices, 0
    if idx is not None:
        n_idx = int(idx.numel())
        if n_idx == 0:
            idx = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    stats = Stats(POISON8, POISON8, POISON8)
    total = lib.rj_scan_records_translate(scan._h, vp(t.d_text), len(t.text), ctypes.c_void_p(t.d_begins.data_ptr() + table_shift) if len(t.begins) else None,
                                          vp(t.d_ends), len(t.begins), vp(idx), n_idx, table, tc.drop_bits(delete) if delete else None, fill, lead, gap,
                                          ctypes.c_void_p(out.data_ptr() + out_shift) if cap or out_shift else None, cap, vp(begins) if with_begin else None,
                                          vp(ends) if with_end else None, ctypes.byref(stats) if want_stats else None,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return (int(total), out.cpu().numpy().tobytes()[:cap + ROOM_BYTES], begins.cpu().numpy(), ends.cpu().numpy(),
            {f: int(getattr(stats, f)) for f, _ in Stats._fields_})


def check(rj, scan, t, table=None, delete=b"", fill=10, lead=0, gap=1, ctx=None, query=True, want_stats=True, rows=None):
    """the size query, then the call with an exact capacity, against translate_cases"""
    rows = t.rows() if rows is None else rows
    text, begins, ends = tc.layout(tc.translate(rows, table, delete), fill, lead, gap)
    k = len(begins)
    c = (ctx, k, table is not None, delete[:8], fill, lead, gap)
    want = tc.stats(rows, table, delete) if want_stats else None
    if query:
        total, out, gb, ge, st = translate_poisoned(rj, scan, t, table, delete, fill, lead, gap, cap=0, want_stats=want_stats)
        assert total == len(text), (c, total, rj.load_library().rj_last_error())
        assert out == bytes([POISON8]) * ROOM_BYTES and (gb[:k] == begins).all() and (ge[:k] == ends).all(), c
        assert want is None or st == want, (c, st, want)
    total, out, gb, ge, st = translate_poisoned(rj, scan, t, table, delete, fill, lead, gap, cap=len(text), want_stats=want_stats)
    assert total == len(text), (c, total, rj.load_library().rj_last_error())
    if out[:total] != text:
        at = next(i for i in range(total) if out[i] != text[i])
        raise AssertionError((c, "first differing byte", at, out[max(at - 30, 0):at + 30], text[max(at - 30, 0):at + 30]))
    assert out[total:] == bytes([POISON8]) * ROOM_BYTES, c
    assert (gb[:k] == begins).all() and (ge[:k] == ends).all() and (gb[k:] == POISON).all() and (ge[k:] == POISON).all(), c
    assert want is None or st == want, (c, st, want)
    return text, begins, ends


def lines_table(k, max_len, seed, alphabet=None):
    """k random lines of 0..max_len bytes, a line break behind each -> (text, begins, ends), made with numpy"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, max_len + 1, size=k)
    ends = np.cumsum(lengths + 1) - 1
    begins = ends - lengths
    alphabet = np.frombuffer(alphabet or bytes(range(0x20, 0x7F)), dtype=np.uint8)
    data = alphabet[rng.integers(0, len(alphabet), size=int(ends[-1]) + 1)]
    data[ends] = 10
    return data.tobytes(), begins.tolist(), ends.tolist()


# ------------------------------------------------------------------------------------------------ 1. meaning
def test_all_byte_values_under_random_maps_and_drop_sets(rj, scan):
    t = Table((bytes(range(256)), [0], [256]))
    for seed in range(20):
        rng = random.Random(seed)
        perm = list(range(256))
        rng.shuffle(perm)
        delete = bytes(rng.sample(range(256), rng.randrange(0, 200)))
        check(rj, scan, t, bytes(perm), delete, ctx=seed, query=seed < 3)
    for table, delete in ((None, b""), (tc.IDENTITY, b""), (tc.LOWER, b""), (tc.UPPER, b""), (None, b"\r\x00,"), (tc.LOWER, b"")):
        check(rj, scan, t, table, delete, ctx="named")
        check(rj, scan, t, table, delete, ctx="named, no stats", want_stats=False)
    # a byte that is both mapped and dropped is dropped: judged on the source byte, before the map
    text, _, _ = check(rj, scan, t, tc.LOWER, b"Aq", ctx="mapped and dropped")
    # ('A' goes, so only the source's own 'a' is an 'a'; the source's 'q' goes, and the one 'q' left is the mapped 'Q')
    assert b"A" not in text and b"Q" not in text and text.count(b"a") == 1 and text.count(b"q") == 1
    assert (tc.LOWER, tc.UPPER) == (bytes(range(256)).lower(), bytes(range(256)).upper())


def test_the_python_layer_and_its_tables(rj, scan):
    from rejit_amd import records
    assert records.ASCII_LOWER == tc.LOWER and records.ASCII_UPPER == tc.UPPER
    assert records.byte_map(b"abca", b"xyzw") == bytes.maketrans(b"bca", b"yzw") and records.byte_map() == tc.IDENTITY
    assert bytes(records.drop_set(b"\r,\xff")) == tc.drop_bits(b"\r,\xff") and len(records.drop_set(b"")) == 32
    with pytest.raises(ValueError):
        records.byte_map(b"ab", b"c")
    t = Table(tc.table([0, 5, 17, 40, 0, 3], 3, alphabet=b"aAbB,\r"))
    want = tc.layout(tc.translate(t.rows(), tc.UPPER, b",\r"), 0x2E, 2, 3)
    for delete in (b",\r", records.drop_set(b",\r")):
        out, ob, oe, st = scan.translate_records(t.d_text, t.d_begins, t.d_ends, table=records.ASCII_UPPER, delete=delete, fill=0x2E, lead=2, gap=3, stats=True)
        assert (out.cpu().numpy().tobytes(), ob.cpu().tolist(), oe.cpu().tolist()) == want
        assert st == tc.stats(t.rows(), tc.UPPER, b",\r")
    out, ob, oe = scan.translate_records(t.d_text, t.d_begins, t.d_ends)          # identity: pack_records with the separator
    packed = scan.pack_records(t.d_text, t.d_begins, t.d_ends)
    assert out.cpu().tolist() == packed[0].cpu().tolist() and ob.cpu().tolist() == packed[1].cpu().tolist()


# ------------------------------------------------------------------------------------------------ 2. seams
def planted(lengths, seed, delete_byte=0x2C):
    """a text with one record per length (random letters, junk between), and the dropped byte planted on each side of every slab
    seam of the virtual stream and of every row's two ends -> (text, begins, ends)"""
    rng = random.Random(seed)
    text, begins, ends = tc.table(lengths, seed, junk=3, alphabet=b"abcdXYZ")
    text = bytearray(text)
    sb, S = tc.stream_places(lengths)
    for seam in range(SLAB, S, SLAB):
        for d in (-18, -17, -16, -2, -1, 0, 1, 15, 16, 17):
            q = seam + d
            j = bisect.bisect_right(sb, q) - 1
            if 0 <= q < S and q - sb[j] < lengths[j]:          # a byte of row j, not its terminator
                text[begins[j] + q - sb[j]] = delete_byte
    for j, length in enumerate(lengths):
        if length and rng.randrange(2):
            text[begins[j]] = delete_byte
        if length > 1 and rng.randrange(2):
            text[ends[j] - 1] = delete_byte
    return bytes(text), begins, ends


def test_rows_begin_and_end_at_every_offset_around_every_slab_seam(rj, scan):
    """three slabs of virtual stream; the tables of translate_cases.seam_lengths put a row's end and the next row's begin at
    every offset within +-17 of both seams; over them text shifts 0..15, leads 0..17 (every output alignment), gaps 0, 1, 2 and
    5000 (more than one turn of the image), with and without the drop set"""
    rng = random.Random(21)
    tables = tc.seam_lengths(SLAB, 3, 17, rng)
    assert len(tables) == 35
    shifts, leads, gaps, met = set(), set(), set(), set()
    for i, lengths in enumerate(tables):
        sb, S = tc.stream_places(lengths)
        assert 2 * SLAB < S <= 3 * SLAB
        met |= {(q + length) - seam for q, length in zip(sb, lengths) for seam in (SLAB, 2 * SLAB) if abs(q + length - seam) <= 17}
        shift, lead, gap = i % 16, (5 * i) % 18, (0, 1, 2, 5000)[i % 4]
        shifts.add(shift), leads.add(lead), gaps.add(gap)
        t = Table(planted(lengths, 30 + i), shift=shift)
        check(rj, scan, t, tc.UPPER, b",", fill=0x2E, lead=lead, gap=gap, ctx=("seam", i), query=False)
        check(rj, scan, t, tc.UPPER, b"", fill=0x2E, lead=lead, gap=gap, ctx=("seam, nothing dropped", i), query=i % 8 == 0, want_stats=False)
    assert met == set(range(-17, 18)) and shifts == set(range(16)) and leads == set(range(18)) and gaps == {0, 1, 2, 5000}


def test_every_text_shift_with_every_output_alignment(rj, scan):
    lengths = [0, 1, 33, 16, 100, 17, 31, 32, 64, 5, 48, 0, 0, 15]
    for shift in range(16):
        t = Table(planted(lengths, 70 + shift), shift=shift)
        for lead in range(shift % 3, 18, 3):
            check(rj, scan, t, tc.LOWER, b"," if lead % 2 else b"", lead=lead, gap=lead % 3, ctx=(shift, lead), query=False)


# ------------------------------------------------------------------------------------------------ 3. balance shapes (answers, not time)
def test_empty_rows_alone_and_interleaved(rj, scan):
    """300 000 empty rows, gap 1: more than one pass of unit_grid()'s 262 144 rows, and slabs that hold terminators only"""
    k = 300000
    assert k > UNIT_GRID_ROWS
    t = Table((b"xyz", [1] * k, [1] * k))
    check(rj, scan, t, None, b"x", ctx="empty rows", query=False)
    check(rj, scan, t, None, b"", ctx="empty rows, nothing dropped", query=False)
    begins = [1 + (j & 1) * 0 for j in range(k)]
    ends = [1 + (j & 1) for j in range(k)]                # every second row is the one byte "y"
    t = Table((b"xyz", begins, ends))
    check(rj, scan, t, tc.UPPER, b"x", ctx="interleaved", query=False)
    check(rj, scan, t, tc.UPPER, b"y", ctx="interleaved, all dropped", query=False)


def test_one_long_row_nearly_all_dropped_and_one_kept_whole(rj, scan):
    n = (1 << 20) + 5
    data = bytearray(b",") * n
    for i in list(range(0, n, 4097)) + [n - 1]:
        data[i] = 0x41 + i % 26
    t = Table((bytes(data), [0], [n]))
    text, _, _ = check(rj, scan, t, tc.LOWER, b",", ctx="1 MiB + 5, nearly all dropped")
    assert len(text) == len(range(0, n, 4097)) + 1 + 1
    rng = np.random.default_rng(4)
    whole = rng.integers(0, 256, size=1 << 20, dtype=np.uint8).tobytes()
    t = Table((whole, [0], [1 << 20]), shift=3)
    check(rj, scan, t, tc.UPPER, b"", ctx="1 MiB kept whole", lead=5)
    check(rj, scan, t, None, b"\x00", ctx="1 MiB, NUL dropped", lead=5, query=False)


# ------------------------------------------------------------------------------------------------ 4. beyond one grid pass
def test_more_than_one_pass_of_the_slab_grid(rj, scan):
    """about 9 MB of random lines: more than kCopyGrid x kSlab = 8 MiB of virtual stream, so the count's tickets and the emit's
    stride go round again; with and without a drop set, the rows under a permutation"""
    table = lines_table(220000, 80, 90)
    assert len(table[0]) > SLAB_GRID_BYTES + (1 << 19)
    order = np.random.default_rng(91).permutation(len(table[1])).tolist()
    t = Table(table, order)
    rows = t.rows()
    check(rj, scan, t, tc.LOWER, b"aeiou \n", ctx="9 MB, dropped", query=False, rows=rows)
    check(rj, scan, t, tc.LOWER, b"", ctx="9 MB, kept", query=False, rows=rows, want_stats=False)


def test_repeated_rows_make_units_of_several_slabs(rj, scan):
    """200 000 rows that all name one record of 100 bytes of a 120-byte text: the virtual stream is 5 000 times the text and its
    rows, so a unit is many slabs"""
    text = bytes(0x30 + i % 75 for i in range(120))
    t = Table((text, [7, 0], [107, 0]), [0] * 100000 + [1] * 3 + [0] * 100000)
    rows = t.rows()
    check(rj, scan, t, tc.LOWER, b"0AZ", ctx="repeats, dropped", query=False, rows=rows)
    check(rj, scan, t, tc.LOWER, b"", ctx="repeats, kept", query=False, rows=rows, want_stats=False)


# ------------------------------------------------------------------------------------------------ 5. capacity
def test_the_size_query_and_capacities_around_the_total(rj, scan):
    import torch
    t = Table(planted([random.Random(5).randrange(0, 90) for _ in range(900)], 100))
    for delete in (b",", b""):
        want, begins, ends = tc.layout(tc.translate(t.rows(), tc.UPPER, delete), 0x2C, 2, 1)
        total = len(want)
        for cap in (0, total - 1, total, total + 53):
            got, out, gb, ge, _ = translate_poisoned(rj, scan, t, tc.UPPER, delete, 0x2C, 2, 1, cap=cap)
            assert got == total, (cap, got, total)                                   # the return value is always the total
            shown = min(cap, total)
            assert out[:shown] == want[:shown] and out[shown:] == bytes([POISON8]) * (len(out) - shown), cap
            assert (gb[:900] == begins).all() and (ge[:900] == ends).all() and (gb[900:] == POISON).all()   # tables also in the size query
        with pytest.raises(rj.RejitError):
            scan.translate_records(t.d_text, t.d_begins, t.d_ends, table=tc.UPPER, delete=delete, fill=0x2C, lead=2,
                                   out=torch.empty(total - 1, dtype=torch.uint8, device="cuda:0"))
        out, ob, oe = scan.translate_records(t.d_text, t.d_begins, t.d_ends, table=tc.UPPER, delete=delete, fill=0x2C, lead=2,
                                             out=torch.empty(total + 64, dtype=torch.uint8, device="cuda:0"))
        assert out.cpu().numpy().tobytes() == want and ob.cpu().tolist() == begins and oe.cpu().tolist() == ends
    for with_begin, with_end in ((False, True), (True, False), (False, False)):
        want, begins, ends = tc.layout(tc.translate(t.rows(), None, b","), 10, 0, 1)
        got, out, gb, ge, _ = translate_poisoned(rj, scan, t, None, b",", cap=len(want), with_begin=with_begin, with_end=with_end)
        assert got == len(want) and out[:got] == want
        assert (gb[:900] == begins).all() if with_begin else (gb == POISON).all()
        assert (ge[:900] == ends).all() if with_end else (ge == POISON).all()


def test_no_rows_is_the_lead(rj, scan):
    base = tc.table([4, 5], 7)
    for t in (Table(base, []), Table((b"abc", [], []))):
        for lead in (0, 1, 16, 300):
            for delete in (b"", b"a"):
                check(rj, scan, t, tc.UPPER, delete, lead=lead, fill=0x2D, ctx=("no rows", lead))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_a_bad_row_in_a_later_plan_unit_is_named_and_nothing_is_written(rj, scan):
    k = 70000
    table = lines_table(k, 12, 110)
    for kind in ("index", "row"):
        begins, ends, idx = list(table[1]), list(table[2]), list(range(k))
        first, later = 300, 66000
        if kind == "index":
            idx[first] = k
            idx[later] = 1 << 50
        else:
            begins[first] = ends[first] + 1
            ends[later] = len(table[0]) + 1
        for bad in ((first, later), (later,)):
            b, e, i = list(table[1]), list(table[2]), list(range(k))
            for j in bad:
                b[j], e[j], i[j] = begins[j], ends[j], idx[j]
            t = Table((table[0], b, e), i)
            for cap, delete in ((0, b"a"), (1 << 20, b"a"), (1 << 20, b"")):
                total, out, gb, ge, _ = translate_poisoned(rj, scan, t, tc.UPPER, delete, cap=cap)
                message = rj.load_library().rj_last_error().decode()
                assert total == RJ_BAD_ARGUMENT and ("row %d " % bad[0]) in message, (kind, bad, cap, total, message)
                assert out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all(), (kind, bad, cap)
            with pytest.raises(rj.RejitError) as err:
                scan.translate_records(t.d_text, t.d_begins, t.d_ends, indices=t.d_indices, delete=b"a", fill=10)
            assert err.value.status == RJ_BAD_ARGUMENT and ("row %d " % bad[0]) in err.value.message


def test_refused_arguments_write_nothing(rj, scan):
    t = Table(tc.table([5, 9, 0, 20], 120))
    for kw in ({"table_shift": 4}, {"out_shift": 8, "cap": 64}, {"fill": -1, "cap": 64}, {"fill": 256, "cap": 64}, {"gap": 1 << 42}, {"lead": 1 << 62}):
        total, out, gb, ge, _ = translate_poisoned(rj, scan, t, tc.UPPER, b"a", **kw)
        assert total == RJ_BAD_ARGUMENT, (kw, total)
        assert out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all(), kw
    check(rj, scan, t, tc.UPPER, b"a", ctx="behind the refusals")


# ------------------------------------------------------------------------------------------------ 7. the scan's state
def test_the_scan_keeps_its_spans_stats_and_selection(rj, scan):
    import torch
    from rejit_amd import records
    text = torch.from_numpy(np.frombuffer(b"ab 12\ncd\ne 6 7\n", dtype=np.uint8).copy()).to("cuda:0")
    assert scan.run_tensor(text) == 3
    spans, stats = scan.spans(), scan.stats()
    t = Table(tc.table([0, 3, 9, 40] * 25, 150, alphabet=b"abAB,"))
    scan.translate_records(t.d_text, t.d_begins, t.d_ends, table=tc.LOWER, delete=b",")
    assert scan.spans() == spans == [(2, 3), (10, 11), (12, 13)] and scan.stats() == stats
    begins, ends = records.line_records(text)
    begins, ends = begins[:-1].contiguous(), ends[:-1].contiguous()
    scan.run_records(text, begins, ends)
    before = scan.select_records().cpu().tolist()
    scan.translate_records(t.d_text, t.d_begins, t.d_ends, table=tc.LOWER, delete=b",", stats=True)
    scan.translate_records(t.d_text, t.d_begins, t.d_ends, table=tc.LOWER)
    assert scan.select_records().cpu().tolist() == before == [0, 2]


# ------------------------------------------------------------------------------------------------ 8. compositions
def test_lower_then_group_is_uniq_ci(rj, scan):
    rng = random.Random(160)
    words = [b"Alpha", b"ALPHA", b"alpha", b"Beta", b"bEtA", b"gamma", b"", b"Delta9", b"DELTA9", b"x"]
    lines = [rng.choice(words) for _ in range(5000)]
    t = Table(tc.layout(lines))
    low, lb, le = scan.translate_records(t.d_text, t.d_begins, t.d_ends, table=tc.LOWER, fill=10)
    group, rep, count = scan.group_records(low, lb, le)
    want = collections.Counter(w.lower() for w in lines)            # (a Counter keeps first-appearance order)
    host = low.cpu().numpy().tobytes()
    b, e = lb.cpu().tolist(), le.cpu().tolist()
    got = [(host[b[r]:e[r]], c) for r, c in zip(rep.cpu().tolist(), count.cpu().tolist())]
    assert got == list(want.items())


def test_drop_commas_then_parse_and_drop_cr(rj, scan):
    rng = random.Random(170)
    numbers = [rng.randrange(-10 ** 15, 10 ** 15) for _ in range(3000)] + [0, 1234567, -1234567]
    lines = [format(v, ",").encode() for v in numbers]
    assert b"1,234,567" in lines
    t = Table(tc.layout(lines))
    bare, bb, be = scan.translate_records(t.d_text, t.d_begins, t.d_ends, delete=b",", fill=10)
    values, status = scan.parse_records(bare, bb, be, kind="int64")
    assert (status.cpu().numpy() == rj.PARSE_OK).all() and values.cpu().tolist() == [int(s.replace(b",", b"")) for s in lines] == numbers
    # a CRLF file without its \r is the LF file
    rows = [bytes(rng.choice(b"ab \tz") for _ in range(rng.randrange(0, 30))) for _ in range(2000)]
    crlf = tc.layout([r + b"\r" for r in rows])
    t = Table(crlf)
    out, ob, oe = scan.translate_records(t.d_text, t.d_begins, t.d_ends, delete=b"\r", fill=10)
    assert (out.cpu().numpy().tobytes(), ob.cpu().tolist(), oe.cpu().tolist()) == tc.layout(rows)


# ------------------------------------------------------------------------------------------------ 9. the sample
SAMPLE_LINES = [b"GET /Index 200", b"get /index 200", b"POST /Form 500", b"Get /INDEX 404", b"put /x 200", b"GET /index 200", b"post /form 200", b"HEAD /y 301"]


@pytest.mark.parametrize("case", ["count", "numbers", "lines", "groups"])
def test_linegrep_sample_ignores_case(rj, tmp_path, case):
    """-i: `grep -i -c`, `grep -i -n` and `grep -i` (the ORIGINAL lines) for a lower-case pattern, written in Python; -u: uniq -ci"""
    path = str(tmp_path / "access.log")
    with open(path, "wb") as fh:
        fh.write(b"\n".join(SAMPLE_LINES) + b"\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    hits = [i for i, line in enumerate(SAMPLE_LINES) if b"get /index" in line.lower()]
    assert hits == [0, 1, 3, 5]
    groups = collections.Counter(line.split(b" ")[0].lower() for line in SAMPLE_LINES)
    options, want = {"count": (["get /index", "-i", "-c"], b"%d\n" % len(hits)),
                     "numbers": (["get /index", "-i", "-n"], b"".join(b"%d\n" % (i + 1) for i in hits)),
                     "lines": (["get /index", "-i", "-p"], b"".join(SAMPLE_LINES[i] + b"\n" for i in hits)),
                     "groups": ([" ", "-i", "-f", "1", "-u"], b"".join(b"%7d %s\n" % (c, w) for w, c in groups.items()))}[case]
    done = subprocess.run([sys.executable, sample, path] + options, capture_output=True, timeout=300)
    assert done.returncode == 0, done.stderr.decode()[-800:]
    assert done.stdout == want, (done.stdout, want)
