"""GPU tests (-m gpu) of rj_scan_records_zip (rejit_amd/csrc/record_zip.hip; Scan.zip_records): the rows of several record
tables put side by side into lines on the device, laid out as a pack.

The meaning is tests/zip_cases.py's, written in Python independently of the library: sep.join of rjust / ljust, and the layout
arithmetic.  Every comparison is exact.  Outputs are poisoned first, with room behind the text and the tables that must stay
poisoned."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zip_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_BAD_ARGUMENT = -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON8 = 0xA5
ROOM = 7                          # spare table rows
ROOM_BYTES = 53                   # spare output bytes
EMIT_CHUNK = 4096                 # rejit_amd/csrc/record_zip.h: kEmitChunk, the output bytes of one chunk of the emit
STREAM_BYTES = 32                 # rejit_amd/csrc/record_zip.h: kStreamBytes, the tier threshold T
UNIT_GRID_ROWS = 1024 * 256       # record_frame.h: unit_grid() workgroups of 256 rows, one pass of the resolve and of the plan
EMIT_GRID_BYTES = 256 * 8 * EMIT_CHUNK   # record_frame.h: kCopyGrid workgroups, a chunk each: one turn of the emit
assert (EMIT_CHUNK, STREAM_BYTES) == (zc.EMIT_CHUNK, zc.STREAM_BYTES)


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


class Col:
    """a column: the host's (text, begins, ends[, indices]) and the same on the device; `shift`: the text's first byte stands at
    that offset past a 16-byte boundary"""

    def __init__(self, table, indices=None, shift=0):
        import torch
        self.text, self.begins, self.ends = table
        self.indices = None if indices is None else [int(i) for i in indices]
        room = torch.full((len(self.text) + 32,), 0x7E, dtype=torch.uint8, device="cuda:0")
        assert room.data_ptr() % 16 == 0
        self.d_text = room[shift:shift + len(self.text)]
        if len(self.text):
            self.d_text.copy_(torch.from_numpy(np.frombuffer(self.text, dtype=np.uint8).copy()))
        assert self.d_text.data_ptr() % 16 == shift and self.d_text.is_contiguous()
        self.d_begins, self.d_ends = dev(self.begins), dev(self.ends)
        self.d_indices = None if indices is None else dev(self.indices)

    def pieces(self):
        return zc.pieces(self.text, self.begins, self.ends, self.indices)

    def arg(self):
        return (self.d_text, self.d_begins, self.d_ends) if self.d_indices is None else (self.d_text, self.d_begins, self.d_ends, self.d_indices)


def zip_poisoned(rj, scan, args, widths=None, sep=b"", pad=32, fill=10, lead=0, gap=1, cap=0, flags=0, with_begin=True, with_end=True, reserved=0, k=None,
                 n_cols=None, sep_len=None, out_shift=0, table_shift=None):
    """the raw call into poisoned buffers -> (return value, out bytes with the spare ones, begins, ends with the spare rows);
    args: (text, begins, ends[, indices]) device tensors per column"""
    import torch
    from rejit_amd.api import ZipColumn
    lib = rj.load_library()
    widths = [0] * len(args) if widths is None else widths
    cols = (ZipColumn * max(len(args), 1))()
    keep = []
    for c, a in enumerate(args):
        idx = a[3] if len(a) == 4 else None
        if idx is not None and idx.numel() == 0:
            idx = torch.zeros(1, dtype=torch.int64, device="cuda:0")
            keep.append(idx)
        rows = int(a[3].numel()) if len(a) == 4 else int(a[1].numel())
        k = rows if k is None else k
        shift = table_shift[1] if table_shift is not None and table_shift[0] == c else 0
        cols[c] = ZipColumn(a[0].data_ptr() if a[0].numel() else 0, int(a[0].numel()), a[1].data_ptr() + shift if a[1].numel() else 0,
                            a[2].data_ptr() if a[2].numel() else 0, int(a[1].numel()), 0 if idx is None else idx.data_ptr(), 0 if idx is None else int(a[3].numel()),
                            widths[c], reserved)
    out = torch.full((cap + ROOM_BYTES + 16,), POISON8, dtype=torch.uint8, device="cuda:0")
    begins = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    ends = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    assert out.data_ptr() % 16 == 0
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    total = lib.rj_scan_records_zip(scan._h, cols, len(args) if n_cols is None else n_cols, sep, len(sep) if sep_len is None else sep_len, pad, flags, fill, lead, gap,
                                    ctypes.c_void_p(out.data_ptr() + out_shift) if cap else None, cap, vp(begins) if with_begin else None,
                                    vp(ends) if with_end else None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return int(total), out.cpu().numpy().tobytes()[:cap + ROOM_BYTES], begins.cpu().numpy(), ends.cpu().numpy()


def check(rj, scan, cols, widths=None, sep=b"", pad=32, fill=10, lead=0, gap=1, ctx=None, query=True):
    """the size query, then the call with an exact capacity, against zip_cases"""
    widths = [0] * len(cols) if widths is None else widths
    text, begins, ends = zc.layout(zc.lines([c.pieces() for c in cols], sep, widths, pad), fill, lead, gap)
    args = [c.arg() for c in cols]
    k = len(begins)
    c = (ctx, len(cols), widths, sep, pad, fill, lead, gap)
    if query:
        total, out, gb, ge = zip_poisoned(rj, scan, args, widths, sep, pad, fill, lead, gap, cap=0)
        assert total == len(text), (c, total, rj.load_library().rj_last_error())
        assert out == bytes([POISON8]) * ROOM_BYTES and (gb[:k] == begins).all() and (ge[:k] == ends).all(), c
    total, out, gb, ge = zip_poisoned(rj, scan, args, widths, sep, pad, fill, lead, gap, cap=len(text))
    assert total == len(text), (c, total, rj.load_library().rj_last_error())
    if out[:total] != text:
        at = next(i for i in range(total) if out[i] != text[i])
        raise AssertionError((c, "first differing byte", at, out[max(at - 30, 0):at + 30], text[max(at - 30, 0):at + 30]))
    assert out[total:] == bytes([POISON8]) * ROOM_BYTES, c
    assert (gb[:k] == begins).all() and (ge[:k] == ends).all() and (gb[k:] == POISON).all() and (ge[k:] == POISON).all(), c
    return text, begins, ends


def random_table(k, lengths, seed, junk=3):
    rng = random.Random(seed)
    return zc.table([rng.choice(lengths) for _ in range(k)], seed + 100, junk)


# ------------------------------------------------------------------------------------------------ 1. seams
def test_every_boundary_at_every_offset_of_a_group_and_across_a_chunk_end(rj, scan):
    """600 rows x 3 columns of pieces of 0, 1, 15, 16, 17 and 33 bytes, width 7 on column 0, a 2-byte separator, lead 0..31.
    Asserted from the Python rule BEFORE anything runs: every kind of boundary -- piece start, padding start, separator start,
    row end, gap start -- fell at every offset 0..15 of a 16-byte group, and a chunk's end fell inside a segment of every kind."""
    tables = zc.seam_columns(600)
    widths, sep, gap = [7, 0, 0], b", ", 2
    columns = [zc.pieces(*t) for t in tables]
    assert len(zc.layout(zc.lines(columns, sep, widths, 32), 10, 0, gap)[0]) > 2 * EMIT_CHUNK
    offsets, crossed = zc.seam_coverage(columns, sep, widths, 32, range(32), gap, EMIT_CHUNK)
    for kind in ("piece", "pad", "sep", "row", "gap"):
        assert offsets[kind] == set(range(16)), (kind, offsets[kind])
        assert crossed[kind] >= 1, (kind, crossed)
    cols = [Col(t) for t in tables]
    for lead in range(32):
        check(rj, scan, cols, widths, sep, lead=lead, gap=gap, ctx="seams", query=lead == 0)


# ------------------------------------------------------------------------------------------------ 2. source alignment
def test_every_source_misalignment_and_rows_at_the_texts_two_ends(rj, scan):
    """each column's text starts at every offset 0..15 past a 16-byte boundary; its first row begins at the text's first byte and
    its last row ends at its last one, both long enough to stream: the guarded loads at the two ends"""
    lengths = [0, 1, 33, 16, 100, 17, 31, 32, 64, 5, 48]
    tables = [zc.table([40 + c] + lengths[c:] + lengths[:c] + [50 - c], 20 + c, junk=0) for c in range(3)]
    for t in tables:
        assert t[1][0] == 0 and t[2][-1] == len(t[0]) and t[2][0] - t[1][0] >= STREAM_BYTES and t[2][-1] - t[1][-1] >= STREAM_BYTES
    for shift in range(16):
        cols = [Col(t, shift=(shift + 5 * c) % 16) for c, t in enumerate(tables)]
        assert cols[0].d_text.data_ptr() % 16 == shift
        check(rj, scan, cols, [0, -3, 7], b"|", lead=shift % 3, ctx=("misaligned", shift), query=False)


# ------------------------------------------------------------------------------------------------ 3. long pieces
def test_a_piece_of_100_kb_and_pieces_around_the_tier_threshold(rj, scan):
    T = STREAM_BYTES
    short = [3, 0, 8, 1, 20, 5]
    for position in range(3):      # the long piece in every column position, spanning 25 chunks
        tables = [zc.table(short[:3] + [100 * 1024] + short[3:] if c == position else short[:3] + [7] + short[3:], 30 + c + 3 * position) for c in range(3)]
        cols = [Col(t) for t in tables]
        text, _, _ = check(rj, scan, cols, [7, 0, 0], b" ", ctx=("100 KB", position))
        assert len(text) > 25 * EMIT_CHUNK
    around = [T - 1, T, T + 1]
    for position in range(3):
        tables = [zc.table([around[(j + c) % 3] if c == position else short[j % 6] for j in range(90)], 40 + c + 3 * position) for c in range(3)]
        check(rj, scan, [Col(t) for t in tables], [0, 0, 0], b"", ctx=("threshold", position))
        check(rj, scan, [Col(t) for t in tables], [T + 8, -(T + 8), T], b";", pad=0x2E, gap=0, ctx=("threshold, padded", position), query=False)


# ------------------------------------------------------------------------------------------------ 4. same text, reordered rows
def test_two_fields_of_one_split_swapped(rj, scan):
    """awk '{print $2, $1}': both columns are fields of ONE split_records over one text"""
    import torch
    from rejit_amd import records
    rng = random.Random(50)
    lines = [b"%s %d" % (bytes(rng.choice(b"abcdefgh") for _ in range(rng.randrange(1, 12))), rng.randrange(10 ** rng.randrange(1, 9))) for _ in range(2000)]
    data = b"\n".join(lines) + b"\n"
    text = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    begins, ends = records.line_records(text)
    begins, ends = begins[:-1].contiguous(), ends[:-1].contiguous()
    result = scan.run_records(text, begins, ends)
    pb, pe, pf = scan.split_records(begins, ends, result, int(text.numel()), what="between")
    b1, e1, _ = records.field_records(pb, pe, pf, 0)
    b2, e2, _ = records.field_records(pb, pe, pf, 1)
    out, ob, oe = scan.zip_records([(text, b2.contiguous(), e2.contiguous()), (text, b1.contiguous(), e1.contiguous())], sep=b" ")
    want = b"".join(b" ".join(reversed(line.split(b" "))) + b"\n" for line in lines)
    assert out.cpu().numpy().tobytes() == want
    assert ob.cpu().tolist() == [0] + list(np.cumsum([len(line) + 1 for line in lines])[:-1]) and (oe - ob).cpu().tolist() == [len(line) for line in lines]


def test_three_texts_and_index_lists_with_repeats_and_a_reversed_permutation(rj, scan):
    k = 700
    tables = [random_table(k, (0, 2, 9, 20, 50), 60 + c) for c in range(3)]
    rng = random.Random(63)
    repeats = [rng.randrange(k) for _ in range(k)]
    cols = [Col(tables[0], repeats), Col(tables[1], list(reversed(range(k)))), Col(tables[2])]
    check(rj, scan, cols, [5, -5, 0], b"\t", ctx="three texts")
    one = [Col(tables[0], repeats), Col(tables[0]), Col(tables[0], list(reversed(range(k))))]
    check(rj, scan, one, None, b" ", gap=0, lead=3, ctx="one text, three orders")
    few = [Col(tables[0], [7] * 50), Col(tables[1], [k - 1, 0] * 25)]
    check(rj, scan, few, None, b"--", ctx="k from the lists")


# ------------------------------------------------------------------------------------------------ 5. number columns
def test_counts_words_and_sums_as_uniq_c_prints_them(rj, scan):
    import torch
    rng = random.Random(70)
    k = 3000
    counts = [rng.randrange(10 ** rng.randrange(1, 9)) for _ in range(k)]
    sums = [rng.randrange(-10 ** 12, 10 ** 12) for _ in range(k)]
    fsums = [rng.uniform(-1e6, 1e6) * 10.0 ** rng.randrange(-8, 8) for _ in range(k)]
    words = random_table(k, (1, 3, 8, 12), 71)
    w = Col(words)
    count_col = scan.format_records(dev(counts))
    for values, column in ((sums, scan.format_records(dev(sums))), (fsums, scan.format_records(dev(fsums, np.float64)))):
        out, ob, oe = scan.zip_records([count_col, w.arg(), column], sep=b" ", widths=[7, 0, 0])
        want = b"".join(b"%7d %s %s\n" % (c, p, repr(v).encode()) for c, p, v in zip(counts, w.pieces(), values))
        assert out.cpu().numpy().tobytes() == want
        assert int(oe[-1]) + 1 == len(want) and int(ob[0]) == 0


# ------------------------------------------------------------------------------------------------ 6. the pack identity
def test_one_column_is_pack_records_byte_for_byte(rj, scan):
    table = random_table(1500, (0, 1, 15, 16, 17, 33, 90, 400), 80)
    rng = random.Random(81)
    for indices, lead, gap, fill in ((None, 0, 1, 10), ([rng.randrange(1500) for _ in range(999)], 5, 0, 0x2C), (list(reversed(range(1500))), 3, 7, 0)):
        col = Col(table, indices)
        packed, pb, pe = scan.pack_records(col.d_text, col.d_begins, col.d_ends, indices=col.d_indices, fill=fill, lead=lead, gap=gap)
        for sep in (b"", b"::"):
            zipped, zb, ze = scan.zip_records([col.arg()], sep=sep, fill=fill, lead=lead, gap=gap)
            assert zipped.cpu().numpy().tobytes() == packed.cpu().numpy().tobytes() and (zb == pb).all() and (ze == pe).all()
        check(rj, scan, [col], None, b"::", fill=fill, lead=lead, gap=gap, ctx="one column")


# ------------------------------------------------------------------------------------------------ 7. column count limits
def test_sixteen_columns_work_and_seventeen_are_refused(rj, scan):
    tables = [random_table(300, (0, 2, 9, 40), 90 + c) for c in range(4)]
    cols = [Col(tables[c % 4], None if c < 4 else [(j * (c + 1)) % 300 for j in range(300)]) for c in range(16)]
    check(rj, scan, cols, [(7, 0, -7, 40)[c % 4] for c in range(16)], b", ", ctx="16 columns")
    with pytest.raises(rj.RejitError) as err:
        scan.zip_records([c.arg() for c in cols] + [cols[0].arg()])
    assert "17 columns" in str(err.value)
    total, out, gb, ge = zip_poisoned(rj, scan, [cols[0].arg()] * 17, cap=4096)
    assert total == RJ_BAD_ARGUMENT and out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all()


# ------------------------------------------------------------------------------------------------ 8. beyond one pass of the plan
def test_one_row_more_than_a_pass_of_the_unit_grid(rj, scan):
    """262 145 rows drawn from three small tables: the resolve and the plan take their units round again.  Then one bad index in
    column 2 in the second pass: the call is refused naming row and column, and output and tables stay poisoned."""
    k = UNIT_GRID_ROWS + 1
    R = 1000
    tables = [random_table(R, (0, 1, 4, 9, 35), 100 + c) for c in range(3)]
    picks = [np.random.RandomState(103 + c).randint(0, R, k).astype(np.int64) for c in range(3)]
    cols = [Col(t, pk) for t, pk in zip(tables, picks)]
    text, begins, ends = check(rj, scan, cols, [7, 0, 0], b" ", ctx="two passes", query=False)
    bad = picks[2].copy()
    at = k - 1                                   # the one row of the second pass
    assert UNIT_GRID_ROWS <= at < k
    bad[at] = R
    args = [cols[0].arg(), cols[1].arg(), (cols[2].d_text, cols[2].d_begins, cols[2].d_ends, dev(bad))]
    total, out, gb, ge = zip_poisoned(rj, scan, args, [7, 0, 0], b" ", cap=len(text))
    msg = rj.load_library().rj_last_error().decode()
    assert total == RJ_BAD_ARGUMENT and "row %d column 2 " % at in msg, (total, msg)
    assert out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all()
    check(rj, scan, [Col(t, pk[:5000]) for t, pk in zip(tables, picks)], [7, 0, 0], b" ", ctx="behind a refusal")


# ------------------------------------------------------------------------------------------------ 9. beyond one turn of the emit
def test_the_output_passes_one_turn_of_the_emit_grid(rj, scan):
    """10 000 rows of 24 bytes with gap = 4096: 41 MB of output, five turns of the emit's 2048 workgroups of 4 KiB, most chunks
    without a row's begin, rows that cross a chunk's end"""
    k, gap = 10000, 4096
    assert k * (24 + gap) > 4 * EMIT_GRID_BYTES
    a, b = zc.table([5] * k, 110), zc.table([11] * k, 111)
    cols = [Col(a), Col(b)]
    total, out, gb, ge = zip_poisoned(rj, scan, [c.arg() for c in cols], [8, -15], b"=", gap=gap, cap=k * (24 + gap))
    assert total == k * (24 + gap), (total, rj.load_library().rj_last_error())
    got = np.frombuffer(out, dtype=np.uint8)
    assert (got[total:] == POISON8).all()
    rows = got[:total].reshape(k, 24 + gap)
    assert (rows[:, 24:] == 10).all()
    assert rows[:, :24].tobytes() == b"".join(zc.lines([cols[0].pieces(), cols[1].pieces()], b"=", [8, -15], 32))
    assert (gb[:k] == np.arange(k) * (24 + gap)).all() and (ge[:k] == gb[:k] + 24).all()


# ------------------------------------------------------------------------------------------------ 10. edges and refusals
def test_no_rows_and_all_empty_rows(rj, scan):
    import torch
    table = random_table(50, (1, 5), 120)
    none = Col(table, [])
    total, out, gb, ge = zip_poisoned(rj, scan, [none.arg(), none.arg()], None, b" ", fill=0x2C, lead=5, cap=16)
    assert total == 5 and out == b"," * 5 + bytes([POISON8]) * (11 + ROOM_BYTES) and (gb == POISON).all() and (ge == POISON).all()
    text, ob, oe = scan.zip_records([none.arg()], lead=3)
    assert text.cpu().numpy().tobytes() == b"\n\n\n" and ob.numel() == 0 and oe.numel() == 0
    empty = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    text, ob, oe = scan.zip_records([(none.d_text, empty, empty)])
    assert text.numel() == 0 and ob.numel() == 0
    hollow = Col(zc.table([0] * 5000, 121))
    for lead in (0, 5):
        text, begins, ends = check(rj, scan, [hollow, hollow, hollow], None, b"", lead=lead, gap=0, ctx="all empty")
        assert len(text) == lead and begins == [lead] * 5000
    mixed = Col(zc.table([0] * 2000 + [5] + [0] * 2000 + [40] + [0] * 998, 122))
    check(rj, scan, [mixed, hollow], None, b"", gap=0, ctx="runs of empty rows")


def test_out_too_small_the_size_query_and_out_given(rj, scan):
    import torch
    cols = [Col(random_table(900, (0, 2, 9, 40), 130 + c)) for c in range(3)]
    want, begins, ends = zc.layout(zc.lines([c.pieces() for c in cols], b" ", [7, 0, 0], 32), 0x2C, 2, 1)
    args = [c.arg() for c in cols]
    room = torch.full((len(want) + 64,), POISON8, dtype=torch.uint8, device="cuda:0")
    text, ob, oe = scan.zip_records(args, sep=b" ", widths=[7, 0, 0], fill=0x2C, lead=2, out=room)
    assert text.data_ptr() == room.data_ptr() and text.cpu().numpy().tobytes() == want and ob.cpu().tolist() == begins and oe.cpu().tolist() == ends
    assert (room[len(want):] == POISON8).all()
    small = torch.full((len(want) - 1,), POISON8, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(rj.RejitError) as err:
        scan.zip_records(args, sep=b" ", widths=[7, 0, 0], fill=0x2C, lead=2, out=small)
    assert "%d bytes" % len(want) in str(err.value)
    assert small.cpu().numpy().tobytes() == want[:-1]                     # nothing at or beyond out_cap was written, the rest is complete
    for cap in (len(want) - 17, EMIT_CHUNK + 5, 1):
        total, out, gb, ge = zip_poisoned(rj, scan, args, [7, 0, 0], b" ", fill=0x2C, lead=2, cap=cap)
        assert total == len(want) and out[:cap] == want[:cap] and out[cap:] == bytes([POISON8]) * ROOM_BYTES, cap
        assert (gb[:900] == begins).all() and (ge[:900] == ends).all()
    for kw in ({"with_begin": False}, {"with_end": False}, {"with_begin": False, "with_end": False}):
        total, out, gb, ge = zip_poisoned(rj, scan, args, [7, 0, 0], b" ", fill=0x2C, lead=2, cap=len(want), **kw)
        assert total == len(want) and out[:total] == want
        assert (gb == POISON).all() if not kw.get("with_begin", True) else (gb[:900] == begins).all()
        assert (ge == POISON).all() if not kw.get("with_end", True) else (ge[:900] == ends).all()


def test_the_tail_store_under_an_out_cap_sweep(rj, scan):
    """an output of two chunks and 21 bytes whose last row ends in a piece that streams: below min(out_cap, total) the reference's
    bytes, at and beyond it the sentinel, and the total returned whatever out_cap is"""
    target = 2 * EMIT_CHUNK + 21
    tables = [random_table(400, (0, 2, 9, 40), 140), zc.table([40] * 400, 141)]
    rows = zc.lines([zc.pieces(*t) for t in tables], b" ", [7, 0], 32)
    k = max(n for n in range(1, 401) if sum(len(r) + 1 for r in rows[:n]) <= target)
    lead = target - sum(len(r) + 1 for r in rows[:k])
    cols = [Col((t[0], t[1][:k], t[2][:k])) for t in tables]
    text, begins, ends = zc.layout(rows[:k], 0x2C, lead, 1)
    total = len(text)
    assert total == target and k > 100 and len(rows[k - 1]) >= 40 >= STREAM_BYTES
    args = [c.arg() for c in cols]
    for cap in (1, 15, 16, 17, 4095, 4096, 4097, total - 17, total - 16, total - 1, total, total + 16):
        got, out, gb, ge = zip_poisoned(rj, scan, args, [7, 0], b" ", fill=0x2C, lead=lead, cap=cap)
        below = min(cap, total)
        assert got == total, (cap, got, rj.load_library().rj_last_error())
        assert out[:below] == text[:below] and out[below:] == bytes([POISON8]) * (cap + ROOM_BYTES - below), cap
        assert (gb[:k] == begins).all() and (ge[:k] == ends).all(), cap


def test_refusals_write_nothing(rj, scan):
    import torch
    lib = rj.load_library()
    k = 300
    a, b, c = (Col(random_table(k, (0, 3, 9), 140 + i)) for i in range(3))
    short = Col(random_table(k - 1, (1, 2), 145))
    args = [a.arg(), b.arg(), c.arg()]

    def refused(word, cols=args, status=RJ_BAD_ARGUMENT, **kw):
        total, out, gb, ge = zip_poisoned(rj, scan, cols, kw.pop("widths", None), kw.pop("sep", b" "), cap=kw.pop("cap", 4096), k=k, **kw)
        msg = lib.rj_last_error().decode()
        assert total == status and word in msg, (word, total, msg)
        assert out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all(), word

    refused("0 columns", n_cols=0)
    refused("column 0 and column 2", cols=[a.arg(), b.arg(), short.arg()])
    refused("sep_len 65", sep=b"x" * 65)
    refused("width 4097", widths=[0, 4097, 0])
    refused("width -4097", widths=[0, 0, -4097])
    refused("reserved", reserved=1)
    for flags in (1, 2, 4, 0x80000000):
        refused("flags", flags=flags)
    refused("pad 256", pad=256)
    refused("pad -1", pad=-1)
    refused("fill 256", fill=256)
    refused("fill -1", fill=-1)
    refused("2^42", gap=1 << 42)
    refused("2^62", lead=1 << 62)
    refused("16-byte aligned", out_shift=8)
    refused("column 1: a table or d_indices is not 8-byte aligned", table_shift=(1, 4))
    bad_index = dev([0, 1, 2, k, 5, k + 7] + [0] * (k - 6))
    refused("row 3 column 1 ", cols=[a.arg(), (b.d_text, b.d_begins, b.d_ends, bad_index), c.arg()])
    # a bad row in a later column at an earlier row than a bad row in column 0
    refused("row 2 column 2 ", cols=[(a.d_text, a.d_begins, a.d_ends, bad_index), b.arg(), (c.d_text, c.d_begins, c.d_ends, dev([0, 1, k + 1] + [0] * (k - 3)))])
    ends_beyond = c.d_ends.clone()
    ends_beyond[k - 1] = len(c.text) + 1
    refused("row %d column 2 " % (k - 1), cols=[a.arg(), b.arg(), (c.d_text, c.d_begins, ends_beyond)])
    with pytest.raises(rj.RejitError):
        scan.zip_records(args, flags=1)
    with pytest.raises(rj.RejitError):
        scan.zip_records(args, sep=b"x" * 65)
    with pytest.raises(ValueError):
        scan.zip_records(args, widths=[1, 2])
    check(rj, scan, [a, b, c], [7, 0, 0], b" ", ctx="behind the refusals")


def test_the_scan_keeps_its_spans_stats_and_selection(rj, scan):
    import torch
    from rejit_amd import records
    text = torch.from_numpy(np.frombuffer(b"ab 12\ncd\ne 6 7\n", dtype=np.uint8).copy()).to("cuda:0")
    assert scan.run_tensor(text) == 3
    spans, stats = scan.spans(), scan.stats()
    col = Col(random_table(100, (0, 3, 9), 150))
    scan.zip_records([col.arg(), col.arg()], sep=b" ")
    assert scan.spans() == spans == [(2, 3), (10, 11), (12, 13)] and scan.stats() == stats
    begins, ends = records.line_records(text)
    begins, ends = begins[:-1].contiguous(), ends[:-1].contiguous()
    scan.run_records(text, begins, ends)
    before = scan.select_records().cpu().tolist()
    scan.zip_records([col.arg(), col.arg()], sep=b" ")
    assert scan.select_records().cpu().tolist() == before == [0, 2]


# ------------------------------------------------------------------------------------------------ 11. the sample
SAMPLE_LINES = [b"/a 200 0.25", b"/b 500 1e3", b"/a 200 -3.5", b"/c 404", b"/b 200 12abc", b"/a 301  5", b"/b 200 \t1.5", b"/c 200 0.30000000000000004",
                b"/a 200 -40", b"/d 200 1e999", b"/d 7 0", b"/e 200 6.02214076e23", b"/f 1 -0.125", b"/g 7 1e-400", b"/h 9 1e16", b"/h 9 9e15", b"/i 3 1e-7"]


@pytest.mark.parametrize("options", [[" ", "-f", "1", "-u"], [" ", "-f", "1", "-u", "-a", "2"], [" ", "-f", "1", "-u", "-A", "3"],
                                     [" ", "-f", "1", "-u", "-t", "3", "-A", "3"], [" ", "-f", "1", "-u", "-b", "-a", "2"]])
def test_linegrep_sample_lines_zipped_on_the_device(rj, tmp_path, options):
    """-Z: the printed lines are zipped on the device; the output is byte for byte the output without it"""
    path = str(tmp_path / "access.log")
    with open(path, "wb") as fh:
        fh.write(b"\n".join(SAMPLE_LINES) + b"\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    plain = subprocess.run([sys.executable, sample, path] + options, capture_output=True, timeout=300)
    device = subprocess.run([sys.executable, sample, path] + options + ["-Z"], capture_output=True, timeout=300)
    assert plain.returncode == device.returncode == 0, (plain.stderr.decode()[-500:], device.stderr.decode()[-500:])
    assert device.stdout == plain.stdout and len(plain.stdout) > 10, (device.stdout, plain.stdout)
    assert b"      4 /a" in device.stdout
