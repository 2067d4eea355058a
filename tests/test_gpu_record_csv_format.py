"""GPU tests (-m gpu) of rj_scan_records_format_csv (rejit_amd/csrc/record_csv_format.hip; Scan.format_csv_records,
records.csv_cut, samples/csvcut_gpu.py -C): the rows of several record tables written as quoted CSV lines on the device, laid
out as a pack.

The meaning is tests/csv_format_cases.py's, written in Python independently of the library: the rule over bytes, and the
layout arithmetic.  Every comparison is exact.  Outputs are poisoned first, with room behind the text and the tables that must
stay poisoned."""
import csv
import ctypes
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import csv_cases as cc
import csv_format_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_BAD_ARGUMENT = -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON8 = 0xA5
ROOM = 7                          # spare table rows
ROOM_BYTES = 53                   # spare output bytes
UNIT_GRID_ROWS = 1024 * 256       # record_frame.h: unit_grid() workgroups of 256 rows, one pass of the classify and of the plan
EMIT_GRID_BYTES = 256 * 8 * fc.EMIT_CHUNK   # record_frame.h: kCopyGrid workgroups, a chunk each: one turn of the emit


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
        return fc.pieces(self.text, self.begins, self.ends, self.indices)

    def arg(self):
        return (self.d_text, self.d_begins, self.d_ends) if self.d_indices is None else (self.d_text, self.d_begins, self.d_ends, self.d_indices)


def mask_of(listed):
    return sum(1 << c for c in set(listed))


def format_poisoned(rj, scan, args, d=44, q=34, always=(), raw=(), fill=10, lead=0, gap=1, cap=0, with_tables=True, stats=None):
    """the raw call into poisoned buffers -> (return value, out bytes with the spare ones, begins, ends with the spare rows);
    args: (text, begins, ends[, indices]) device tensors per column"""
    import torch
    from rejit_amd.api import ZipColumn
    lib = rj.load_library()
    cols = (ZipColumn * max(len(args), 1))()
    keep = []
    k = None
    for c, a in enumerate(args):
        idx = a[3] if len(a) == 4 else None
        if idx is not None and idx.numel() == 0:
            idx = torch.zeros(1, dtype=torch.int64, device="cuda:0")
            keep.append(idx)
        rows = int(a[3].numel()) if len(a) == 4 else int(a[1].numel())
        k = rows if k is None else k
        cols[c] = ZipColumn(a[0].data_ptr() if a[0].numel() else 0, int(a[0].numel()), a[1].data_ptr() if a[1].numel() else 0,
                            a[2].data_ptr() if a[2].numel() else 0, int(a[1].numel()), 0 if idx is None else idx.data_ptr(), 0 if idx is None else int(a[3].numel()), 0, 0)
    out = torch.full((cap + ROOM_BYTES + 16,), POISON8, dtype=torch.uint8, device="cuda:0")
    begins = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    ends = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    assert out.data_ptr() % 16 == 0
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    total = lib.rj_scan_records_format_csv(scan._h, cols, len(args), d, q, mask_of(always), mask_of(raw), 0, fill, lead, gap, vp(out) if cap else None, cap,
                                           vp(begins) if with_tables else None, vp(ends) if with_tables else None,
                                           None if stats is None else ctypes.byref(stats), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return int(total), out.cpu().numpy().tobytes()[:cap + ROOM_BYTES], begins.cpu().numpy(), ends.cpu().numpy()


def check(rj, scan, cols, d=44, q=34, always=(), raw=(), fill=10, lead=0, gap=1, ctx=None, query=True):
    """the size query, then the call with an exact capacity, against csv_format_cases"""
    from rejit_amd.api import _CsvFormatStats
    columns = [c.pieces() for c in cols]
    text, begins, ends = fc.layout(fc.lines(columns, d, q, always, raw), fill, lead, gap)
    args = [c.arg() for c in cols]
    k = len(begins)
    c = (ctx, len(cols), d, q, always, raw, fill, lead, gap)
    if query:
        total, out, gb, ge = format_poisoned(rj, scan, args, d, q, always, raw, fill, lead, gap, cap=0)
        assert total == len(text), (c, total, rj.load_library().rj_last_error())
        assert out == bytes([POISON8]) * ROOM_BYTES and (gb[:k] == begins).all() and (ge[:k] == ends).all(), c
    st = _CsvFormatStats()
    total, out, gb, ge = format_poisoned(rj, scan, args, d, q, always, raw, fill, lead, gap, cap=len(text), stats=st)
    assert total == len(text), (c, total, rj.load_library().rj_last_error())
    if out[:total] != text:
        at = next(i for i in range(total) if out[i] != text[i])
        raise AssertionError((c, "first differing byte", at, out[max(at - 30, 0):at + 30], text[max(at - 30, 0):at + 30]))
    assert out[total:] == bytes([POISON8]) * ROOM_BYTES, c
    assert (gb[:k] == begins).all() and (ge[:k] == ends).all() and (gb[k:] == POISON).all() and (ge[k:] == POISON).all(), c
    assert (st.n_rows, st.n_fields, st.total) == (k, k * len(cols), total) and (st.n_quoted, st.n_doubled) == fc.stats(columns, d, q, always, raw), c
    return text, begins, ends


def columns_of(cols, seed=0, junk=3):
    return [fc.column_of(col, seed + c, junk) for c, col in enumerate(cols)]


# ------------------------------------------------------------------------------------------------ 1. tiers
@pytest.mark.parametrize("raw", [(), (0,)], ids=["value", "raw"])
def test_tier_thresholds_with_no_quote_one_quote_at_every_position_and_all_quotes(rj, scan, raw):
    pieces = fc.tier_pieces()
    assert {len(p) for p in pieces} == set(fc.TIER_LENGTHS)
    short = [b"k%d" % (i % 7) for i in range(len(pieces))]
    cols = [Col(t) for t in columns_of([pieces, short], 8)]
    check(rj, scan, cols, raw=raw, ctx="tiers")
    check(rj, scan, [cols[1], cols[0]], raw=tuple(1 - c for c in raw), always=(0,), lead=7, gap=0, ctx="tiers, second column", query=False)


def test_every_source_misalignment_and_rows_at_the_texts_two_ends(rj, scan):
    """the text starts at every offset 0..15 past a 16-byte boundary; its first row begins at the text's first byte and its last
    row ends at its last one, in every tier: the guarded loads at the two ends"""
    plain, quoted = b"p" * 40, b'q"' * 20
    tables = [fc.column_of([first] + [b"", b"a", b'"', b"x" * 33, b'y"' * 17, b"z" * 16] + [last], 1, junk=0) for first, last in ((plain, quoted), (quoted, plain), (b"s,", b'"'))]
    for t in tables:
        assert t[1][0] == 0 and t[2][-1] == len(t[0])
    for shift in range(16):
        cols = [Col(t, shift=(shift + 5 * c) % 16) for c, t in enumerate(tables)]
        assert cols[0].d_text.data_ptr() % 16 == shift
        check(rj, scan, cols, lead=shift % 3, raw=(1,) if shift % 2 else (), ctx=("misaligned", shift), query=False)


# ------------------------------------------------------------------------------------------------ 2. seams
@pytest.mark.parametrize("boundary", [fc.EMIT_CHUNK, fc.EMIT_CHUNK + 16, 2 * fc.EMIT_CHUNK], ids=["chunk", "group", "second-chunk"])
def test_quotes_doubled_quotes_and_delimiters_across_chunk_and_group_seams(rj, scan, boundary):
    """the opening quote, both bytes of a doubled quote, the closing quote and a delimiter at every offset -2..+2 around a chunk's
    boundary and around a 16-byte group's, for a short piece and for one that expands"""
    cases = fc.seam_cases(boundary)
    assert len(cases) == 2 * 5 * 5
    made = {}
    for name, columns, lead in cases:
        key = id(columns)
        if key not in made:
            made[key] = [Col(t) for t in columns_of(columns, 2)]
        text, begins, _ = check(rj, scan, made[key], lead=lead, ctx=name, query=False)
        assert begins[0] == lead and len(text) > boundary


# ------------------------------------------------------------------------------------------------ 3. long pieces
def test_long_expanding_pieces(rj, scan):
    quotes = Col(fc.column_of([b'"' * 5000], 1))
    text, _, _ = check(rj, scan, [quotes], ctx="5000 quotes")
    assert text == b'"' * 10002 + b"\n"                          # three chunks, the later two begin inside the piece
    check(rj, scan, [quotes, quotes], lead=9, ctx="5000 quotes twice", query=False)
    body = bytearray(b"m" * 9000)
    for at in (15, 16, 1023, 1024, 8999):
        body[at] = 34
    cols = [Col(fc.column_of([bytes(body), b"tail"], 2)), Col(fc.column_of([b"x", bytes(body)], 3))]
    for lead in (0, 1, fc.EMIT_CHUNK - 17):
        check(rj, scan, cols, lead=lead, ctx=("9000 bytes", lead), query=False)
    check(rj, scan, cols, raw=(0, 1), ctx="9000 bytes raw", query=False)


def test_expanding_pieces_that_leave_checkpoints(rj, scan):
    """pieces of CHECKPOINT_BYTES and more (one byte less walks from its begin): many chunks begin inside them, at a lead that
    puts the piece's first byte last in a chunk too; and a short output, where nothing behind out_cap is walked or written"""
    spread = bytearray(b"s" * 65536)
    spread[::61] = b'"' * len(spread[::61])
    exact, below = b'x"' + b"y" * (fc.CHECKPOINT_BYTES - 2), b'"' + b"z" * (fc.CHECKPOINT_BYTES - 2)
    pieces = [bytes(spread), b'"' * 20000, exact, below, b"mid"]
    cols = [Col(fc.column_of(pieces, 1)), Col(fc.column_of(list(reversed(pieces)), 2))]
    for lead in (0, 3, fc.EMIT_CHUNK - 1):
        text, _, _ = check(rj, scan, cols, lead=lead, ctx=("checkpoints", lead), query=lead == 0)
    for cap in (3 * fc.EMIT_CHUNK + 5, 40000):
        total, out, gb, ge = format_poisoned(rj, scan, [c.arg() for c in cols], lead=fc.EMIT_CHUNK - 1, cap=cap)
        assert total == len(text) and out[:cap] == text[:cap] and out[cap:] == bytes([POISON8]) * ROOM_BYTES, cap
    check(rj, scan, cols, raw=(1,), always=(0,), ctx="checkpoints, one raw column", query=False)


# ------------------------------------------------------------------------------------------------ 4. grid passes
def test_no_rows_and_one_empty_row(rj, scan):
    some = fc.column_of([b"a", b"b"], 1)
    for lead in (0, 5):
        check(rj, scan, [Col(some, indices=[]), Col(some, indices=[])], lead=lead, ctx="k = 0")
    text, _, _ = check(rj, scan, [Col(fc.column_of([b""], 1))], ctx="k = 1, the lone empty field")
    assert text == b'""\n'
    text, _, _ = check(rj, scan, [Col(fc.column_of([b""], 1))] * 2, gap=0, ctx="k = 1, two empty fields")
    assert text == b","


def test_more_than_one_pass_of_the_classify_and_plan_grid(rj, scan):
    k = UNIT_GRID_ROWS + 1
    words = [b"", b"a", b"bc", b'"', b"d,e", b"fgh"]
    table = fc.column_of(words, 1)
    rng = random.Random(3)
    first, second = [rng.randrange(len(words)) for _ in range(k)], [rng.randrange(len(words)) for _ in range(k)]
    check(rj, scan, [Col(table, indices=first), Col(table, indices=second)], ctx="k past one grid pass", query=False)


def test_more_than_one_turn_of_the_emit(rj, scan):
    pieces = [b"r" * 2900 + b'"' + b"s" * 99, b"t" * 3000, b"u,v" * 1000]
    k = EMIT_GRID_BYTES // 3000 + 8
    col = Col(fc.column_of(pieces, 1), indices=[j % 3 for j in range(k)])
    text, _, _ = check(rj, scan, [col], ctx="past one turn of the emit", query=False)
    assert len(text) > EMIT_GRID_BYTES


# ------------------------------------------------------------------------------------------------ 5. the call's contract
def test_the_call_contract(rj, scan):
    k = 300
    values = fc.random_rows(k, 2, 44, upto=40, nul=True)
    one, other = (Col(t) for t in columns_of(values, 13))
    rng = random.Random(9)
    perm = list(range(k))
    rng.shuffle(perm)
    repeats = [rng.randrange(k) for _ in range(k)]
    check(rj, scan, [one] * 16, ctx="16 columns sharing one text")
    check(rj, scan, [Col(one_t, indices=i) for one_t, i in (((one.text, one.begins, one.ends), perm), ((one.text, one.begins, one.ends), repeats))] + [other],
          always=(1,), raw=(2,), d=0, ctx="a permutation, repeats, a NUL delimiter")
    # out_cap one short (and shorter): total is returned, nothing at or beyond out_cap is written; the tables are complete
    text, begins, ends = fc.layout(fc.lines(values))
    for cap in (len(text) - 1, len(text) - 17, 1):
        total, out, gb, ge = format_poisoned(rj, scan, [one.arg(), other.arg()], cap=cap)
        assert total == len(text) and out[:cap] == text[:cap] and out[cap:] == bytes([POISON8]) * ROOM_BYTES, cap
        assert (gb[:k] == begins).all() and (ge[:k] == ends).all() and (gb[k:] == POISON).all()
    total, out, gb, ge = format_poisoned(rj, scan, [one.arg(), other.arg()], cap=len(text), with_tables=False)
    assert total == len(text) and out[:total] == text and (gb == POISON).all() and (ge == POISON).all()
    # a bad row: the first (row, column) is named, no byte and no table row is written
    bad = list(range(k))
    bad[77] = k
    worse = list(range(k))
    worse[76], worse[200] = 1 << 40, k
    total, out, gb, ge = format_poisoned(rj, scan, [Col((one.text, one.begins, one.ends), indices=bad).arg(), Col((other.text, other.begins, other.ends), indices=worse).arg()],
                                         cap=len(text))
    message = rj.load_library().rj_last_error().decode()
    assert total == RJ_BAD_ARGUMENT and message.startswith("rj_scan_records_format_csv: ") and "row 76 column 1 " in message, (total, message)
    assert set(out) == {POISON8} and (gb == POISON).all() and (ge == POISON).all()
    # a refusal before any launch
    total, out, gb, ge = format_poisoned(rj, scan, [one.arg(), other.arg()], raw=(2,), cap=len(text))
    assert total == RJ_BAD_ARGUMENT and "raw_mask 0x4 " in rj.load_library().rj_last_error().decode() and set(out) == {POISON8} and (gb == POISON).all()
    with pytest.raises(rj.RejitError) as err:
        scan.format_csv_records([one.arg()], delimiter=b"\n")
    assert err.value.status == RJ_BAD_ARGUMENT and "line break" in err.value.message


def test_the_tail_store_under_an_out_cap_sweep(rj, scan):
    """an output of two chunks and 21 bytes, fields of every tier, the last row's last field one that streams: below
    min(out_cap, total) the reference's bytes, at and beyond it the sentinel, and the total returned whatever out_cap is"""
    target = 2 * fc.EMIT_CHUNK + 21
    kinds = [b"ab", b'q"r', b"", b"x" * 40, b'y"' * 20, b"c,d"]
    values = [[kinds[(j + c) % len(kinds)] for j in range(400)] for c in range(2)]
    values[1] = [b"z" * 40] * 400
    rows = fc.lines(values)
    k = max(n for n in range(1, 401) if sum(len(r) + 1 for r in rows[:n]) <= target)
    lead = target - sum(len(r) + 1 for r in rows[:k])
    values = [col[:k] for col in values]
    cols = [Col(t) for t in columns_of(values, 17)]
    text, begins, ends = fc.layout(rows[:k], 0x2C, lead, 1)
    total = len(text)
    assert total == target and k > 60
    args = [c.arg() for c in cols]
    for cap in (1, 15, 16, 17, 4095, 4096, 4097, total - 17, total - 16, total - 1, total, total + 16):
        got, out, gb, ge = format_poisoned(rj, scan, args, fill=0x2C, lead=lead, cap=cap)
        below = min(cap, total)
        assert got == total, (cap, got, rj.load_library().rj_last_error())
        assert out[:below] == text[:below] and out[below:] == bytes([POISON8]) * (cap + ROOM_BYTES - below), cap
        assert (gb[:k] == begins).all() and (ge[:k] == ends).all(), cap


def test_the_python_interface(rj, scan):
    import torch
    values = fc.random_rows(500, 3, 5, upto=12)
    cols = [Col(t) for t in columns_of(values, 3)]
    for kw, meaning in (({}, {}), ({"delimiter": b";", "quote": b"'", "always": (0, 2), "raw": (1,), "fill": 0, "lead": 3, "gap": 2},
                                   {"d": 59, "q": 39, "always": (0, 2), "raw": (1,)})):
        lines = fc.lines(values, **meaning)
        text, begins, ends = fc.layout(lines, kw.get("fill", 10), kw.get("lead", 0), kw.get("gap", 1))
        out, ob, oe, st = scan.format_csv_records([c.arg() for c in cols], stats=True, **kw)
        assert out.cpu().numpy().tobytes() == text and ob.cpu().tolist() == begins and oe.cpu().tolist() == ends
        quoted, doubled = fc.stats(values, **meaning)
        assert st == {"n_rows": 500, "n_fields": 1500, "n_quoted": quoted, "n_doubled": doubled, "total": len(text)}
        room = torch.full((len(text) + 64,), POISON8, dtype=torch.uint8, device="cuda:0")
        out, ob, oe = scan.format_csv_records([c.arg() for c in cols], out=room, **kw)
        assert out.cpu().numpy().tobytes() == text and set(room[len(text):].cpu().tolist()) == {POISON8}
        with pytest.raises(rj.RejitError):
            scan.format_csv_records([c.arg() for c in cols], out=room[:len(text) - 1 & ~15], **kw)
    assert fc.lines(values) == fc.python_lines(values)            # ... and the default call is csv.writer's


# ------------------------------------------------------------------------------------------------ 6. round trip and csv_cut
def test_round_trip_through_csv_records(rj, scan):
    from rejit_amd import records
    from rejit_amd.api import CSV_MALFORMED
    k, n_cols = 2000, 3
    values = fc.random_rows(k, n_cols, 17, upto=20)
    values[0][:4] = [b'""', b'"', b"\r\n", b'a"",""b']
    cols = [Col(t) for t in columns_of(values, 4)]
    out, _, _ = scan.format_csv_records([c.arg() for c in cols], fill=10, gap=1)
    table = scan.csv_records(out)
    assert (table.n_rows, table.n_fields) == (k, k * n_cols) and table.stats["first_bad"] is None
    assert not bool(((table.field_flags & CSV_MALFORMED) != 0).any())
    vt, vb, ve = records.csv_values(scan, out, table.field_begin, table.field_end, table.field_flags)
    want_text, want_b, want_e = fc.layout([values[c][j] for j in range(k) for c in range(n_cols)])
    assert vt.cpu().numpy().tobytes() == want_text and vb.cpu().tolist() == want_b and ve.cpu().tolist() == want_e


def python_cut(text, picks, d=","):
    """csv.reader -> pick -> csv.writer (a line at a time, lineterminator "\\r\\n" as the rule states it), an absent column as an
    empty field; a line feed behind every line"""
    rows = [row or [""] for row in csv.reader(io.StringIO(text.decode("latin-1"), newline=""), strict=True, delimiter=d)]
    columns = [[(row[c] if -len(row) <= c < len(row) else "").encode("latin-1") for row in rows] for c in picks]
    return b"".join(line + b"\n" for line in fc.python_lines(columns, ord(d)))


def test_csv_cut_against_python(rj, scan):
    import torch
    from rejit_amd import records
    texts = [cc.generated(300, seed, n_cols=5, d=b",", final_break=seed % 2 == 0)[0] for seed in (1, 2)]
    texts.append(b'only\n"q,1",x,"say ""hi"""\na,"b\r\nc",,d,e\n"",""\n')                     # ragged rows
    for text in texts:
        t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
        table = scan.csv_records(t, rows=False)
        assert table.stats["first_bad"] is None
        for picks in ((0,), (2, 0), (4, 1, 1, -1)):
            out, ob, oe = records.csv_cut(scan, t, table, picks)
            assert out.cpu().numpy().tobytes() == python_cut(text, picks), picks
            assert ob.numel() == table.n_rows


def test_csvcut_sample_writes_csv(rj, tmp_path):
    """samples/csvcut_gpu.py -C on a file with embedded delimiters, quotes and line breaks: csv.reader(strict=True) reads the output
    back to the chosen columns"""
    text = cc.generated(200, 7, n_cols=4, d=b",")[0]
    path = tmp_path / "in.csv"
    path.write_bytes(text)
    theirs = list(csv.reader(io.StringIO(text.decode("latin-1"), newline=""), strict=True))
    assert any("," in f for row in theirs for f in row) and any('"' in f for row in theirs for f in row) and any("\n" in f for row in theirs for f in row)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "samples", "csvcut_gpu.py"), str(path), "-C", "3,1"], capture_output=True, timeout=300)
    assert done.returncode == 0, done.stderr.decode()
    assert done.stdout == python_cut(text, (2, 0))
    back = list(csv.reader(io.StringIO(done.stdout.decode("latin-1"), newline=""), strict=True))
    assert back == [[row[2], row[0]] for row in theirs]
