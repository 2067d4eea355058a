"""GPU tests (-m gpu) of rj_scan_records_csv (rejit_amd/csrc/record_csv.hip; Scan.csv_records, records.csv_column / csv_bad_rows /
csv_values, samples/csvcut_gpu.py): the rows and fields of a CSV text with quoted fields as record tables.

The meaning is tests/csv_cases.py's, written in Python independently of the library: the rule byte by byte (numpy for the
text of megabytes) and Python's csv.  Every comparison is exact.  Tables are poisoned first, with room behind them that must
stay poisoned."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import csv_cases as cc
import csv_sweep as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_BAD_ARGUMENT = -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON32 = -0x5A5A5A5B
ROOM = 7                          # spare table entries
TABLES = ("row_first", "row_begin", "row_end", "field_begin", "field_end", "field_flags")
UNIT, GRID, WAVES = 4096, 2048, 4  # rejit_amd/csrc/record_csv.h: kUnit, kGrid, kWavesPerGroup (tests/test_record_csv.py checks the mirror)
assert (UNIT, GRID, WAVES) == (sw.DEFAULT_UNIT, sw.DEFAULT_GRID, sw.WAVES_PER_GROUP)


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


@pytest.fixture
def geometry(monkeypatch):
    def force(unit=None, grid=None):
        for name, value in (("RJ_CSV_UNIT", unit), ("RJ_CSV_GRID", grid)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(value))
    force()
    return force


def upload(text, shift=0):
    """the text on the device, its first byte `shift` bytes past a 16-byte boundary"""
    import torch
    room = torch.full((len(text) + 32,), 0x22, dtype=torch.uint8, device="cuda:0")     # (quote bytes around it: nothing outside [0, n) may count)
    assert room.data_ptr() % 16 == 0
    d_text = room[shift:shift + len(text)]
    if len(text):
        d_text.copy_(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()))
    return d_text


def raw(rj, scan, d_text, d=44, q=34, row_cap=0, field_cap=0, query=False, stream=None, with_stats=True, shifts=None, n=None, text_null=False):
    """the raw call into poisoned tables -> (return value, stats dict (poison where untouched), the tables with their spare entries as numpy)"""
    import torch
    from rejit_amd.api import _CsvStats as Stats
    lib = rj.load_library()
    i64 = lambda k: torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    t = {"row_first": i64(row_cap + 1), "row_begin": i64(row_cap), "row_end": i64(row_cap), "field_begin": i64(field_cap), "field_end": i64(field_cap),
         "field_flags": torch.full((field_cap + ROOM,), POISON32, dtype=torch.int32, device="cuda:0")}
    vp = lambda name: None if query else ctypes.c_void_p(t[name].data_ptr() + (shifts or {}).get(name, 0))
    stats = Stats(*([0xA5] * 9))
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = lib.rj_scan_records_csv(scan._h, None if text_null or not d_text.numel() else ctypes.c_void_p(d_text.data_ptr()), int(d_text.numel()) if n is None else n,
                                 d, -1 if q is None else q, vp("row_first"), vp("row_begin"), vp("row_end"), 0 if query else row_cap, vp("field_begin"),
                                 vp("field_end"), vp("field_flags"), 0 if query else field_cap, ctypes.byref(stats) if with_stats else None, ctypes.c_void_p(st))
    torch.cuda.synchronize()
    return int(rc), {f: int(getattr(stats, f)) for f, _ in Stats._fields_}, {k: v.cpu().numpy() for k, v in t.items()}


def compare(got, want, row_cap, field_cap, ctx):
    rows, fields = want["stats"]["n_rows"], want["stats"]["n_fields"]
    for name, count, cap in (("row_first", rows + 1, row_cap + 1), ("row_begin", rows, row_cap), ("row_end", rows, row_cap), ("field_begin", fields, field_cap),
                             ("field_end", fields, field_cap), ("field_flags", fields, field_cap)):
        shown = min(count, cap)
        w = np.asarray(want[name][:shown], dtype=got[name].dtype)
        if not np.array_equal(got[name][:shown], w):
            at = int(np.nonzero(got[name][:shown] != w)[0][0])
            raise AssertionError((ctx, name, "entry", at, "got", int(got[name][at]), "want", int(w[at])))
        poison = POISON32 if name == "field_flags" else POISON
        assert (got[name][shown:] == poison).all(), (ctx, name, "written at or beyond the cap or the counts")


def check(rj, scan, text, d=44, q=34, want=None, ctx=None, shift=0, python=False):
    """the size query, then the fill with exact caps, against csv_cases"""
    want = cc.tables(text, d, q) if want is None else want
    d_text = upload(text, shift)
    stats_want = want["stats"]
    rc, stats, got = raw(rj, scan, d_text, d, q, query=True)
    assert rc == stats_want["n_fields"] and stats == stats_want, (ctx, "size query", rc, stats, stats_want)
    assert all((got[name] == (POISON32 if name == "field_flags" else POISON)).all() for name in TABLES), (ctx, "size query")
    rows, fields = stats_want["n_rows"], stats_want["n_fields"]
    rc, stats, got = raw(rj, scan, d_text, d, q, row_cap=rows, field_cap=fields)
    assert rc == fields and stats == stats_want, (ctx, rc, stats, stats_want)
    compare(got, want, rows, fields, ctx)
    if python:
        cc.check_against_python(text, want, d, q)
    return want


@pytest.fixture(scope="module")
def generated():
    text, vals = cc.generated(720, 21)
    assert 36 << 10 < len(text) < 48 << 10
    return text, vals, cc.tables(text)


# ------------------------------------------------------------------------------------------------------------------ parity
def test_generated_text(rj, scan, generated, geometry):
    text, vals, want = generated
    assert want["stats"]["n_quoted"] > 1000 and want["stats"]["n_escapes"] > 100 and not any(f & cc.MALFORMED for f in want["field_flags"])
    assert [[v.encode("latin-1") for v in row] for row in cc.values(text, want)] == vals
    for shift in (0, 5):
        check(rj, scan, text, want=want, shift=shift, python=True)
    geometry(unit=1024, grid=1)          # four spans of ten and more units each
    check(rj, scan, text, want=want)


@pytest.mark.parametrize("kind", ["bad_quote", "bad_close", "bare_cr", "open", "all"])
def test_planted_offences(rj, scan, generated, kind):
    text, _, whole = generated
    row = b'alpha,"beta",gamma\n'
    at = len(text)
    text = text + row + text[:whole["row_begin"][80]]
    # (where, the byte, its flag, the offending byte: a bad close is named by its quote)
    plants = {"bad_quote": (at + 2, b'"', cc.BAD_QUOTE, at + 2), "bad_close": (at + 12, b"x", cc.BAD_CLOSE, at + 11), "bare_cr": (at + 15, b"\r", cc.BARE_CR, at + 15)}
    flag = cc.OPEN
    for name, (p, byte, f, _) in plants.items():
        if kind in (name, "all"):
            text, flag = cc.plant(text, p, byte), f
    if kind in ("open", "all"):
        text += b'tail,"never closed\nand on'
    want = check(rj, scan, text, python=True, ctx=kind)
    if kind == "all":      # (the first offence changes what the later bytes are: only it is certain)
        assert any(f & cc.BAD_QUOTE for f in want["field_flags"]) and want["stats"]["first_bad"] == at + 2
        return
    assert any(f & flag for f in want["field_flags"])
    if kind in plants:
        assert want["stats"]["first_bad"] == plants[kind][3]
    if kind == "open":
        assert want["stats"]["open_at_end"] == 1 and want["field_flags"][-1] == cc.OPEN and want["stats"]["first_bad"] == len(text)


def test_no_quote_and_tab(rj, scan):
    text, _ = cc.generated(300, 22, d=b"\t")
    check(rj, scan, text, d=9, python=True)
    plain, _ = cc.generated(300, 23, d=b"\t", kinds=("plain", "number", "empty"))
    plain = plain.replace(b'"', b"'")
    want = check(rj, scan, plain, d=9, q=None)
    lines = plain.replace(b"\r\n", b"\n").split(b"\n")[:-1]
    assert [[plain[b:e] for b, e, _ in row] for row in cc.rows_of(want)] == [line.split(b"\t") for line in lines]
    # a quote byte is an ordinary byte without a quote
    want = check(rj, scan, text, d=9, q=None)
    assert want["stats"]["n_quoted"] == 0 and not any(want["field_flags"])


def test_no_final_line_break(rj, scan):
    text, _ = cc.generated(200, 24, final_break=False)
    want = check(rj, scan, text, python=True)
    assert want["row_end"][-1] == len(text)
    check(rj, scan, text + b",", python=True)
    check(rj, scan, text + b"\r", python=True)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17])
def test_tiny_texts(rj, scan, n):
    rng = random.Random(n)
    texts = {bytes(rng.choice(b'a",\n\r') for _ in range(n)) for _ in range(40)} | {b"a" * n, b'"' * n, b"," * n, b"\n" * n, (b"\r\n" * n)[:n]}
    for text in sorted(texts):
        for shift in (0, 3):
            check(rj, scan, text, shift=shift, python=True, ctx=text)


# ------------------------------------------------------------------------------------------------------------------ seams
@pytest.mark.parametrize("motif", list(sw.MOTIFS))
@pytest.mark.parametrize("name", list(sw.GEOMETRIES))
def test_seams(rj, scan, geometry, name, motif):
    unit, grid, n = sw.GEOMETRIES[name]
    geometry(unit=unit, grid=grid)
    for m, byte, offset, starts in sw.plan(name):
        if m != motif:
            continue
        text = sw.planted(name, m, starts)
        assert len(text) == n
        check(rj, scan, text, ctx=(name, m, byte, offset))


def test_quoted_field_over_three_units(rj, scan, geometry):
    """the units 1, 2 and 3 hold neither a quote nor a structural byte: only the parity the resolve hands on tells them from rows"""
    head = b'id,"' + b"y" * (UNIT - 3 - 4)
    text = head + b"x,\n" + (b"in, side\n" * UNIT)[:3 * UNIT] + b'z",end\r\nnext,"row"\n'
    want = cc.tables(text)
    assert want["stats"]["n_rows"] == 2 and want["field_end"][1] - want["field_begin"][1] > 3 * UNIT
    for unit, grid in ((UNIT, 2), (UNIT, 1), (None, None), (1024, 1)):
        geometry(unit=unit, grid=grid)
        check(rj, scan, text, want=want, ctx=(unit, grid))
    cc.check_against_python(text, want)


def test_past_one_unit_per_wave_at_the_default_geometry(rj, scan, geometry):
    """more units than the default grid has waves: every wave's span is two units, but for the last ones"""
    import torch
    geometry()
    n = GRID * WAVES * UNIT + 3 * UNIT + 17
    block, _ = cc.generated(900, 25)
    text = block * (n // len(block))              # (whole blocks, so that the text is well-formed ...)
    text += b"x" * (n - len(text))               # (... and the odd tail is one last, long field without a line break)
    assert len(text) == n and n > GRID * WAVES * UNIT and n % 16 == 1
    want = cc.tables_numpy(text)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    got = scan.csv_records(t)
    assert got.n_rows == want["row_begin"].size and got.n_fields == want["field_begin"].size and got.stats["first_bad"] is None
    assert got.stats["n_escapes"] >= int((want["field_flags"] != 0).sum()) > 0
    for name in TABLES:
        assert np.array_equal(getattr(got, name).cpu().numpy().astype(np.int64), want[name]), name
    given = scan.csv_records(t, row_cap=got.n_rows + 3, field_cap=got.n_fields + 3)      # the fill alone
    for name in TABLES:
        assert torch.equal(getattr(given, name), getattr(got, name)), name


# ------------------------------------------------------------------------------------------------------------------ contract
def test_caps_and_size_query(rj, scan, generated):
    text, _, want = generated
    text = text[:6000]
    want = cc.tables(text)
    d_text = upload(text)
    rows, fields = want["stats"]["n_rows"], want["stats"]["n_fields"]
    for row_cap in (rows - 1, rows, rows + 5):
        for field_cap in (fields - 1, fields, fields + 5):
            rc, stats, got = raw(rj, scan, d_text, row_cap=row_cap, field_cap=field_cap)
            assert rc == fields and stats == want["stats"]
            compare(got, want, row_cap, field_cap, (row_cap, field_cap))
    rc, stats, got = raw(rj, scan, d_text, row_cap=0, field_cap=0)
    assert rc == fields and stats == want["stats"] and got["row_first"][0] == 0 and (got["row_first"][1:] == POISON).all()


def test_the_scan_keeps_its_own_state(rj, generated):
    import torch
    text, _, want = generated
    d_text = upload(text)
    scan = rj.Scan(rj.Program(b"[a-j]+"))
    count = scan.run_tensor(d_text)
    spans, stats = scan.spans_tensor(d_text.device).clone(), scan.stats()
    got = scan.csv_records(d_text)
    assert got.n_fields == want["stats"]["n_fields"]
    assert count > 0 and torch.equal(scan.spans_tensor(d_text.device), spans) and scan.stats() == stats


def test_a_refused_call_leaves_poison(rj, scan):
    d_text = upload(b"a,b\nc,d\n")
    for kw in ({"text_null": True, "n": 8}, {"with_stats": False}, {"shifts": {"row_begin": 4}}, {"shifts": {"field_begin": 2}}, {"shifts": {"field_flags": 2}},
               {"d": -1}, {"d": 256}, {"q": -2}, {"q": 256}, {"d": 10}, {"d": 13}, {"q": 10}, {"q": 13}, {"d": 34}, {"n": 1 << 42}):
        rc, stats, got = raw(rj, scan, d_text, row_cap=2, field_cap=4, **kw)
        assert rc == RJ_BAD_ARGUMENT, kw
        assert "rj_scan_records_csv" in rj.load_library().rj_last_error().decode(), kw
        assert all(v == 0xA5 for v in stats.values()), kw
        for name in TABLES:
            assert (got[name] == (POISON32 if name == "field_flags" else POISON)).all(), (kw, name)
    rc, stats, _ = raw(rj, scan, d_text, row_cap=2, field_cap=4)
    assert rc == 4 and stats["n_rows"] == 2


def test_two_streams(rj, generated):
    import torch
    text, _, want = generated
    d_text = upload(text)
    torch.cuda.synchronize()
    results = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        scan = rj.Scan(rj.Program(b" "))
        with torch.cuda.stream(stream):
            results.append(scan.csv_records(d_text, stream=stream.cuda_stream))
    torch.cuda.synchronize()
    for name in TABLES:
        assert torch.equal(getattr(results[0], name), getattr(results[1], name)), name
        assert getattr(results[0], name).cpu().tolist() == want[name], name
    assert results[0].stats == results[1].stats


# ------------------------------------------------------------------------------------------------------------------ composition
def test_values_unescape_inside_the_packed_text(rj, scan):
    import torch
    from rejit_amd import records
    text = b'k,v\r\n1,"""a"\n2,"a""""b"\n3,""\n4,plain\n5,"q,""r"""\n6\n'
    theirs, err = cc.python_rows(text)
    assert err is None
    t = upload(text)
    table = scan.csv_records(t)
    assert table.n_rows == 7 and not bool(records.csv_bad_rows(table.row_first, table.field_flags).any())
    for c in (0, 1, -1):
        index, present = records.csv_column(table.row_first, c)
        rows = torch.nonzero(present).reshape(-1)
        out, ob, oe = records.csv_values(scan, t, table.field_begin, table.field_end, table.field_flags, indices=index[rows].contiguous())
        packed = out.cpu().numpy().tobytes()
        got = [packed[b:e].decode("latin-1") for b, e in zip(ob.cpu().tolist(), oe.cpu().tolist())]
        assert got == [theirs[r][c] for r in rows.cpu().tolist()], c
    index, present = records.csv_column(table.row_first, 1)
    assert present.cpu().tolist() == [True] * 6 + [False]
    every, ob, oe = records.csv_values(scan, t, table.field_begin, table.field_end, table.field_flags)
    packed = every.cpu().numpy().tobytes()
    assert [packed[b:e].decode("latin-1") for b, e in zip(ob.cpu().tolist(), oe.cpu().tolist())] == [v for row in theirs for v in row]
    bad = scan.csv_records(upload(b'a,b\nc"d"x,e\nf,g\n'))
    assert records.csv_bad_rows(bad.row_first, bad.field_flags).cpu().tolist() == [False, True, False]


def sales_file(n_rows, seed, quote_amounts=0):
    """-> (text, rows): name, amount, tag per row; a field is quoted when it has to be, every quote_amounts-th amount as well"""
    rng = random.Random(seed)
    names = ["Smith, John", 'O"Neil', "plain", "Line\nBreak", "", "Zo\xc3\xab"]
    rows = [(rng.choice(names), rng.randint(-5000, 5000), rng.choice(["x", "y,z"])) for _ in range(n_rows)]
    field = lambda s, force=False: '"' + s.replace('"', '""') + '"' if force or any(c in s for c in ',"\n\r') else s
    lines = [",".join((field(name), field("%d" % amount, bool(quote_amounts) and i % quote_amounts == 0), field(tag))) for i, (name, amount, tag) in enumerate(rows)]
    return ("\n".join(lines) + "\n").encode("latin-1"), rows


def test_a_quoted_numeric_column_sums(rj, scan):
    from rejit_amd import records
    text, rows = sales_file(1000, 31, quote_amounts=3)
    t = upload(text)
    table = scan.csv_records(t)
    assert table.n_rows == 1000 and table.stats["first_bad"] is None and table.stats["n_quoted"] > 600
    index, present = records.csv_column(table.row_first, 1)
    assert bool(present.all())
    vt, vb, ve = records.csv_values(scan, t, table.field_begin, table.field_end, table.field_flags, indices=index)
    values, status = scan.parse_records(vt, vb, ve, kind="int64", trim=True)
    assert bool((status == rj.PARSE_OK).all()) and int(values.sum()) == sum(a for _, a, _ in rows)


def test_csvcut_sample(rj, tmp_path):
    """samples/csvcut_gpu.py against the same queries in Python on a 1000-row file with quoted fields"""
    import csv
    import io
    text, rows = sales_file(1000, 32, quote_amounts=4)
    path = tmp_path / "sales.csv"
    path.write_bytes(text)
    theirs = list(csv.reader(io.StringIO(text.decode("latin-1"), newline=""), strict=True))
    assert len(theirs) == 1000
    sums = {}
    for name, amount, _ in theirs:
        sums[name] = sums.get(name, 0) + int(amount)
    run = lambda *args: subprocess.run([sys.executable, os.path.join(ROOT, "samples", "csvcut_gpu.py"), str(path), *args], capture_output=True, timeout=300)
    done = run("-g", "1", "-a", "2")
    assert done.returncode == 0, done.stderr.decode()
    assert done.stdout.decode("latin-1") == "".join("%s\t%d\n" % (name, total) for name, total in sums.items())
    done = run("-c", "3,1")
    assert done.returncode == 0, done.stderr.decode()
    assert done.stdout.decode("latin-1") == "".join("%s\t%s\n" % (tag, name) for name, _, tag in theirs)
