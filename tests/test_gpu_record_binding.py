"""GPU tests (-m gpu) of the ctypes binding of the record calls (rejit_amd/api.py: the 16 *_records methods of Scan): every
method through the real library on one tiny table, with every kind of row list and every flag combination that changes what
a method returns.

The table is the smallest with an empty row, a duplicate row and an order that is not sorted.  What the calls must give is
written here in plain Python (slicing, sorted, dict, int, datetime, re, csv), independently of the binding; every comparison
is exact.  The kernels have their own tests (tests/test_gpu_record_*.py); this one is about the arguments the binding hands
them: the empty row list that must not read as "every row", fill=None, `out`, and the number of values a call returns."""
import csv
import datetime
import io
import re

import pytest

pytestmark = pytest.mark.gpu

TEXT = b"b,1\n\nA,22\nb,1\n"
NUMBERS = b"7\n-3\nx\n\n"
DATES = b"2024-02-29\n1970-01-01\n1999-12-31\n\n"      # three ISO dates and an empty row
PATTERN = rb"[0-9]+"
ROW_LISTS = (None, [], [3, 0, 0, 2])
LEAD, GAP, FILL = 2, 1, 0x7C
OK, EMPTY, MALFORMED = 0, 1, 2


def lines_of(text):
    """-> (begins, ends) of the line records of a text that ends with a line break"""
    begins, ends, at = [], [], 0
    for line in text.split(b"\n")[:-1]:
        begins.append(at)
        ends.append(at + len(line))
        at += len(line) + 1
    return begins, ends


def picked(rows, idx):
    return list(rows) if idx is None else [rows[i] for i in idx]


def layout(rows, fill, lead=LEAD, gap=GAP):
    """-> (text, begins, ends): `lead` fill bytes, then every row with `gap` fill bytes behind it"""
    f = bytes([fill])
    text, begins, ends = f * lead, [], []
    for row in rows:
        begins.append(len(text))
        ends.append(len(text) + len(row))
        text += row + f * gap
    return text, begins, ends


@pytest.fixture(scope="module")
def rj():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rejit_amd
    import rejit_amd.records  # noqa: F401  (ASCII_LOWER)
    rejit_amd.build()
    rejit_amd.load_library()
    return rejit_amd


def dev(values, dtype=None):
    import torch
    return torch.tensor(list(values), dtype=torch.int64 if dtype is None else dtype, device="cuda:0")


def text_dev(b):
    import torch
    return torch.tensor(list(b), dtype=torch.uint8, device="cuda:0")


def rows_dev(idx):
    return None if idx is None else dev(idx)


def host(t):
    return t.cpu().tolist()


def raw(t):
    return bytes(host(t))


class Table:
    def __init__(self, text):
        self.text = text
        self.begins, self.ends = lines_of(text)
        self.rows = [text[b:e] for b, e in zip(self.begins, self.ends)]
        self.d_text, self.d_begins, self.d_ends = text_dev(text), dev(self.begins), dev(self.ends)

    def args(self):
        return self.d_text, self.d_begins, self.d_ends


@pytest.fixture(scope="module")
def table(rj):
    t = Table(TEXT)
    assert t.rows == [b"b,1", b"", b"A,22", b"b,1"]
    return t


@pytest.fixture(scope="module")
def scan(rj):
    return rj.Scan(rj.Program(PATTERN))


def check_text_call(rj, call, rows, fill, extra=0):
    """call(out) -> what the binding returns: without `out`, with an `out` of exactly `total` bytes, of total + 3 and of
    total - 1; -> the values behind (out_text, out_begin, out_end) of the last good call"""
    import torch

    text, begins, ends = layout(rows, fill)
    got = None
    for room in (None, 0, 3):
        out = None if room is None else torch.full((len(text) + room,), 0xA5, dtype=torch.uint8, device="cuda:0")
        got = call(out)
        assert isinstance(got, tuple) and len(got) == 3 + extra
        assert got[0].dtype == torch.uint8 and got[0].numel() == len(text) and raw(got[0]) == text
        assert host(got[1]) == begins and host(got[2]) == ends
        if out is not None:
            assert got[0].data_ptr() == out.data_ptr() and raw(out[len(text):]) == b"\xa5" * room
    with pytest.raises(rj.RejitError) as e:
        call(torch.empty(len(text) - 1, dtype=torch.uint8, device="cuda:0"))
    assert e.value.status == -4
    return got[3:]


def test_run_and_select_records(rj, scan, table):
    res = scan.run_records(*table.args())
    counts = [len(re.findall(PATTERN, r)) for r in table.rows]
    spans = [(m.start(), m.end()) for m in re.finditer(PATTERN, TEXT)]
    assert isinstance(res, rj.api.RecordsResult) and res.n_records == 4
    assert (res.n_kept, res.n_matching, res.n_crossing, res.n_matches) == (3, 3, 0, 3)
    assert host(res.counts) == counts == [1, 0, 1, 1]
    assert scan.spans() == spans
    first = host(res.first)
    for i, (b, e) in enumerate(zip(table.begins, table.ends)):
        mine = [s for s in spans if b <= s[0] <= e]
        assert spans[first[i]:first[i] + counts[i]] == mine
    with_match = [i for i, c in enumerate(counts) if c]
    assert host(scan.select_records()) == with_match == [0, 2, 3] and scan.n_selected == 3
    assert host(scan.select_records(invert=True)) == [1] and scan.n_selected == 1
    assert host(scan.select_records(cap=1)) == [0] and scan.n_selected == 3
    # tensors of the caller's
    import torch
    c, f = torch.empty(4, dtype=torch.int32, device="cuda:0"), torch.empty(4, dtype=torch.int64, device="cuda:0")
    res = scan.run_records(*table.args(), counts=c, first=f)
    assert res.counts is c and res.first is f and host(c) == counts


@pytest.mark.parametrize("idx", ROW_LISTS)
@pytest.mark.parametrize("fill", (FILL, None))
def test_pack_translate_replace(rj, scan, table, idx, fill):
    separator = scan.program.batch_separator()
    assert 0 <= separator < 256
    byte = separator if fill is None else fill
    rows = picked(table.rows, idx)
    kw = dict(indices=rows_dev(idx), fill=fill, lead=LEAD, gap=GAP)
    check_text_call(rj, lambda out: scan.pack_records(*table.args(), out=out, **kw), rows, byte)
    lower = [r.lower() for r in rows]
    check_text_call(rj, lambda out: scan.translate_records(*table.args(), table=rj.records.ASCII_LOWER, out=out, **kw), lower, byte)
    stats, = check_text_call(rj, lambda out: scan.translate_records(*table.args(), table=rj.records.ASCII_LOWER, out=out, stats=True, **kw), lower, byte,
                             extra=1)
    assert stats == {"bytes_in": sum(len(r) for r in rows), "bytes_dropped": 0, "bytes_changed": sum(a != b for r, l in zip(rows, lower) for a, b in zip(r, l))}
    res = scan.run_records(*table.args())
    check_text_call(rj, lambda out: scan.replace_records(*table.args(), res, b"#", out=out, **kw), [re.sub(PATTERN, b"#", r) for r in rows], byte)


@pytest.mark.parametrize("idx", ROW_LISTS)
@pytest.mark.parametrize("what", ("between", "matches"))
def test_split_records(rj, scan, table, idx, what):
    res = scan.run_records(*table.args())
    got = scan.split_records(table.d_begins, table.d_ends, res, len(TEXT), indices=rows_dev(idx), what=what)
    assert isinstance(got, tuple) and len(got) == 3
    begins, ends, first = [], [], [0]
    for r in picked(range(4), idx):
        at, stop = table.begins[r], table.ends[r]
        found = [(at + m.start(), at + m.end()) for m in re.finditer(PATTERN, table.rows[r])]
        if what == "matches":
            pieces = found
        else:
            pieces = list(zip([at] + [e for _, e in found], [b for b, _ in found] + [stop]))
        begins += [b for b, _ in pieces]
        ends += [e for _, e in pieces]
        first.append(len(begins))
    assert host(got[0]) == begins and host(got[1]) == ends and host(got[2]) == first
    if idx is None:
        fields = [TEXT[b:e] for b, e in zip(begins, ends)]
        assert fields == ([b"1", b"22", b"1"] if what == "matches" else [b"b,", b"", b"", b"A,", b"", b"b,", b""])


@pytest.mark.parametrize("idx", ROW_LISTS)
def test_group_and_sort_records(rj, scan, table, idx):
    rows = picked(table.rows, idx)
    got = scan.group_records(*table.args(), indices=rows_dev(idx))
    assert isinstance(got, tuple) and len(got) == 3
    number, rep, count = {}, [], []
    for j, r in enumerate(rows):
        if r not in number:
            number[r] = len(rep)
            rep.append(j)
            count.append(0)
        count[number[r]] += 1
    assert host(got[0]) == [number[r] for r in rows] and host(got[1]) == rep and host(got[2]) == count
    if idx is None:
        assert (host(got[0]), rep, count) == ([0, 1, 2, 0], [0, 1, 2], [2, 1, 1])

    import torch
    order = sorted(range(len(rows)), key=lambda j: rows[j])
    got = scan.sort_records(*table.args(), indices=rows_dev(idx))
    assert isinstance(got, torch.Tensor) and host(got) == order
    got = scan.sort_records(*table.args(), indices=rows_dev(idx), stats=True)
    assert isinstance(got, tuple) and len(got) == 2 and host(got[0]) == order
    assert sorted(got[1]) == ["keyed_rows", "long_rows", "rounds", "skip_rows"] and all(isinstance(v, int) for v in got[1].values())
    if idx is None:
        assert order == [1, 2, 0, 3]
    if len(rows) < 2:
        assert got[1]["rounds"] == 0


@pytest.mark.parametrize("set_idx", ROW_LISTS)
@pytest.mark.parametrize("idx", ROW_LISTS)
def test_lookup_records(rj, scan, table, set_idx, idx):
    import torch
    set_rows, rows = picked(table.rows, set_idx), picked(table.rows, idx)
    smallest = {}
    for j, r in enumerate(set_rows):
        smallest.setdefault(r, j)
    index = [smallest.get(r, -1) for r in rows]
    hits = [0] * len(set_rows)
    for j in index:
        if j >= 0:
            hits[j] += 1
    stats = {"n_found": sum(j >= 0 for j in index), "n_set_distinct": len(smallest), "n_set_hit": sum(h > 0 for h in hits)}
    for want_hits in (False, True):
        for want_stats in (False, True):
            got = scan.lookup_records(*table.args(), *table.args(), set_indices=rows_dev(set_idx), indices=rows_dev(idx), hits=want_hits, stats=want_stats)
            if not (want_hits or want_stats):
                assert isinstance(got, torch.Tensor)
                got = (got,)
            assert isinstance(got, tuple) and len(got) == 1 + want_hits + want_stats
            assert host(got[0]) == index
            if want_hits:
                assert host(got[1]) == hits
            if want_stats:
                assert sorted(got[-1]) == ["long_rows", "n_found", "n_set_distinct", "n_set_hit"]
                assert {f: got[-1][f] for f in stats} == stats
    if set_idx is None and idx is None:
        assert index == [0, 1, 2, 0] and hits == [2, 1, 1, 0]


@pytest.mark.parametrize("idx", ROW_LISTS)
def test_parse_and_format_records(rj, scan, idx):
    import torch
    numbers = Table(NUMBERS)
    assert numbers.rows == [b"7", b"-3", b"x", b""]
    values, status = [], []
    for r in picked(numbers.rows, idx):
        try:
            values.append(int(r.decode()))
            status.append(OK)
        except ValueError:
            values.append(0)
            status.append(MALFORMED if r else EMPTY)
    assert (rj.PARSE_OK, rj.PARSE_EMPTY, rj.PARSE_MALFORMED) == (OK, EMPTY, MALFORMED)
    got = scan.parse_records(*numbers.args(), indices=rows_dev(idx))
    assert isinstance(got, tuple) and len(got) == 2
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.uint8 and host(got[0]) == values and host(got[1]) == status
    got = scan.parse_records(*numbers.args(), indices=rows_dev(idx), kind="int64", stats=True)
    assert isinstance(got, tuple) and len(got) == 3 and host(got[0]) == values and host(got[1]) == status
    assert got[2] == {"n_ok": status.count(OK), "n_empty": status.count(EMPTY), "n_malformed": status.count(MALFORMED), "n_range": 0, "n_inexact": 0}

    # the whole parsed column and its status, formatted through the row list
    column, column_status = scan.parse_records(*numbers.args())
    assert host(column) == [7, -3, 0, 0] and host(column_status) == [OK, OK, MALFORMED, EMPTY]
    rows = picked([b"7", b"-3", b"", b""], idx)
    kw = dict(status=column_status, indices=rows_dev(idx), lead=LEAD, gap=GAP)
    check_text_call(rj, lambda out: scan.format_records(column, out=out, fill=FILL, **kw), rows, FILL)
    check_text_call(rj, lambda out: scan.format_records(column, out=out, **kw), rows, 10)
    check_text_call(rj, lambda out: scan.format_records(column, indices=rows_dev(idx), lead=LEAD, gap=GAP, out=out), picked([b"7", b"-3", b"0", b"0"], idx), 10)


@pytest.mark.parametrize("idx", ROW_LISTS)
def test_parse_time_and_format_time_records(rj, scan, idx):
    import torch
    dates = Table(DATES)
    fmt = "%Y-%m-%d"
    epoch = datetime.datetime(1970, 1, 1)
    values, status = [], []
    for r in picked(dates.rows, idx):
        if r:
            values.append(int((datetime.datetime.strptime(r.decode(), fmt) - epoch) // datetime.timedelta(seconds=1)))
            status.append(OK)
        else:
            values.append(0)
            status.append(EMPTY)
    got = scan.parse_time_records(*dates.args(), fmt, indices=rows_dev(idx))
    assert isinstance(got, tuple) and len(got) == 2
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.uint8 and host(got[0]) == values and host(got[1]) == status
    got = scan.parse_time_records(*dates.args(), fmt, indices=rows_dev(idx), stats=True)
    assert isinstance(got, tuple) and len(got) == 3 and host(got[0]) == values and host(got[1]) == status
    assert got[2] == {"n_ok": status.count(OK), "n_empty": status.count(EMPTY), "n_malformed": 0, "n_range": 0, "n_inexact": 0}

    column, column_status = scan.parse_time_records(*dates.args(), fmt)
    assert host(column) == [19782 * 86400, 0, 10956 * 86400, 0] and host(column_status) == [OK, OK, OK, EMPTY]
    rows = picked(dates.rows, idx)
    kw = dict(status=column_status, indices=rows_dev(idx), lead=LEAD, gap=GAP)
    check_text_call(rj, lambda out: scan.format_time_records(column, fmt, out=out, fill=FILL, **kw), rows, FILL)
    check_text_call(rj, lambda out: scan.format_time_records(column, fmt, out=out, **kw), rows, 10)
    stats, = check_text_call(rj, lambda out: scan.format_time_records(column, fmt, out=out, stats=True, **kw), rows, 10, extra=1)
    assert stats == {"n_ok": sum(1 for r in rows if r), "n_null": sum(1 for r in rows if not r), "n_range": 0}


def zip_column(t, idx):
    return t.args() if idx is None else t.args() + (dev(idx),)


@pytest.mark.parametrize("idx", ROW_LISTS)
def test_zip_and_format_csv_records(rj, scan, table, idx):
    other = None if idx is None else idx[::-1]
    left, right = picked(table.rows, idx), picked(table.rows, other)
    columns = [zip_column(table, idx), zip_column(table, other)]
    lines = [a.rjust(4, b" ") + b"|" + b for a, b in zip(left, right)]
    kw = dict(sep=b"|", widths=[4, 0], lead=LEAD, gap=GAP)
    check_text_call(rj, lambda out: scan.zip_records(columns, out=out, fill=FILL, **kw), lines, FILL)
    check_text_call(rj, lambda out: scan.zip_records(columns, out=out, **kw), lines, 10)

    lines, n_quoted = [], 0
    for a, b in zip(left, right):
        buf = io.StringIO()
        csv.writer(buf, lineterminator="").writerow([a.decode(), b.decode()])
        lines.append(buf.getvalue().encode())
        n_quoted += sum(b"," in f for f in (a, b))
    if idx is None:
        assert lines == [b'"b,1","b,1"', b",", b'"A,22","A,22"', b'"b,1","b,1"']
    kw = dict(lead=LEAD, gap=GAP)
    check_text_call(rj, lambda out: scan.format_csv_records(columns, out=out, fill=FILL, **kw), lines, FILL)
    check_text_call(rj, lambda out: scan.format_csv_records(columns, b",", b'"', out=out, **kw), lines, 10)
    stats, = check_text_call(rj, lambda out: scan.format_csv_records(columns, 44, 34, out=out, stats=True, **kw), lines, 10, extra=1)
    assert sorted(stats) == ["n_doubled", "n_fields", "n_quoted", "n_rows", "total"]
    assert (stats["n_rows"], stats["n_fields"], stats["n_quoted"], stats["n_doubled"]) == (len(lines), 2 * len(lines), n_quoted, 0)


def test_csv_records(rj, scan, table):
    parsed = [r or [""] for r in csv.reader(io.StringIO(TEXT.decode(), newline=""), strict=True)]
    assert parsed == [["b", "1"], [""], ["A", "22"], ["b", "1"]]
    n_rows, n_fields = len(parsed), sum(len(r) for r in parsed)
    row_first = [0]
    for r in parsed:
        row_first.append(row_first[-1] + len(r))
    flat = [f.encode() for r in parsed for f in r]
    for rows in (True, False):
        for caps in ({}, {"row_cap": n_rows, "field_cap": n_fields}):
            got = scan.csv_records(table.d_text, rows=rows, **caps)
            assert isinstance(got, rj.api.CsvResult) and (got.n_rows, got.n_fields) == (n_rows, n_fields)
            assert host(got.row_first) == row_first
            assert [TEXT[b:e] for b, e in zip(host(got.field_begin), host(got.field_end))] == flat and host(got.field_flags) == [0] * n_fields
            if rows:
                assert host(got.row_begin) == table.begins and host(got.row_end) == table.ends
            else:
                assert got.row_begin is None and got.row_end is None
            assert got.stats == {"n_rows": n_rows, "n_fields": n_fields, "n_quoted": 0, "n_escapes": 0, "n_bad_quote": 0, "n_bad_close": 0, "n_bare_cr": 0,
                                 "open_at_end": 0, "first_bad": None}
    with pytest.raises(rj.RejitError):
        scan.csv_records(table.d_text, row_cap=n_rows - 1, field_cap=n_fields)
    got = scan.csv_records(table.d_text, delimiter=44, quote=None)
    assert (got.n_rows, got.n_fields) == (n_rows, n_fields)
