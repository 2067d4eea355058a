"""GPU tests (-m gpu) of rj_scan_records_parse (rejit_amd/csrc/record_parse.hip; Scan.parse_records), of records.group_sums
and of samples/linegrep_gpu.py -a.

The meaning is tests/parse_cases.py's, written in Python independently of the library: re.fullmatch of the three grammars,
int() and the type's range for the integer kinds, decimal.Decimal for (m, q) and the bits of float() for the doubles; a row
that is not OK has the value 0.  Every comparison is exact, bit patterns included.  Outputs are poisoned first, with ROOM
extra rows that must stay poisoned."""
import ctypes
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import parse_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_TOO_LARGE, RJ_BAD_ARGUMENT = -2, -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON_U = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 7
KS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1500)
LENS = (0, 1, 15, 16, 17, 31, 32, 33, 700)
STATS = ("n_ok", "n_empty", "n_malformed", "n_range", "n_inexact")      # rj_parse_stats: five uint64

meaning = functools.lru_cache(maxsize=None)(pc.meaning)


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
    text, records = pc.lay(rows, **kw)
    return Table(text, records)


def parse_poisoned(rj, scan, T, kind, trim, want_status=True, want_stats=True):
    """rj_scan_records_parse into poisoned tables -> (return value, values as uint64, status: the whole buffers, stats or None)"""
    import torch
    lib = rj.load_library()
    k = T.k()
    values = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    status = torch.full((k + ROOM,), POISON8, dtype=torch.uint8, device="cuda:0")
    keep = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
    idx = None if T.idx_t is None else (T.idx_t if k else keep)      # (a non-null pointer with a count of 0: no rows)
    out = (ctypes.c_uint64 * 5)(*([0xA5A5] * 5))
    total = lib.rj_scan_records_parse(scan._h, vp(T.d), int(T.d.numel()), vp(T.rb_t), vp(T.re_t), len(T.records),
                                      ctypes.c_void_p(idx.data_ptr()) if idx is not None else None, k if idx is not None else 0, kind, 1 if trim else 0,
                                      vp(values), vp(status) if want_status else None,
                                      ctypes.cast(out, lib.rj_scan_records_parse.argtypes[12]) if want_stats else None,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    stats = dict(zip(STATS, (int(x) for x in out))) if want_stats else None
    return int(total), values.cpu().numpy().view(np.uint64), status.cpu().numpy(), stats


def check(rj, scan, T, kinds=pc.KINDS, trims=(False, True), api=False, ctx=None):
    """the raw call into poisoned tables -- with d_status and stats, and each of them NULL -- against the meaning; Scan.parse_records"""
    import torch
    k, strings = T.k(), T.strings()
    for kind in kinds:
        for trim in trims:
            want = [meaning(s, kind, trim) for s in strings]
            w_status = np.array([w[0] for w in want], dtype=np.uint8)
            w_bits = np.array([w[1] for w in want], dtype=np.uint64)
            w_stats = dict(zip(STATS, (int((w_status == c).sum()) for c in range(5))))
            c = (ctx, kind, trim, k)
            for want_status, want_stats in ((True, True), (False, True), (True, False)):
                total, values, status, stats = parse_poisoned(rj, scan, T, kind, trim, want_status, want_stats)
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
                a_values, a_status, a_stats = scan.parse_records(T.d, T.rb_t, T.re_t, indices=T.idx_t, kind=pc.KIND_NAMES[kind], trim=trim, stats=True)
                assert a_values.numel() == k and a_status.numel() == k and a_status.dtype == torch.uint8 and a_stats == w_stats, c
                assert a_values.dtype == (torch.float64 if kind == pc.FLOAT64 else torch.int64), c
                assert (a_values.cpu().numpy().view(np.uint64) == w_bits).all() and (a_status.cpu().numpy() == w_status).all(), c
                only = scan.parse_records(T.d, T.rb_t, T.re_t, indices=T.idx_t, kind=pc.KIND_NAMES[kind], trim=trim)
                assert len(only) == 2 and (only[0].cpu().numpy().view(np.uint64) == w_bits).all()


@pytest.fixture(scope="module")
def pool():
    """every named family of tests/parse_cases.py and a seeded mix, shuffled: 1500 rows and more"""
    rows = pc.all_case_rows() + pc.random_rows(900, 31)
    random.Random(3).shuffle(rows)
    assert len(rows) >= 1500
    return rows


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("k", KS)
def test_sizes_equal_the_meaning_for_every_kind_and_flag(rj, scan, pool, k):
    check(rj, scan, laid(pool[:k]), api=k in (0, 65, 1500), ctx="sizes")


def test_every_family_of_cases(rj, scan):
    rows = pc.all_case_rows()
    T = laid(rows)
    check(rj, scan, T, ctx="families")
    for kind in pc.KINDS:
        assert {meaning(r, kind, True)[0] for r in rows} == {pc.OK, pc.EMPTY, pc.MALFORMED, pc.INEXACT if kind == pc.FLOAT64 else pc.RANGE}


# ------------------------------------------------------------------------------------------------ alignment, length, the text's ends
def test_every_misalignment_of_a_rows_begin_and_the_group_lengths(rj, scan):
    """Rows of 0, 1, 15, 16, 17, 31, 32, 33 and 700 bytes -- a number that fills them, one with a point, one spoilt at its last
    byte -- beginning at every residue 0..15; the first row at offset 0, the last one ending at byte n, n no multiple of 16."""
    rows, text, records = [], bytearray(), []
    for length in LENS:
        shapes = [b"0" * max(length - 1, 0) + b"7" * min(length, 1)]
        if length >= 3:
            shapes += [b"0" * (length - 3) + b"1.5", b"0" * (length - 1) + b"x", b"9" * length, b" " * (length - 2) + b"-3"]
        for mis in range(16):
            for s in shapes:
                while len(text) % 16 != mis:
                    text += b"|"
                records.append((len(text), len(text) + len(s)))
                text += s
                rows.append(s)
    text += b"|" * ((5 - len(text)) % 16) + b"12345"
    records.append((len(text) - 5, len(text)))
    assert records[0][0] == 0 and len(text) % 16 == 10 and records[-1][1] == len(text)
    assert {b % 16 for b, _ in records} == set(range(16))
    T = Table(bytes(text), records)
    assert int(T.d.data_ptr()) % 16 == 0
    check(rj, scan, T, ctx="misalignment")
    # the same rows behind one byte more: every begin moves by one against the device's 16-byte blocks
    check(rj, scan, Table(b"#" + bytes(text), [(b + 1, e + 1) for b, e in records]), kinds=(pc.FLOAT64,), trims=(True,), ctx="shifted")


def test_a_row_of_a_mebibyte_is_one_lanes_walk(rj, scan):
    zeros = b"0" * (1 << 20)
    T = laid([b"17", zeros, zeros + b"7", b"1" + zeros, b"-4"], sep_of=lambda i: b"|")
    check(rj, scan, T, kinds=(pc.INT64, pc.FLOAT64), trims=(False,), ctx="MiB")
    assert meaning(zeros, pc.INT64, False) == (pc.OK, 0) and meaning(b"1" + zeros, pc.FLOAT64, False) == (pc.INEXACT, 0)


# ------------------------------------------------------------------------------------------------ index lists
def test_index_lists_with_repeats_and_permutations(rj, scan, pool):
    T = laid(pool[:400])
    rng = random.Random(9)
    perm = list(range(400))
    rng.shuffle(perm)
    for name, rows in (("permutation", perm), ("repeats", [rng.randrange(400) for _ in range(1000)]), ("one row", [123] * 300), ("none", []),
                       ("reversed", list(range(399, -1, -1)))):
        check(rj, scan, T.take(rows), kinds=(pc.INT64, pc.FLOAT64), api=name == "repeats", ctx=name)


# ------------------------------------------------------------------------------------------------ the doubles
def test_the_boundary_table_has_floats_bits_on_the_device(rj, scan):
    """Every q in [-22, 22] x the boundary mantissas 2^53 - 1, 2^53, 2^53 + 1 and twenty more: the device's one multiplication or
    division must give float()'s bits -- this is the test that decides whether the compiler's IEEE division is correctly rounded
    on this part.  Then the window's edges and one value in many spellings."""
    rows = pc.boundary_table()
    assert len(rows) == 45 * 22
    T = laid(rows)
    check(rj, scan, T, kinds=(pc.FLOAT64,), ctx="boundary")
    ok = [r for r in rows if meaning(r, pc.FLOAT64, False)[0] == pc.OK]
    assert len(ok) == 45 * 21 and all(meaning(r, pc.FLOAT64, False)[0] == pc.INEXACT for r in rows if r not in ok)      # (2^53 + 1 is outside)
    check(rj, scan, laid(pc.window_rows() + pc.spelling_rows()), kinds=(pc.FLOAT64,), ctx="window")
    # a seeded mix inside the window: m below 2^53, every q
    rng = random.Random(77)
    mixed = []
    for _ in range(3000):
        m, q = rng.randrange(1, 1 << rng.randrange(1, 54)), rng.randrange(-22, 23)
        mixed.append(b"%de%d" % (m, q) if rng.randrange(2) else b"%d.%0*d" % (m, rng.randrange(1, 23), rng.randrange(1000)))
    check(rj, scan, laid(mixed), kinds=(pc.FLOAT64,), trims=(False,), ctx="mixed")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_first_row_and_write_nothing(rj, scan, pool):
    import torch
    lib = rj.load_library()
    T = laid(pool[:700])
    n = len(T.data)

    def refused(why, T2, message):
        for kind in pc.KINDS:
            total, values, status, _ = parse_poisoned(rj, scan, T2, kind, True)
            msg = lib.rj_last_error().decode()
            assert total == RJ_BAD_ARGUMENT and message in msg, (why, total, msg)
            assert (values == POISON_U).all() and (status == POISON8).all(), why
        with pytest.raises(rj.RejitError) as err:
            scan.parse_records(T2.d, T2.rb_t, T2.re_t, indices=T2.idx_t)
        assert err.value.status == RJ_BAD_ARGUMENT and message in err.value.message
        check(rj, scan, T.take(range(0, 700, 9)), kinds=(pc.INT64,), trims=(True,))      # the same scan answers a good call

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
    f = lib.rj_scan_records_parse
    out = torch.full((708,), POISON, dtype=torch.int64, device="cuda:0")
    out8 = torch.full((708,), POISON8, dtype=torch.uint8, device="cuda:0")
    good = [scan._h, vp(T.d), n, vp(T.rb_t), vp(T.re_t), 700, None, 0, pc.INT64, 0, vp(out), vp(out8), None, st]
    assert f(*good) >= 0
    out.fill_(POISON), out8.fill_(POISON8)
    for at in (0, 1, 3, 4, 10):                                            # the scan, the text, either table, d_value
        args = list(good)
        args[at] = None
        assert f(*args) == RJ_BAD_ARGUMENT and lib.rj_last_error().decode() == "rj_scan_records_parse: null argument", at
    off = lambda x: ctypes.c_void_p(x.data_ptr() + 4)
    for at, x in ((3, T.rb_t), (4, T.re_t), (6, T.rb_t), (10, out)):
        args = list(good)
        args[at] = off(x)
        if at == 6:
            args[7] = 5
        assert f(*args) == RJ_BAD_ARGUMENT and lib.rj_last_error().decode() == "rj_scan_records_parse: a table is not 8-byte aligned", at
    for kind in (-1, 3, 7):
        args = list(good)
        args[8] = kind
        assert f(*args) == RJ_BAD_ARGUMENT and "kind" in lib.rj_last_error().decode(), kind
    for flags in (2, 3, 0x80000000):
        args = list(good)
        args[9] = flags
        assert f(*args) == RJ_BAD_ARGUMENT and "flag" in lib.rj_last_error().decode(), flags
    args = list(good)
    args[5] = 1 << 31
    assert f(*args) == RJ_TOO_LARGE and "2^31" in lib.rj_last_error().decode()
    args = list(good)
    args[6], args[7] = vp(T.rb_t), 1 << 31
    assert f(*args) == RJ_TOO_LARGE
    assert bool((out == POISON).all()) and bool((out8 == POISON8).all())
    # no rows: nothing is needed, nothing is touched
    assert f(scan._h, None, 0, None, None, 0, None, 0, pc.FLOAT64, 1, None, None, None, st) == 0
    args = list(good)
    args[6], args[7], args[10] = vp(T.rb_t), 0, None
    assert f(*args) == 0 and bool((out8 == POISON8).all())
    # a status byte table at any alignment is fine
    args = list(good)
    args[11] = ctypes.c_void_p(out8.data_ptr() + 1)
    assert f(*args) >= 0 and int(out8[0]) == POISON8 and int(out8[701]) == POISON8


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
    check(rj, s, laid(pool[:300]), kinds=(pc.INT64, pc.FLOAT64), trims=(True,), api=True)
    assert torch.equal(s.spans_tensor(d.device), spans0) and torch.equal(s.select_records(), sel0) and s.stats() == stats0
    # the matches of [0-9]+ themselves, as a record table over the scan's own span list
    spans = spans0.contiguous()
    mb, me = spans[:, 0].contiguous(), spans[:, 1].contiguous()
    values, status = s.parse_records(d, mb, me, kind="uint64")
    data = t.tobytes()
    want = [pc.meaning(data[b:e], pc.UINT64, False) for b, e in spans0.cpu().tolist()]
    assert status.cpu().tolist() == [w[0] for w in want] and (values.cpu().numpy().view(np.uint64) == np.array([w[1] for w in want], dtype=np.uint64)).all()
    assert torch.equal(s.spans_tensor(d.device), spans0) and s.run_records(d, rb_t, re_t).n_kept == res.n_kept


# ------------------------------------------------------------------------------------------------ group_sums
def test_group_sums_over_split_fields_equal_a_dict(rj):
    import torch
    from rejit_amd import records as R
    rng = random.Random(13)
    keys = [b"/p%d" % i for i in range(23)]
    spoilt = (b"", b"-", b"12abc", b"1.9", b"1e3", b"99999999999999999999", b"0x10")
    lines = []
    for i in range(2000):
        value = rng.choice(spoilt) if rng.randrange(7) == 0 else b"%d" % rng.randrange(-5000, 5000)
        if rng.randrange(11) == 0:
            value = b" " + value + b"\t"
        quarter = b"%d.%s" % (rng.randrange(-99, 99), rng.choice((b"0", b"25", b"5", b"75")))
        lines.append(rng.choice(keys) + b"," + value + b"," + quarter if rng.randrange(40) else rng.choice(keys))      # (some lines have one field)
    data = b"\n".join(lines)
    d = dev_text(data)
    s = rj.Scan(rj.Program(b","))
    rb_t, re_t = R.line_records(d)
    res = s.run_records(d, rb_t, re_t)
    pb, pe, pf = s.split_records(rb_t, re_t, res, len(data), what="between")
    kb, ke, _ = R.field_records(pb, pe, pf, 0)
    group, rep, count = s.group_records(d, kb, ke)
    n_groups = int(rep.numel())
    names = [lines[j].split(b",")[0] for j in rep.cpu().tolist()]
    assert n_groups == 23 and len(set(names)) == 23
    for field, kind, kind_name in ((1, pc.INT64, "int64"), (2, pc.FLOAT64, "float64")):
        vb, ve, _ = R.field_records(pb, pe, pf, field)
        values, status = s.parse_records(d, vb, ve, kind=kind_name, trim=True)
        ok = status == rj.PARSE_OK
        sums, counts = R.group_sums(group, values, ok, n_groups), R.group_counts_ok(group, ok, n_groups)
        want_sum, want_count = {k: 0 for k in names}, {k: 0 for k in names}
        for ln in lines:
            parts = ln.split(b",")
            st, bits = pc.meaning(parts[field] if len(parts) > field else b"", kind, True)
            if st == pc.OK:
                v = np.array([bits], dtype=np.uint64).view(np.int64 if kind == pc.INT64 else np.float64)[0]
                want_sum[parts[0]] += int(v) if kind == pc.INT64 else float(v)      # (sums of quarters are exact in any order)
                want_count[parts[0]] += 1
        assert sums.cpu().tolist() == [want_sum[k] for k in names], kind_name
        assert counts.cpu().tolist() == [want_count[k] for k in names] and 0 < sum(want_count.values()) < len(lines)


# ------------------------------------------------------------------------------------------------ the sample
SAMPLE_LINES = [b"/a 200 10", b"/b 500 7", b"/a 200 -3", b"/c 404", b"/b 200 12abc", b"/a 301  5", b"/b 200 1.9", b"/c 200 1e3", b"/a 200 +40",
                b"/d 200 99999999999999999999", b"/b 500 \t8", b"/d 200 0", b"/c 200 9223372036854775807"]


def _expected(lines, key_field, sum_field, byte_order=False, top=None):
    seen, count, total = [], {}, {}
    for ln in lines:
        parts = ln.split(b" ")
        key = parts[key_field - 1] if len(parts) >= key_field else b""
        if key not in count:
            seen.append(key)
            count[key], total[key] = 0, 0
        count[key] += 1
        st, bits = pc.meaning(parts[sum_field - 1] if len(parts) >= sum_field else b"", pc.INT64, True)
        if st == pc.OK:
            total[key] += bits - (1 << 64) if bits >> 63 else bits
    if byte_order:
        seen.sort()
    if top is not None:
        seen = sorted(seen, key=lambda k: -count[k])[:top]      # (stable: ties in the order so far)
    return b"".join(b"%7d %s %d\n" % (count[k], k, total[k]) for k in seen)


@pytest.mark.parametrize("opts,kw", [([], {}), (["-b"], {"byte_order": True}), (["-t", "2"], {"top": 2})], ids=["plain", "b", "t2"])
def test_linegrep_sample_sums_a_field_per_distinct_value_of_another(rj, tmp_path, opts, kw):
    """-f 1 -u -a 3: count, value of field 1, the int64 sum of field 3 over its lines; a missing, spoilt, fractional or too
    large field adds 0 (not awk's numeric prefix)."""
    path = str(tmp_path / "access.log")
    with open(path, "wb") as fh:
        fh.write(b"\n".join(SAMPLE_LINES) + b"\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    # (the separator is ONE space: "/a 301  5" has an empty third field and adds 0; " \t8" is cut at the space and adds 8)
    r = subprocess.run([sys.executable, sample, path, " ", "-f", "1", "-u", "-a", "3"] + opts, capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-500:])
    assert r.stdout == _expected(SAMPLE_LINES, 1, 3, **kw), r.stdout
    if not opts:
        assert r.stdout == (b"      4 /a 47\n      4 /b 15\n      3 /c 9223372036854775807\n      2 /d 0\n")


def test_linegrep_sample_refuses_a_without_f_and_u(rj, tmp_path):
    path = str(tmp_path / "x.log")
    with open(path, "wb") as fh:
        fh.write(b"a 1\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    for opts in (["-a", "2"], ["-f", "1", "-a", "2"], ["-o", "-u", "-a", "2"], ["-f", "1", "-u", "-a", "0"], ["-f", "1", "-u", "-a", "x"]):
        r = subprocess.run([sys.executable, sample, path, " "] + opts, capture_output=True, timeout=60)
        assert r.returncode == 2 and r.stdout == b"", opts
