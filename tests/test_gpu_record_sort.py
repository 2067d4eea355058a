"""GPU tests (-m gpu) of rj_scan_records_sort (rejit_amd/csrc/record_sort.hip; Scan.sort_records), of records.sorted_groups and
of samples/linegrep_gpu.py -b.

The meaning: with row j = text[rec_begin[r(j)], rec_end[r(j)]),
    order = sorted(range(k), key=lambda j: (row(j), j))
over the host copies of the rows' bytes (Python compares bytes as unsigned values, a proper prefix first); every comparison
is exact.  d_order is poisoned first and has guard words behind k: every row of [0, k) is written and nothing behind them.
RJ_SORT_SKIP and RJ_SORT_LONG_BYTES are the library's test knobs, read at every call."""
import collections
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_record_group import ADDRESS, address_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_TOO_LARGE, RJ_BAD_ARGUMENT = -2, -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
ROOM = 7
KS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1500)
LENGTHS = (0, 1, 6, 7, 8, 13, 14, 15, 21, 63, 64, 65, 70)
ALPHABETS = (bytes([0, 1]), b"ab", bytes([0, 0x80, 0xFF]) + b"a", bytes(range(256)))


STATS = ("rounds", "keyed_rows", "skip_rows", "long_rows")


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


def meaning(data, rb, re_, rows=None):
    rows = range(len(rb)) if rows is None else rows
    strings = [data[rb[r]:re_[r]] for r in rows]
    return sorted(range(len(strings)), key=lambda j: (strings[j], j))


def sort_poisoned(rj, scan, d, rb_t, re_t, indices=None, want_stats=True):
    """rj_scan_records_sort into a poisoned table -> (return value, order: the whole buffer as numpy, stats dict)"""
    import torch
    lib = rj.load_library()
    k = int(rb_t.numel()) if indices is None else int(indices.numel())
    order = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    keep = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = None if indices is None else (indices if k else keep)
    stats = rj.api._SortStats()
    total = lib.rj_scan_records_sort(scan._h, vp(d), int(d.numel()), vp(rb_t), vp(re_t), int(rb_t.numel()),
                                     ctypes.c_void_p(idx.data_ptr()) if idx is not None else None, k, vp(order),
                                     ctypes.byref(stats) if want_stats else None, st)
    return int(total), order.cpu().numpy(), {f: int(getattr(stats, f)) for f in STATS}


def check(rj, scan, data, d, rb, re_, rb_t=None, re_t=None, rows=None, api=True):
    """the raw call into a poisoned table against sorted(), and Scan.sort_records -> the stats"""
    rb_t = dev(rb) if rb_t is None else rb_t
    re_t = dev(re_) if re_t is None else re_t
    k = len(rb) if rows is None else len(rows)
    idx = None if rows is None else dev(rows)
    want = np.array(meaning(data, rb, re_, rows), dtype=np.int64)
    total, order, stats = sort_poisoned(rj, scan, d, rb_t, re_t, indices=idx)
    ctx = (len(rb), None if rows is None else len(rows), stats)
    assert total == k, (ctx, total, rj.load_library().rj_last_error())
    assert (order[:k] == want).all() and (order[k:] == POISON).all(), ctx
    assert stats["rounds"] == 0 if k < 2 else stats["rounds"] >= 1, ctx
    if api:
        a_order, a_stats = scan.sort_records(d, rb_t, re_t, indices=idx, stats=True)
        assert a_order.numel() == k and (a_order.cpu().numpy() == want).all() and a_stats == stats, ctx
        assert (scan.sort_records(d, rb_t, re_t, indices=idx).cpu().numpy() == want).all()
    return stats


def table(rng, k, alphabet, prefix=0, lengths=LENGTHS, lead=5):
    """k rows over `alphabet` behind a shared prefix; every third row repeats an earlier one, every fifth is a prefix of one;
    0..3 bytes between the rows, `lead` bytes in front, the last row ends at n -> (data, rec_begin, rec_end)"""
    alphabet = list(alphabet)
    shared = bytes(rng.choice(alphabet, prefix).tolist()) if prefix else b""
    rows = []
    for j in range(k):
        if rows and j % 3 == 2:
            s = rows[rng.randint(len(rows))]
        elif rows and j % 5 == 4:
            s = rows[rng.randint(len(rows))]
            s = s[:rng.randint(len(s) + 1)]
        else:
            ln = int(rng.choice(lengths))
            s = shared + (bytes(rng.choice(alphabet, ln).tolist()) if ln else b"")
        rows.append(s)
    return lay_out(rng, rows, lead)


def lay_out(rng, rows, lead=0, gaps=True):
    text, rb, re_ = bytearray(b"#" * lead), [], []
    for s in rows:
        text += b"|" * (int(rng.randint(4)) if gaps else 0)
        rb.append(len(text))
        text += s
        re_.append(len(text))
    return bytes(text), np.array(rb, dtype=np.int64), np.array(re_, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ shapes
def _run_shapes(rj, scan, ks, api):
    import torch
    n = 0
    for k in ks:
        if k == 0:
            empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
            d = dev_text(b"abc")
            total, order, stats = sort_poisoned(rj, scan, d, empty, empty)
            assert total == 0 and (order == POISON).all() and stats["rounds"] == 0
            assert scan.sort_records(d, empty, empty).numel() == 0
            continue
        for alphabet in ALPHABETS:
            for prefix in (0, 9, 40):
                n += 1
                rng = np.random.RandomState(1000 * k + n)
                data, rb, re_ = table(rng, k, alphabet, prefix)
                d = dev_text(data)
                rb_t, re_t = dev(rb), dev(re_)
                check(rj, scan, data, d, rb, re_, rb_t, re_t, api=api)
                check(rj, scan, data, d, rb, re_, rb_t, re_t, rows=rng.permutation(k).tolist(), api=False)
                check(rj, scan, data, d, rb, re_, rb_t, re_t, rows=rng.randint(0, k, k + 3).tolist(), api=api and k < 100)
            check(rj, scan, data, d, rb, re_, rb_t, re_t, rows=[], api=False)


@pytest.mark.parametrize("skip,long_bytes", [(None, None), ("0", None), (None, "1"), (None, "16")], ids=["default", "no skip", "L=1", "L=16"])
def test_shapes_equal_sorted(rj, scan, monkeypatch, skip, long_bytes):
    """k across the wave seams and the 256-row unit seams of the compaction, row lengths around the 7-byte window and the
    16-byte group, alphabets {0,1}, ab, {0,0x80,0xFF,a} and all 256 values, with and without a shared prefix of 9 or 40
    bytes; all rows, a permutation, a take with repeats, an empty take; through the C ABI and through Scan.sort_records."""
    if skip is not None:
        monkeypatch.setenv("RJ_SORT_SKIP", skip)
    if long_bytes is not None:
        monkeypatch.setenv("RJ_SORT_LONG_BYTES", long_bytes)
    _run_shapes(rj, scan, KS, api=skip is None and long_bytes is None)


def test_all_equal_all_distinct_sorted_and_reversed(rj, scan):
    rng = np.random.RandomState(4)
    for k in (2, 65, 300):
        rows = sorted({bytes(rng.choice(list(b"abc"), int(rng.choice(LENGTHS))).tolist()) for _ in range(k)})
        for ordered in (rows, rows[::-1], [rows[len(rows) // 2]] * k):
            data, rb, re_ = lay_out(rng, ordered, lead=3)
            check(rj, scan, data, dev_text(data), rb, re_)


def test_more_than_65536_segments_in_one_round(rj, scan):
    """Rows of 8 bytes drawn from 70000 seven-byte prefixes, two per prefix: the second round sorts by 17 bits of segment number."""
    rng = np.random.RandomState(6)
    prefixes = rng.choice(1 << 24, 70000, replace=False)
    heads = np.zeros((70000, 8), dtype=np.uint8)
    heads[:, 0:3] = np.frombuffer(b"rec", dtype=np.uint8)
    heads[:, 3], heads[:, 4], heads[:, 5], heads[:, 6] = prefixes >> 16, (prefixes >> 8) & 255, prefixes & 255, ord(":")
    rows = np.repeat(heads, 2, axis=0)
    rows[:, 7] = rng.randint(0, 256, len(rows))
    rows = rows[rng.permutation(len(rows))]
    k = len(rows)
    data = rows.tobytes()
    rb = np.arange(k, dtype=np.int64) * 8
    # the expectation by numpy: the rows as big-endian 64-bit numbers, a stable sort
    want = np.argsort(rows.view(">u8").reshape(-1), kind="stable")
    total, order, stats = sort_poisoned(rj, scan, dev_text(data), dev(rb), dev(rb + 8))
    assert total == k and (order[:k] == want).all() and (order[k:] == POISON).all()
    assert stats["rounds"] == 2 and stats["keyed_rows"] == 2 * k and stats["skip_rows"] == k, stats


# ------------------------------------------------------------------------------------------------ the skip
def _skip_tables(ln, rng):
    base = bytes(rng.randint(ord("a"), ord("z") + 1, ln).astype(np.uint8).tolist())
    last = [base[:-1] + bytes([c]) for c in (0, 0x7F, 0x80, 0xFF, base[-1])]
    prefixes = [base[:n] for n in sorted({0, 1, 7, 8, ln // 2, ln - 1, ln})]
    return {"equal": [base] * 9, "last byte": [last[i % 5] for i in range(23)], "prefixes": [prefixes[(3 * i) % len(prefixes)] for i in range(20)]}


@pytest.mark.parametrize("long_bytes", ["1", "16"])
@pytest.mark.parametrize("ln", [70, 3000])
def test_both_tiers_of_the_skip_on_small_texts(rj, scan, monkeypatch, long_bytes, ln):
    """RJ_SORT_LONG_BYTES in {1, 16} sends rows that agree with their segment's head on more than that to the wave tier: rows
    of 70 bytes (one wave iteration) and of 3000 (three) that share all their bytes, differ only in the last byte, or are a
    prefix of one another.  Without the skip the order is the same, and an all-equal table takes max_len // 7 + 1 rounds --
    at most 2 with it."""
    monkeypatch.setenv("RJ_SORT_LONG_BYTES", long_bytes)
    rng = np.random.RandomState(ln)
    for name, rows in _skip_tables(ln, rng).items():
        data, rb, re_ = lay_out(rng, rows, lead=int(rng.randint(16)))
        d = dev_text(data)
        monkeypatch.delenv("RJ_SORT_SKIP", raising=False)
        stats = check(rj, scan, data, d, rb, re_, api=False)
        assert stats["skip_rows"] > 0 and stats["long_rows"] > 0, (name, stats)
        if name == "equal":
            assert stats["rounds"] <= 2, stats
        monkeypatch.setenv("RJ_SORT_SKIP", "0")
        plain = check(rj, scan, data, d, rb, re_, api=False)
        assert plain["skip_rows"] == 0 and plain["long_rows"] == 0, (name, plain)
        if name == "equal":
            assert plain["rounds"] == ln // 7 + 1, plain
        assert plain["rounds"] >= stats["rounds"]


# ------------------------------------------------------------------------------------------------ indices
def test_a_rows_identity_is_j_not_the_record(rj, scan):
    data = b"xx|yy|xx|zz"
    d = dev_text(data)
    rb, re_ = np.array([0, 3, 6, 9]), np.array([2, 5, 8, 11])
    # the same record named three times comes out in ascending j, between the rows its bytes belong between
    order = scan.sort_records(d, dev(rb), dev(re_), indices=dev([3, 1, 2, 1, 0, 1]))
    assert order.cpu().tolist() == [2, 4, 1, 3, 5, 0]
    order = scan.sort_records(d, dev(rb), dev(re_), indices=dev([3, 2, 1, 0]))
    assert order.cpu().tolist() == [1, 3, 2, 0]
    rng = np.random.RandomState(3)
    data, rb, re_ = table(rng, 600, b"ab", 9)
    check(rj, scan, data, dev_text(data), rb, re_, rows=list(range(599, -1, -1)))


# ------------------------------------------------------------------------------------------------ skew
def test_one_row_of_4_mib_twice_among_100000_short_ones(rj, scan):
    """P3 on the device: the two long rows share 4 MiB; the prefix skip takes them to their end in one round."""
    big = 4 << 20
    rng = np.random.RandomState(31)
    body = rng.randint(ord("f"), ord("z") + 1, big).astype(np.uint8)
    small = rng.randint(ord("a"), ord("e") + 1, 700000).astype(np.uint8)
    t = np.concatenate([np.frombuffer(b"abc", dtype=np.uint8), body, small, body])
    o_small = 3 + big
    lens = rng.randint(0, 13, 100000)
    rb = np.empty(100002, dtype=np.int64)
    rb[:100000] = o_small + rng.randint(0, len(small) - 12, 100000)
    re_ = rb.copy()
    re_[:100000] += lens
    rb[100000:], re_[100000:] = [3, o_small + len(small)], [3 + big, len(t)]
    at = np.concatenate([np.arange(0, 40000), [100001], np.arange(40000, 100000), [100000]])
    rb, re_ = rb[at], re_[at]
    data = t.tobytes()
    want = np.array(meaning(data, rb.tolist(), re_.tolist()), dtype=np.int64)
    assert want[-2:].tolist() == [40000, 100001]
    total, order, stats = sort_poisoned(rj, scan, dev_text(data), dev(rb), dev(re_))
    assert total == 100002 and (order[:100002] == want).all() and (order[100002:] == POISON).all()
    assert stats["rounds"] <= 3 and stats["long_rows"] >= 1, stats


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_the_scans_state_stays(rj):
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    lib = rj.load_library()
    t = W.log_like_numpy(1 << 16, 3)
    n = len(t)
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    scan = rj.Scan(rj.Program(b"[0-9]+"))
    rb_t, re_t = R.line_records(d)
    rb, re_ = rb_t.cpu().numpy(), re_t.cpu().numpy()
    k = len(rb)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matching > 20 and k > 100
    sel0 = scan.select_records().clone()
    spans0 = scan.spans_tensor(d.device).clone()
    stats0 = scan.stats()

    def refused(why, row, b_t=rb_t, e_t=re_t, idx=None):
        total, order, _ = sort_poisoned(rj, scan, d, b_t, e_t, indices=idx)
        msg = lib.rj_last_error().decode()
        assert total == RJ_BAD_ARGUMENT, (why, total)
        assert ("row %d " % row) in msg, (why, msg)
        assert (order == POISON).all(), why
        with pytest.raises(rj.RejitError) as err:
            scan.sort_records(d, b_t, e_t, indices=idx)
        assert err.value.status == RJ_BAD_ARGUMENT and ("row %d " % row) in err.value.message
        check(rj, scan, data, d, rb, re_, rb_t, re_t, rows=list(range(0, k, 3)), api=False)      # the same scan answers a good call

    take = list(range(0, k, 2))
    for at in (0, len(take) // 2, len(take) - 1):
        bad = list(take)
        bad[at] = k
        refused("an index == n_records at row %d" % at, at, idx=dev(bad))
    bad = list(take)
    bad[7], bad[len(take) - 2] = -1, k + 5
    refused("two bad rows: the smaller is named", 7, idx=dev(bad))
    e = re_.copy()
    e[k - 1] = n + 1
    refused("end > n", k - 1, e_t=dev(e))
    e = re_.copy()
    e[k // 2] = int(rb[k // 2]) - 1
    refused("begin > end", k // 2, e_t=dev(e))
    refused("one bad row alone (no round runs)", 0, idx=dev([k]))
    # arguments
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    f = lib.rj_scan_records_sort
    out = torch.full((k + 8,), POISON, dtype=torch.int64, device="cuda:0")
    assert f(None, vp(d), n, vp(rb_t), vp(re_t), k, None, 0, vp(out), None, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, None, n, vp(rb_t), vp(re_t), k, None, 0, vp(out), None, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, None, vp(re_t), k, None, 0, vp(out), None, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, vp(rb_t), None, k, None, 0, vp(out), None, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    assert "null" in lib.rj_last_error().decode()
    off = lambda x: ctypes.c_void_p(x.data_ptr() + 4)
    for b, e_, i, o_ in ((off(rb_t), vp(re_t), None, vp(out)), (vp(rb_t), off(re_t), None, vp(out)), (vp(rb_t), vp(re_t), off(rb_t), vp(out)),
                         (vp(rb_t), vp(re_t), None, off(out))):
        assert f(scan._h, vp(d), n, b, e_, k - 1, i, k - 1 if i else 0, o_, None, st) == RJ_BAD_ARGUMENT
        assert "aligned" in lib.rj_last_error().decode()
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, vp(rb_t), 1 << 31, vp(out), None, st) == RJ_TOO_LARGE
    assert "2^31" in lib.rj_last_error().decode()
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), 1 << 31, None, 0, vp(out), None, st) == RJ_TOO_LARGE
    assert f(scan._h, None, 0, None, None, 0, None, 0, None, None, st) == 0
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, vp(rb_t), 0, vp(out), None, st) == 0          # no rows
    assert bool((out == POISON).all())
    # the scan's state stays: its list, its stats and its last join are what they were
    assert torch.equal(scan.spans_tensor(d.device), spans0) and torch.equal(scan.select_records(), sel0) and scan.stats() == stats0
    assert scan.run_records(d, rb_t, re_t).n_kept == res.n_kept


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def log_file(tmp_path_factory):
    data, lines = address_log()
    path = str(tmp_path_factory.mktemp("sort") / "access.log")
    with open(path, "wb") as fh:
        fh.write(data)
    want = collections.Counter()
    for ln in lines:
        want.update(re.findall(ADDRESS, ln))
    assert len(lines) == 20000 and len(want) == 300
    return path, data, lines, want


def _uniq_c(pairs):
    return b"".join(b"%7d %s\n" % (c, w) for w, c in pairs)


def test_sorted_groups_of_a_logs_addresses(rj, log_file):
    """run_records -> split_records(what="matches") -> records.sorted_groups equals sorted(collections.Counter(...).items()),
    and group_sorted maps every row to its string's rank."""
    import torch
    from rejit_amd import records as R
    _, data, _, want = log_file
    d = dev_text(data)
    rb_t, re_t = R.line_records(d)
    s = rj.Scan(rj.Program(ADDRESS))
    res = s.run_records(d, rb_t, re_t)
    pb, pe, _ = s.split_records(rb_t, re_t, res, len(data), what="matches")
    rep, count, group = R.sorted_groups(s, d, pb, pe)
    packed, _, _ = s.pack_records(d, pb, pe, indices=rep, fill=10, lead=0, gap=1)
    words = packed.cpu().numpy().tobytes().split(b"\n")[:-1]
    assert list(zip(words, count.cpu().tolist())) == sorted(want.items())
    rank = {w: i for i, w in enumerate(sorted(want))}
    pieces = [data[b:e] for b, e in zip(pb.cpu().tolist(), pe.cpu().tolist())]
    assert group.cpu().tolist() == [rank[p] for p in pieces]
    # ... with indices: every second match, in reverse
    idx = torch.arange(pb.numel() - 1, -1, -2, dtype=torch.int64, device="cuda:0")
    rep, count, group = R.sorted_groups(s, d, pb, pe, indices=idx)
    taken = [pieces[i] for i in idx.cpu().tolist()]
    sub = collections.Counter(taken)
    packed, _, _ = s.pack_records(d, pb, pe, indices=idx[rep], fill=10, lead=0, gap=1)
    assert list(zip(packed.cpu().numpy().tobytes().split(b"\n")[:-1], count.cpu().tolist())) == sorted(sub.items())
    rank = {w: i for i, w in enumerate(sorted(sub))}
    assert group.cpu().tolist() == [rank[p] for p in taken]


@pytest.mark.parametrize("opts", [["-o", "-u", "-b"], ["-o", "-u"], ["-p", "-b"], ["-o", "-b"]], ids=["-o -u -b", "-o -u", "-p -b", "-o -b"])
def test_linegrep_sample_prints_in_byte_order(rj, log_file, opts):
    path, _, lines, want = log_file
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    r = subprocess.run([sys.executable, sample, path, ADDRESS.decode()] + opts, capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-500:])
    if opts == ["-o", "-u", "-b"]:
        expect = _uniq_c(sorted(want.items()))                                  # ... | sort | uniq -c
    elif opts == ["-o", "-u"]:
        expect = _uniq_c(want.items())                                          # without -b: what it prints today
    elif opts == ["-p", "-b"]:
        expect = b"".join(ln + b"\n" for ln in sorted(ln for ln in lines if re.search(ADDRESS, ln)))
    else:
        expect = b"".join(w + b"\n" for w in sorted(w for ln in lines for w in re.findall(ADDRESS, ln)))
    assert r.stdout == expect


def test_linegrep_sample_refuses_b_alone(rj, log_file):
    path = log_file[0]
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    r = subprocess.run([sys.executable, sample, path, ADDRESS.decode(), "-c", "-b"], capture_output=True, timeout=60)
    assert r.returncode == 2 and r.stdout == b""


# ------------------------------------------------------------------------------------------------ determinism, sequence
def test_five_calls_on_one_scan_give_identical_orders(rj, scan):
    import torch
    rng = np.random.RandomState(1500)
    data, rb, re_ = table(rng, 1500, b"ab", 9)
    d = dev_text(data)
    rb_t, re_t = dev(rb), dev(re_)
    first = scan.sort_records(d, rb_t, re_t)
    assert first.cpu().tolist() == meaning(data, rb, re_)
    for _ in range(4):
        assert torch.equal(first, scan.sort_records(d, rb_t, re_t))


def test_a_sort_between_a_run_and_its_select_and_replace(rj):
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    t = W.log_like_numpy(1 << 16, 9)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = R.line_records(d)
    plain, mixed = rj.Scan(rj.Program(b"[0-9]+")), rj.Scan(rj.Program(b"[0-9]+"))
    res_p, res_m = plain.run_records(d, rb_t, re_t), mixed.run_records(d, rb_t, re_t)
    stats0 = mixed.stats()
    order = mixed.sort_records(d, rb_t, re_t)
    assert sorted(order.cpu().tolist()) == list(range(rb_t.numel()))
    sel_p, sel_m = plain.select_records(), mixed.select_records()
    assert torch.equal(sel_p, sel_m) and sel_p.numel() == res_p.n_matching == res_m.n_matching
    mixed.sort_records(d, rb_t, re_t, indices=sel_m)
    out_p = plain.replace_records(d, rb_t, re_t, res_p, b"<N>", indices=sel_p, fill=10, lead=0, gap=1)
    out_m = mixed.replace_records(d, rb_t, re_t, res_m, b"<N>", indices=sel_m, fill=10, lead=0, gap=1)
    assert all(torch.equal(a, b) for a, b in zip(out_p, out_m)) and out_p[0].numel() > 1000
    assert torch.equal(plain.spans_tensor(d.device), mixed.spans_tensor(d.device)) and mixed.stats() == stats0
