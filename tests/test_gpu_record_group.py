"""GPU tests (-m gpu) of rj_scan_records_group (rejit_amd/csrc/record_group.hip; Scan.group_records), of records.top_groups and
of samples/linegrep_gpu.py -u / -t.

The meaning: with row j = text[rec_begin[r(j)], rec_end[r(j)]) and the distinct strings numbered in order of first appearance,
    group[j] = the number of row j's string, rep[g] = the smallest j with string g, count[g] = the number of its rows.
The expected answer is a Python dict over the host copies of the rows' bytes, in insertion order; every comparison is exact.
Outputs are poisoned first: every row of [0, G) and [0, k) is written and nothing behind them.  RJ_GROUP_HASH_BITS and
RJ_GROUP_LONG_BYTES are the library's test knobs, read at every call."""
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
KS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 1500)
LENS = (0, 1, 15, 16, 17, 40, 700)
LONG_LENS = (33, 1023, 1024, 1025, 2047, 2048, 2049, 5000)


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


def meaning(data, rb, re_, rows):
    """the dict, in insertion order -> (group, rep, count) as int64 arrays"""
    seen, group, rep, count = {}, [], [], []
    for j, r in enumerate(rows):
        s = data[rb[r]:re_[r]]
        g = seen.get(s)
        if g is None:
            g = seen[s] = len(rep)
            rep.append(j)
            count.append(0)
        group.append(g)
        count[g] += 1
    as64 = lambda x: np.array(x, dtype=np.int64)
    return as64(group), as64(rep), as64(count)


def group_poisoned(rj, scan, d, rb_t, re_t, indices=None, cap=0, room_for=0, want_group=True, tables=True):
    """rj_scan_records_group into poisoned tables -> (G, group, rep, count): the whole buffers as numpy"""
    import torch
    lib = rj.load_library()
    k = int(rb_t.numel()) if indices is None else int(indices.numel())
    g = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    rep = torch.full((max(cap, room_for) + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    cnt = torch.full((max(cap, room_for) + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    keep = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = None if indices is None else (indices if k else keep)
    total = lib.rj_scan_records_group(scan._h, vp(d), int(d.numel()), vp(rb_t), vp(re_t), int(rb_t.numel()),
                                      ctypes.c_void_p(idx.data_ptr()) if idx is not None else None, k, vp(g) if want_group else None,
                                      vp(rep) if tables and cap else None, vp(cnt) if tables and cap else None, cap if tables else 0, st)
    return int(total), g.cpu().numpy(), rep.cpu().numpy(), cnt.cpu().numpy()


def check(rj, scan, data, d, rb, re_, rb_t=None, re_t=None, rows=None, api=True):
    """the raw call into poisoned tables against the dict, and Scan.group_records (one size query, exact tables)"""
    rb_t = dev(rb) if rb_t is None else rb_t
    re_t = dev(re_) if re_t is None else re_t
    k = len(rb) if rows is None else len(rows)
    idx = None if rows is None else dev(rows)
    w_group, w_rep, w_count = meaning(data, rb, re_, range(len(rb)) if rows is None else rows)
    G = len(w_rep)
    total, g, rep, cnt = group_poisoned(rj, scan, d, rb_t, re_t, indices=idx, cap=G, room_for=G)
    ctx = (len(rb), None if rows is None else len(rows), G)
    assert total == G, (ctx, total, rj.load_library().rj_last_error())
    assert (g[:k] == w_group).all() and (g[k:] == POISON).all(), ctx
    assert (rep[:G] == w_rep).all() and (rep[G:] == POISON).all(), ctx
    assert (cnt[:G] == w_count).all() and (cnt[G:] == POISON).all(), ctx
    if api:
        a_g, a_rep, a_cnt = scan.group_records(d, rb_t, re_t, indices=idx)
        assert a_g.numel() == k and a_rep.numel() == G == a_cnt.numel()
        assert (a_g.cpu().numpy() == w_group).all() and (a_rep.cpu().numpy() == w_rep).all() and (a_cnt.cpu().numpy() == w_count).all(), ctx
    return w_group, w_rep, w_count


# ------------------------------------------------------------------------------------------------ shapes
def _pool(d, rng, lens):
    """d distinct strings of lower-case letters with lengths from `lens`: among them strings that share everything but their
    last byte (so a 16-byte prefix and more) and strings that are prefixes of one another"""
    pool, seen, tries = [], set(), 0
    while len(pool) < d:
        kind = tries % 4
        tries += 1
        if kind == 1 and pool and len(pool[-1]) > 0:
            s = pool[-1][:-1] + bytes([ord("a") + (pool[-1][-1] - ord("a") + 1) % 26])
        elif kind == 2 and pool and len(pool[-1]) > 1:
            s = pool[-1][:int(rng.choice([n for n in sorted(set(lens) | {1}) if n < len(pool[-1])]))]
        else:
            s = rng.randint(ord("a"), ord("z") + 1, int(rng.choice(lens))).astype(np.uint8).tobytes()
        if s not in seen:
            seen.add(s)
            pool.append(s)
    return pool


def _table(k, d, rng, lens=LENS, lead=5):
    """k rows drawn from a pool of d strings, 0..3 bytes of text between them; with d >= 3 and k > 257 two strings appear
    only at rows 255 and 256, either side of the numbering scan's first unit seam, and with d >= 2 one only at the last row
    -> (text as uint8 array, rec_begin, rec_end)"""
    pool = _pool(d, rng, lens)
    picks = rng.permutation(d) if d == k else rng.randint(0, d, k)
    if d != k and d >= 3 and k > 257:
        picks = rng.randint(0, d - 2, k)
        picks[255], picks[256] = d - 2, d - 1
    elif d != k and d >= 2 and k >= 2:
        picks = rng.randint(0, d - 1, k)
        picks[k - 1] = d - 1
    parts, rb, re_ = [bytes([ord("a") + i % 26 for i in range(lead)])], [], []
    at = lead
    for p in picks.tolist():
        seam = int(rng.randint(0, 4))
        parts.append(b"z" * seam)
        at += seam
        rb.append(at)
        parts.append(pool[p])
        at += len(pool[p])
        re_.append(at)
    parts.append(b"tail")
    t = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return t, np.array(rb, dtype=np.int64), np.array(re_, dtype=np.int64)


def _ds(k, most=None):
    return sorted({d for d in (1, 2, 7, k // 2, k) if 1 <= d <= k and (most is None or d <= most)})


def _run_shapes(rj, scan, ks, most_d=None):
    import torch
    for k in ks:
        if k == 0:
            empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
            d = torch.from_numpy(np.frombuffer(b"abc", dtype=np.uint8).copy()).to("cuda:0")
            total, g, rep, cnt = group_poisoned(rj, scan, d, empty, empty, cap=3)
            assert total == 0 and (g == POISON).all() and (rep == POISON).all() and (cnt == POISON).all()
            a_g, a_rep, a_cnt = scan.group_records(d, empty, empty)
            assert a_g.numel() == 0 and a_rep.numel() == 0 and a_cnt.numel() == 0
            continue
        for dd in _ds(k, most_d):
            rng = np.random.RandomState(1000 * k + dd)
            t, rb, re_ = _table(k, dd, rng)
            data = t.tobytes()
            d = torch.from_numpy(t).to("cuda:0")
            rb_t, re_t = dev(rb), dev(re_)
            _, w_rep, _ = check(rj, scan, data, d, rb, re_, rb_t, re_t)
            assert len(w_rep) == dd if dd in (1, 2, k) else 2 < len(w_rep) <= dd
            check(rj, scan, data, d, rb, re_, rb_t, re_t, rows=rng.permutation(k).tolist(), api=False)
            check(rj, scan, data, d, rb, re_, rb_t, re_t, rows=rng.randint(0, k, k + 3).tolist(), api=False)
            check(rj, scan, data, d, rb, re_, rb_t, re_t, rows=[], api=dd == 1)


@pytest.mark.parametrize("ks", [KS[:7], KS[7:10], KS[10:]], ids=["k<=255", "k=256..513", "k=1500"])
def test_shapes_equal_the_dict(rj, scan, ks):
    """k across the wave seams and the 256-row unit seams of the numbering scan, row lengths 0, 1, 15, 16, 17, 40, 700 (the
    last in the wave tier), pools of 1, 2, 7, k/2 and k distinct strings; all rows, a permutation, a take with repeats, an
    empty take."""
    _run_shapes(rj, scan, ks)


@pytest.mark.parametrize("bits", [0, 2])
def test_forced_collisions_leave_everything_to_the_byte_compare_and_the_probing(rj, scan, monkeypatch, bits):
    """RJ_GROUP_HASH_BITS: with 2 bits the strings share four probe chains, with 0 every row walks ONE chain (d <= 40 there)."""
    monkeypatch.setenv("RJ_GROUP_HASH_BITS", str(bits))
    _run_shapes(rj, scan, [k for k in KS if 0 < k <= 600], most_d=40 if bits == 0 else None)


# ------------------------------------------------------------------------------------------------ the wave tier
def test_the_wave_tier_on_small_texts(rj, scan, monkeypatch):
    """RJ_GROUP_LONG_BYTES=32 sends rows of 33 bytes and more to the wave kernels: lengths around one and two wave iterations
    (1 KiB each), pools drawn from them; long rows that differ only in their last byte, in the byte at 1024 or in the first
    byte; a long row at the text's very begin and one at its very end (the guarded loads); every misalignment of the begin."""
    import torch
    monkeypatch.setenv("RJ_GROUP_LONG_BYTES", "32")
    for k, dd in ((9, 3), (64, 8), (257, 40)):
        rng = np.random.RandomState(k)
        t, rb, re_ = _table(k, dd, rng, lens=LONG_LENS + (0, 16, 32))
        check(rj, scan, t.tobytes(), torch.from_numpy(t).to("cuda:0"), rb, re_)
    rng = np.random.RandomState(77)
    for ln in LONG_LENS:
        base = rng.randint(ord("a"), ord("z") + 1, ln).astype(np.uint8)
        variants = [base.copy() for _ in range(5)]
        variants[1][-1] ^= 1                         # the last byte
        variants[2][0] ^= 1                          # the first byte
        variants[3][min(1024, ln - 1)] ^= 2          # the byte at 1024 (the second iteration's first), or the last
        variants[3][ln // 3] ^= 4
        rows = [variants[i] for i in (0, 1, 0, 2, 3, 4, 1, 3)]
        for mis in range(16):
            # the first row begins at 0 when mis == 0 and the last row ends at n; `mis` bytes in front shift every begin
            parts, rb, re_, at = [b"q" * mis], [], [], mis
            for i, r in enumerate(rows):
                rb.append(at)
                at += ln
                re_.append(at)
                parts.append(r.tobytes())
                if i + 1 < len(rows):
                    parts.append(b"q" * (i % 3))
                    at += i % 3
            data = b"".join(parts)
            assert re_[-1] == len(data)
            d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
            assert d.data_ptr() % 16 == 0
            w_group, w_rep, w_count = check(rj, scan, data, d, np.array(rb), np.array(re_), api=mis == 0)
            assert w_group.tolist() == [0, 1, 0, 2, 3, 0, 1, 3] and w_count.tolist() == [3, 2, 1, 2], (ln, mis)


# ------------------------------------------------------------------------------------------------ indices
def test_a_rows_identity_is_j_not_the_record(rj, scan):
    import torch
    data = b"xx|yy|xx|zz"
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    rb, re_ = np.array([0, 3, 6, 9]), np.array([2, 5, 8, 11])
    # the representative is the smallest j, not the smallest r(j): rows 0 and 2 name records 2 and 0
    g, rep, cnt = scan.group_records(d, dev(rb), dev(re_), indices=dev([2, 1, 0, 2, 3]))
    assert g.cpu().tolist() == [0, 1, 0, 0, 2] and rep.cpu().tolist() == [0, 1, 4] and cnt.cpu().tolist() == [3, 1, 1]
    # a reversed permutation: the numbering follows the rows, not the records
    g, rep, cnt = scan.group_records(d, dev(rb), dev(re_), indices=dev([3, 2, 1, 0]))
    assert g.cpu().tolist() == [0, 1, 2, 1] and rep.cpu().tolist() == [0, 1, 2] and cnt.cpu().tolist() == [1, 2, 1]
    rng = np.random.RandomState(3)
    t, rb, re_ = _table(600, 9, rng)
    check(rj, scan, t.tobytes(), torch.from_numpy(t).to("cuda:0"), rb, re_, rows=list(range(599, -1, -1)))


# ------------------------------------------------------------------------------------------------ caps
def test_the_size_query_caps_and_missing_tables(rj, scan):
    import torch
    rng = np.random.RandomState(21)
    t, rb, re_ = _table(700, 37, rng)
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    w_group, w_rep, w_count = meaning(data, rb, re_, range(700))
    G = len(w_rep)
    assert G == 37
    # the size query: no rep / count row; d_group is still written -- and not asked for
    total, g, rep, cnt = group_poisoned(rj, scan, d, rb_t, re_t, cap=0, room_for=G)
    assert total == G and (g[:700] == w_group).all() and (g[700:] == POISON).all() and (rep == POISON).all() and (cnt == POISON).all()
    total, g, rep, cnt = group_poisoned(rj, scan, d, rb_t, re_t, cap=0, room_for=G, want_group=False)
    assert total == G and (g == POISON).all() and (rep == POISON).all() and (cnt == POISON).all()
    for cap in (1, G - 1, G, G + 5):
        for want_group in (True, False):
            total, g, rep, cnt = group_poisoned(rj, scan, d, rb_t, re_t, cap=cap, room_for=G + 5, want_group=want_group)
            lim = min(cap, G)
            assert total == G, cap
            assert (rep[:lim] == w_rep[:lim]).all() and (cnt[:lim] == w_count[:lim]).all(), cap
            assert (rep[lim:] == POISON).all() and (cnt[lim:] == POISON).all(), cap
            assert ((g[:700] == w_group).all() if want_group else (g == POISON).all()) and (g[700:] == POISON).all()


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
        total, g, rep, cnt = group_poisoned(rj, scan, d, b_t, e_t, indices=idx, cap=k)
        msg = lib.rj_last_error().decode()
        assert total == RJ_BAD_ARGUMENT, (why, total)
        assert ("row %d " % row) in msg, (why, msg)
        assert (g == POISON).all() and (rep == POISON).all() and (cnt == POISON).all(), why
        with pytest.raises(rj.RejitError) as err:
            scan.group_records(d, b_t, e_t, indices=idx)
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
    # arguments
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    f = lib.rj_scan_records_group
    out = torch.full((k + 8,), POISON, dtype=torch.int64, device="cuda:0")
    out2, out3 = out.clone(), out.clone()
    assert f(None, vp(d), n, vp(rb_t), vp(re_t), k, None, 0, None, None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, None, n, vp(rb_t), vp(re_t), k, None, 0, vp(out), None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, None, vp(re_t), k, None, 0, vp(out), None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, vp(rb_t), None, k, None, 0, vp(out), None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, None, 0, vp(out), None, vp(out3), 5, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, None, 0, vp(out), vp(out2), None, 5, st) == RJ_BAD_ARGUMENT
    assert "null" in lib.rj_last_error().decode()
    off = lambda x: ctypes.c_void_p(x.data_ptr() + 4)
    for args in ((off(rb_t), vp(re_t), None, vp(out), vp(out2), vp(out3)), (vp(rb_t), off(re_t), None, vp(out), vp(out2), vp(out3)),
                 (vp(rb_t), vp(re_t), off(rb_t), vp(out), vp(out2), vp(out3)), (vp(rb_t), vp(re_t), None, off(out), vp(out2), vp(out3)),
                 (vp(rb_t), vp(re_t), None, vp(out), off(out2), vp(out3)), (vp(rb_t), vp(re_t), None, vp(out), vp(out2), off(out3))):
        b, e_, i, g_, r_, c_ = args
        assert f(scan._h, vp(d), n, b, e_, k - 1, i, k - 1 if i else 0, g_, r_, c_, k, st) == RJ_BAD_ARGUMENT
        assert "aligned" in lib.rj_last_error().decode()
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, vp(rb_t), 1 << 31, vp(out), None, None, 0, st) == RJ_TOO_LARGE
    assert "2^31" in lib.rj_last_error().decode()
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), 1 << 31, None, 0, vp(out), None, None, 0, st) == RJ_TOO_LARGE
    assert f(scan._h, None, 0, None, None, 0, None, 0, None, None, None, 0, st) == 0
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, vp(rb_t), 0, vp(out), vp(out2), vp(out3), 5, st) == 0          # no rows
    assert bool((out == POISON).all()) and bool((out2 == POISON).all()) and bool((out3 == POISON).all())
    # the scan's state stays: its list, its stats and its last join are what they were
    assert torch.equal(scan.spans_tensor(d.device), spans0) and torch.equal(scan.select_records(), sel0) and scan.stats() == stats0
    assert scan.run_records(d, rb_t, re_t).n_kept == res.n_kept


# ------------------------------------------------------------------------------------------------ skew
def test_one_row_of_4_mib_among_100000_tiny_ones(rj, scan):
    """Correctness only: one row of 4 MiB, two equal to it, one that differs in its last byte, among 100 000 empty and one-byte
    rows.  The expectation is written out with numpy (the dict over 4-MiB keys says the same, slowly)."""
    import torch
    big = 4 << 20
    rng = np.random.RandomState(31)
    body = rng.randint(ord("a"), ord("z") + 1, big).astype(np.uint8)
    other = body.copy()
    other[-1] = ord("A")
    small = rng.randint(ord("a"), ord("e") + 1, 50000).astype(np.uint8)
    # layout: 3 | body | body | small bytes | other | body(again, via a repeated record)
    t = np.concatenate([np.frombuffer(b"abc", dtype=np.uint8), body, body, small, other])
    o_small = 3 + 2 * big
    o_other = o_small + len(small)
    n = len(t)
    assert n == o_other + big
    rb = np.empty(100004, dtype=np.int64)
    re_ = np.empty(100004, dtype=np.int64)
    kind = np.empty(100004, dtype=np.int64)          # the row's string as a number: 0..4 a one-byte row's letter, 5 empty, 6 body, 7 other
    at = np.arange(50000)
    rb[0:100000:2], re_[0:100000:2], kind[0:100000:2] = o_small + at, o_small + at + 1, small - ord("a")
    rb[1:100000:2], re_[1:100000:2], kind[1:100000:2] = o_small + at, o_small + at, 5
    # the long rows sit in the middle and at the end of the table
    rb[100000:], re_[100000:], kind[100000:] = [3, 3 + big, o_other, 3], [3 + big, 3 + 2 * big, n, 3 + big], [6, 6, 7, 6]
    order = np.concatenate([np.arange(0, 40000), [100000, 100002], np.arange(40000, 100000), [100001, 100003]])
    rb, re_, kind = rb[order], re_[order], kind[order]
    _, first = np.unique(kind, return_index=True)
    w_rep = np.sort(first)
    number = {int(kind[j]): g for g, j in enumerate(w_rep.tolist())}
    w_group = np.array([number[int(x)] for x in kind.tolist()], dtype=np.int64)
    w_count = np.bincount(w_group)
    d = torch.from_numpy(t).to("cuda:0")
    g, rep, cnt = scan.group_records(d, dev(rb), dev(re_))
    assert (rep.cpu().numpy() == w_rep).all() and (cnt.cpu().numpy() == w_count).all() and (g.cpu().numpy() == w_group).all()
    assert len(w_rep) == 8 and int(w_count[number[6]]) == 3 and int(w_count[number[7]]) == 1


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def log_file(tmp_path_factory):
    data, lines = address_log()
    path = str(tmp_path_factory.mktemp("group") / "access.log")
    with open(path, "wb") as fh:
        fh.write(data)
    want = collections.Counter()
    for ln in lines:
        want.update(re.findall(ADDRESS, ln))
    assert len(lines) == 20000 and len(want) == 300
    return path, data, want


def _uniq_c(pairs):
    return b"".join(b"%7d %s\n" % (c, w) for w, c in pairs)


def test_top_client_addresses_of_a_log(rj, log_file):
    """run_records -> split_records(what="matches") -> group_records -> top_groups equals collections.Counter over re.findall
    per line (test_record_group.py asserts on the CPU that `re` and the oracle agree on this pattern and this log)."""
    import torch
    from rejit_amd import records as R
    _, data, want = log_file
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    rb_t, re_t = R.line_records(d)
    s = rj.Scan(rj.Program(ADDRESS))
    res = s.run_records(d, rb_t, re_t)
    assert res.n_crossing == 0 and res.n_kept == sum(want.values())
    pb, pe, _ = s.split_records(rb_t, re_t, res, len(data), what="matches")
    group, rep, count = s.group_records(d, pb, pe)
    assert rep.numel() == 300 and int(count.sum()) == pb.numel() == group.numel()
    # the dictionary, in order of first appearance: the Counter's insertion order
    packed, _, _ = s.pack_records(d, pb, pe, indices=rep, fill=10, lead=0, gap=1)
    words = packed.cpu().numpy().tobytes().split(b"\n")[:-1]
    assert words == list(want.keys()) and count.cpu().tolist() == list(want.values())
    assert [words[g] for g in group.cpu().tolist()[:2000]] == [data[b:e] for b, e in zip(pb.cpu().tolist()[:2000], pe.cpu().tolist()[:2000])]
    # the ten most frequent: descending count, ties in order of first appearance -- Counter.most_common's rule
    t_count, t_rep, t_group = R.top_groups(count, rep, 10)
    got = [(words[g], c) for g, c in zip(t_group.cpu().tolist(), t_count.cpu().tolist())]
    assert got == want.most_common(10) and torch.equal(t_rep, rep[t_group])
    assert R.top_groups(count, rep, 1000)[0].numel() == 300 and R.top_groups(count, rep, 0)[0].numel() == 0


@pytest.mark.parametrize("opts", [["-o", "-u"], ["-o", "-u", "-t", "10"]], ids=["-o -u", "-o -u -t 10"])
def test_linegrep_sample_prints_uniq_c(rj, log_file, opts):
    path, _, want = log_file
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    r = subprocess.run([sys.executable, sample, path, ADDRESS.decode()] + opts, capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-500:])
    assert r.stdout == _uniq_c(want.most_common(10) if "-t" in opts else want.items())


def test_linegrep_sample_groups_a_field_and_refuses_u_alone(rj, log_file):
    path, data, _ = log_file
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    r = subprocess.run([sys.executable, sample, path, " ", "-f", "1", "-u", "-t", "5"], capture_output=True, timeout=300)
    want = collections.Counter(ln.split(b" ")[0] for ln in data.split(b"\n")[:-1])
    assert r.returncode == 0 and r.stdout == _uniq_c(want.most_common(5)), r.stderr.decode()[-500:]
    r = subprocess.run([sys.executable, sample, path, " ", "-u"], capture_output=True, timeout=60)
    assert r.returncode == 2 and r.stdout == b""


# ------------------------------------------------------------------------------------------------ determinism, sequence
def test_five_runs_on_one_scan_give_identical_tables(rj, scan):
    import torch
    rng = np.random.RandomState(1500)
    t, rb, re_ = _table(1500, 750, rng)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    first = scan.group_records(d, rb_t, re_t)
    for _ in range(4):
        again = scan.group_records(d, rb_t, re_t)
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_a_group_call_between_a_run_and_its_select_and_replace(rj):
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    t = W.log_like_numpy(1 << 16, 9)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = R.line_records(d)
    plain, mixed = rj.Scan(rj.Program(b"[0-9]+")), rj.Scan(rj.Program(b"[0-9]+"))
    res_p, res_m = plain.run_records(d, rb_t, re_t), mixed.run_records(d, rb_t, re_t)
    stats0 = mixed.stats()
    g, rep, cnt = mixed.group_records(d, rb_t, re_t)
    assert int(cnt.sum()) == rb_t.numel() and rep.numel() > 10
    sel_p, sel_m = plain.select_records(), mixed.select_records()
    assert torch.equal(sel_p, sel_m) and sel_p.numel() == res_p.n_matching == res_m.n_matching
    mixed.group_records(d, rb_t, re_t, indices=sel_m)
    out_p = plain.replace_records(d, rb_t, re_t, res_p, b"<N>", indices=sel_p, fill=10, lead=0, gap=1)
    out_m = mixed.replace_records(d, rb_t, re_t, res_m, b"<N>", indices=sel_m, fill=10, lead=0, gap=1)
    assert all(torch.equal(a, b) for a, b in zip(out_p, out_m)) and out_p[0].numel() > 1000
    assert torch.equal(plain.spans_tensor(d.device), mixed.spans_tensor(d.device)) and mixed.stats() == stats0
