"""GPU tests (-m gpu) of rj_scan_records_lookup (rejit_amd/csrc/record_lookup.hip; Scan.lookup_records), of records.join_rows
and of samples/linegrep_gpu.py -k.

The meaning: with set row i = set_text[set_begin[rs(i)], set_end[rs(i)]) and probe row j = text[rec_begin[r(j)], rec_end[r(j)]),
    index[j] = the smallest i whose set row has probe row j's bytes, or -1 (RJ_LOOKUP_NONE as int64);
    hits[i]  = the number of j with index[j] == i (so 0 at a later duplicate);  n_found = the number of j with index[j] >= 0.
The expected answer is a Python dict over the host copies of the rows' bytes; every comparison is exact.  Outputs are poisoned
first, with ROOM extra rows that must stay poisoned.  RJ_GROUP_HASH_BITS, RJ_GROUP_LONG_BYTES and RJ_GROUP_PEEL are the
library's test knobs, read at every call."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_TOO_LARGE, RJ_BAD_ARGUMENT = -2, -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
ROOM = 7
KS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 1500)
LENS = (0, 1, 15, 16, 17, 40, 700)
LONG_LENS = (33, 1023, 1024, 1025, 2047, 2048, 2049, 5000)
KNOBS = [(lb, hb) for lb in (16, 64) for hb in (0, 4, 64)]


STATS = ("n_found", "n_set_distinct", "n_set_hit", "long_rows")      # rj_lookup_stats: four uint64


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


class Side:
    """one table: the host bytes, the device text, the record tables on both, an optional index list"""

    def __init__(self, data, rb, re_, rows=None, d=None):
        self.data, self.rb, self.re = data, list(rb), list(re_)
        self.rows = None if rows is None else list(rows)
        self.d = dev_text(data) if d is None else d
        self.rb_t, self.re_t = dev(self.rb), dev(self.re)
        self.idx_t = None if rows is None else dev(self.rows)

    def k(self):
        return len(self.rb) if self.rows is None else len(self.rows)

    def strings(self):
        rows = range(len(self.rb)) if self.rows is None else self.rows
        return [self.data[self.rb[r]:self.re[r]] for r in rows]

    def take(self, rows):
        return Side(self.data, self.rb, self.re, rows, d=self.d)


def meaning(S, P, long_bytes=64):
    """the dict -> (index, hits as int64 arrays, stats as a dict)"""
    first = {}
    for i, s in enumerate(S.strings()):
        first.setdefault(s, i)
    probes = P.strings()
    index = np.array([first.get(s, -1) for s in probes], dtype=np.int64)
    hits = np.bincount(index[index >= 0], minlength=S.k()).astype(np.int64) if S.k() else np.zeros(0, dtype=np.int64)
    stats = {"n_found": int((index >= 0).sum()), "n_set_distinct": len(first), "n_set_hit": int((hits > 0).sum()),
             "long_rows": sum(1 for s in probes if len(s) > long_bytes)}
    return index, hits, stats


def lookup_poisoned(rj, scan, S, P, want_hits=True, want_stats=True):
    """rj_scan_records_lookup into poisoned tables -> (return value, index, hits: the whole buffers as numpy, stats or None)"""
    import torch
    lib = rj.load_library()
    ks, kp = S.k(), P.k()
    index = torch.full((kp + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    hits = torch.full((ks + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    keep = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def side(T, k):
        idx = None if T.idx_t is None else (T.idx_t if k else keep)      # (a non-null pointer with a count of 0: no rows)
        return (vp(T.d), int(T.d.numel()), vp(T.rb_t), vp(T.re_t), len(T.rb), ctypes.c_void_p(idx.data_ptr()) if idx is not None else None, k if idx is not None else 0)
    out = (ctypes.c_uint64 * 4)(*([0xA5A5] * 4))
    total = lib.rj_scan_records_lookup(scan._h, *side(S, ks), *side(P, kp), vp(index), vp(hits) if want_hits else None,
                                       ctypes.cast(out, lib.rj_scan_records_lookup.argtypes[17]) if want_stats else None, st)
    stats = dict(zip(STATS, (int(x) for x in out))) if want_stats else None
    return int(total), index.cpu().numpy(), hits.cpu().numpy(), stats


def check(rj, scan, S, P, long_bytes=64, api=False, ctx=None):
    """the raw call into poisoned tables, with hits and stats and as pure membership, against the dict; Scan.lookup_records"""
    ks, kp = S.k(), P.k()
    w_index, w_hits, w_stats = meaning(S, P, long_bytes)
    ctx = (ctx, ks, kp)
    total, index, hits, stats = lookup_poisoned(rj, scan, S, P)
    assert total == w_stats["n_found"], (ctx, total, rj.load_library().rj_last_error())
    assert (index[:kp] == w_index).all() and (index[kp:] == POISON).all(), ctx
    assert (hits[:ks] == w_hits).all() and (hits[ks:] == POISON).all() and int(w_hits.sum()) == total, ctx
    assert stats == w_stats, (ctx, stats, w_stats)
    total, index, hits, _ = lookup_poisoned(rj, scan, S, P, want_hits=False, want_stats=False)      # is_in: no atomics on the counts
    assert total == w_stats["n_found"] and (index[:kp] == w_index).all() and (index[kp:] == POISON).all() and (hits == POISON).all(), ctx
    if api:
        a_index, a_hits, a_stats = scan.lookup_records(S.d, S.rb_t, S.re_t, P.d, P.rb_t, P.re_t, set_indices=S.idx_t, indices=P.idx_t, hits=True, stats=True)
        assert a_index.numel() == kp and a_hits.numel() == ks and a_stats == w_stats, ctx
        assert (a_index.cpu().numpy() == w_index).all() and (a_hits.cpu().numpy() == w_hits).all(), ctx
        only = scan.lookup_records(S.d, S.rb_t, S.re_t, P.d, P.rb_t, P.re_t, set_indices=S.idx_t, indices=P.idx_t)
        assert (only.cpu().numpy() == w_index).all()
    return w_index, w_hits, w_stats


# ------------------------------------------------------------------------------------------------ tables
def _pool(d, rng, lens):
    """d distinct strings of lower-case letters with lengths from `lens`: among them strings that share everything but their
    last byte and strings that are prefixes of one another"""
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


def _lay(strings, rng, lead, filler, last_long=None):
    """the strings with 0..3 filler bytes between them behind `lead` filler bytes; the last row ends at the text's very end
    (and is `last_long` when given) -> (data, rec_begin, rec_end)"""
    strings = list(strings)
    if last_long is not None and strings:
        strings[-1] = last_long
    parts, rb, re_, at = [filler * lead], [], [], lead
    for s in strings:
        seam = int(rng.randint(0, 4))
        parts.append(filler * seam)
        at += seam
        rb.append(at)
        parts.append(s)
        at += len(s)
        re_.append(at)
    return b"".join(parts), rb, re_


def _two_tables(ks, kp, rng, lens, shared=False):
    """ks set rows from the first two thirds of a pool, kp probe rows from all of it (some are absent, most occur more than
    once), in two texts with different leads, fillers and lengths -- or, shared, in ONE buffer, the set's part in front.  The
    set's last row is the pool's longest string and ends at the set text's very end."""
    d = min(40, max(ks, kp) // 3 + 2)
    pool = _pool(d, rng, lens)
    set_pool = pool[:(2 * d) // 3 + 1]
    longest = max(set_pool, key=len)
    s_data, s_rb, s_re = _lay([set_pool[i] for i in rng.randint(0, len(set_pool), ks)], rng, 5, b"|", last_long=longest)
    p_data, p_rb, p_re = _lay([pool[i] for i in rng.randint(0, d, kp)], rng, 18, b"~")
    if not shared:
        return Side(s_data, s_rb, s_re), Side(p_data, p_rb, p_re)
    both = s_data + p_data
    d_both = dev_text(both)
    off = len(s_data)
    return Side(both, s_rb, s_re, d=d_both), Side(both, [b + off for b in p_rb], [e + off for e in p_re], d=d_both)


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("ks", KS)
def test_sizes_tiers_and_forced_collisions_equal_the_dict(rj, scan, monkeypatch, ks):
    """ks x kp across the wave seams and the 256-row unit seams, row lengths 0 .. 5000, in two distinct device texts and again
    in one shared buffer; RJ_GROUP_LONG_BYTES in {16, 64} x RJ_GROUP_HASH_BITS in {0, 4, 64}: both tiers on each side, with 4
    bits the strings share sixteen probe chains, with 0 every row walks ONE chain."""
    for kp in KS:
        rng = np.random.RandomState(5000 * ks + kp)
        for shared in (False, True):
            S, P = _two_tables(ks, kp, rng, LENS + LONG_LENS, shared=shared)
            for long_bytes, bits in KNOBS:
                monkeypatch.setenv("RJ_GROUP_LONG_BYTES", str(long_bytes))
                monkeypatch.setenv("RJ_GROUP_HASH_BITS", str(bits))
                check(rj, scan, S, P, long_bytes=long_bytes, api=(long_bytes, bits) == (64, 64) and not shared, ctx=(shared, long_bytes, bits))


def test_index_lists_on_both_sides_and_a_rows_identity(rj, scan):
    import torch
    rng = np.random.RandomState(9)
    S, P = _two_tables(300, 500, rng, LENS)
    for s_rows, p_rows in ((rng.permutation(300), rng.permutation(500)), (rng.randint(0, 300, 700), rng.randint(0, 500, 257)), ([], rng.randint(0, 500, 65)),
                           (rng.randint(0, 300, 64), []), (list(range(299, -1, -1)), None), (None, list(range(499, -1, -1)))):
        check(rj, scan, S if s_rows is None else S.take(s_rows), P if p_rows is None else P.take(p_rows), api=True)
    # the index is the smallest set ROW, not the smallest record: set rows 0 and 2 name records 2 and 0
    S = Side(b"xx|yy|xx", [0, 3, 6], [2, 5, 8], rows=[2, 1, 0, 1])
    P = Side(b"yy xx zz", [0, 3, 6], [2, 5, 8], rows=[1, 1, 2, 0])
    index, hits = scan.lookup_records(S.d, S.rb_t, S.re_t, P.d, P.rb_t, P.re_t, set_indices=S.idx_t, indices=P.idx_t, hits=True)
    assert index.cpu().tolist() == [0, 0, -1, 1] and hits.cpu().tolist() == [2, 1, 0, 0]
    # "ab" and "ab\0" are different, empty rows are equal to each other
    S = Side(b"ab|ab\0||\0", [0, 3, 7, 8], [2, 6, 7, 9])
    P = Side(b"\0ab\0ab", [1, 1, 0, 6, 3, 0], [4, 3, 1, 6, 3, 0])
    index = scan.lookup_records(S.d, S.rb_t, S.re_t, P.d, P.rb_t, P.re_t)
    assert index.cpu().tolist() == [1, 0, 3, 2, 2, 2]
    assert torch.equal(index >= 0, torch.ones(6, dtype=torch.bool, device="cuda:0"))


# ------------------------------------------------------------------------------------------------ rows that differ late
@pytest.mark.parametrize("long_bytes", [16, 64])
def test_long_rows_that_differ_late(rj, scan, monkeypatch, long_bytes):
    """Probe rows longer than L against set rows of the same length: equal; different only in the last byte; different only
    in byte 1024 (the second wave iteration's first); equal bytes but one byte longer, and one byte shorter -- at every
    misalignment of the probe text, the last probe row ending at its text's very end."""
    monkeypatch.setenv("RJ_GROUP_LONG_BYTES", str(long_bytes))
    rng = np.random.RandomState(77)
    bases = [rng.randint(ord("a"), ord("z") + 1, ln).astype(np.uint8).tobytes() for ln in LONG_LENS if ln > long_bytes]
    s_data, s_rb, s_re = _lay(bases + bases[:2], rng, 3, b"|")
    S = Side(s_data, s_rb, s_re)
    probes = []
    for b in bases:
        ln = len(b)
        last = b[:-1] + bytes([b[-1] ^ 1])
        mid = b[:1024] + bytes([b[1024] ^ 2]) + b[1025:] if ln > 1024 else b[:ln // 2] + bytes([b[ln // 2] ^ 2]) + b[ln // 2 + 1:]
        probes += [b, last, mid, b + b"a", b[:-1]]
    for mis in range(16):
        p_data, p_rb, p_re = _lay(probes + [bases[-1]], rng, mis, b"~")
        P = Side(p_data, p_rb, p_re)
        assert p_re[-1] == len(p_data) and P.d.data_ptr() % 16 == 0
        w_index, w_hits, w_stats = check(rj, scan, S, P, long_bytes=long_bytes, api=mis == 0, ctx=mis)
        want = []
        for i in range(len(bases)):
            want += [i, -1, -1, -1, -1]
        assert w_index.tolist() == want + [len(bases) - 1] and w_stats["long_rows"] == len(probes) + 1
        assert w_hits.tolist() == [1] * (len(bases) - 1) + [2, 0, 0]


# ------------------------------------------------------------------------------------------------ skew
@pytest.mark.parametrize("peel", ["1", "0"])
def test_every_probe_row_equal_to_one_set_row(rj, scan, monkeypatch, peel):
    """1500 probe rows, all equal to one set row (which has a later duplicate): with hits -- one atomic add per wave with the
    peel, one per lane with RJ_GROUP_PEEL=0 -- and without (the instantiation that issues no atomics); the hits add up to
    n_found."""
    monkeypatch.setenv("RJ_GROUP_PEEL", peel)
    S = Side(b"cold|hot|hot|colder", [0, 5, 9, 13], [4, 8, 12, 19])
    P = Side(b"~hot", [1], [4], rows=[0] * 1500)
    w_index, w_hits, w_stats = check(rj, scan, S, P, api=True)
    assert w_index.tolist() == [1] * 1500 and w_hits.tolist() == [0, 1500, 0, 0] and w_stats["n_found"] == 1500 and w_stats["n_set_hit"] == 1
    # ... and a second popular string in the same waves, which the peel leaves to the lanes' own atomics
    P = Side(b"~hot colder", [1, 5], [4, 11], rows=[0, 0, 1] * 500)
    _, w_hits, _ = check(rj, scan, S, P)
    assert w_hits.tolist() == [0, 1000, 0, 500]


# ------------------------------------------------------------------------------------------------ cross-checks
def test_the_group_call_over_both_index_lists_implies_the_same_index(rj, scan):
    """On one shared text: group_records over cat(set_idx, probe_idx); a probe row's group has a representative, and that
    is the answer when it is a set row (below ks).  Independent of the Python dict."""
    import torch
    rng = np.random.RandomState(41)
    S, P = _two_tables(400, 900, rng, LENS + (33, 1025), shared=True)
    n_set = len(S.rb)
    rb_t, re_t = torch.cat([S.rb_t, P.rb_t]), torch.cat([S.re_t, P.re_t])
    for set_idx, probe_idx in ((torch.arange(n_set, device="cuda:0"), torch.arange(n_set, n_set + 900, device="cuda:0")),
                               (dev(rng.randint(0, n_set, 300)), dev(n_set + rng.randint(0, 900, 1100)))):
        ks = int(set_idx.numel())
        group, rep, _ = scan.group_records(S.d, rb_t, re_t, indices=torch.cat([set_idx, probe_idx]).contiguous())
        first = rep[group[ks:]]
        want = torch.where(first < ks, first, torch.full_like(first, -1))
        index = scan.lookup_records(S.d, rb_t, re_t, S.d, rb_t, re_t, set_indices=set_idx.contiguous(), indices=probe_idx.contiguous())
        assert torch.equal(index, want) and int((want >= 0).sum()) > 100 and int((want < 0).sum()) > 100


def test_a_lookup_against_the_groups_dictionary_gives_group_numbers_and_join_rows_the_inner_join(rj, scan):
    import torch
    from rejit_amd import records as R
    rng = np.random.RandomState(43)
    S, P = _two_tables(257, 513, rng, LENS)
    group, rep, count = scan.group_records(S.d, S.rb_t, S.re_t)
    # the set's own rows against its dictionary: its own group numbers
    own = scan.lookup_records(S.d, S.rb_t, S.re_t, S.d, S.rb_t, S.re_t, set_indices=rep)
    assert torch.equal(own, group)
    index = scan.lookup_records(S.d, S.rb_t, S.re_t, P.d, P.rb_t, P.re_t, set_indices=rep)
    probe_row, set_row = R.join_rows(index, group, count)
    s_rows, p_rows = S.strings(), P.strings()
    want = [(j, i) for j in range(513) for i in range(257) if p_rows[j] == s_rows[i]]
    assert list(zip(probe_row.cpu().tolist(), set_row.cpu().tolist())) == want and len(want) > 513


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_table_and_the_first_row_and_write_nothing(rj, scan):
    import torch
    lib = rj.load_library()
    rng = np.random.RandomState(51)
    S, P = _two_tables(300, 700, rng, LENS)

    def refused(why, S2, P2, message):
        for want_hits in (True, False):
            total, index, hits, _ = lookup_poisoned(rj, scan, S2, P2, want_hits=want_hits, want_stats=want_hits)
            msg = lib.rj_last_error().decode()
            assert total == RJ_BAD_ARGUMENT and message in msg and (message.startswith("set") or "set row" not in msg), (why, total, msg)
            assert (index == POISON).all() and (hits == POISON).all(), why
        with pytest.raises(rj.RejitError) as err:
            scan.lookup_records(S2.d, S2.rb_t, S2.re_t, P2.d, P2.rb_t, P2.re_t, set_indices=S2.idx_t, indices=P2.idx_t, hits=True)
        assert err.value.status == RJ_BAD_ARGUMENT and message in err.value.message
        check(rj, scan, S, P)                                              # the same scan answers a good call

    bad = list(range(0, 300, 2))
    bad[11], bad[140] = 300, -1
    bad_set = S.take(bad)
    refused("two bad set indices: the smaller row is named", bad_set, P, "set row 11 ")
    e = list(S.re)
    e[299] = len(S.data) + 1
    refused("a set row ends behind the SET text", Side(S.data, S.rb, e, d=S.d), P, "set row 299 ")
    assert len(P.data) > len(S.data) + 1                                   # (inside the probe text: each row is held against its own text)
    bad = list(range(700))
    bad[0], bad[699] = 700, 700
    refused("a bad probe index at the first row", S, P.take(bad), "row 0 ")
    e = list(P.re)
    e[650] = P.rb[650] - 1
    bad_probe = Side(P.data, P.rb, e, d=P.d)
    refused("begin > end in the probe table", S, bad_probe, "row 650 ")
    refused("both tables are bad: the set is checked first", bad_set, bad_probe, "set row 11 ")
    # arguments
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    f = lib.rj_scan_records_lookup
    out = torch.full((708,), POISON, dtype=torch.int64, device="cuda:0")
    out2 = out.clone()
    good = [scan._h, vp(S.d), len(S.data), vp(S.rb_t), vp(S.re_t), 300, None, 0, vp(P.d), len(P.data), vp(P.rb_t), vp(P.re_t), 700, None, 0, vp(out), vp(out2), None, st]
    for at in (0, 1, 3, 4, 8, 10, 11, 15):                                 # the scan, either text, a table of either side, d_index
        args = list(good)
        args[at] = None
        assert f(*args) == RJ_BAD_ARGUMENT and "null" in lib.rj_last_error().decode(), at
    off = lambda x: ctypes.c_void_p(x.data_ptr() + 4)
    for at, x in ((3, S.rb_t), (4, S.re_t), (6, S.rb_t), (10, P.rb_t), (11, P.re_t), (13, P.rb_t), (15, out), (16, out2)):
        args = list(good)
        args[at] = off(x)
        if at in (6, 13):
            args[at + 1] = 5
        assert f(*args) == RJ_BAD_ARGUMENT and "aligned" in lib.rj_last_error().decode(), at
    for at in (5, 12):
        args = list(good)
        args[at] = 1 << 31
        assert f(*args) == RJ_TOO_LARGE and "2^31" in lib.rj_last_error().decode()
    args = list(good)
    args[6], args[7] = vp(S.rb_t), 1 << 31
    assert f(*args) == RJ_TOO_LARGE
    assert bool((out == POISON).all()) and bool((out2 == POISON).all())
    assert f(scan._h, None, 0, None, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, None, None, st) == 0


# ------------------------------------------------------------------------------------------------ the scan's state
def test_the_scans_state_stays_and_group_and_sort_share_the_scratch(rj):
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    t = W.log_like_numpy(1 << 16, 3)
    d = torch.from_numpy(t).to("cuda:0")
    data = t.tobytes()
    s = rj.Scan(rj.Program(b"[0-9]+"))
    rb_t, re_t = R.line_records(d)
    k = int(rb_t.numel())
    res = s.run_records(d, rb_t, re_t)
    sel0 = s.select_records().clone()
    spans0 = s.spans_tensor(d.device).clone()
    stats0 = s.stats()
    assert res.n_matching > 20 and k > 100
    lines = Side(data, rb_t.cpu().tolist(), re_t.cpu().tolist(), d=d)
    check(rj, s, lines.take(range(0, k, 3)), lines.take(sel0.cpu().tolist()), api=True)
    assert torch.equal(s.spans_tensor(d.device), spans0) and torch.equal(s.select_records(), sel0) and s.stats() == stats0
    # the group and the sort use the same scratch right behind it
    strings = lines.strings()
    group, rep, count = s.group_records(d, rb_t, re_t)
    seen = {}
    assert group.cpu().tolist() == [seen.setdefault(x, len(seen)) for x in strings] and int(count.sum()) == k
    order = s.sort_records(d, rb_t, re_t)
    assert order.cpu().tolist() == sorted(range(k), key=lambda j: (strings[j], j))
    check(rj, s, lines, lines.take(rep.cpu().tolist()))
    assert s.run_records(d, rb_t, re_t).n_kept == res.n_kept


# ------------------------------------------------------------------------------------------------ the sample
@pytest.fixture(scope="module")
def grep_files(tmp_path_factory):
    rng = np.random.RandomState(61)
    users = [b"user%d" % i for i in range(30)]
    lines = []
    for i in range(400):
        kind = i % 7
        if kind == 0:
            lines.append(users[int(rng.randint(0, 30))])                                   # a line that is a key, or could be
        elif kind == 1:
            lines.append(b"short")                                                         # one field only
        else:
            lines.append(b"%d %s GET /p%d" % (i, users[int(rng.randint(0, 30))], int(rng.randint(0, 9))))
    root = tmp_path_factory.mktemp("lookup")
    log, keys_nl, keys_plain, keys_none = (str(root / n) for n in ("access.log", "keys_nl.txt", "keys_plain.txt", "keys_none.txt"))
    keys = [users[i] for i in (3, 7, 7, 11, 19, 23)] + [b"short", b"user"]
    with open(log, "wb") as fh:
        fh.write(b"\n".join(lines) + b"\n")
    with open(keys_nl, "wb") as fh:
        fh.write(b"\n".join(keys) + b"\n")
    with open(keys_plain, "wb") as fh:
        fh.write(b"\n".join(keys))
    with open(keys_none, "wb") as fh:
        fh.write(b"nobody\nnothing\n")
    return log, lines, {"nl": (keys_nl, set(keys)), "plain": (keys_plain, set(keys)), "none": (keys_none, {b"nobody", b"nothing"})}


def _selected(lines, keys, pattern, field, invert):
    import re
    out = []
    for i, ln in enumerate(lines):
        if field is None:
            sel = re.search(pattern, ln) is not None and ln in keys
        else:
            parts = re.split(pattern, ln)
            sel = len(parts) >= field and parts[field - 1] in keys
        if sel != invert:
            out.append(i)
    return out


@pytest.mark.parametrize("which,pattern,opts", [
    ("nl", "[a-z]+", ["-c"]), ("nl", "[a-z]+", []), ("plain", "[a-z]+", ["-n"]), ("nl", "[a-z]+", ["-p"]), ("plain", "[0-9]", ["-v", "-n"]),
    ("nl", " ", ["-f", "2", "-n"]), ("plain", " ", ["-f", "2", "-p"]), ("nl", " ", ["-f", "1", "-v", "-c"]), ("nl", " ", ["-f", "4", "-c"]),
    ("none", "[a-z]+", ["-c"]), ("none", " ", ["-f", "2", "-p"])],
    ids=lambda x: "_".join(x) if isinstance(x, list) else None)
def test_linegrep_sample_looks_lines_and_fields_up_in_a_keys_file(rj, grep_files, which, pattern, opts):
    """-k KEYS: the lines with a match of PATTERN that are a line of KEYS, or with -f N the lines whose field N is one; -v
    inverts the whole selection; a KEYS file with and without a final line break; exit status 0 and 1."""
    log, lines, keys = grep_files
    path, key_set = keys[which]
    field = int(opts[opts.index("-f") + 1]) if "-f" in opts else None
    want = _selected(lines, key_set, pattern.encode(), field, "-v" in opts)
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    r = subprocess.run([sys.executable, sample, log, pattern, "-k", path] + opts, capture_output=True, timeout=300)
    assert r.returncode == (0 if want else 1), (r.returncode, r.stderr.decode()[-500:])
    if "-n" in opts:
        assert r.stdout == b"".join(b"%d\n" % (i + 1) for i in want)
    elif "-p" in opts:
        assert r.stdout == b"".join(lines[i] + b"\n" for i in want)
    else:
        assert r.stdout == b"%d\n" % len(want)
    if which == "none" or opts[:2] == ["-f", "4"]:
        assert not want                                                  # (exit status 1)
    else:
        assert 0 < len(want) < len(lines)


@pytest.mark.parametrize("opts", [["-o"], ["-s", "x"], ["-f", "2", "-u"], ["-p", "-b"], ["-f", "2", "-u", "-t", "3"]], ids=lambda x: "_".join(x))
def test_linegrep_sample_refuses_other_options_beside_k(rj, grep_files, opts):
    log, _, keys = grep_files
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    r = subprocess.run([sys.executable, sample, log, " ", "-k", keys["nl"][0]] + opts, capture_output=True, timeout=60)
    assert r.returncode == 2 and r.stdout == b""
