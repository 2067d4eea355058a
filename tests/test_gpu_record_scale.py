"""GPU tests (-m gpu) of the four row-layer record calls -- rj_scan_records_group, _sort, _lookup, _parse -- on tables of MORE
rows than one pass of their persistent grids covers: unit_grid() of rejit_amd/csrc/record_frame.h allows 1024 workgroups of
256 rows (K0 = 262144 rows a pass), record_parse.hip's kParseGrid 2048 (2 K0), and the wave-tier kernels stride by 4096 waves.

tests/record_scale.py draws the tables from a small pool of strings and gathers every expectation, with numpy, from a plain
reference over the pool; tests/test_record_scale_plan.py checks it row by row on the CPU, and checks -- from the inputs alone --
that these tables reach what they are here for.  The calls go through the poisoned-output helpers of the four calls' own GPU
tests: every comparison is exact, and the ROOM rows behind every output stay poisoned."""
import numpy as np
import pytest

import parse_cases as pc
import record_scale as RS
from test_gpu_record_group import POISON, group_poisoned
from test_gpu_record_lookup import lookup_poisoned
from test_gpu_record_parse import POISON8, POISON_U, parse_poisoned
from test_gpu_record_sort import sort_poisoned

pytestmark = pytest.mark.gpu
RJ_BAD_ARGUMENT = -4
K0 = RS.K0
BEYOND = K0 + 257                   # the k that also runs with the knobs forced


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
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


class Uploaded:
    """a pool on the device, once: its text and its own record table"""

    def __init__(self, pool):
        self.pool = pool
        self.d, self.rb_t, self.re_t = dev(pool.text), dev(pool.rb), dev(pool.re)


class Table:
    """A table of a call as the four modules' helpers ask for it (their Side / Table, from numpy arrays): the device text, the
    record tables, the index list or None; `rb` and `records` are asked for their length only."""

    def __init__(self, d, rb_t, re_t, idx_t=None):
        self.d, self.rb_t, self.re_t, self.idx_t = d, rb_t, re_t, idx_t
        self.rb = self.records = range(int(rb_t.numel()))

    def k(self):
        return len(self.rb) if self.idx_t is None else int(self.idx_t.numel())


def direct(up, pk):
    rb, re_, _ = RS.direct(up.pool, pk)
    return Table(up.d, dev(rb), dev(re_))


def indexed(up, pk):
    return Table(up.d, up.rb_t, up.re_t, dev(pk))


@pytest.fixture(scope="module")
def strings(rj):
    return Uploaded(RS.string_pool())


@pytest.fixture(scope="module")
def numbers(rj):
    return Uploaded(RS.parse_pool())


# ------------------------------------------------------------------------------------------------ the four checks
def check_group(rj, scan, T, want, ctx):
    w_group, w_rep, w_count = want
    k, G = len(w_group), len(w_rep)
    total, g, rep, cnt = group_poisoned(rj, scan, T.d, T.rb_t, T.re_t, indices=T.idx_t, cap=G, room_for=G)
    assert total == G, (ctx, total, G, rj.load_library().rj_last_error())
    assert (g[:k] == w_group).all() and (g[k:] == POISON).all(), (ctx, first_difference(g[:k], w_group))
    assert (rep[:G] == w_rep).all() and (rep[G:] == POISON).all(), (ctx, first_difference(rep[:G], w_rep))
    assert (cnt[:G] == w_count).all() and (cnt[G:] == POISON).all() and int(w_count.sum()) == k, (ctx, first_difference(cnt[:G], w_count))


def check_sort(rj, scan, T, want, ctx, rounds=3):
    k = len(want)
    total, order, stats = sort_poisoned(rj, scan, T.d, T.rb_t, T.re_t, indices=T.idx_t)
    assert total == k, (ctx, total, rj.load_library().rj_last_error())
    assert (order[:k] == want).all() and (order[k:] == POISON).all(), (ctx, stats, first_difference(order[:k], want))
    assert stats["rounds"] >= rounds, (ctx, stats)
    return stats


def check_lookup(rj, scan, S, P, want, ctx, hits_and_stats=True):
    w_index, w_hits, w_stats = want
    ks, kp = len(w_hits), len(w_index)
    total, index, hits, stats = lookup_poisoned(rj, scan, S, P, want_hits=hits_and_stats, want_stats=hits_and_stats)
    assert total == w_stats["n_found"], (ctx, total, w_stats, rj.load_library().rj_last_error())
    assert (index[:kp] == w_index).all() and (index[kp:] == POISON).all(), (ctx, first_difference(index[:kp], w_index))
    if hits_and_stats:
        assert (hits[:ks] == w_hits).all() and (hits[ks:] == POISON).all() and int(w_hits.sum()) == total, (ctx, first_difference(hits[:ks], w_hits))
        assert stats == w_stats, (ctx, stats, w_stats)
    else:
        assert (hits == POISON).all() and stats is None, ctx


def check_parse(rj, scan, T, want, kind, trim, ctx, want_status=True):
    w_status, w_bits, w_stats = want
    k = len(w_status)
    total, values, status, stats = parse_poisoned(rj, scan, T, kind, trim, want_status=want_status)
    assert total == w_stats["n_ok"], (ctx, total, w_stats, rj.load_library().rj_last_error())
    assert (values[:k] == w_bits).all() and (values[k:] == POISON_U).all(), (ctx, first_difference(values[:k], w_bits))
    if want_status:
        assert (status[:k] == w_status).all() and (status[k:] == POISON8).all(), (ctx, first_difference(status[:k], w_status))
    else:
        assert (status == POISON8).all(), ctx
    assert stats == w_stats and sum(stats.values()) == k, (ctx, stats, w_stats)


def first_difference(got, want):
    """(the first row that differs, what it has, what it should have) -- for the message of a failed comparison"""
    at = np.nonzero(got != want)[0]
    return None if at.size == 0 else (int(at[0]), int(got[at[0]]), int(want[at[0]]), int(at.size))


# ------------------------------------------------------------------------------------------------ group
@pytest.mark.parametrize("k", RS.KS)
def test_group_beyond_one_pass(rj, scan, strings, monkeypatch, k):
    """Hash, insert, number and emit take their unit loops round again (K0: exactly one pass): group, rep, count and G of
    the direct and of the indexed table.  For K0 + 257 also with RJ_GROUP_LONG_BYTES=16 -- more than 4096 rows in the wave
    kernels' lists, their stride at the capped grid -- and with RJ_GROUP_HASH_BITS=2 over 40 strings: four probe chains."""
    pool = strings.pool
    pk = RS.group_pick(pool, k)
    want = RS.group_meaning(pool, pk)
    tables = (("direct", direct(strings, pk)), ("indexed", indexed(strings, pk)))
    for name, T in tables:
        check_group(rj, scan, T, want, (k, name))
    if k != BEYOND:
        return
    monkeypatch.setenv("RJ_GROUP_LONG_BYTES", str(RS.FORCED_LONG))
    for name, T in tables:
        check_group(rj, scan, T, want, (k, name, "L=16"))
    monkeypatch.delenv("RJ_GROUP_LONG_BYTES")
    monkeypatch.setenv("RJ_GROUP_HASH_BITS", "2")
    pk = RS.group_small_pick(pool, k)
    want = RS.group_meaning(pool, pk)
    assert len(want[1]) <= RS.SMALL_POOL
    for name, T in (("direct", direct(strings, pk)), ("indexed", indexed(strings, pk))):
        check_group(rj, scan, T, want, (k, name, "2 hash bits"))


# ------------------------------------------------------------------------------------------------ sort
@pytest.mark.parametrize("k", RS.KS)
def test_sort_beyond_one_pass(rj, scan, strings, monkeypatch, k):
    """Init, compact (1024 workgroups take more than 1024 tickets), skip, key and cut take their loops round again -- in the
    second round too, which still lists nearly every row (test_record_scale_plan.py) -- and a third round follows: order and the
    returned k of the direct and of the indexed table.  For K0 + 257 also with RJ_SORT_LONG_BYTES=16: more than 4096 rows in the
    wave tier's list."""
    pool = strings.pool
    pk = RS.sort_pick(pool, k)
    want = RS.sort_meaning(pool, pk)
    tables = (("direct", direct(strings, pk)), ("indexed", indexed(strings, pk)))
    for name, T in tables:
        stats = check_sort(rj, scan, T, want, (k, name))
        assert stats["keyed_rows"] >= k + RS.open_after_round_one(pool, pk), (k, name, stats)
    if k != BEYOND:
        return
    monkeypatch.setenv("RJ_SORT_LONG_BYTES", str(RS.FORCED_LONG))
    for name, T in tables:
        stats = check_sort(rj, scan, T, want, (k, name, "L=16"))
        assert stats["long_rows"] > RS.WAVE_STRIDE, (k, name, stats)


# ------------------------------------------------------------------------------------------------ lookup
@pytest.mark.parametrize("ks,kp", RS.LOOKUP_SIZES)
def test_lookup_beyond_one_pass(rj, scan, strings, monkeypatch, ks, kp):
    """The set's build, the probe (one unit per workgroup), the wave probe, emit and hits beyond one pass on either side: with
    hits and stats, with neither (no atomics on the counts), with RJ_GROUP_PEEL=0; for the first pair also with
    RJ_GROUP_LONG_BYTES=16."""
    pool = strings.pool
    set_pk, probe_pk = RS.lookup_picks(pool, ks, kp)
    want = RS.lookup_meaning(pool, set_pk, probe_pk)
    assert 0 < want[2]["n_found"] < kp and want[2]["n_set_hit"] < want[2]["n_set_distinct"]
    S_direct, S_indexed = direct(strings, set_pk), indexed(strings, set_pk)
    P_direct, P_indexed = direct(strings, probe_pk), indexed(strings, probe_pk)
    check_lookup(rj, scan, S_direct, P_direct, want, (ks, kp, "direct, direct"))
    check_lookup(rj, scan, S_indexed, P_indexed, want, (ks, kp, "indexed, indexed, is_in"), hits_and_stats=False)
    monkeypatch.setenv("RJ_GROUP_PEEL", "0")
    check_lookup(rj, scan, S_indexed, P_direct, want, (ks, kp, "indexed, direct, no peel"))
    monkeypatch.delenv("RJ_GROUP_PEEL")
    if (ks, kp) != RS.LOOKUP_SIZES[0]:
        return
    monkeypatch.setenv("RJ_GROUP_LONG_BYTES", str(RS.FORCED_LONG))
    want = RS.lookup_meaning(pool, set_pk, probe_pk, long_bytes=RS.FORCED_LONG)
    assert want[2]["long_rows"] > RS.WAVE_STRIDE
    check_lookup(rj, scan, S_direct, P_indexed, want, (ks, kp, "direct, indexed, L=16"))
    check_lookup(rj, scan, S_direct, P_indexed, want, (ks, kp, "direct, indexed, L=16, is_in"), hits_and_stats=False)


# ------------------------------------------------------------------------------------------------ parse
@pytest.mark.parametrize("k", RS.PARSE_KS)
def test_parse_beyond_one_pass(rj, scan, numbers, k):
    """The check kernel (unit_grid) and the parse kernel (kParseGrid) beyond one pass of each: values, statuses, the five
    counts -- a wave adds them up over all its units -- and the return value, for the three kinds under TRIM; without d_status
    once; for the last k int64 without TRIM and the indexed table as well."""
    pool = numbers.pool
    pk = RS.parse_pick(pool, k)
    last = k == RS.PARSE_KS[-1]
    tables = [("direct", direct(numbers, pk))] + ([("indexed", indexed(numbers, pk))] if last else [])
    for name, T in tables:
        for kind, trim in [(kind, True) for kind in pc.KINDS] + ([(pc.INT64, False)] if last else []):
            want = RS.parse_meaning(pool, pk, kind, trim)
            assert all(want[2][s] > 0 for s in RS.PARSE_STATS if s != ("n_range" if kind == pc.FLOAT64 else "n_inexact")), want[2]
            check_parse(rj, scan, T, want, kind, trim, (k, name, kind, trim))
        want = RS.parse_meaning(pool, pk, pc.UINT64, True)
        check_parse(rj, scan, T, want, pc.UINT64, True, (k, name, "no d_status"), want_status=False)


# ------------------------------------------------------------------------------------------------ one string
def test_one_string_in_every_row(rj, scan):
    """K0 + 257 rows of one string of 17 bytes, then of the empty string: one slot takes more than K0 joins and more than K0
    hits, one segment stays whole (the empty rows close in the first round, the others in the second).  Then the number 17 in
    every row: one status count takes them all."""
    k = BEYOND
    zeros, rows = np.zeros(k, dtype=np.int64), np.arange(k, dtype=np.int64)
    hits = zeros.copy()
    hits[0] = k
    stats = {"n_found": k, "n_set_distinct": 1, "n_set_hit": 1, "long_rows": 0}
    for string in (b"seventeen bytes !", b""):
        text, rb, re_ = RS.one_string_table(k, string)
        T = Table(dev(text), dev(rb), dev(re_))
        check_group(rj, scan, T, (zeros, np.array([0], dtype=np.int64), np.array([k], dtype=np.int64)), ("one string", len(string)))
        check_sort(rj, scan, T, rows, ("one string", len(string)), rounds=2 if string else 1)
        check_lookup(rj, scan, T, T, (zeros, hits, stats), ("one string", len(string)))
        check_lookup(rj, scan, T, T, (zeros, hits, stats), ("one string", len(string), "is_in"), hits_and_stats=False)
    text, rb, re_ = RS.one_string_table(k, b"17")
    T = Table(dev(text), dev(rb), dev(re_))
    want = (np.zeros(k, dtype=np.uint8), np.full(k, 17, dtype=np.uint64), dict(zip(RS.PARSE_STATS, (k, 0, 0, 0, 0))))
    check_parse(rj, scan, T, want, pc.INT64, False, "17 in every row")


# ------------------------------------------------------------------------------------------------ a bad row in a later pass
def test_a_bad_row_in_a_later_pass_is_named_and_nothing_is_written(rj, scan, strings, numbers):
    """2 K0 + 65 rows with a bad index at row K0 + 5 -- the second pass of the kernel that checks the rows -- and another at row
    2 K0 + 1: each of the four calls refuses, names row K0 + 5 and writes no output row; the same scan then answers a good call."""
    lib = rj.load_library()
    pool = strings.pool
    pk = RS.group_pick(pool, RS.BAD_K)
    bad = indexed(strings, RS.bad_index_list(pool, pk))
    good_pk = RS.group_pick(pool, 5000)
    good = indexed(strings, good_pk)
    named = "row %d " % RS.BAD_ROWS[0]

    total, g, rep, cnt = group_poisoned(rj, scan, bad.d, bad.rb_t, bad.re_t, indices=bad.idx_t, cap=pool.P, room_for=pool.P)
    msg = lib.rj_last_error().decode()
    assert total == RJ_BAD_ARGUMENT and named in msg, (total, msg)
    assert (g == POISON).all() and (rep == POISON).all() and (cnt == POISON).all()
    check_group(rj, scan, good, RS.group_meaning(pool, good_pk), "group, behind a refusal")

    total, order, _ = sort_poisoned(rj, scan, bad.d, bad.rb_t, bad.re_t, indices=bad.idx_t)
    msg = lib.rj_last_error().decode()
    assert total == RJ_BAD_ARGUMENT and named in msg, (total, msg)
    assert (order == POISON).all()
    check_sort(rj, scan, good, RS.sort_meaning(pool, good_pk), "sort, behind a refusal", rounds=2)

    set_pk, probe_pk = RS.lookup_picks(pool, 5000, 5000)
    good_set, good_probe = indexed(strings, set_pk), indexed(strings, probe_pk)
    want = RS.lookup_meaning(pool, set_pk, probe_pk)
    for S, P, message in ((bad, good_probe, "set " + named), (good_set, bad, named)):
        for hits_and_stats in (True, False):
            total, index, hits, _ = lookup_poisoned(rj, scan, S, P, want_hits=hits_and_stats, want_stats=hits_and_stats)
            msg = lib.rj_last_error().decode()
            assert total == RJ_BAD_ARGUMENT and message in msg and (message.startswith("set") or "set row" not in msg), (total, msg)
            assert (index == POISON).all() and (hits == POISON).all(), message
        check_lookup(rj, scan, good_set, good_probe, want, "lookup, behind a refusal")

    pool = numbers.pool
    pk = RS.parse_pick(pool, RS.BAD_K)
    bad = indexed(numbers, RS.bad_index_list(pool, pk))
    good_pk = RS.parse_pick(pool, 5000)
    for kind in pc.KINDS:
        total, values, status, _ = parse_poisoned(rj, scan, bad, kind, True)
        msg = lib.rj_last_error().decode()
        assert total == RJ_BAD_ARGUMENT and named in msg, (kind, total, msg)
        assert (values == POISON_U).all() and (status == POISON8).all(), kind
    check_parse(rj, scan, indexed(numbers, good_pk), RS.parse_meaning(pool, good_pk, pc.INT64, True), pc.INT64, True, "parse, behind a refusal")
