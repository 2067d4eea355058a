"""CPU test of tests/record_scale.py, the builder of the tables tests/test_gpu_record_scale.py runs: every vectorised meaning
against a row-by-row one written here (a dict in insertion order, sorted(), a dict, parse_cases.meaning per row); the row
counts against the constants of the sources they are derived from; and the conditions, computed from the inputs alone, that
keep the GPU test from quietly missing what it is there for -- a second pass of every persistent loop at the capped grid,
the wave tier at its 4096-wave stride, a second sort round of more than one pass."""
import os
import re
import time

import numpy as np
import pytest

import parse_cases as pc
import record_scale as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rejit_amd", "csrc")
K0 = RS.K0
BEYOND = K0 + 257


@pytest.fixture(scope="module")
def pool():
    return RS.string_pool()


@pytest.fixture(scope="module")
def numbers():
    return RS.parse_pool()


def strings_of(pool, pk):
    return [pool.strings[p] for p in pk.tolist()]


# ------------------------------------------------------------------------------------------------ the pools
def test_the_string_pool_has_the_lengths_the_neighbours_and_two_copies_of_every_string(pool):
    assert 1500 <= pool.P <= 2500 and len(pool.ids) * 2 == pool.P
    data = pool.text.tobytes()
    assert [data[b:e] for b, e in zip(pool.rb.tolist(), pool.re.tolist())] == pool.strings
    distinct = [pool.strings[p] for p in pool.ids.tolist()]
    assert len(set(distinct)) == len(distinct) and set(RS.LENS) <= {len(s) for s in distinct}
    assert {int(b) % 16 for b in pool.rb} == set(range(16))
    gaps = np.sort(pool.rb)[1:] - np.sort(pool.re)[:-1]
    assert gaps.min() >= 0 and set(np.unique(gaps).tolist()) >= {0, 1, 2, 3}
    # strings that share everything but their last byte, that are a prefix of another, that differ once behind the first window
    have = set(distinct)
    assert sum(1 for s in distinct if len(s) > 16 and any(s[:-1] + bytes([c]) in have for c in range(97, 123) if c != s[-1])) >= 50
    assert sum(1 for s in distinct if len(s) > 16 and any(s[:n] in have for n in RS.LENS if RS.WINDOW <= n < len(s))) >= 50
    middle = 0
    for s in distinct:
        if len(s) > 16:
            middle += any(s[:at] + bytes([c]) + s[at + 1:] in have for at in (8, len(s) // 2) for c in range(97, 123) if c != s[at])
    assert middle >= 50
    # every string twice: equal bytes at another offset and another misalignment
    d = len(pool.ids)
    assert (pool.canon[d:] == np.arange(d)).all() and (pool.canon[:d] == np.arange(d)).all()
    assert ((pool.rb[d:] - pool.rb[:d]) % 16 != 0).all() and (pool.rb[d:] != pool.rb[:d]).all()


def test_the_parse_pool_holds_every_status_for_every_kind(numbers):
    assert numbers.strings == pc.all_case_rows() + pc.random_rows(900, 31) and 1500 <= numbers.P <= 2500
    assert {int(b) % 16 for b in numbers.rb} == set(range(16))
    data = numbers.text.tobytes()
    assert [data[b:e] for b, e in zip(numbers.rb.tolist(), numbers.re.tolist())] == numbers.strings
    for kind in pc.KINDS:
        for trim in (False, True):
            status, _ = numbers.parsed(kind, trim)
            assert set(status.tolist()) == {pc.OK, pc.EMPTY, pc.MALFORMED, pc.INEXACT if kind == pc.FLOAT64 else pc.RANGE}, (kind, trim)


# ------------------------------------------------------------------------------------------------ the picks
@pytest.mark.parametrize("k", RS.KS + RS.PARSE_KS[-1:])
def test_a_pick_places_its_three_single_strings_at_the_seam_and_at_the_last_row(pool, numbers, k):
    for which, pk in ((pool, RS.group_pick(pool, k)), (pool, RS.sort_pick(pool, k)), (pool, RS.lookup_picks(pool, k, k)[1]), (numbers, RS.parse_pick(numbers, k))):
        assert len(pk) == k and pk.min() >= 0 and pk.max() < which.P
        once = np.nonzero(np.bincount(which.canon[pk], minlength=which.P)[which.canon[pk]] == 1)[0].tolist()
        seam = K0 if k > K0 else 256
        assert once == sorted({seam - 1, seam, k - 1} - {k}), (k, once)
        assert (RS.pick(which, k, 77) != RS.pick(which, k, 78)).any() and (RS.pick(which, k, 77) == RS.pick(which, k, 77)).all()
        if which is pool:            # both copies of the strings are in use: equal rows at different addresses
            d = len(pool.ids)
            assert (pk < d).sum() > k // 4 and (pk >= d).sum() > k // 4


# ------------------------------------------------------------------------------------------------ the meanings, row by row
def group_by_rows(strings):
    seen, group, rep, count = {}, [], [], []
    for j, s in enumerate(strings):
        g = seen.get(s)
        if g is None:
            g = seen[s] = len(rep)
            rep.append(j)
            count.append(0)
        group.append(g)
        count[g] += 1
    return group, rep, count


def lookup_by_rows(set_strings, probe_strings, long_bytes):
    first = {}
    for i, s in enumerate(set_strings):
        first.setdefault(s, i)
    index = [first.get(s, -1) for s in probe_strings]
    hits = [0] * len(set_strings)
    for i in index:
        if i >= 0:
            hits[i] += 1
    stats = {"n_found": sum(1 for i in index if i >= 0), "n_set_distinct": len(first), "n_set_hit": sum(1 for h in hits if h),
             "long_rows": sum(1 for s in probe_strings if len(s) > long_bytes)}
    return index, hits, stats


def check_meanings(pool, numbers, k, kinds):
    took = {}
    pk = RS.group_pick(pool, k)
    strings = strings_of(pool, pk)
    t0 = time.perf_counter()
    got = RS.group_meaning(pool, pk)
    took["group"] = time.perf_counter() - t0
    assert [x.tolist() for x in got] == list(group_by_rows(strings)) and all(x.dtype == np.int64 for x in got)
    small = RS.group_small_pick(pool, k)
    assert [x.tolist() for x in RS.group_meaning(pool, small)] == list(group_by_rows(strings_of(pool, small)))

    pk = RS.sort_pick(pool, k)
    strings = strings_of(pool, pk)
    t0 = time.perf_counter()
    got = RS.sort_meaning(pool, pk)
    took["sort"] = time.perf_counter() - t0
    assert got.tolist() == sorted(range(k), key=lambda j: (strings[j], j)) and got.dtype == np.int64

    for ks, kp in ((k, k + 3), (min(k, 300), k)):
        set_pk, probe_pk = RS.lookup_picks(pool, ks, kp)
        for long_bytes in (64, RS.FORCED_LONG):
            t0 = time.perf_counter()
            index, hits, stats = RS.lookup_meaning(pool, set_pk, probe_pk, long_bytes)
            took["lookup"] = time.perf_counter() - t0
            w_index, w_hits, w_stats = lookup_by_rows(strings_of(pool, set_pk), strings_of(pool, probe_pk), long_bytes)
            assert index.tolist() == w_index and hits.tolist() == w_hits and stats == w_stats and index.dtype == hits.dtype == np.int64

    pk = RS.parse_pick(numbers, k)
    strings = strings_of(numbers, pk)
    memo = {}
    for kind, trim in kinds:
        t0 = time.perf_counter()
        status, bits, stats = RS.parse_meaning(numbers, pk, kind, trim)
        took["parse"] = time.perf_counter() - t0
        want = []
        for s in strings:            # (row by row; a string's meaning is worked out once)
            if s not in memo or (kind, trim) not in memo[s]:
                memo.setdefault(s, {})[(kind, trim)] = pc.meaning(s, kind, trim)
            want.append(memo[s][(kind, trim)])
        assert status.tolist() == [w[0] for w in want] and bits.tolist() == [w[1] for w in want], (kind, trim)
        assert stats == {name: sum(1 for w in want if w[0] == c) for c, name in enumerate(RS.PARSE_STATS)} and sum(stats.values()) == k
        assert status.dtype == np.uint8 and bits.dtype == np.uint64
    return took


@pytest.mark.parametrize("k", RS.SMALL_KS)
def test_meanings_equal_the_row_by_row_ones(pool, numbers, k):
    check_meanings(pool, numbers, k, [(kind, trim) for kind in pc.KINDS for trim in (False, True)])


def test_meanings_equal_the_row_by_row_ones_beyond_one_pass(pool, numbers):
    took = check_meanings(pool, numbers, BEYOND, [(pc.INT64, False), (pc.FLOAT64, True)])
    assert max(took.values()) < 2.0, took            # the builder's own share: a vectorised meaning is a few numpy lines


def test_one_string_tables_and_the_bad_index_list(pool):
    for s in (b"seventeen bytes !", b""):
        text, rb, re_ = RS.one_string_table(1001, s)
        data = text.tobytes()
        assert all(data[b:e] == s for b, e in zip(rb.tolist(), re_.tolist())) and len(set(rb.tolist())) == 2
        assert len(s) == 0 or (rb[0] - rb[1]) % 16 != 0
    pk = RS.group_pick(pool, RS.BAD_K)
    bad = RS.bad_index_list(pool, pk)
    differ = np.nonzero(bad != pk)[0].tolist()
    assert differ == list(RS.BAD_ROWS) and bad[differ[0]] == pool.P and bad[differ[1]] == -1
    # the two bad rows lie in the second and in the third pass of a capped unit grid, and in different workgroups' units
    assert [RS.units(r + 1) - 1 >= RS.UNIT_GRID_CAP * p for r, p in zip(RS.BAD_ROWS, (1, 2))] == [True, True]
    assert RS.BAD_ROWS[0] < 2 * K0 and RS.BAD_ROWS[1] < RS.BAD_K


# ------------------------------------------------------------------------------------------------ the sources' constants
def source_constants(frame, parse):
    """the three constants record_scale's row counts are derived from, read from the sources' text"""
    follow = ": tests/record_scale.py derives K0, KS and PARSE_KS from it -- record_scale.KS has to follow"
    m = re.search(r"inline unsigned unit_grid\(uint64_t n_units\)\s*\{\s*return static_cast<unsigned>\(n_units < 1 \? 1 : n_units < (\d+) \? n_units : (\d+)\);", frame)
    assert m, "record_frame.h: unit_grid() is not the capped grid it was" + follow
    assert m.group(1) == m.group(2) == str(RS.UNIT_GRID_CAP), "record_frame.h: unit_grid() caps at %s, not %d%s" % (m.group(2), RS.UNIT_GRID_CAP, follow)
    m = re.search(r"constexpr int kThreads = (\d+);", frame)
    assert m and int(m.group(1)) == RS.UNIT_ROWS, "record_frame.h: kThreads is not %d%s" % (RS.UNIT_ROWS, follow)
    m = re.search(r"constexpr unsigned kParseGrid = (\d+) \* (\d+);", parse)
    assert m and int(m.group(1)) * int(m.group(2)) == RS.PARSE_GRID, "record_parse.hip: kParseGrid is not %d%s" % (RS.PARSE_GRID, follow)
    assert re.search(r"dim3 block\(kThreads\), grid\(static_cast<unsigned>\(n_units < kParseGrid \? n_units : kParseGrid\)\);", parse), \
        "record_parse.hip: the parse kernel's grid is no longer min(n_units, kParseGrid)" + follow
    assert "record_parse_check_kernel, dim3(unit_grid(n_units))" in parse, "record_parse.hip: the check kernel no longer takes unit_grid()" + follow


def test_the_row_counts_follow_the_sources_constants():
    with open(os.path.join(CSRC, "record_frame.h")) as fh:
        frame = fh.read()
    with open(os.path.join(CSRC, "record_parse.hip")) as fh:
        parse = fh.read()
    source_constants(frame, parse)
    # the guard itself: an edited cap, unit or parse grid is seen, and the message says what has to follow
    for text, edited in ((frame, frame.replace("n_units < 1024 ? n_units : 1024", "n_units < 2048 ? n_units : 2048")),
                         (frame, frame.replace("kThreads = 256;", "kThreads = 512;")), (parse, parse.replace("kParseGrid = 256 * 8;", "kParseGrid = 256 * 4;"))):
        assert edited != text
        with pytest.raises(AssertionError, match="record_scale.KS has to follow"):
            source_constants(edited if text is frame else frame, edited if text is parse else parse)
    assert RS.KS == (K0, K0 + 1, K0 + 257, 2 * K0 + 65) and RS.PARSE_KS == (K0 + 1, 2 * K0, 2 * K0 + 1, 4 * K0 + 65) and K0 == 1024 * 256
    # the wave tier's stride at the capped grid: kWaves = kThreads / 64 waves per workgroup
    assert RS.WAVE_STRIDE == RS.UNIT_GRID_CAP * (RS.UNIT_ROWS // 64) == 4096


# ------------------------------------------------------------------------------------------------ what the GPU cases reach
def test_every_k_needs_more_than_one_pass(pool):
    for k in RS.KS:
        assert (RS.units(k) == RS.UNIT_GRID_CAP) if k == K0 else (RS.units(k) > RS.UNIT_GRID_CAP), k
    assert RS.units(RS.KS[1]) == RS.UNIT_GRID_CAP + 1 and RS.units(RS.KS[2]) == RS.UNIT_GRID_CAP + 2 and RS.units(RS.KS[3]) > 2 * RS.UNIT_GRID_CAP
    # parse: the check kernel's passes and the parse kernel's
    assert [RS.units(k) > RS.UNIT_GRID_CAP for k in RS.PARSE_KS] == [True] * 4
    assert [RS.units(k) - RS.PARSE_GRID for k in RS.PARSE_KS[:3]] == [-RS.UNIT_GRID_CAP + 1, 0, 1] and RS.units(RS.PARSE_KS[3]) > 2 * RS.PARSE_GRID
    for ks, kp in RS.LOOKUP_SIZES:
        assert RS.units(kp) > RS.UNIT_GRID_CAP and (ks == 300 or RS.units(ks) > RS.UNIT_GRID_CAP)
    assert RS.units(RS.BAD_K) > 2 * RS.UNIT_GRID_CAP


def test_the_sort_tables_keep_more_than_one_pass_open_behind_the_first_round(pool):
    """A row is listed in round 2 when it has WINDOW bytes and shares them with another row.  More than K0 such rows need
    more than K0 rows to begin with: for K0 and K0 + 1 (the pool has rows of 0 and 1 bytes, which close in round 1) the list
    still fills all 1024 units of one pass, for the two larger tables it goes round the capped grid again."""
    for k in RS.KS:
        pk = RS.sort_pick(pool, k)
        still_open = RS.open_after_round_one(pool, pk)
        assert still_open >= k - RS.SHORT_ROWS - 3 and RS.units(still_open) >= RS.UNIT_GRID_CAP, (k, still_open)
        if k >= K0 + 257:
            assert still_open > K0 and RS.units(still_open) > RS.UNIT_GRID_CAP, (k, still_open)
        # rows that are a proper prefix of another row's string, at WINDOW bytes or more, and occur twice: a third round
        strings = {pool.strings[p] for p in np.unique(pk).tolist()}
        assert sum(1 for s in strings if len(s) >= 2 * RS.WINDOW and any(s[:n] in strings for n in RS.LENS if RS.WINDOW <= n <= len(s) - RS.WINDOW)) >= 20


def test_the_wave_tier_goes_round_at_its_4096_wave_stride_with_16_bytes_forced(pool):
    tables = [("group", RS.group_pick(pool, k)) for k in RS.KS] + [("sort", RS.sort_pick(pool, k)) for k in RS.KS]
    for ks, kp in RS.LOOKUP_SIZES:
        set_pk, probe_pk = RS.lookup_picks(pool, ks, kp)
        tables += [("probe", probe_pk)] + ([("set", set_pk)] if ks >= K0 else [])      # (16 bytes are forced for the first pair only)
    for name, pk in tables:
        assert RS.longer_than(pool, pk, RS.FORCED_LONG) > RS.WAVE_STRIDE, name
        assert RS.longer_than(pool, pk, 64) > RS.WAVE_STRIDE, name                      # ... and without the knob: the rows of 700 bytes


def test_the_small_pool_and_the_lookup_sides(pool):
    small = RS.group_small_pick(pool, BEYOND)
    assert 30 <= len(np.unique(pool.canon[small])) <= RS.SMALL_POOL
    set_ids, probe_ids = RS.lookup_sides(pool)
    assert len(np.intersect1d(set_ids, probe_ids)) * 4 in range(len(pool.ids) - 4, len(pool.ids) + 5)
    for ks, kp in RS.LOOKUP_SIZES:
        set_pk, probe_pk = RS.lookup_picks(pool, ks, kp)
        index, hits, stats = RS.lookup_meaning(pool, set_pk, probe_pk)
        assert 0.10 * kp <= stats["n_found"] <= 0.90 * kp, (ks, kp, stats)
        assert stats["n_set_hit"] < stats["n_set_distinct"] and stats["n_set_hit"] > 0, stats
        # from the inputs alone: a set string that no probe row has
        assert len(np.setdiff1d(pool.canon[set_pk], pool.canon[probe_pk])) > 0
