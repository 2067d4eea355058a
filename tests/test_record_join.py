"""CPU tests of the record join (rejit_amd/csrc/record_join.h): the rule that hands a whole-text run's matches to the caller's
records, and the tile search record_join.hip's kernel makes for it.

The header is compiled with g++ into the test-only driver tests/support/record_exec.cc, which walks the table tile by tile as
the kernel does (one pair of searches per tile, the range staged when it fits, else every record searches the list).  The
expectation is a brute-force attribution in Python, straight from the rule's text: a match with begin b belongs to the LAST
record i with rec_begin[i] <= b, and is kept iff b <= rec_end[i]; a kept match whose end lies beyond rec_end[i] crosses.
Tiles of 1 .. 300 records; a staging capacity of 0, 1 and 7 begins forces the search in the list itself."""
import ctypes
import random

import pytest

from exec_build import headers, shared_driver

DEPS = headers(("record_join.h",))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
NONE = (1 << 64) - 1
TILES = (1, 2, 3, 7, 64, 256, 300)
CAPS = (0, 1, 7, 4096)


@pytest.fixture(scope="module")
def rx():
    lib = shared_driver("record_exec", DEPS)
    lib.re_join.restype = ctypes.c_long
    lib.re_join.argtypes = [_u64p, ctypes.c_uint64, _u64p, _u64p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                            _u32p, _u64p, _u64p]
    lib.re_saturate32.restype = ctypes.c_uint32
    lib.re_saturate32.argtypes = [ctypes.c_uint64]
    return lib


def join(lib, spans, records, n, tile, cap):
    """-> (counts, first, kept, matching, crossing, first bad row or None, staged tiles, list tiles)"""
    m, k = len(spans), len(records)
    sp = (ctypes.c_uint64 * max(2 * m, 1))(*[x for be in spans for x in be])
    rb = (ctypes.c_uint64 * max(k, 1))(*[b for b, _ in records])
    re_ = (ctypes.c_uint64 * max(k, 1))(*[e for _, e in records])
    counts = (ctypes.c_uint32 * max(k, 1))(*([0xDEADBEEF] * max(k, 1)))   # (nothing is cleared for the join: it writes every row)
    first = (ctypes.c_uint64 * max(k, 1))(*([NONE] * max(k, 1)))
    summ = (ctypes.c_uint64 * 6)()
    assert lib.re_join(sp, m, rb, re_, k, n, tile, cap, counts, first, summ) == 0, "a search left its range"
    bad = None if summ[3] == NONE else int(summ[3])
    return list(counts)[:k], list(first)[:k], int(summ[0]), int(summ[1]), int(summ[2]), bad, int(summ[4]), int(summ[5])


def brute(spans, records):
    """The rule, literally.  -> (counts, first or None per record, kept, matching, crossing)"""
    counts = [0] * len(records)
    first = [None] * len(records)
    crossing = 0
    for k, (b, e) in enumerate(spans):
        rec = None
        for i, (rb, _) in enumerate(records):
            if rb <= b:
                rec = i          # the LAST record that begins at or before b
        if rec is None or b > records[rec][1]:
            continue             # before the first record, or in a gap
        if counts[rec] == 0:
            first[rec] = k
        counts[rec] += 1
        crossing += e > records[rec][1]
    return counts, first, sum(counts), sum(c > 0 for c in counts), crossing


def check(lib, spans, records, n, tiles=TILES, caps=CAPS):
    want_counts, want_first, kept, matching, crossing = brute(spans, records)
    lb = lambda x: sum(1 for b, _ in spans if b < x)
    seen_staged = seen_list = 0
    for tile in tiles:
        for cap in caps:
            counts, first, g_kept, g_matching, g_crossing, bad, staged, listed = join(lib, spans, records, n, tile, cap)
            ctx = (tile, cap, spans[:6], records[:6])
            assert bad is None, ctx
            assert counts == want_counts, ctx
            # a record without a match still gets first = lb(rec_begin): where its matches would be
            assert first == [lb(rb) if w is None else w for w, (rb, _) in zip(want_first, records)], ctx
            assert (g_kept, g_matching, g_crossing) == (kept, matching, crossing), ctx
            seen_staged += staged
            seen_list += listed
    return seen_staged, seen_list


def random_case(rng, base=0):
    """Records with empty ones, a leading gap, gaps of several bytes and touching seams; a non-overlapping ascending match list
    with empty matches on seams and record ends, matches inside gaps and matches that cross their record's end."""
    k = rng.choice([1, 2, 5, 40, 300, 700])
    at = base + rng.choice([0, 0, 1, 9])
    records = []
    for _ in range(k):
        size = rng.choice([0, 0, 1, 2, 5, 30])
        records.append((at, at + size))
        at += size + rng.choice([0, 0, 1, 1, 4])
    n = at + rng.choice([0, 3])
    spans, p = [], base
    density = rng.choice([0.05, 0.4, 1.5])
    while p <= n:
        if rng.random() < density:
            length = rng.choice([0, 0, 1, 1, 2, 7])
            e = min(p + length, n)
            spans.append((p, e))
            p = e if e > p else p + 1    # (left-most longest, non-overlapping: an empty match moves the start on by one)
        else:
            p += 1
    return spans, records, n


def test_random_tables_equal_the_brute_force_rule(rx):
    rng = random.Random(20)
    staged = listed = crossing = gaps = 0
    for _ in range(60):
        spans, records, n = random_case(rng)
        s, l = check(rx, spans, records, n, tiles=rng.sample(TILES, 3))
        staged += s
        listed += l
        c, _, kept, _, cr = brute(spans, records)
        crossing += cr
        gaps += len(spans) - kept
    assert staged and listed and crossing and gaps      # both branches of the tile search, crossing matches, matches in gaps


def test_the_seams_one_by_one(rx):
    # touching records, an empty match on the seam: the NEXT record's
    assert brute([(5, 5)], [(0, 5), (5, 9)])[0] == [0, 1]
    check(rx, [(5, 5)], [(0, 5), (5, 9)], 9)
    # a gap behind the record: an empty match at rec_end is the record's own, one inside the gap nobody's
    assert brute([(5, 5), (6, 6)], [(0, 5), (7, 9)])[0] == [1, 0]
    check(rx, [(5, 5), (6, 6)], [(0, 5), (7, 9)], 9)
    # a match beginning at rec_end before a gap and running into it: kept, and crossing
    assert brute([(5, 7)], [(0, 5), (8, 9)])[2:] == (1, 1, 1)
    check(rx, [(5, 7)], [(0, 5), (8, 9)], 9)
    # a leading gap, a match across two touching records (it is the first one's and crosses), empty records in a row
    check(rx, [(0, 1), (3, 8), (8, 8)], [(2, 6), (6, 8), (8, 8), (8, 8), (8, 12)], 12)
    assert brute([(0, 1), (3, 8), (8, 8)], [(2, 6), (6, 8), (8, 8), (8, 8), (8, 12)]) == ([1, 0, 0, 0, 1], [1, None, None, None, 2], 2, 2, 1)
    # the empty match at the very end of the text
    check(rx, [(12, 12)], [(0, 12)], 12)
    check(rx, [(12, 12)], [(0, 11)], 12)


def test_no_matches_and_no_records(rx):
    check(rx, [], [(0, 3), (3, 3), (5, 9)], 9)
    counts, first, kept, matching, crossing, bad, staged, listed = join(rx, [(1, 2)], [], 5, 4, 7)
    assert (counts, first, kept, matching, crossing, bad, staged + listed) == ([], [], 0, 0, 0, None, 0)
    check(rx, [], [], 0)


def test_one_record_with_more_matches_than_the_stage(rx):
    spans = [(3 * i, 3 * i + 2) for i in range(500)]
    records = [(0, 10), (10, 1400), (1400, 1500)]
    staged, listed = check(rx, spans, records, 1500, tiles=(1, 2, 300), caps=(0, 7, 100, 4096))
    assert staged and listed


def test_offsets_beyond_32_bits(rx):
    """Synthetic numbers, no text: begins, ends and the table above 2^32 and 2^40."""
    rng = random.Random(7)
    for base in ((1 << 32) - 40, (1 << 40) + 5, (1 << 63) - 10000):
        for _ in range(6):
            spans, records, n = random_case(rng, base=base)
            check(rx, spans, records, n, tiles=(3, 256), caps=(1, 4096))
    assert rx.re_saturate32((1 << 32) - 1) == 0xFFFFFFFF and rx.re_saturate32(1 << 32) == 0xFFFFFFFF and rx.re_saturate32(1 << 40) == 0xFFFFFFFF
    assert rx.re_saturate32(0xFFFFFFFE) == 0xFFFFFFFE


@pytest.mark.parametrize("records,n,want", [
    ([(0, 3), (10, 12), (5, 7), (20, 22)], 30, 1),      # descending begins: row 1's end lies beyond row 2's begin
    ([(0, 3), (4, 9), (8, 12)], 30, 1),                 # overlapping
    ([(0, 3), (7, 5), (9, 12)], 30, 1),                 # end < begin
    ([(0, 3), (4, 5), (9, 31)], 30, 2),                 # end > n
    ([(5, 4)], 30, 0),
    ([(0, 3)] + [(4, 4)] * 400 + [(3, 3), (9, 9)], 30, 400),   # the first bad row of several, deep inside the table
    ([(0, 3), (9, 12), (9, 8), (2, 1)], 30, 1),
])
def test_bad_tables_report_their_first_bad_row(rx, records, n, want):
    spans = [(1, 2), (4, 4), (9, 11), (29, 30)]
    for tile in TILES:
        for cap in CAPS:
            bad = join(rx, spans, records, n, tile, cap)[5]   # (and no search left the list: join() asserts that)
            assert bad == want, (tile, cap)
