"""CPU tests of the record split (rejit_amd/csrc/record_split.h): the arithmetic of rj_scan_records_split -- the fields (the
pieces between a record's own matches) or the matches of the chosen records as a piece table with Arrow-style offsets.

The header is compiled with g++ into the test-only driver tests/support/split_exec.cc, which walks the plan unit by unit and
the emit chunk by chunk as record_split.hip's kernels do, every access checked against its range and every row written at
most once.  The expectation is the meaning written out literally in Python, a loop over each row's own matches:
    between: piece t of row j = [t == 0 ? rb : e_{t-1}, t == c ? re : b_t), c + 1 of them
    matches: piece t of row j = [b_t, e_t), c of them
    piece_first[0] = 0, piece_first[j + 1] = piece_first[j] + (pieces of row j)
counts / first come from the join rule of record_join.h written out in Python (test_record_replace.join).  Units of 1, 3 and
256 rows, chunks of 1, 3, 16 and 4096 pieces, a stage of 0, 1, 7 and 1024 rows; the tables are poisoned with 0xA5 first."""
import ctypes
import random
import subprocess

import pytest

from exec_build import _arr, headers, sanitized_program, shared_driver
from test_record_replace import RECORDS, SPANS, join, splice

DEPS = headers(("record_split.h", "record_replace.h", "record_pack.h"), ("checked_table.h",))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
NONE = (1 << 64) - 1
SAT = (1 << 32) - 1
POISON = 0xA5A5A5A5A5A5A5A5
UNITS = (1, 3, 256)
CHUNKS = (1, 3, 16, 4096)
CAPS = (0, 1, 7, 1024)
BETWEEN, MATCHES = 0, 1
OK, BAD_INDEX, BAD_ROW, SATURATED, BAD_RANGE, BEGINS_BEFORE, CROSSES = range(7)      # replace::Kind


@pytest.fixture(scope="module")
def sx():
    lib = shared_driver("split_exec", DEPS)
    u64 = ctypes.c_uint64
    lib.sp_split.restype = ctypes.c_long
    lib.sp_split.argtypes = [u64, _u64p, _u64p, u64, _u32p, _u64p, _u64p, u64, _u64p, ctypes.c_int, u64, ctypes.c_int, u64, u64, u64, _u64p, _u64p, _u64p,
                             u64, _u64p]
    lib.sp_sums_fit.argtypes = [u64, u64]
    return lib


def pieces_of(rb, re_, own, what):
    """The meaning, literally: the pieces of one record with its own matches"""
    if what == MATCHES:
        return [(b, e) for b, e in own]
    out, pos = [], rb
    for b, e in own:
        out.append((pos, b))
        pos = e
    return out + [(pos, re_)]


def brute(records, spans, counts, first, indices, what):
    """-> (pieces, piece_first)"""
    rows = range(len(records)) if indices is None else indices
    pieces, pf = [], []
    for r in rows:
        pf.append(len(pieces))
        pieces += pieces_of(records[r][0], records[r][1], spans[first[r]:first[r] + counts[r]], what)
    return pieces, pf + [len(pieces)]


def run(lib, n, records, spans, counts, first, indices, what, unit, chunk, cap, piece_cap=None, room=None, offsets=True):
    """-> (rc, P, first bad row or None, its kind, piece_begin, piece_end (the whole poisoned buffers), piece_first, summary)"""
    k = len(records) if indices is None else len(indices)
    rb, re_ = _arr([b for b, _ in records]), _arr([e for _, e in records])
    flat = _arr([x for s in spans for x in s])
    idx = None if indices is None else _arr(indices)
    if room is None:
        room = (piece_cap or 0) + 4
    if piece_cap is None:
        piece_cap = room - 4
    pb, pe = _arr([POISON] * room), _arr([POISON] * room)
    pf = _arr([POISON] * (k + 3)) if offsets else None
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.sp_split(n, rb, re_, len(records), _arr(counts, ctypes.c_uint32), _arr(first), flat, len(spans), idx, int(indices is not None),
                      0 if indices is None else len(indices), what, unit, chunk, cap, pf, pb, pe, piece_cap, summ)
    bad = None if summ[1] == NONE else int(summ[1])
    return rc, int(summ[0]), bad, int(summ[2]), list(pb), list(pe), (list(pf) if offsets else None), [int(x) for x in summ]


def check(lib, n, records, spans, indices=None, whats=(BETWEEN, MATCHES), units=UNITS, chunks=CHUNKS, caps=CAPS, piece_caps=(None,), joined=None):
    counts, first = joined if joined is not None else join(records, spans)
    k = len(records) if indices is None else len(indices)
    seen = [0] * 8
    for what in whats:
        want, w_pf = brute(records, spans, counts, first, indices, what)
        for unit in units:
            for chunk in chunks:
                for cap in caps:
                    for piece_cap in piece_caps:
                        pc = len(want) + 3 if piece_cap is None else piece_cap
                        rc, total, bad, _, pb, pe, pf, summ = run(lib, n, records, spans, counts, first, indices, what, unit, chunk, cap, piece_cap=pc)
                        ctx = (what, unit, chunk, cap, piece_cap, records[:6], None if indices is None else indices[:6])
                        assert rc == 0, ("an access left its range, or a row was written twice", ctx)
                        assert bad is None and total == len(want), ctx                  # P comes back whatever piece_cap is
                        limit = min(pc, len(want))
                        assert list(zip(pb[:limit], pe[:limit])) == want[:limit], ctx
                        assert pb[limit:] == [POISON] * (len(pb) - limit) and pe[limit:] == [POISON] * (len(pe) - limit), ctx
                        assert pf[:k + 1] == w_pf and pf[k + 1:] == [POISON, POISON], ctx
                        seen = [a + b for a, b in zip(seen, summ)]
        # without the caller's offsets (the emit then reads the driver's own) the pieces are the same
        rc, total, _, _, pb, pe, _, _ = run(lib, n, records, spans, counts, first, indices, what, units[-1], chunks[0], caps[-1], piece_cap=len(want),
                                            offsets=False)
        assert rc == 0 and total == len(want) and list(zip(pb[:total], pe[:total])) == want and pb[total:] == [POISON] * 4
    return seen


def test_the_hand_made_table_every_kind_of_match(sx):
    """test_record_replace's table: matches at a record's first and last byte, matches that touch, empty matches at the begin,
    in the middle and at the end of a record, a record that is one match, empty records, 40 matches in one record."""
    seen = check(sx, 260, RECORDS, SPANS)
    assert seen[3] and seen[4], seen                                            # staged chunks and chunks that searched the table
    counts, first = join(RECORDS, SPANS)
    pieces, pf = brute(RECORDS, SPANS, counts, first, None, BETWEEN)
    assert pf[1] - pf[0] == 7 and pieces[0] == (3, 3) and pieces[6] == (43, 43)      # a match at the first / last byte: an empty field
    assert pieces[pf[0] + 4] == (37, 37)                                             # two matches that touch
    assert pieces[pf[1]:pf[2]] == [(43, 43), (59, 59)]                               # a record that is one match: two empty fields
    assert pieces[pf[4]:pf[5]] == [(62, 62), (62, 62)]                               # an empty record's own empty match
    assert pieces[pf[10]:pf[11]] == [(203, 203), (203, 250), (250, 250)]             # empty matches at the record's begin and end cut there
    pieces, pf = brute(RECORDS, SPANS, counts, first, None, MATCHES)
    assert pf[2] == pf[3] and pf[9] - pf[8] == 40 and len(pieces) == sum(counts)


def test_rows_with_0_1_2_and_5000_matches_among_match_less_and_empty_records(sx):
    n = 15000
    lens = (1, 0, 2)
    big = [(100 + 3 * i, 100 + 3 * i + lens[i % 3]) for i in range(5000)]
    records = [(2, 2)] * 300 + [(10, 30), (30, 50), (50, 90)] + [(95, 95)] * 3 + [(100, 100 + n)] + [(100 + n + 3, 100 + n + 3)] * 300 + [(100 + n + 10, 100 + n + 20)]
    spans = [(35, 36), (50, 51), (89, 90)] + big + [(100 + n + 12, 100 + n + 13)]
    counts, first = join(records, spans)
    assert [counts[i] for i in (300, 301, 302, 306)] == [0, 1, 2, 5000]
    seen = check(sx, 100 + n + 20, records, spans, units=(3, 256), chunks=(1, 16, 4096), caps=(0, 7, 1024))
    assert seen[3] and seen[4], seen


def test_indices_as_a_permutation_and_as_a_take_with_repeats(sx):
    rng = random.Random(3)
    perm = list(range(len(RECORDS)))
    rng.shuffle(perm)
    check(sx, 260, RECORDS, SPANS, indices=perm, units=(3, 256))
    check(sx, 260, RECORDS, SPANS, indices=[8, 8, 0, 4, 8, 10, 10, 1, 4, 2, 2], units=(1, 256))
    # k == 0: indices non-NULL with 0 rows, and no records at all -- piece_first[0] = 0 is still written
    check(sx, 260, RECORDS, SPANS, indices=[], units=(3,), chunks=(1, 16))
    check(sx, 260, [], [], units=(3,), chunks=(1, 16))
    check(sx, 260, [], SPANS, units=(256,), chunks=(16,))


def test_piece_cap_inside_a_row_at_a_row_boundary_and_the_size_query(sx):
    counts, first = join(RECORDS, SPANS)
    for what in (BETWEEN, MATCHES):
        want, pf = brute(RECORDS, SPANS, counts, first, None, what)
        caps = (0, 1, pf[1] - 1, pf[1], pf[1] + 1, pf[8], pf[8] + 17, pf[9], len(want) - 1, len(want), len(want) + 50)
        check(sx, 260, RECORDS, SPANS, whats=(what,), piece_caps=caps, units=(3,), caps=(0, 1024))
        # the size query: no piece row at all, the offsets still written
        rc, total, bad, _, pb, pe, got_pf, _ = run(sx, 260, RECORDS, SPANS, counts, first, None, what, 3, 16, 7, piece_cap=0, room=8)
        assert rc == 0 and bad is None and total == len(want) and got_pf[:len(RECORDS) + 1] == pf and pb == [POISON] * 8 and pe == [POISON] * 8


def test_a_foreign_match_belongs_to_no_row(sx):
    """A match that begins in a gap is no record's: it cuts no field and is nobody's match.  So with a match the row's count
    leaves out."""
    records = [(0, 10), (13, 30), (30, 50)]
    spans = [(2, 4), (11, 16), (20, 22), (35, 36), (40, 44)]
    counts, first = join(records, spans)
    assert counts == [1, 1, 2] and first == [0, 2, 3]
    check(sx, 60, records, spans)
    pieces, _ = brute(records, spans, counts, first, None, BETWEEN)
    assert pieces == [(0, 2), (4, 10), (13, 20), (22, 30), (30, 35), (36, 40), (44, 50)]
    check(sx, 60, records, spans, joined=([1, 1, 1], [0, 2, 3]))
    check(sx, 60, records, spans, joined=([0, 0, 1], [0, 0, 4]))


@pytest.mark.parametrize("why,want,kind", [
    ("an index == n_records", 2, BAD_INDEX),
    ("end < begin", 1, BAD_ROW),
    ("end > n", 3, BAD_ROW),
    ("first + count > m", 2, BAD_RANGE),
    ("first > m", 0, BAD_RANGE),
    ("a saturated count", 1, SATURATED),
    ("the first match begins before the record", 2, BEGINS_BEFORE),
    ("the last match ends beyond the record", 1, CROSSES),
    ("two bad rows", 1, CROSSES),
    ("a bad row reached through the indices only at j = 4", 4, BAD_RANGE),
    ("... and not reached at all", None, OK),
])
def test_refusals_name_the_first_bad_row_and_no_piece_row_is_written(sx, why, want, kind):
    n = 100
    records = [(0, 20), (20, 45), (50, 70), (70, 100)]
    spans = [(5, 6), (30, 32), (40, 45), (55, 56), (80, 90)]
    counts, first = join(records, spans)
    m = len(spans)
    indices = None
    if why == "an index == n_records":
        indices = [0, 1, 4, 2]
    elif why == "end < begin":
        records[1] = (20, 19)
    elif why == "end > n":
        records[3] = (70, 101)
    elif why == "first + count > m":
        counts[2] = m - first[2] + 1
    elif why == "first > m":
        first[0], counts[0] = m + 1, 0
    elif why == "a saturated count":
        counts[1] = SAT
    elif why == "the first match begins before the record":
        first[2] -= 1
    elif why == "the last match ends beyond the record":
        records[1] = (20, 44)
    elif why == "two bad rows":
        records[1] = (20, 44)
        counts[3] = SAT
    elif why.startswith("a bad row reached") or why.startswith("..."):
        counts[3] = 9
        indices = [0, 1, 2, 0, 3] if why.startswith("a bad row") else [0, 1, 2, 0]
    for what in (BETWEEN, MATCHES):
        for unit in UNITS:
            for chunk in (1, 4096):
                for cap in (0, 1024):
                    rc, _, bad, got_kind, pb, pe, _, _ = run(sx, n, records, spans, counts, first, indices, what, unit, chunk, cap, piece_cap=64)
                    assert rc == 0, "an access left its range"
                    assert bad == want and got_kind == kind, (why, what, unit, chunk, cap)
                    if want is not None:
                        assert pb == [POISON] * len(pb) and pe == [POISON] * len(pe)          # a refused call writes no piece row


def test_a_hand_made_list_with_offsets_beyond_2_to_the_32(sx):
    base = (1 << 32) + 5
    n = (1 << 40) + 100
    records = [(3, 9), (base, base + 100), (base + 100, 1 << 40), ((1 << 40) + 1, (1 << 40) + 1)]
    spans = [(4, 5), (base, base + 1), (base + 50, base + 50), (base + 99, base + 100), ((1 << 33), (1 << 34)), ((1 << 40) - 1, 1 << 40), ((1 << 40) + 1, (1 << 40) + 1)]
    counts, first = join(records, spans)
    assert counts == [1, 3, 2, 1]
    check(sx, n, records, spans, units=(3, 256), chunks=(1, 16), caps=(0, 1024))
    check(sx, n, records, spans, indices=[3, 2, 2, 1, 0], units=(1,), chunks=(3,), caps=(1, 7))


def test_the_bounds_on_the_sums_at_their_edges(sx):
    f = sx.sp_sums_fit                                    # (k, m)
    assert f(40 << 20, 1 << 28) == 1                      # 40 M lines, 2^28 matches
    assert f((1 << 60) - 1, 0) == 1 and f(1 << 60, 0) == 0                           # the row number shares a word with its kind
    assert f((1 << 60) - 1, 3) == 1 and f((1 << 60) - 1, 4) == 0                     # k * (m + 1) < 2^62
    assert f(1 << 30, (1 << 32) - 2) == 1 and f(1 << 30, (1 << 32) - 1) == 0        # 2^62 - 2^30 / 2^62
    assert f(1, (1 << 62) - 2) == 1 and f(1, (1 << 62) - 1) == 0
    assert f(0, (1 << 62) - 1) == 1 and f(0, 1 << 62) == 0 and f(3, NONE) == 0
    # the driver refuses what the call refuses
    assert run(sx, 10, [(0, 5)], [], [0], [0], None, 2, 3, 16, 7, piece_cap=4)[0] == -2       # what outside {0, 1}


def _random_table(rng):
    k = rng.choice([1, 2, 9, 70, 300])
    records, spans, at = [], [], rng.choice([0, 1, 9])
    for _ in range(k):
        size = rng.choice([0, 0, 1, 2, 15, 16, 17, 31, 100])
        seam = rng.choice([0, 0, 1, 4])
        records.append((at, at + size))
        pos = at + rng.choice([0, 0, 1, 5])
        dense = rng.random() < 0.5
        while pos <= at + size and rng.random() < (0.95 if dense else 0.6):
            ln = min(rng.choice([0, 1, 1, 2, 16, 100]), at + size - pos)
            if spans and spans[-1] == (pos, pos):
                break
            if ln == 0 and pos == at + size and seam == 0:
                break       # (it would be the next record's by the rule; the next record plants its own)
            spans.append((pos, pos + ln))
            pos += ln + (rng.choice([1, 3]) if ln == 0 else rng.choice([0, 0, 1, 7]))
        at += size + seam
    return records, spans, at + rng.choice([0, 3])


def test_random_tables_equal_the_brute_force(sx):
    rng = random.Random(11)
    seen = [0] * 8
    for _ in range(60):
        records, spans, n = _random_table(rng)
        k = len(records)
        indices = None if rng.random() < 0.5 else [rng.randrange(k) for _ in range(rng.choice([0, 1, k, 2 * k]))]
        s = check(sx, n, records, spans, indices=indices, units=(rng.choice(UNITS),), chunks=rng.sample(CHUNKS, 2), caps=rng.sample(CAPS, 2))
        seen = [a + b for a, b in zip(seen, s)]
    assert seen[3] and seen[4], seen


def test_joining_a_rows_fields_with_the_replacement_is_the_replace(sx):
    """with.join(pieces of row j) == R(r(j)), test_record_replace's splice -- the BETWEEN pieces are what the replace copies as
    text -- with the pieces taken from the driver."""
    rng = random.Random(29)
    for _ in range(20):
        records, spans, n = _random_table(rng)
        text = bytes(rng.randrange(32, 127) for _ in range(n))
        counts, first = join(records, spans)
        k = len(records)
        indices = None if rng.random() < 0.5 else [rng.randrange(k) for _ in range(k + 2)]
        rows = list(range(k)) if indices is None else indices
        rc, total, bad, _, pb, pe, pf, _ = run(sx, n, records, spans, counts, first, indices, BETWEEN, 256, 16, 7, piece_cap=len(rows) + len(spans) * 3 + 4)
        assert rc == 0 and bad is None
        for repl in (b"", b"#", b"<with>"):
            for j, r in enumerate(rows):
                joined = repl.join(text[pb[p]:pe[p]] for p in range(pf[j], pf[j + 1]))
                assert joined == splice(text, records[r][0], records[r][1], spans[first[r]:first[r] + counts[r]], repl), (j, r, repl)


def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: a fixed set of cases against the meaning written out in C++, exact allocations.  (The sanitizers' runtimes
    are linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("split_exec", DEPS)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"96 cases" in r.stdout
