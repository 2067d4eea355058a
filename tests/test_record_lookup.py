"""CPU tests of the record lookup (rejit_amd/csrc/record_lookup.h on top of record_group.h): the arithmetic of
rj_scan_records_lookup -- the rows of one record table looked up in the rows of another, each over a text of its own -- and
of records.join_rows.

The header is compiled with g++ into the test-only driver tests/support/lookup_exec.cc, which builds the table with the
group's functions (the set rows inserted ONE AT A TIME in an order the test chooses), then visits the probe rows in an order
and in units the test chooses through record_lookup.h's read-only walk, every access checked against its range and every
write to the table behind the build an error.  The expectation is a Python dict over the rows' bytes:
    index[j] = the first set row with probe row j's string, or NONE;  hits[i] = the probe rows that found set row i.
The answer must be the same for every insert order, probe order, unit size and number of hash bits.  All comparisons are exact."""
import ctypes
import random
import subprocess

import pytest

from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_lookup.h", "record_group.h", "record_rows.h", "record_pack.h"), ("checked_text.h", "checked_table.h"))
_u64p = ctypes.POINTER(ctypes.c_uint64)
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
ROOM = 3
BITS = (0, 1, 4, 64)
UNITS = (1, 3, 64, 256)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33)


@pytest.fixture(scope="module")
def lx():
    lib = shared_driver("lookup_exec", DEPS)
    u64, u32, cp, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int
    lib.lk_rows_fit.argtypes = [u64, u64]
    lib.lk_layout.restype = None
    lib.lk_layout.argtypes = [u64, u64, _u64p]
    lib.lk_rows_equal.restype = ctypes.c_long
    lib.lk_rows_equal.argtypes = [cp, u64, u64, cp, u64, u64, u64, u64]
    lib.lk_lookup.restype = ctypes.c_long
    lib.lk_lookup.argtypes = [cp, u64, _u64p, _u64p, u64, _u64p, ci, u64, cp, u64, _u64p, _u64p, u64, _u64p, ci, u64, u32, _u64p, _u64p, u64, ci, ci,
                              _u64p, _u64p, _u64p]
    return lib


class Table:
    """a text, its records as (begin, end) pairs, and an optional index list"""

    def __init__(self, text, records, indices=None):
        self.text, self.records, self.indices = text, records, indices

    def rows(self):
        return range(len(self.records)) if self.indices is None else self.indices

    def k(self):
        return len(self.records) if self.indices is None else len(self.indices)

    def row(self, r):
        return self.text[self.records[r][0]:self.records[r][1]]


def meaning(S, P):
    """the dict -> (index, hits, n_found, n_set_distinct, n_set_hit)"""
    first = {}
    for i, r in enumerate(S.rows()):
        first.setdefault(S.row(r), i)
    index, hits = [], [0] * S.k()
    for r in P.rows():
        i = first.get(P.row(r), NONE)
        index.append(i)
        if i != NONE:
            hits[i] += 1
    return index, hits, sum(hits), len(first), sum(1 for h in hits if h)


def run(lib, S, P, bits=64, insert_order=None, probe_order=None, unit=256, want_hits=True, peel=True):
    """-> (rc, summary, index, hits: the whole poisoned buffers)"""
    ks, kp = S.k(), P.k()
    io = list(range(ks)) if insert_order is None else insert_order
    po = list(range(kp)) if probe_order is None else probe_order
    index, hits = _arr([POISON] * (kp + ROOM)), _arr([POISON] * (ks + ROOM))
    summ = (ctypes.c_uint64 * 8)()

    def side(T):
        idx = None if T.indices is None else _arr(T.indices)
        return (T.text, len(T.text), _arr([b for b, _ in T.records]), _arr([e for _, e in T.records]), len(T.records), idx, int(T.indices is not None),
                0 if T.indices is None else len(T.indices))
    rc = lib.lk_lookup(*side(S), *side(P), bits, _arr(io), _arr(po), unit, int(want_hits), int(peel), index, hits if want_hits else None, summ)
    return rc, [int(x) for x in summ], list(index), list(hits)


def check(lib, S, P, bits=BITS, insert_orders=(None,), probe_orders=(None,), units=(256,), peels=(True,)):
    ks, kp = S.k(), P.k()
    w_index, w_hits, w_found, w_distinct, w_hit = meaning(S, P)
    for b in bits:
        for io in insert_orders:
            for po in probe_orders:
                for unit in units:
                    for peel in peels:
                        for want_hits in (True, False):
                            rc, summ, index, hits = run(lib, S, P, b, io, po, unit, want_hits, peel)
                            ctx = (b, unit, peel, want_hits, ks, kp)
                            assert rc == 0, ("an access left its range, a row was written twice or the probe wrote the table", rc, ctx)
                            assert summ[1] == NONE and summ[2] == NONE and summ[0] == w_found, (ctx, summ)
                            assert index[:kp] == w_index and index[kp:] == [POISON] * ROOM, ctx
                            if want_hits:
                                assert hits[:ks] == w_hits and hits[ks:] == [POISON] * ROOM, ctx
                                assert summ[3] == w_distinct and summ[4] == w_hit and sum(w_hits) == w_found, ctx
                            else:
                                assert hits == [POISON] * (ks + ROOM), ctx
    return w_index, w_hits


def _lay(strings, lead=b"", sep_of=lambda i: b"|" * (i % 4), tail=b""):
    """the strings laid out one after another -> (text, records)"""
    text, records = lead, []
    for i, s in enumerate(strings):
        text += sep_of(i)
        records.append((len(text), len(text) + len(s)))
        text += s
    return text + tail, records


def _orders(rng, k, count):
    out = [None, list(range(k - 1, -1, -1))]
    for _ in range(count):
        o = list(range(k))
        rng.shuffle(o)
        out.append(o)
    return out


# ------------------------------------------------------------------------------------------------ the compare across two texts
def test_equal_strings_at_every_alignment_in_two_different_texts(lx):
    """One string of every length at offsets 0..15 in the set text and 0..15 in the probe text, the two texts of different
    lengths and different filler bytes: equal, with the groups dealt to 1, 3 and 64 lanes; one changed byte: different."""
    rng = random.Random(1)
    for ln in LENGTHS + (1023, 1024, 1025):
        row = bytes(rng.randrange(1, 256) for _ in range(ln))
        for a in range(16):
            set_text = b"\xA5" * a + row + b"\xA5" * 40
            for b in (0, 5, 15) if ln > 33 else range(16):
                text = b"\x00" * b + row                                  # the probe row ends at its text's last byte
                for lanes in (1, 3, 64):
                    assert lx.lk_rows_equal(set_text, len(set_text), a, text, len(text), b, ln, lanes) == 1, (ln, a, b, lanes)
                    assert lx.lk_rows_equal(text, len(text), b, set_text, len(set_text), a, ln, lanes) == 1     # ... and the set row at ITS text's end
                if ln:
                    for at in sorted({0, ln // 2, ln - 1}):
                        other = bytearray(row)
                        other[at] ^= 0x40
                        text2 = b"\xFF" * b + bytes(other)
                        assert lx.lk_rows_equal(set_text, len(set_text), a, text2, len(text2), b, ln, 1) == 0, (ln, a, b, at)
                        assert lx.lk_rows_equal(text2, len(text2), b, set_text, len(set_text), a, ln, 64) == 0


def test_alignments_and_text_ends_through_the_whole_lookup(lx):
    """The same strings at offsets 0..15 in two different texts; the last set row ends at the set text's last byte and the
    last probe row at the probe text's (the guarded loads), the texts' lengths differ."""
    rng = random.Random(2)
    strings = [bytes(rng.choice(b"abc") for _ in range(ln)) for ln in LENGTHS if ln]
    for off in range(16):
        set_text, set_rec = _lay(strings, lead=b"#" * off, sep_of=lambda i: b"|" * ((i * 5) % 16))
        text, rec = _lay(list(reversed(strings)) + [strings[0] + b"x"], lead=b"~" * (3 * off + 7), sep_of=lambda i: b"~" * ((i * 3) % 16))
        assert set_rec[-1][1] == len(set_text) and rec[-1][1] == len(text) and len(set_text) != len(text)
        w_index, _ = check(lx, Table(set_text, set_rec), Table(text, rec), units=(1, 256))
        assert w_index == list(range(len(strings) - 1, -1, -1)) + [NONE]


def test_a_zero_byte_is_a_byte_and_empty_rows_are_equal(lx):
    set_text, set_rec = _lay([b"ab", b"", b"ab\0", b"\0"], sep_of=lambda i: b"|")
    text, rec = _lay([b"ab\0", b"ab", b"\0", b"", b"a", b"ab\0\0", b""], sep_of=lambda i: b"\0")     # zero bytes around the rows, too
    w_index, w_hits = check(lx, Table(set_text, set_rec), Table(text, rec), units=UNITS)
    assert w_index == [2, 0, 3, 1, NONE, NONE, 1] and w_hits == [1, 2, 1, 1]
    # "ab" in a set of {"ab\0"} only, "" in a set of {"\0"} only: absent
    set_text, set_rec = _lay([b"ab\0", b"\0"])
    w_index, _ = check(lx, Table(set_text, set_rec), Table(b"ab", [(0, 2), (2, 2), (0, 0)]))
    assert w_index == [NONE, NONE, NONE]


def test_lengths_around_the_group_size(lx):
    rng = random.Random(4)
    base = bytes(rng.choice(b"xyz") for _ in range(40))
    strings = [base[:ln] for ln in LENGTHS]                      # prefixes of one another: only the length tells them apart
    set_text, set_rec = _lay(strings)
    probes = strings + [base[:ln] + b"!" for ln in LENGTHS] + [base[:ln - 1] + b"!" for ln in LENGTHS if ln]
    text, rec = _lay(probes, lead=b"..", sep_of=lambda i: b"." * (i % 5))
    w_index, w_hits = check(lx, Table(set_text, set_rec), Table(text, rec), units=UNITS)
    assert w_index[:len(LENGTHS)] == list(range(len(LENGTHS))) and set(w_index[len(LENGTHS):]) == {NONE} and w_hits == [1] * len(LENGTHS)


# ------------------------------------------------------------------------------------------------ orders
def _pool(rng, d):
    pool, tries = [], 0
    while len(pool) < d:
        kind = tries % 4
        tries += 1
        if kind == 1 and pool and pool[-1]:
            s = pool[-1][:-1] + bytes([pool[-1][-1] ^ 1])
        elif kind == 2 and pool:
            s = pool[-1][:len(pool[-1]) // 2]
        else:
            s = bytes(rng.choice(b"abc") for _ in range(rng.choice(LENGTHS + (40, 700))))
        if s not in pool:
            pool.append(s)
    return pool


def test_every_insert_order_and_probe_order_gives_the_dicts_answer(lx):
    """Set duplicates: the index is the SMALLEST set row of the string whichever of its rows was inserted first; 20 random
    insert orders, the identity and its reverse, against 4 probe orders, four unit sizes, with and without the peel."""
    rng = random.Random(5)
    pool = _pool(rng, 30)
    set_text, set_rec = _lay([rng.choice(pool[:20]) for _ in range(90)])
    text, rec = _lay([rng.choice(pool) for _ in range(140)], lead=b"~~~", sep_of=lambda i: b"~" * (i % 3))
    S, P = Table(set_text, set_rec), Table(text, rec)
    w_index, w_hits = check(lx, S, P, insert_orders=_orders(rng, 90, 20), units=(64,))
    check(lx, S, P, bits=(0, 64), insert_orders=_orders(rng, 90, 1), probe_orders=_orders(rng, 140, 2), units=UNITS, peels=(True, False))
    assert NONE in w_index and max(w_hits) > 3 and w_hits.count(0) > 50          # absent strings, a popular one, later duplicates
    firsts = {S.row(r): i for i, r in reversed(list(enumerate(S.rows())))}
    assert all(i == NONE or firsts[P.row(j)] == i for j, i in enumerate(w_index))
    # with 0 bits every probe walks ONE chain from slot 0: the slot reads grow with the number of distinct set strings
    _, summ, _, _ = run(lx, S, P, bits=0)
    assert summ[6] > 140 * 3 and summ[5] == 256


def test_no_rows_on_either_side(lx):
    set_text, set_rec = _lay([b"aa", b"bb", b"aa"])
    text, rec = _lay([b"bb", b"cc", b"aa"])
    S, P = Table(set_text, set_rec), Table(text, rec)
    for empty_set in (Table(set_text, set_rec, indices=[]), Table(b"", [])):
        w_index, _ = check(lx, empty_set, P, units=(1, 256))                     # ks == 0: every index is NONE, n_found 0
        assert w_index == [NONE] * 3
    for empty_probe in (Table(text, rec, indices=[]), Table(b"", [])):
        _, w_hits = check(lx, S, empty_probe)                                   # kp == 0: the hits are still written, all zero
        assert w_hits == [0, 0, 0]
    check(lx, Table(b"", []), Table(b"", []))


def test_index_lists_with_repeats_on_both_sides(lx):
    rng = random.Random(7)
    pool = _pool(rng, 12)
    set_text, set_rec = _lay(pool[:8])
    text, rec = _lay(pool)
    for _ in range(5):
        S = Table(set_text, set_rec, indices=[rng.randrange(8) for _ in range(rng.choice([1, 7, 40]))])
        P = Table(text, rec, indices=[rng.randrange(12) for _ in range(rng.choice([1, 9, 70]))])
        check(lx, S, P, bits=(0, 64), units=(3, 256), insert_orders=_orders(rng, S.k(), 1))
    # a row's identity is its position, not its record: set rows 0 and 2 name records 2 and 0
    S, P = Table(b"xx|yy|xx", [(0, 2), (3, 5), (6, 8)], indices=[2, 1, 0, 1]), Table(b"yy xx zz", [(0, 2), (3, 5), (6, 8)], indices=[1, 1, 2, 0])
    w_index, w_hits = check(lx, S, P)
    assert w_index == [0, 0, NONE, 1] and w_hits == [2, 1, 0, 0]


def test_the_same_buffer_as_both_texts(lx):
    rng = random.Random(8)
    pool = _pool(rng, 15)
    text, rec = _lay([rng.choice(pool) for _ in range(80)])
    idx = list(range(80))
    rng.shuffle(idx)
    S, P = Table(text, rec, indices=idx[:30]), Table(text, rec, indices=idx[20:])          # ten records are on both sides
    w_index, _ = check(lx, S, P, units=(3, 256))
    assert all(w_index[j] != NONE for j in range(10))
    check(lx, Table(text, rec), Table(text, rec), bits=(4,))                               # a table against itself: its own first occurrences


# ------------------------------------------------------------------------------------------------ refusals
def test_the_first_bad_row_of_each_side_and_the_set_wins(lx):
    set_text, set_rec = b"aa|bb|cc|dd", [(0, 2), (3, 5), (6, 8), (9, 11)]
    text, rec = b"bb cc", [(0, 2), (3, 5)]
    bad_sets = [(Table(set_text, set_rec, [0, 4, 1]), 1), (Table(set_text, set_rec, [0, 1, 5, 4]), 2), (Table(set_text, set_rec[:3] + [(9, 12)]), 3),
                (Table(set_text, [set_rec[0], (5, 4), (6, 8), (9, 12)]), 1)]
    bad_probes = [(Table(text, rec, [1, 0, 2, 0, 7]), 2), (Table(text, [(0, 2), (3, 6)]), 1), (Table(text, [(2, 1), (3, 6)]), 0)]
    good_set, good_probe = Table(set_text, set_rec), Table(text, rec)
    for S, want in bad_sets:
        for P in [good_probe] + [p for p, _ in bad_probes]:                       # the set is checked first: a bad probe row is not even named
            for bits in (0, 64):
                rc, summ, index, hits = run(lx, S, P, bits=bits)
                assert rc == 0 and summ[1] == want and summ[2] == NONE and summ[0] == 0
                assert index == [POISON] * len(index) and hits == [POISON] * len(hits)
    for P, want in bad_probes:
        for unit in UNITS:
            for po in (None, list(range(P.k() - 1, -1, -1))):                     # the FIRST bad row, whatever the order of the visit
                rc, summ, index, hits = run(lx, good_set, P, unit=unit, probe_order=po)
                assert rc == 0 and summ[1] == NONE and summ[2] == want and summ[0] == 0
                assert index == [POISON] * len(index) and hits == [POISON] * len(hits)
    assert run(lx, good_set, good_probe, unit=0)[0] == -2
    assert run(lx, good_set, good_probe, insert_order=[0, 1, 1, 2])[0] == -4


def test_limits_and_the_scratch_layout(lx):
    assert lx.lk_rows_fit(0, 0) == 1 and lx.lk_rows_fit((1 << 31) - 1, (1 << 31) - 1) == 1
    assert lx.lk_rows_fit(1 << 31, 0) == 0 and lx.lk_rows_fit(0, 1 << 31) == 0 and lx.lk_rows_fit(NONE, 1) == 0
    out = (ctypes.c_uint64 * 5)()
    for ks, kp in ((0, 0), (1, 1), (33, 1000), (10 ** 4, 10 ** 7), ((1 << 20) + 1, 3)):
        lx.lk_layout(ks, kp, out)
        total, hits, staged, long_list, set_bytes = (int(x) for x in out)
        slots = 64
        while slots < 2 * ks:
            slots *= 2
        pad = lambda x: (x + 15) & ~15
        # the group's layout for the set side, 4 bytes per slot of hit counts, 4 + 4 bytes per probe row
        assert hits == set_bytes and staged == hits + 4 * slots and long_list == staged + pad(4 * kp) and total == long_list + pad(4 * kp)
        assert all(x % 16 == 0 for x in (total, hits, staged, long_list))


# ------------------------------------------------------------------------------------------------ join_rows
def _group(strings):
    seen, group, rep, count = {}, [], [], []
    for j, s in enumerate(strings):
        if s not in seen:
            seen[s] = len(rep)
            rep.append(j)
            count.append(0)
        group.append(seen[s])
        count[seen[s]] += 1
    return seen, group, rep, count


def test_join_rows_equals_a_nested_loop_join_on_cpu_tensors():
    import torch
    from rejit_amd import records
    rng = random.Random(11)
    for ks, kp, d in ((0, 5, 3), (5, 0, 3), (1, 1, 1), (7, 9, 3), (40, 60, 11), (60, 40, 50), (30, 30, 1)):
        pool = [b"k%d" % i for i in range(d)]
        set_rows = [rng.choice(pool[:max(1, (2 * d) // 3)]) for _ in range(ks)]
        probe_rows = [rng.choice(pool) for _ in range(kp)]
        seen, group, _, count = _group(set_rows)
        index = torch.tensor([seen.get(s, -1) for s in probe_rows], dtype=torch.int64)       # a lookup against the dictionary: group numbers
        pr, sr = records.join_rows(index, torch.tensor(group, dtype=torch.int64), torch.tensor(count, dtype=torch.int64))
        want = [(j, i) for j in range(kp) for i in range(ks) if probe_rows[j] == set_rows[i]]
        assert pr.dtype == torch.int64 and sr.dtype == torch.int64
        assert list(zip(pr.tolist(), sr.tolist())) == want, (ks, kp, d)


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: 192 seeded random cases against a std::map, two texts or one, exact allocations.  (The sanitizers' runtimes
    are linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("lookup_exec", DEPS)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"192 cases" in r.stdout
