"""CPU tests of the record sort (rejit_amd/csrc/record_sort.h): the arithmetic of rj_scan_records_sort -- the rows of a record
table in the order of their bytes: unsigned bytes, a proper prefix first, equal rows in ascending row number.

The header is compiled with g++ into the test-only driver tests/support/sort_exec.cc, which walks the rounds the way the kernels
do (compaction unit by unit, both tiers of the prefix skip, keys, a stable sort by key and then by the bits of the segment
number, the cut) through a Text and a Mem policy that check every access, and asserts the header's properties P1..P4 INSIDE its
loop for every table (it returns -3 and says which one broke).  The expectation here is Python's
    sorted(range(k), key=lambda j: (rows[j], j))
All comparisons are exact."""
import ctypes
import random
import subprocess

import pytest

from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_sort.h", "record_rows.h", "record_pack.h"), ("checked_text.h", "checked_table.h"))
_u64p = ctypes.POINTER(ctypes.c_uint64)
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
UNITS = (1, 3, 256)
LS = (1, 16, 64)
KS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1500)
LENGTHS = (0, 1, 6, 7, 8, 13, 14, 15, 21, 63, 64, 65, 70)
ALPHABETS = (bytes([0, 1]), b"ab", bytes([0, 0x80, 0xFF]) + b"a", bytes(range(256)))


@pytest.fixture(scope="module")
def sx():
    lib = shared_driver("sort_exec", DEPS)
    u64, u32, cp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p
    lib.so_key.restype = ctypes.c_long
    lib.so_key.argtypes = [cp, u64, u64, u64, u64, _u64p]
    lib.so_rows_fit.argtypes = [u64]
    lib.so_scratch_bytes.restype = u64
    lib.so_scratch_bytes.argtypes = [u64]
    lib.so_seg_bits.restype = ctypes.c_uint
    lib.so_seg_bits.argtypes = [u64]
    lib.so_skip_row.restype = ctypes.c_long
    lib.so_skip_row.argtypes = [cp, u64, u64, u64, u64, u64, u64, u32, _u64p]
    lib.so_sort.restype = ctypes.c_long
    lib.so_sort.argtypes = [cp, u64, _u64p, _u64p, u64, _u64p, ctypes.c_int, u64, u64, u32, ctypes.c_int, _u64p, _u64p]
    return lib


def key_of(lib, text, begin, ln, d=0):
    """-> (key, the guarded load was taken)"""
    out = (ctypes.c_uint64 * 2)()
    rc = lib.so_key(text, len(text), begin, ln, d, out)
    assert rc == 0, ("a read left the text", rc, begin, ln, d, len(text))
    return int(out[0]), bool(out[1])


def meaning(text, records, indices=None):
    rows = range(len(records)) if indices is None else indices
    strings = [text[records[r][0]:records[r][1]] for r in rows]
    return sorted(range(len(strings)), key=lambda j: (strings[j], j))


def run(lib, text, records, indices=None, unit=256, L=64, skip=1, room=3):
    """-> (rc, first bad row or None, order: the whole poisoned buffer, stats dict)"""
    k = len(records) if indices is None else len(indices)
    rb, re_ = _arr([b for b, _ in records]), _arr([e for _, e in records])
    idx = None if indices is None else _arr(indices)
    order = _arr([POISON] * (k + room))
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.so_sort(text, len(text), rb, re_, len(records), idx, int(indices is not None), 0 if indices is None else len(indices), unit, L, skip, order, summ)
    bad = None if summ[1] == NONE else int(summ[1])
    stats = dict(rounds=int(summ[0]), keyed_rows=int(summ[2]), skip_rows=int(summ[3]), long_rows=int(summ[4]), segments=int(summ[5]), broke=int(summ[6]),
                 guarded=int(summ[7]))
    return rc, bad, list(order), stats


def check(lib, text, records, indices=None, units=(256,), ls=(64,), skips=(1, 0)):
    k = len(records) if indices is None else len(indices)
    want = meaning(text, records, indices)
    last = None
    for unit in units:
        for L in ls:
            for skip in skips:
                rc, bad, order, stats = run(lib, text, records, indices, unit=unit, L=L, skip=skip)
                ctx = (k, unit, L, skip, stats)
                assert rc == 0, ("an access left its range or a row was written twice (-1), a property broke (-3: stats['broke'] says which)", rc, ctx)
                assert bad is None, ctx
                assert order[:k] == want and order[k:] == [POISON] * 3, ctx
                assert stats["rounds"] == 0 if k < 2 else stats["rounds"] >= 1, ctx
                last = stats
    return last


def table(rng, k, alphabet, prefix=0, lengths=LENGTHS, gaps=True, pool=None):
    """k rows over `alphabet` behind a shared prefix; every third row repeats an earlier one, every fifth is a prefix of one;
    0..3 bytes between the rows, the last row ends at n -> (text, records)"""
    shared = bytes(rng.choice(alphabet) for _ in range(prefix))
    rows = []
    for j in range(k):
        if rows and j % 3 == 2:
            s = rng.choice(rows)
        elif rows and j % 5 == 4:
            s = rng.choice(rows)
            s = s[:rng.randrange(len(s) + 1)]
        else:
            s = shared + bytes(rng.choice(alphabet) for _ in range(rng.choice(lengths)))
        rows.append(s)
    return lay_out(rng, rows, gaps)


def lay_out(rng, rows, gaps=True):
    text, records = bytearray(), []
    for s in rows:
        text += b"|" * (rng.randrange(4) if gaps else 0)
        records.append((len(text), len(text) + len(s)))
        text += s
    return bytes(text), records


# ------------------------------------------------------------------------------------------------ the key
def test_equal_windows_give_equal_keys_whatever_the_alignment_and_what_follows(sx):
    rng = random.Random(1)
    for ln in (0, 1, 6, 7, 8, 15, 40):
        row = bytes(rng.randrange(256) for _ in range(ln))
        for d in sorted({0, min(ln, 1), max(ln - 7, 0), max(ln - 3, 0), ln}):
            got = set()
            for mis in range(16):
                for poison in (b"\xA5", b"\x00", b"\xFF"):
                    got.add(key_of(sx, poison * (32 + mis) + row + poison * 40, 32 + mis, ln, d)[0])
                    got.add(key_of(sx, poison * mis + row, mis, ln, d)[0])          # the row ends at n
            assert len(got) == 1, (ln, d, got)
            c = min(ln - d, 7)
            want = int.from_bytes(row[d:d + c].ljust(7, b"\0"), "big") << 8 | c
            assert got.pop() == want, (ln, d)


def test_the_keys_order_is_byte_order_with_a_prefix_first(sx):
    k = lambda s: key_of(sx, s + b"zzzzzzzzzzzzzzzzzzzz", 0, len(s))[0]
    assert k(b"ab") < k(b"ab\0") < k(b"ab\0\0") < k(b"ab\0\0\0\0\0") < k(b"ab\1")
    assert k(b"") < k(b"\0") < k(b"\0\0")
    assert k(b"\x7F") < k(b"\x80") < k(b"\xFF") and k(b"a\x7Fz") < k(b"a\x80") < k(b"a\xFF")
    assert k(b"\xFF" * 6) < k(b"\xFF" * 7) == k(b"\xFF" * 9)
    # the count decides between rows that end and rows that go on: 7 means "more may follow"
    assert k(b"abcdefg") & 0xFF == 7 == k(b"abcdefgh") & 0xFF and k(b"abcdef") & 0xFF == 6


def test_rows_at_the_texts_end_take_the_guarded_load(sx):
    text = bytes(range(1, 41))
    n = len(text)
    for ln in (1, 5, 7, 15, 16):
        for back in range(0, 16):
            if n - back - ln < 0:
                continue
            begin = n - back - ln
            for d in sorted({0, ln // 2, ln}):
                key, guarded = key_of(sx, text, begin, ln, d)
                c = min(ln - d, 7)
                assert key == int.from_bytes(text[begin + d:begin + d + c].ljust(7, b"\0"), "big") << 8 | c
                assert guarded == (c > 0 and begin + d + 16 > n), (ln, back, d)
    assert key_of(sx, b"", 0, 0)[0] == 0 and key_of(sx, b"x", 1, 0)[0] == 0


def test_the_lane_tier_of_the_skip(sx):
    """skip_row: the depth it reports lies between D and the common prefix, is the common prefix when no more than L bytes were
    needed, and `more` says exactly when both rows go on behind L agreeing bytes."""
    rng = random.Random(2)
    for _ in range(300):
        la, lb = rng.choice([0, 1, 7, 16, 17, 40, 100]), rng.choice([0, 1, 7, 16, 17, 40, 100])
        a = bytes(rng.choice(b"ab") for _ in range(la))
        b = (a[:rng.randrange(la + 1)] + bytes(rng.choice(b"ab") for _ in range(lb)))[:lb]
        text = b"#" * rng.randrange(5) + a
        hb = len(text) - la
        text += b"|" * rng.randrange(3) + b
        rb = len(text) - lb
        lcp = next((i for i in range(min(la, lb)) if a[i] != b[i]), min(la, lb))
        for L in (1, 16, 64):
            D = rng.randrange(lcp + 1)
            out = (ctypes.c_uint64 * 2)()
            assert sx.so_skip_row(text, len(text), hb, la, rb, len(b), D, L, out) == 0
            depth, more = int(out[0]), bool(out[1])
            assert depth == min(lcp, D + L), (a, b, D, L, depth)
            assert more == (lcp >= D + L and min(la, lb) > D + L), (a, b, D, L)


# ------------------------------------------------------------------------------------------------ tables
def test_tables_of_every_shape_against_sorted(sx):
    rng = random.Random(3)
    n = 0
    for k in KS:
        for ai, alphabet in enumerate(ALPHABETS):
            for prefix in (0, 9, 40):
                text, records = table(rng, k, alphabet, prefix)
                check(sx, text, records, units=(UNITS[n % 3],), ls=LS)
                check(sx, text, records, units=UNITS, ls=(64,), skips=(1,))
                n += 1


def test_all_equal_all_distinct_sorted_and_reversed(sx):
    rng = random.Random(4)
    for k in (2, 65, 300):
        for ln in (0, 6, 7, 8, 70):
            text, records = lay_out(rng, [b"q" * ln] * k)
            st = check(sx, text, records, ls=LS)
            st = run(sx, text, records, skip=0)[3]
            assert st["rounds"] == ln // 7 + 1                            # P2's bound is met: 7 bytes a round
            st = run(sx, text, records, skip=1)[3]
            assert st["rounds"] <= 2 and st["keyed_rows"] <= 2 * k
        rows = sorted({bytes(rng.choice(b"abc") for _ in range(rng.choice(LENGTHS))) for _ in range(k)})
        for order in (rows, rows[::-1]):
            text, records = lay_out(rng, order)
            check(sx, text, records, units=UNITS, ls=LS)
    # 53 rows of 4 KiB that differ only in the last byte: 586 rounds without the skip, 2 with it (P3)
    rows = [b"x" * 4095 + bytes([200 - i]) for i in range(53)]
    text, records = lay_out(rng, rows)
    for L in LS:
        rc, _, order, st = run(sx, text, records, L=L)
        assert rc == 0 and order[:53] == list(range(52, -1, -1)) and st["rounds"] == 2 and st["long_rows"] == 52, st
    rc, _, order, st = run(sx, text, records, skip=0)
    assert rc == 0 and order[:53] == list(range(52, -1, -1)) and st["rounds"] == 586 and st["skip_rows"] == 0, st


def test_indices_with_repeats_in_any_order(sx):
    rng = random.Random(5)
    for k in (1, 3, 64, 257):
        text, records = table(rng, k, b"ab", 9)
        perm = list(range(k))
        rng.shuffle(perm)
        check(sx, text, records, indices=perm, units=(3,), ls=LS)
        check(sx, text, records, indices=[rng.randrange(k) for _ in range(2 * k + 1)], units=UNITS)
        check(sx, text, records, indices=list(range(k - 1, -1, -1)))
    # a row's identity is j, not r(j): the same record named three times comes out in ascending j
    text, records = b"xx|yy|xx", [(0, 2), (3, 5), (6, 8)]
    rc, _, order, _ = run(sx, text, records, indices=[1, 2, 0, 2, 1, 2])
    assert rc == 0 and order[:6] == [1, 2, 3, 5, 0, 4]
    # no rows
    rc, bad, order, st = run(sx, text, records, indices=[])
    assert rc == 0 and bad is None and order == [POISON] * 3 and st["rounds"] == 0
    assert run(sx, b"", [])[0] == 0


def test_more_segments_than_one_and_than_two_radix_digits_hold(sx):
    """Rows of 8 bytes drawn from 70000 seven-byte prefixes, two per prefix: behind the first round every prefix is an open
    segment of its own -- more than 65536 dense segment numbers in one round, 17 bits for the second radix pass."""
    rng = random.Random(6)
    prefixes = rng.sample(range(1 << 24), 70000)
    rows = []
    for p in prefixes:
        head = b"rec" + p.to_bytes(3, "big") + b":"
        rows += [head + bytes([rng.randrange(256)]), head + bytes([rng.randrange(256)])]
    rng.shuffle(rows)
    text, records = lay_out(rng, rows, gaps=False)
    for skip in (1, 0):
        rc, bad, order, st = run(sx, text, records, skip=skip)
        assert rc == 0 and bad is None, (rc, st)
        assert order[:len(rows)] == meaning(text, records)
        assert st["segments"] == 70000 and st["rounds"] == 2 and st["keyed_rows"] == 2 * len(rows), st
    assert [sx.so_seg_bits(x) for x in (0, 1, 2, 3, 256, 257, 65536, 65537, 70000, 1 << 30)] == [0, 0, 1, 2, 8, 9, 16, 17, 17, 30]
    # a few hundred segments: two digits of an 8-bit radix are not needed, nine bits are
    rows = [bytes([i % 256, i // 256]) + b"segmt" + bytes([rng.randrange(3)]) for i in range(300) for _ in range(2)]
    rng.shuffle(rows)
    text, records = lay_out(rng, rows)
    check(sx, text, records, units=UNITS)
    assert run(sx, text, records)[3]["segments"] == 300


# ------------------------------------------------------------------------------------------------ refusals, limits
def test_refusals_name_the_first_bad_row_and_write_nothing(sx):
    text = b"aa|bb|cc|dd"
    records = [(0, 2), (3, 5), (6, 8), (9, 11)]
    cases = [
        (records, [0, 4, 1], 1), (records, [4, 0, 1], 0), (records, [0, 1, 4], 2), (records, [0, 5, 4, 1], 1),
        (records[:3] + [(9, 12)], None, 3),                      # end > n
        ([records[0], (5, 4)] + records[2:], None, 1),           # begin > end
        ([records[0], (5, 4), (6, 8), (9, 12)], None, 1),        # two bad rows
        ([(0, 12)], None, 0),                                    # one row (no round runs): still checked
    ]
    for recs, idx, want in cases:
        for skip in (0, 1):
            rc, bad, order, st = run(sx, text, recs, indices=idx, skip=skip)
            assert rc == 0 and bad == want and st["rounds"] == 0, (recs, idx)
            assert order == [POISON] * len(order)


def test_limits_and_the_layouts_size(sx):
    assert sx.so_rows_fit(0) == 1 and sx.so_rows_fit((1 << 31) - 1) == 1 and sx.so_rows_fit(1 << 31) == 0 and sx.so_rows_fit(NONE) == 0
    assert run(sx, b"ab", [(0, 1)], unit=0)[0] == -2
    # 1 + 4 + 8 + 4 + 4 x 8 + 4 bytes per row, 8 + 8 + 4 per segment, at most k / 2 segments: 63 bytes per row
    for k in (1 << 20, (1 << 20) + 1, 10 ** 7):
        per_row = sx.so_scratch_bytes(k) / k
        assert 62.99 <= per_row <= 63.01, (k, per_row)
    assert sx.so_scratch_bytes(1) == 16 * 12
    assert sx.so_scratch_bytes((1 << 31) - 1) < 1 << 38


def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: a fixed set of cases with exact allocations, P1..P4 asserted inside.  (The sanitizers' runtimes are linked
    statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("sort_exec", DEPS)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"270 cases" in r.stdout
