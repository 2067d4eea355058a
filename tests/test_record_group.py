"""CPU tests of the record group (rejit_amd/csrc/record_group.h): the arithmetic of rj_scan_records_group -- the rows of a
record table grouped by their bytes, numbered in order of first appearance.

The header is compiled with g++ into the test-only driver tests/support/group_exec.cc, which hashes the rows, inserts them ONE
AT A TIME in an order the test chooses (the kernels' lanes interleave; every order must give the same tables) with the two
invariants of the table checked behind every insert, numbers unit by unit and emits, every access checked against its range.
The expectation is a Python dict over the rows' bytes, in insertion order:
    group[j] = the number of row j's string, rep[g] = the first j with string g, count[g] = how many rows have it.
All comparisons are exact."""
import ctypes
import random
import subprocess

import pytest

from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_group.h", "record_rows.h", "record_pack.h"), ("checked_text.h", "checked_table.h"))
_u64p = ctypes.POINTER(ctypes.c_uint64)
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
BITS = (0, 1, 4, 64)
UNITS = (1, 3, 256)


@pytest.fixture(scope="module")
def gx():
    lib = shared_driver("group_exec", DEPS)
    u64, u32, cp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p
    lib.gr_hash.restype = ctypes.c_long
    lib.gr_hash.argtypes = [cp, u64, u64, u64, u64, ctypes.c_int, u32, _u64p]
    lib.gr_rows_equal.restype = ctypes.c_long
    lib.gr_rows_equal.argtypes = [cp, u64, u64, u64, u64, u64, u32]
    lib.gr_table_slots.restype = u64
    lib.gr_table_slots.argtypes = [u64]
    lib.gr_rows_fit.argtypes = [u64]
    lib.gr_scratch_bytes.restype = u64
    lib.gr_scratch_bytes.argtypes = [u64]
    lib.gr_group.restype = ctypes.c_long
    lib.gr_group.argtypes = [cp, u64, _u64p, _u64p, u64, _u64p, ctypes.c_int, u64, u32, _u64p, u64, _u64p, _u64p, _u64p, u64, _u64p]
    return lib


def hash_of(lib, text, begin, ln, lanes=1, blocked=0, bits=64):
    out = ctypes.c_uint64()
    rc = lib.gr_hash(text, len(text), begin, ln, lanes, blocked, bits, ctypes.byref(out))
    assert rc == 0, ("a read left the text", rc, begin, ln, len(text))
    return out.value


def meaning(text, records, indices=None):
    """the dict, in insertion order -> (group, rep, count)"""
    rows = range(len(records)) if indices is None else indices
    seen, group, rep, count = {}, [], [], []
    for j, r in enumerate(rows):
        s = text[records[r][0]:records[r][1]]
        if s not in seen:
            seen[s] = len(rep)
            rep.append(j)
            count.append(0)
        group.append(seen[s])
        count[seen[s]] += 1
    return group, rep, count


def run(lib, text, records, indices=None, bits=64, order=None, unit=256, cap=None, room=3, want_group=True):
    """-> (rc, G, first bad row or None, group, rep, count: the whole poisoned buffers, summary)"""
    k = len(records) if indices is None else len(indices)
    rb, re_ = _arr([b for b, _ in records]), _arr([e for _, e in records])
    idx = None if indices is None else _arr(indices)
    if order is None:
        order = list(range(k))
    if cap is None:
        cap = k
    g = _arr([POISON] * (k + room))
    rep, cnt = _arr([POISON] * (cap + room)), _arr([POISON] * (cap + room))
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.gr_group(text, len(text), rb, re_, len(records), idx, int(indices is not None), 0 if indices is None else len(indices), bits, _arr(order), unit,
                      g if want_group else None, rep, cnt, cap, summ)
    bad = None if summ[1] == NONE else int(summ[1])
    return rc, int(summ[0]), bad, list(g), list(rep), list(cnt), [int(x) for x in summ]


def check(lib, text, records, indices=None, bits=BITS, orders=(None,), units=(256,)):
    k = len(records) if indices is None else len(indices)
    w_group, w_rep, w_count = meaning(text, records, indices)
    G = len(w_rep)
    assert sum(w_count) == k and w_rep == sorted(set(w_rep))
    for b in bits:
        for order in orders:
            for unit in units:
                rc, total, bad, g, rep, cnt, _ = run(lib, text, records, indices, bits=b, order=order, unit=unit, cap=G)
                ctx = (b, unit, None if order is None else order[:8], k)
                assert rc == 0, ("an access left its range (-1), an invariant broke (-3)", rc, ctx)
                assert bad is None and total == G, ctx
                assert g[:k] == w_group and g[k:] == [POISON] * 3, ctx
                assert rep[:G] == w_rep and rep[G:] == [POISON] * 3, ctx
                assert cnt[:G] == w_count and cnt[G:] == [POISON] * 3, ctx
    return G


# ------------------------------------------------------------------------------------------------ hash
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025)


def test_the_hash_depends_on_the_rows_bytes_alone(gx):
    """The same row bytes at every misalignment 0..15 with two different poisons before and behind the row, and with the row
    ending at n, give one value; rows of every length around the group and the wave-iteration sizes."""
    rng = random.Random(1)
    values = {}
    for ln in LENGTHS:
        row = bytes(rng.randrange(256) for _ in range(ln))
        got = set()
        for mis in range(16):
            for poison in (b"\xA5", b"\x00", b"\xFF"):
                got.add(hash_of(gx, poison * (32 + mis) + row + poison * 40, 32 + mis, ln))
                got.add(hash_of(gx, poison * mis + row, mis, ln))                      # the row ends at n (and begins at 0 for mis == 0)
        assert len(got) == 1, (ln, got)
        values[ln] = got.pop()
    assert len(set(values.values())) == len(LENGTHS)


def test_any_deal_of_the_groups_to_lanes_gives_the_same_hash(gx):
    rng = random.Random(2)
    for ln in LENGTHS + (5000,):
        row = bytes(rng.randrange(256) for _ in range(ln))
        text = b"\x11" * 7 + row + b"\x22" * 3
        want = hash_of(gx, text, 7, ln)
        for lanes in (1, 3, 64):
            for blocked in (0, 1):
                assert hash_of(gx, text, 7, ln, lanes, blocked) == want, (ln, lanes, blocked)
        for bits in (0, 1, 4):
            assert hash_of(gx, text, 7, ln, 3, 1, bits) == want & ((1 << bits) - 1)


def test_rows_that_differ_in_one_byte_or_in_length_differ_in_key_and_never_compare_equal(gx):
    rng = random.Random(3)
    for ln in (1, 15, 16, 17, 33, 1024, 1025):
        row = bytearray(rng.randrange(1, 256) for _ in range(ln))
        for at in sorted({0, ln // 2, ln - 1}):
            other = bytearray(row)
            other[at] ^= 0x40
            text = bytes(row) + bytes(other)
            for bits in BITS:
                r = gx.gr_rows_equal(text, len(text), 0, ln, ln, ln, bits)
                assert r >= 0 and not r & 2, (ln, at, bits)          # the bytes never compare equal, whatever the hashes do
            assert gx.gr_rows_equal(text, len(text), 0, ln, ln, ln, 64) == 0
            assert hash_of(gx, text, 0, ln) != hash_of(gx, text, ln, ln)
    # "a" against "a\0": the zero padding of the last group does not make them one key; a row and its prefix; empty rows
    text = b"a\0a"
    assert hash_of(gx, text, 0, 1) == hash_of(gx, text, 2, 1) != hash_of(gx, text, 0, 2)
    for bits in BITS:
        assert gx.gr_rows_equal(text, 3, 0, 1, 0, 2, bits) == 0                         # the lengths differ: not even the keys
        assert gx.gr_rows_equal(text, 3, 0, 1, 2, 1, bits) == 3
        assert gx.gr_rows_equal(text, 3, 1, 0, 3, 0, bits) == 3                         # two empty rows, one of them at n
    zeros = bytes(64)
    assert len({hash_of(gx, zeros, 0, ln) for ln in range(0, 49)}) == 49


# ------------------------------------------------------------------------------------------------ insert
def _pool_table(rng, k, d, gaps=True):
    """k records drawn from d distinct strings: lengths around the group size, strings that share a 16-byte prefix and differ in
    the last byte, strings that are prefixes of one another, the empty string -> (text, records)"""
    pool, tries = [], 0
    while len(pool) < d:
        kind = tries % 4
        tries += 1
        if kind == 1 and pool and pool[-1]:
            s = pool[-1][:-1] + bytes([pool[-1][-1] ^ 1])
        elif kind == 2 and pool:
            s = pool[-1][:len(pool[-1]) // 2]
        else:
            s = bytes(rng.choice(b"abc") for _ in range(rng.choice([0, 1, 15, 16, 17, 31, 32, 33, 40, 700])))
        if s not in pool:
            pool.append(s)
    text, records = b"", []
    for j in range(k):
        s = pool[j] if j < d and rng.random() < 0.5 else rng.choice(pool)
        text += b"|" * (rng.randrange(4) if gaps else 0)
        records.append((len(text), len(text) + len(s)))
        text += s
    return text, records


def test_every_insert_order_gives_the_dicts_tables_and_keeps_the_invariants(gx):
    """One set of rows, 50 random orders and the reverse, hash bits 0, 1, 4 and 64: the tables are the dict's whatever the
    order, and behind every single insert no slot was emptied and no slot's string changed (the driver returns -3 else)."""
    rng = random.Random(5)
    text, records = _pool_table(rng, 150, 23)
    k = len(records)
    orders = [list(range(k - 1, -1, -1))]
    for _ in range(50):
        o = list(range(k))
        rng.shuffle(o)
        orders.append(o)
    G = check(gx, text, records, orders=orders)
    assert 10 < G <= 23
    # with 0 bits every row walks ONE chain from slot 0: the slot reads grow with the number of distinct strings
    _, _, _, _, _, _, summ = run(gx, text, records, bits=0, order=orders[0])
    assert summ[2] > k * 2 and summ[3] == 512


def test_shapes_units_and_indices(gx):
    rng = random.Random(7)
    for k, d in ((1, 1), (2, 1), (2, 2), (32, 7), (33, 33), (257, 2), (300, 150)):
        text, records = _pool_table(rng, k, d)
        check(gx, text, records, units=UNITS)
        perm = list(range(k))
        rng.shuffle(perm)
        check(gx, text, records, indices=perm, bits=(2, 64), units=(3,))
        check(gx, text, records, indices=[rng.randrange(k) for _ in range(2 * k + 1)], bits=(0, 64), units=(3, 256))
        # reversed: the numbering follows the rows, not the records
        rev = list(range(k - 1, -1, -1))
        g, rep, _ = meaning(text, records, rev)
        assert g[0] == 0 and rep[0] == 0
        check(gx, text, records, indices=rev, bits=(64,))
    # the representative is the smallest j, not the smallest r(j)
    text, records = b"xx|yy|xx", [(0, 2), (3, 5), (6, 8)]
    rc, G, _, g, rep, cnt, _ = run(gx, text, records, indices=[2, 1, 0, 2])
    assert rc == 0 and G == 2 and g[:4] == [0, 1, 0, 0] and rep[:2] == [0, 1] and cnt[:2] == [3, 1]
    # no rows
    rc, G, bad, g, rep, cnt, _ = run(gx, text, records, indices=[])
    assert rc == 0 and G == 0 and bad is None and g == [POISON] * 3 and rep == [POISON] * 3
    rc, G, _, _, _, _, _ = run(gx, b"", [])
    assert rc == 0 and G == 0


def test_caps_the_size_query_and_no_group_table(gx):
    rng = random.Random(8)
    text, records = _pool_table(rng, 90, 12)
    w_group, w_rep, w_count = meaning(text, records)
    G = len(w_rep)
    for cap in (0, 1, G - 1, G, G + 5):
        for want_group in (True, False):
            rc, total, _, g, rep, cnt, _ = run(gx, text, records, cap=cap, want_group=want_group, bits=4)
            lim = min(cap, G)
            assert rc == 0 and total == G
            assert rep[:lim] == w_rep[:lim] and cnt[:lim] == w_count[:lim]
            assert rep[lim:] == [POISON] * (len(rep) - lim) and cnt[lim:] == [POISON] * (len(cnt) - lim)
            assert g[:90] == (w_group if want_group else [POISON] * 90) and g[90:] == [POISON] * 3


def test_refusals_name_the_first_bad_row_and_write_nothing(gx):
    text = b"aa|bb|cc|dd"
    records = [(0, 2), (3, 5), (6, 8), (9, 11)]
    cases = [
        (records, [0, 4, 1], 1), (records, [4, 0, 1], 0), (records, [0, 1, 4], 2), (records, [0, 5, 4, 1], 1),
        (records[:3] + [(9, 12)], None, 3),                      # end > n
        ([records[0], (5, 4)] + records[2:], None, 1),           # begin > end
        ([records[0], (5, 4), (6, 8), (9, 12)], None, 1),        # two bad rows
    ]
    for recs, idx, want in cases:
        for bits in (0, 64):
            rc, G, bad, g, rep, cnt, _ = run(gx, text, recs, indices=idx, bits=bits)
            assert rc == 0 and bad == want and G == 0, (recs, idx)
            assert g == [POISON] * len(g) and rep == [POISON] * len(rep) and cnt == [POISON] * len(cnt)


# ------------------------------------------------------------------------------------------------ limits
def test_table_size_and_limits(gx):
    slots = gx.gr_table_slots
    assert [slots(k) for k in (0, 1, 32, 33, 64, 65)] == [64, 64, 64, 128, 128, 256]
    assert slots((1 << 31) - 1) == 1 << 32 and slots(1 << 30) == 1 << 31
    for k in (1, 3, 1000, 12345, (1 << 20) + 1):
        t = slots(k)
        assert t >= 2 * k and t & (t - 1) == 0 and (t == 64 or t < 4 * k)
    assert gx.gr_rows_fit(0) == 1 and gx.gr_rows_fit((1 << 31) - 1) == 1 and gx.gr_rows_fit(1 << 31) == 0 and gx.gr_rows_fit(NONE) == 0
    # the scratch: 8 + 4 bytes per slot (a slot's group takes its count's place) and 8 + 4 + 4 + 4 per row, T = 2k .. 4k
    for k in (1 << 20, (1 << 20) + 1, 10 ** 7):
        per_row = gx.gr_scratch_bytes(k) / k
        assert 44 <= per_row <= 68.001, (k, per_row)
    assert gx.gr_scratch_bytes(1) == 64 * 12 + 4 * 16
    # the driver refuses what the call refuses
    assert run(gx, b"ab", [(0, 1)], unit=0)[0] == -2


# ------------------------------------------------------------------------------------------------ the end-to-end log
# The address pattern [0-9]+\.[0-9]+\.[0-9]+\.[0-9]+ in the library's dialect, which has no `\.` (rejit_amd/csrc/parser.cc: "unexpected
# character", as the reference's parser says): a bracket holds the dot.  The same language; Python's `re` reads both spellings.
ADDRESS = rb"[0-9]+[.][0-9]+[.][0-9]+[.][0-9]+"
ADDRESS_PY = rb"[0-9]+\.[0-9]+\.[0-9]+\.[0-9]+"


def address_log(n_lines=20000, distinct=300, seed=17):
    """A log of n_lines lines with 0..3 of `distinct` client addresses each, drawn with a skew (top addresses, as a real log
    has) -> (data, lines)"""
    rng = random.Random(seed)
    pool = set()
    while len(pool) < distinct:
        pool.add(b"%d.%d.%d.%d" % (rng.randrange(1, 224), rng.randrange(256), rng.randrange(256), rng.randrange(1, 255)))
    pool = sorted(pool)
    rng.shuffle(pool)
    words = [b"GET /index.html", b"POST /api/v1/items", b"status=200", b"status=404 bytes=1532", b"-", b"upstream", b"took 12ms", b"v1.2", b"3.14"]
    lines = []
    for i in range(n_lines):
        parts = [b"peer", pool[i // 50]] if i % 50 == 0 and i // 50 < distinct else []      # (every address occurs)
        for _ in range(rng.choice([0, 1, 1, 1, 2, 3])):
            parts.append(rng.choice(words))
            parts.append(pool[min(int(rng.expovariate(1 / 40.0)), distinct - 1)])
        parts.append(rng.choice(words))
        lines.append(b" ".join(parts))
    return b"\n".join(lines) + b"\n", lines


def test_python_re_and_the_oracle_agree_on_the_address_pattern():
    """The end-to-end GPU test counts re.findall per line: first, on the CPU, Python's leftmost-first `re` and checkers.Oracle's
    leftmost-longest give the same matches of the address pattern over that log, and no match holds a line break."""
    import re
    from checkers import Oracle
    data, lines = address_log()
    want = [(m.start(), m.end()) for m in re.finditer(ADDRESS_PY, data)]
    assert want == [(m.start(), m.end()) for m in re.finditer(ADDRESS, data)]
    assert Oracle().match_all(ADDRESS, data) == want and len(want) > 15000
    assert sum(len(re.findall(ADDRESS, ln)) for ln in lines) == len(want)
    assert len({data[b:e] for b, e in want}) == 300


def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: a fixed set of cases against a std::map, exact allocations.  (The sanitizers' runtimes are linked
    statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("group_exec", DEPS)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"192 cases" in r.stdout
