"""CPU tests of the record parse (rejit_amd/csrc/record_parse.h): the meaning of rj_scan_records_parse -- a row of a record
table read as an int64, a uint64 or a double, exactly or not at all -- and of records.group_sums / group_counts_ok.

The header is compiled with g++ into the test-only driver tests/support/parse_exec.cc, which checks the rows first, then walks
every row in the 16-byte groups of record_rows.h over a text whose every access is checked against its range, and feeds
every row AGAIN at every split of its bytes into two runs of groups: the answer must not depend on where a row is cut.  The
expectation is tests/parse_cases.py's meaning, written in Python independently of the header: re.fullmatch of the grammars,
int(), decimal.Decimal for (m, q) and float() for the bits.  All comparisons are exact."""
import ctypes
import random
import subprocess

import pytest

import parse_cases as pc
from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_parse.h", "record_rows.h", "record_pack.h"), ("checked_text.h",))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 3


@pytest.fixture(scope="module")
def px():
    lib = shared_driver("parse_exec", DEPS)
    u64, cp, ci, cu = ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.pe_known.argtypes = [ci, cu]
    lib.pe_parse.restype = ctypes.c_long
    lib.pe_parse.argtypes = [cp, u64, _u64p, _u64p, u64, _u64p, ci, u64, ci, cu, ci, _u64p, _u8p, _u64p]
    return lib


def run(lib, text, records, indices, kind, trim, splits=True, with_status=True):
    """-> (rc, summary, values, statuses: the whole poisoned buffers)"""
    k = len(records) if indices is None else len(indices)
    values, statuses = _arr([POISON] * (k + ROOM)), _arr([POISON8] * (k + ROOM), ctypes.c_uint8)
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.pe_parse(text, len(text), _arr([b for b, _ in records]), _arr([e for _, e in records]), len(records), None if indices is None else _arr(indices),
                      int(indices is not None), 0 if indices is None else len(indices), kind, 1 if trim else 0, int(splits), values,
                      statuses if with_status else None, summ)
    return rc, [int(x) for x in summ], list(values), list(statuses)


def check(lib, rows, kinds=pc.KINDS, trims=(False, True), indices=None, lead=b"", tail=b"", splits=True):
    """the rows laid into one text, parsed under every kind and flag, against the meaning"""
    text, records = pc.lay(rows, lead=lead, tail=tail)
    order = range(len(rows)) if indices is None else indices
    for kind in kinds:
        for trim in trims:
            want = [pc.meaning(rows[r], kind, trim) for r in order]
            for with_status in (True, False):
                rc, summ, values, statuses = run(lib, text, records, indices, kind, trim, splits, with_status)
                ctx = (kind, trim, with_status)
                assert rc == 0, ("an access left its range, a row was written twice or a split feed differed", rc, ctx)
                k = len(want)
                for j, (w, v, s) in enumerate(zip(want, values, statuses)):
                    assert (w[1], w[0] if with_status else POISON8) == (v, s), (ctx, j, rows[order[j]], w, (s, hex(v)))
                assert values[k:] == [POISON] * ROOM and statuses[k:] == [POISON8] * ROOM, ctx
                if not with_status:
                    assert statuses == [POISON8] * (k + ROOM), ctx
                assert summ[:5] == [sum(1 for w in want if w[0] == c) for c in range(5)] and summ[5] == NONE, (ctx, summ)
                assert sum(summ[:5]) == k
                if splits:
                    assert summ[6] == sum(max(len(rows[r]) - 1, 0) for r in order), ctx
    return text, records


# ------------------------------------------------------------------------------------------------ the meaning itself
def test_the_python_meaning_on_rows_whose_answer_is_known_by_hand():
    M = pc.meaning
    assert M(b"", pc.INT64, False) == (pc.EMPTY, 0) and M(b" \t", pc.FLOAT64, True) == (pc.EMPTY, 0) and M(b" ", pc.INT64, False) == (pc.MALFORMED, 0)
    assert M(b"-9223372036854775808", pc.INT64, False) == (pc.OK, 1 << 63) and M(b"9223372036854775808", pc.INT64, False) == (pc.RANGE, 0)
    assert M(b"9223372036854775808", pc.UINT64, False) == (pc.OK, 1 << 63) and M(b"-0", pc.UINT64, False) == (pc.MALFORMED, 0)
    assert M(b"12\0", pc.INT64, False) == (pc.MALFORMED, 0) and M(b"12\n", pc.INT64, True) == (pc.MALFORMED, 0)
    for spelling in (b"1.50", b"15e-1", b"0.0015e3"):
        assert M(spelling, pc.FLOAT64, False) == (pc.OK, 0x3FF8000000000000)
    assert M(b"-0e999", pc.FLOAT64, False) == (pc.OK, 1 << 63) and M(b"1e23", pc.FLOAT64, False) == (pc.INEXACT, 0)
    assert M(b"9007199254740993", pc.FLOAT64, False) == (pc.INEXACT, 0) and M(b"9007199254740992", pc.FLOAT64, False)[0] == pc.OK
    assert M(b"inf", pc.FLOAT64, False) == (pc.MALFORMED, 0) and M(b"1_0", pc.INT64, False) == (pc.MALFORMED, 0)
    assert pc.decimal_value(b"0.0015", 3) == (15, -1) and pc.decimal_value(b"000", 7) == (0, 7)


def test_every_status_for_every_kind(px):
    rows = pc.status_rows()
    check(px, rows)
    for kind, statuses in ((pc.INT64, (pc.OK, pc.EMPTY, pc.MALFORMED, pc.RANGE)), (pc.UINT64, (pc.OK, pc.EMPTY, pc.MALFORMED, pc.RANGE)),
                           (pc.FLOAT64, (pc.OK, pc.EMPTY, pc.MALFORMED, pc.INEXACT))):
        for trim in (False, True):
            assert {pc.meaning(r, kind, trim)[0] for r in rows} == set(statuses), (kind, trim)


def test_every_part_of_a_number_at_the_group_seams(px):
    check(px, pc.placed_rows())
    check(px, pc.placed_rows(), lead=b"#" * 5)       # (another alignment of every row)


def test_leading_and_trailing_zeros(px):
    check(px, pc.zero_rows())


def test_range_edges_and_long_integers(px):
    rows = pc.edge_rows()
    check(px, rows)
    assert pc.meaning(b"-9223372036854775809", pc.INT64, False)[0] == pc.RANGE and b"-9223372036854775809" in rows
    assert pc.meaning(b"18446744073709551616", pc.UINT64, False)[0] == pc.RANGE and b"18446744073709551616" in rows


def test_the_exact_window_of_the_doubles(px):
    rows = pc.window_rows()
    check(px, rows, kinds=(pc.FLOAT64,))
    for m in pc.MANTISSAS:
        for q in (-23, -22, 22, 23):
            ok = m <= (1 << 53) and abs(q) <= 22
            assert pc.meaning(b"%de%d" % (m, q), pc.FLOAT64, False)[0] == (pc.OK if ok else pc.INEXACT)


def test_the_boundary_table_has_floats_bits(px):
    rows = pc.boundary_table()
    check(px, rows, kinds=(pc.FLOAT64,), trims=(False,))
    assert sum(1 for r in rows if pc.meaning(r, pc.FLOAT64, False)[0] == pc.OK) > len(rows) * 0.8


def test_one_value_in_many_spellings_and_huge_exponents(px):
    rows = pc.spelling_rows()
    check(px, rows)
    assert {pc.meaning(r, pc.FLOAT64, False) for r in rows[:16]} == {(pc.OK, 0x3FF8000000000000)}
    assert pc.meaning(b"1e" + b"0" * 29 + b"5", pc.FLOAT64, False) == (pc.OK, 0x40F86A0000000000)


def test_blanks_with_and_without_trim(px):
    rows = pc.blank_rows()
    check(px, rows)
    assert pc.meaning(b" 12 ", pc.INT64, True) == (pc.OK, 12) and pc.meaning(b" 12 ", pc.INT64, False)[0] == pc.MALFORMED
    assert pc.meaning(b"1 2", pc.INT64, True)[0] == pc.MALFORMED


def test_nul_and_high_bytes_and_what_the_grammar_leaves_out(px):
    check(px, pc.byte_rows())


def test_a_seeded_random_mix(px):
    rows = pc.random_rows(3000, 20)
    check(px, rows)
    for kind in pc.KINDS:
        seen = {pc.meaning(r, kind, True)[0] for r in rows}
        assert len(seen) == 4, (kind, seen)


def test_index_lists_with_repeats_and_permutations(px):
    rows = pc.status_rows() + pc.blank_rows()
    rng = random.Random(5)
    perm = list(range(len(rows)))
    rng.shuffle(perm)
    for indices in (perm, [rng.randrange(len(rows)) for _ in range(150)], [3] * 70, []):
        check(px, rows, indices=indices)


def test_rows_at_the_texts_ends_and_long_rows(px):
    # a row at offset 0 and a row that ends at the last byte of a text whose length is no multiple of 16
    rows = [b"12345", b"-7.25", b"0" * 700 + b"1", b"1" + b"0" * 700, b"0." + b"0" * 699 + b"1", b"9" * 700 + b"x", b"4.5"]
    text, records = check(px, rows, lead=b"")
    assert records[0][0] == 0 and records[-1][1] == len(text) and len(text) % 16 != 0
    # a row of a MiB of zeros is a legal 0 (no split feeds: one walk)
    big = [b"0" * (1 << 20), b"0" * (1 << 20) + b"7", b"1" + b"0" * (1 << 20)]
    check(px, big, trims=(False,), splits=False)
    assert pc.meaning(big[0], pc.FLOAT64, False) == (pc.OK, 0) and pc.meaning(big[2], pc.INT64, False)[0] == pc.RANGE


def test_a_bad_row_refuses_the_call_and_nothing_is_written(px):
    text, records = pc.lay([b"1", b"22", b"333"])
    n = len(text)
    for bad_records, indices, first in (([(0, 1), (3, 2), (0, n + 1)], None, 1), ([(0, 1), (0, 1), (n, n + 1)], None, 2), (records, [0, 3, 1], 1),
                                        (records, [NONE], 0)):
        rc, summ, values, statuses = run(px, text, bad_records, indices, pc.INT64, False)
        assert rc == 0 and summ[5] == first and summ[:5] == [0] * 5
        assert values == [POISON] * len(values) and statuses == [POISON8] * len(statuses)


def test_unknown_kinds_and_flags_are_refused_up_front(px):
    assert [px.pe_known(k, 0) & 1 for k in (-1, 0, 1, 2, 3)] == [0, 1, 1, 1, 0]
    assert [px.pe_known(0, f) >> 1 for f in (0, 1, 2, 3, 0x80000000)] == [1, 1, 0, 0, 0]
    text, records = pc.lay([b"1"])
    assert run(px, text, records, None, 3, False)[0] == -2


# ------------------------------------------------------------------------------------------------ group_sums
def test_group_sums_and_group_counts_ok_equal_a_dict_on_cpu_tensors():
    import torch
    from rejit_amd import records
    rng = random.Random(7)
    for k, n_groups in ((0, 0), (0, 3), (1, 1), (40, 5), (300, 17)):
        group = [rng.randrange(n_groups) for _ in range(k)]
        ok = [rng.randrange(4) != 0 for _ in range(k)]
        ints = [rng.choice((rng.randrange(-1000, 1000), (1 << 63) - 1, -(1 << 63))) for _ in range(k)]
        want_sum, want_count = [0] * n_groups, [0] * n_groups
        for g, v, o in zip(group, ints, ok):
            if o:
                want_sum[g] = (want_sum[g] + v + (1 << 63)) % (1 << 64) - (1 << 63)     # int64 wraps
                want_count[g] += 1
        tg, tok = torch.tensor(group, dtype=torch.int64), torch.tensor(ok, dtype=torch.bool)
        sums = records.group_sums(tg, torch.tensor(ints, dtype=torch.int64), tok, n_groups)
        counts = records.group_counts_ok(tg, tok, n_groups)
        assert sums.dtype == torch.int64 and sums.tolist() == want_sum and counts.dtype == torch.int64 and counts.tolist() == want_count
        floats = [rng.randrange(-64, 64) * 0.25 for _ in range(k)]     # (sums of quarter integers are exact in any order)
        fsum = records.group_sums(tg, torch.tensor(floats, dtype=torch.float64), tok, n_groups)
        want_f = [0.0] * n_groups
        for g, v, o in zip(group, floats, ok):
            if o:
                want_f[g] += v
        assert fsum.dtype == torch.float64 and fsum.tolist() == want_f
        # status tensors work as `ok` too: status == 0
        status = torch.tensor([0 if o else 2 for o in ok], dtype=torch.uint8)
        assert records.group_sums(tg, torch.tensor(ints, dtype=torch.int64), status == 0, n_groups).tolist() == want_sum


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: 48 seeded random cases against a meaning written over std::string with strtod, split feeds included, exact
    allocations.  (The sanitizers' runtimes are linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("parse_exec", DEPS)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"48 cases" in r.stdout
