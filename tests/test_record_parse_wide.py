"""CPU tests of RJ_PARSE_WIDE (rejit_amd/csrc/record_parse.h, pow5_table.h): a FLOAT64 row outside Clinger's window gets its
correctly rounded double by the Eisel-Lemire product, or a status -- RANGE when the double is infinite, INEXACT only when more
than 64 bits of mantissa leave the rounding open.

The header is compiled with g++ into the test-only driver tests/support/parse_wide_exec.cc: parse_exec.cc's discipline (the
rows checked first, every access to the text checked against its range, every row fed AGAIN at every split of its bytes into
two runs of groups, poisoned outputs) with the whole flags word handed through.  The expectation is
tests/parse_wide_cases.py's meaning, written in Python independently of the header: re.fullmatch of the grammar,
decimal.Decimal for S and q, float() for the bits of the whole row or of the two ends of the bracket.  All comparisons are
exact."""
import ctypes
import importlib.util
import os
import subprocess

import pytest

import parse_cases as pc
import parse_wide_cases as pw
from exec_build import _arr, headers, sanitized_program, shared_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPS = headers(("record_parse.h", "pow5_table.h", "record_rows.h", "record_pack.h"), ("checked_text.h",))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 3
F = pc.FLOAT64


@pytest.fixture(scope="module")
def px():
    lib = shared_driver("parse_wide_exec", DEPS)
    u64, cp, ci, cu = ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.pwe_known.argtypes = [ci, cu]
    lib.pwe_table.argtypes = [_u64p, ci]
    lib.pwe_state_bytes.restype = u64
    lib.pwe_parse.restype = ctypes.c_long
    lib.pwe_parse.argtypes = [cp, u64, _u64p, _u64p, u64, _u64p, ci, u64, ci, cu, ci, _u64p, _u8p, _u64p]
    return lib


def run(lib, text, records, indices, kind, flags, splits=True, with_status=True):
    """-> (rc, summary, values, statuses: the whole poisoned buffers)"""
    k = len(records) if indices is None else len(indices)
    values, statuses = _arr([POISON] * (k + ROOM)), _arr([POISON8] * (k + ROOM), ctypes.c_uint8)
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.pwe_parse(text, len(text), _arr([b for b, _ in records]), _arr([e for _, e in records]), len(records), None if indices is None else _arr(indices),
                       int(indices is not None), 0 if indices is None else len(indices), kind, flags, int(splits), values,
                       statuses if with_status else None, summ)
    return rc, [int(x) for x in summ], list(values), list(statuses)


def check(lib, rows, kinds=(F,), trims=(False, True), wide=True, lead=b"", tail=b"", splits=True):
    """the rows laid into one text, parsed under every kind and TRIM setting with (or without) WIDE, against the meaning"""
    text, records = pc.lay(rows, lead=lead, tail=tail)
    M = pw.meaning_of if wide else pc.meaning
    for kind in kinds:
        for trim in trims:
            want = [M(r, kind, trim) for r in rows]
            flags = (pw.TRIM if trim else 0) | (pw.WIDE if wide else 0)
            for with_status in (True, False):
                rc, summ, values, statuses = run(lib, text, records, None, kind, flags, splits, with_status)
                ctx = (kind, flags, with_status)
                assert rc == 0, ("an access left its range, a row was written twice or a split feed differed", rc, ctx)
                k = len(want)
                for j, (w, v, s) in enumerate(zip(want, values, statuses)):
                    assert (w[1], w[0] if with_status else POISON8) == (v, s), (ctx, j, rows[j][:80], w, (s, hex(v)))
                assert values[k:] == [POISON] * ROOM and statuses[k:] == [POISON8] * ROOM, ctx
                assert summ[:5] == [sum(1 for w in want if w[0] == c) for c in range(5)] and summ[5] == NONE, (ctx, summ)
                if splits:
                    assert summ[6] == sum(max(len(r) - 1, 0) for r in rows), ctx
    return text, records


# ------------------------------------------------------------------------------------------------ the meaning itself
def test_the_python_meaning_on_rows_whose_answer_is_known_by_hand():
    M = pw.wide_meaning
    assert M(b"0.30000000000000004", F, False) == (pc.OK, 0x3FD3333333333334) and M(b"1e23", F, False) == (pc.OK, 0x44B52D02C7E14AF6)
    assert M(b"9007199254740993", F, False) == (pc.OK, 0x4340000000000000)                     # the tie goes to the even neighbour
    assert M(b"1.7976931348623158e308", F, False) == (pc.OK, 0x7FEFFFFFFFFFFFFF) and M(b"1.7976931348623159e308", F, False) == (pc.RANGE, 0)
    assert M(b"1e309", F, False) == (pc.RANGE, 0) and M(b"-1e-400", F, False) == (pc.OK, 1 << 63) and M(b"5e-324", F, False) == (pc.OK, 1)
    assert M(b"2.4703282292062327e-324", F, False) == (pc.OK, 0) and M(b"2.4703282292062328e-324", F, False) == (pc.OK, 1)
    assert M(b"18446744073709551615", F, False) == M(b"18446744073709551616", F, False) == (pc.OK, 0x43F0000000000000)
    assert M(b"184467440737095516155", F, False) == (pc.INEXACT, 0)                            # P = 2^64 - 1
    assert M(b"9007199254740993." + b"0" * 19 + b"1", F, False) == (pc.INEXACT, 0)             # just above a tie, beyond 64 bits
    assert M(pw.TENTH_EXACT, F, False) == (pc.OK, pw.bits_of(0.1)) and M(b"1" + b"0" * 18 + b"5", F, False)[0] == pc.OK
    assert M(b" 1e23 ", F, True)[0] == pc.OK and M(b" 1e23 ", F, False) == (pc.MALFORMED, 0) and M(b"", F, True) == (pc.EMPTY, 0)
    assert M(b"9223372036854775808", pc.INT64, False) == (pc.RANGE, 0)                         # the integer kinds: parse_cases.meaning
    assert pw.significant(b"0.0015", 3) == ("15", -1) and pw.significant(b"000", 7) == ("", 7)


# ------------------------------------------------------------------------------------------------ the old rows under WIDE
def test_every_existing_row_set_under_wide(px):
    """all_case_rows() for all kinds and both TRIM settings: the integer kinds equal parse_cases.meaning (the flag is inert), the
    doubles equal the wide meaning, and every row that was OK without the flag keeps its bits"""
    rows = pc.all_case_rows()
    check(px, rows, kinds=pc.KINDS)
    for trim in (False, True):
        for kind in (pc.INT64, pc.UINT64):
            assert all(pw.wide_meaning(r, kind, trim) == pc.meaning(r, kind, trim) for r in rows)
        kept = [(pc.meaning(r, F, trim), pw.meaning_of(r, F, trim)) for r in rows]
        assert all(new == old for old, new in kept if old[0] != pc.INEXACT)
        assert sum(1 for old, new in kept if old[0] == pc.INEXACT and new[0] == pc.OK) > 40
    assert {pw.meaning_of(r, F, True)[0] for r in rows} == {pc.OK, pc.EMPTY, pc.MALFORMED, pc.RANGE}      # (none of them is left INEXACT)
    check(px, pc.random_rows(3000, 20), kinds=pc.KINDS)
    check(px, pc.boundary_table(), trims=(False,))


def test_the_same_rows_without_the_flag_are_as_before(px):
    check(px, pc.all_case_rows() + pw.window_edge_rows() + pw.range_rows() + pw.long_named_rows(), kinds=pc.KINDS, wide=False)


def test_the_old_windows_edges_become_ok(px):
    rows = pw.window_edge_rows()
    check(px, rows)
    assert all(pw.meaning_of(r, F, False)[0] == pc.OK for r in rows)
    assert sum(1 for r in rows if pc.meaning(r, F, False)[0] == pc.INEXACT) >= 10


def test_range_and_subnormal_edges(px):
    rows = pw.range_rows()
    check(px, rows)
    assert [pw.meaning_of(r, F, False)[0] for r in rows[:6]] == [pc.OK, pc.OK, pc.RANGE, pc.OK, pc.RANGE, pc.RANGE]
    assert all(pw.meaning_of(r, F, False)[0] == pc.OK for r in rows[6:16])


def test_repr_of_random_doubles_round_trips(px):
    rows, bits = pw.repr_rows(3000, 41)
    assert [pw.meaning_of(r, F, False) for r in rows] == [(pc.OK, b) for b in bits]
    check(px, rows, trims=(False,))


def test_random_short_mantissas_in_several_spellings(px):
    rows = pw.short_rows(3000, 42)
    check(px, rows)
    assert {pw.meaning_of(r, F, False)[0] for r in rows} == {pc.OK, pc.RANGE}


def test_tie_decimals_and_their_neighbours(px):
    rows = pw.tie_rows(2000, 43)
    check(px, rows, trims=(False,))
    assert all(pw.meaning_of(r, F, False)[0] == pc.OK for r in rows)
    triples = [[pw.meaning_of(r, F, False)[1] & ~pw.SIGN for r in rows[i:i + 3]] for i in range(0, 1998, 3)]
    assert all(a != c and b in (a, c) for a, b, c in triples)      # the neighbours of a tie round apart; the tie goes to one of them


def test_long_mantissas(px):
    rows = pw.long_rows(3000, 44)
    share = pw.inexact_share(rows)
    assert share < 0.01, share                                       # from the meaning alone, before the driver is asked
    check(px, rows)
    named = pw.long_named_rows()
    check(px, named)
    assert [pw.meaning_of(r, F, False)[0] for r in named[:6]] == [pc.OK, pc.OK, pc.OK, pc.OK, pc.INEXACT, pc.INEXACT]
    # a mantissa of a MiB of digits (one walk, no split feeds): far out of range, and scaled back to 1.11...
    big = [b"1" * (1 << 20), b"1" * (1 << 20) + b"e-1048575", b"0." + b"0" * (1 << 20) + b"7" * 30 + b"e1048577"]
    check(px, big, trims=(False,), splits=False)
    assert [pw.meaning_of(r, F, False)[0] for r in big] == [pc.RANGE, pc.OK, pc.OK]


def test_saturation_and_the_dropped_count_at_the_group_seams(px):
    rows = pw.placed_wide_rows()
    check(px, rows)
    check(px, rows, lead=b"#" * 5)       # (another alignment of every row)


def test_the_flag_word(px):
    assert [px.pwe_known(2, f) >> 1 for f in (0, 1, 4, 5)] == [1, 1, 1, 1]
    assert [px.pwe_known(2, f) >> 1 for f in (2, 3, 6, 8, 0x80000000)] == [0, 0, 0, 0, 0]
    text, records = pc.lay([b"1"])
    assert run(px, text, records, None, F, 6)[0] == -2 and run(px, text, records, None, F, 2)[0] == -2
    assert px.pwe_state_bytes() == 40


# ------------------------------------------------------------------------------------------------ the table
def test_the_power_table_is_what_the_generator_writes(px):
    spec = importlib.util.spec_from_file_location("gen_pow5_table", os.path.join(ROOT, "tools", "gen_pow5_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    words = (ctypes.c_uint64 * 1302)()
    assert px.pwe_table(words, 1302) == 651 == gen.ENTRIES
    table = gen.table()
    assert [int(x) for x in words] == [w for entry in table for w in entry]
    with open(os.path.join(ROOT, "rejit_amd", "csrc", "pow5_table.h")) as fh:
        assert fh.read() == gen.header_text()
    # the entries against the definition, with Python integers
    for q, (hi, lo) in zip(range(-342, 309), table):
        c = hi << 64 | lo
        assert c >> 127 == 1
        if q >= 0:
            p, bits = 5 ** q, (5 ** q).bit_length()
            assert c == (p >> (bits - 128) if bits >= 128 else p << (128 - bits))      # the floor of the normalised power
        else:
            p = 5 ** -q
            b = 127 + p.bit_length()
            assert (c - 1) * p <= 1 << b < (c + 1) * p               # 2^b / 5^-q, rounded up (within the truncation's one unit)


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: a fixed set of rows -- the edges above by name, and seeded digits of 17, 1 to 19 and 20 to 40 places -- under
    WIDE and WIDE | TRIM against a meaning written over std::string with strtod, split feeds included, exact allocations.  (The
    sanitizers' runtimes are linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("parse_wide_exec", DEPS)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"parse_wide_exec: 2478 cases" in r.stdout
