"""CPU tests of rj_scan_records_format's arithmetic (rejit_amd/csrc/record_format.h, pow10_table.h): a 64-bit value written as
Python writes it -- str(int), repr(float) -- into the layout of a pack.

The header is compiled with g++ into the test-only driver tests/support/format_exec.cc, which walks a call as the kernels do
(the index check, the plan unit by unit, the emit chunk by chunk through an image of the chunk), checks every access against
its range and every byte and row against a second write, and produces every row's bytes ALSO piecewise at every split.  The
expectation is tests/format_cases.py: str(), repr() and the layout arithmetic, independent of the header.  All comparisons are
exact."""
import ctypes
import importlib.util
import os
import subprocess

import pytest

import format_cases as fc
from exec_build import _arr, headers, sanitized_program, shared_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPS = headers(("record_format.h", "pow10_table.h", "record_parse.h", "pow5_table.h", "record_pack.h"), ("checked_text.h",))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 3          # spare table rows
ROOM_BYTES = 37   # spare output bytes
FLOAT_WIDE = 4    # RJ_PARSE_WIDE
REFUSALS = {"fine": 0, "null": 1, "table_align": 2, "out_align": 3, "kind": 4, "flags": 5, "fill": 6, "sums": 7, "too_many": 8}


@pytest.fixture(scope="module")
def fx():
    lib = shared_driver("format_exec", DEPS)
    u64, ci, cu, vp = ctypes.c_uint64, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p
    lib.fe_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.fe_table.argtypes = [_u64p, ci]
    lib.fe_row.argtypes = [u64, ci, _u8p, _u64p]
    lib.fe_parse.argtypes = [_u8p, ctypes.c_uint32, ci, cu, _u64p]
    lib.fe_format.restype = ctypes.c_long
    lib.fe_format.argtypes = [vp, vp, u64, vp, ci, u64, ci, cu, ci, u64, u64, u64, u64, vp, u64, vp, vp, _u64p]
    return lib


def constants(lib):
    out = (ctypes.c_int64 * 4)()
    lib.fe_constants(out)
    return [int(x) for x in out]


def row_of(lib, word, kind):
    """-> the row's bytes by the header (whole and piecewise, compared by the driver)"""
    buf, small = (ctypes.c_uint8 * 24)(*([POISON8] * 24)), (ctypes.c_uint64 * 2)()
    n = lib.fe_row(word, kind, buf, small)
    assert 1 <= n <= 24, ("a piecewise production differed from the whole, or the length is out of range", n, hex(word), kind)
    assert list(buf[n:]) == [POISON8] * (24 - n)
    return bytes(buf[:n])


def parse_back(lib, row, kind):
    bits = ctypes.c_uint64(POISON)
    status = lib.fe_parse((ctypes.c_uint8 * max(len(row), 1))(*row), len(row), kind, FLOAT_WIDE, ctypes.byref(bits))
    return status, int(bits.value)


def aligned_bytes(n, align=16, shift=0):
    """-> (keep-alive, address): n poisoned bytes at an address that is `shift` past a multiple of `align`"""
    raw = (ctypes.c_uint8 * (n + 2 * align))(*([POISON8] * (n + 2 * align)))
    base = ctypes.addressof(raw)
    return raw, (base + align - 1) // align * align + shift


def run(lib, words, kind, status=None, indices=None, fill=10, lead=0, gap=1, unit=256, chunk=4096, cap=None, flags=0, with_begin=True, with_end=True,
        n_values=None, out_shift=0, table_shift=0, value_null=False):
    """-> (rc, summary, out bytes with the spare ones, begins, ends with the spare rows)"""
    k = len(words) if indices is None else len(indices)
    if cap is None:
        cap = len(fc.layout(words, kind, status, indices, fill, lead, gap)[0])
    keep, out = aligned_bytes(cap + ROOM_BYTES, 16, out_shift)
    begins, ends = _arr([POISON] * (k + ROOM + 1)), _arr([POISON] * (k + ROOM + 1))
    summ = (ctypes.c_uint64 * 8)()
    values = _arr(words)
    st = None if status is None else _arr(status, ctypes.c_uint8)
    idx = None if indices is None else _arr(indices)
    rc = lib.fe_format(None if value_null else ctypes.addressof(values) + table_shift, None if st is None else ctypes.addressof(st),
                       len(words) if n_values is None else n_values, None if idx is None else ctypes.addressof(idx), int(indices is not None),
                       0 if indices is None else len(indices), kind, flags, fill, lead, gap, unit, chunk, out if cap or out_shift else None, cap,
                       ctypes.addressof(begins) if with_begin else None, ctypes.addressof(ends) if with_end else None, summ)
    got = bytes((ctypes.c_uint8 * (cap + ROOM_BYTES)).from_address(out))
    return rc, [int(x) for x in summ], got, list(begins), list(ends), keep


def check(lib, words, kind, status=None, indices=None, fill=10, lead=0, gap=1, **kw):
    text, begins, ends = fc.layout(words, kind, status, indices, fill, lead, gap)
    rc, summ, got, gb, ge, _ = run(lib, words, kind, status, indices, fill, lead, gap, **kw)
    ctx = (kind, indices is not None, status is not None, fill, lead, gap, kw)
    assert rc == 0, ("an access left its range, or a byte or a row was written twice", rc, ctx)
    k = len(begins)
    assert summ[0] == len(text) and summ[1] == NONE, (ctx, summ)
    assert got[:len(text)] == text, (ctx, next(i for i in range(len(text)) if got[i] != text[i]))
    assert got[len(text):] == bytes([POISON8]) * ROOM_BYTES, ctx
    if kw.get("with_begin", True):
        assert gb[:k] == begins and gb[k:] == [POISON] * (ROOM + 1), ctx
    else:
        assert gb == [POISON] * (k + ROOM + 1), ctx
    if kw.get("with_end", True):
        assert ge[:k] == ends and ge[k:] == [POISON] * (ROOM + 1), ctx
    else:
        assert ge == [POISON] * (k + ROOM + 1), ctx
    return summ


# ------------------------------------------------------------------------------------------------ the meaning itself
def test_the_python_meaning_on_values_whose_text_is_known_by_hand():
    T = fc.text_of
    assert T(0, fc.INT64) == b"0" and T(fc.MASK, fc.INT64) == b"-1" and T(fc.MASK, fc.UINT64) == b"18446744073709551615"
    assert T(fc.SIGN, fc.INT64) == b"-9223372036854775808" and T(fc.SIGN, fc.UINT64) == b"9223372036854775808" and T(fc.SIGN, fc.FLOAT64) == b"-0.0"
    F = lambda x: T(fc.bits_of(x), fc.FLOAT64)
    assert [F(x) for x in (1e16, 9999999999999998.0, 1e-4, 1e-5, 1000000000000000.5, 1.2345678901234568e+17, 5e-324)] == \
        [b"1e+16", b"9999999999999998.0", b"0.0001", b"1e-05", b"1000000000000000.5", b"1.2345678901234568e+17", b"5e-324"]
    assert [T(w, fc.FLOAT64) for w in (0x7FF0000000000000, 0xFFF0000000000000)] == [b"inf", b"-inf"] and {T(w, fc.FLOAT64) for w in fc.NANS} == {b"nan"}
    assert fc.layout([5, 12], fc.INT64, [0, 0], None, 10, 2, 1) == (b"\n\n5\n12\n", [2, 4], [3, 6])
    assert fc.layout([5, 12, 7], fc.INT64, [0, 3, 0], [2, 1, 0, 0], 0x2C, 0, 1) == (b"7,,5,5,", [0, 2, 3, 5], [1, 2, 4, 6])


# ------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("kind", [fc.INT64, fc.UINT64])
def test_integers_are_str_of_int_and_read_back(fx, kind):
    words = fc.int_words()
    assert len(words) > 3300
    lengths = set()
    for w in words:
        row = row_of(fx, w, kind)
        assert row == fc.text_of(w, kind), (hex(w), kind, row)
        assert parse_back(fx, row, kind) == (fc.OK, w), (hex(w), kind, row)
        lengths.add(len(row))
    assert lengths == set(range(1, 21))


def floats_checked(fx, words):
    longest = 0
    for w in words:
        row = row_of(fx, w, fc.FLOAT64)
        assert row == fc.text_of(w, fc.FLOAT64), (hex(w), row)
        if fc.finite(w):
            assert parse_back(fx, row, fc.FLOAT64) == (fc.OK, w), (hex(w), row)      # the header's own wide walk gives the bits back
        else:
            assert parse_back(fx, row, fc.FLOAT64)[0] == 2, row                      # MALFORMED: parse has digits only
        longest = max(longest, len(row))
    return longest


def test_named_doubles_are_repr_of_float(fx):
    assert floats_checked(fx, fc.special_words()) == fc.MAX_ROW_BYTES == constants(fx)[0] == 24
    got = {x: row_of(fx, fc.bits_of(x), fc.FLOAT64) for x in (1e16, 1e-4, 9.999999999999999e-05, 123456789012345680.0, 0.1 + 0.2, 1e22, 1e23, -0.0)}
    assert got == {1e16: b"1e+16", 1e-4: b"0.0001", 9.999999999999999e-05: b"9.999999999999999e-05", 123456789012345680.0: b"1.2345678901234568e+17",
                   0.1 + 0.2: b"0.30000000000000004", 1e22: b"1e+22", 1e23: b"1e+23", -0.0: b"-0.0"}


def test_every_power_of_two(fx):
    words = fc.power_of_two_words()
    assert len(words) == 2098 and fc.float_of(words[0]) == 5e-324 and fc.float_of(words[-1]) == 2.0 ** 1023
    floats_checked(fx, words)
    floats_checked(fx, [w | fc.SIGN for w in words[::17]])


def test_every_power_of_ten_with_its_neighbours(fx):
    words = fc.power_of_ten_words()
    assert len(words) == 3 * 632
    floats_checked(fx, words)


def test_random_bit_patterns_and_random_decimals(fx):
    longest = max(floats_checked(fx, fc.random_bit_words()), floats_checked(fx, fc.decimal_words()))
    assert longest == fc.MAX_ROW_BYTES == constants(fx)[0]      # the longest repr met is the header's constant


# ------------------------------------------------------------------------------------------------ the call
@pytest.mark.parametrize("kind", fc.KINDS)
def test_layouts(fx, kind):
    words = fc.words_of(kind)[:600] + fc.words_of(kind)[-400:]
    for lead in (0, 5):
        for gap in (0, 1, 3, 40):
            for fill in (10, 0x2C):
                check(fx, words, kind, fill=fill, lead=lead, gap=gap, chunk=4096 if gap != 3 else 64)


@pytest.mark.parametrize("kind", fc.KINDS)
def test_row_counts_around_a_unit_and_index_lists(fx, kind):
    words = fc.words_of(kind)
    for k in (0, 1, 255, 256, 257):
        check(fx, words[:k], kind, lead=5 if k == 0 else 0)
        check(fx, words[:300], kind, indices=list(range(k)))
    perm = list(range(300))
    import random
    random.Random(5).shuffle(perm)
    check(fx, words[:300], kind, indices=perm)
    check(fx, words[:300], kind, indices=[7, 7, 7, 299, 0, 7, 299] * 40, gap=0)
    check(fx, words[:300], kind, indices=[])


@pytest.mark.parametrize("kind", fc.KINDS)
def test_a_status_column_makes_empty_rows(fx, kind):
    words = fc.words_of(kind)[:700]
    status = fc.status_column(len(words))
    assert set(status) == {0, 1, 2, 3, 4}
    for gap in (0, 1):
        check(fx, words, kind, status=status, gap=gap)
        check(fx, words, kind, status=status, indices=[699, 0, 5, 5, 300] * 30, gap=gap, fill=0x2C)
    check(fx, words[:40], kind, status=[3] * 40, gap=0, lead=5)      # no row has a byte: the text is the lead


@pytest.mark.parametrize("kind", fc.KINDS)
def test_the_size_query_a_short_output_and_missing_tables(fx, kind):
    words = fc.words_of(kind)[:500]
    text, begins, ends = fc.layout(words, kind)
    rc, summ, got, gb, ge, _ = run(fx, words, kind, cap=0)                       # the size query: the tables are still written
    assert rc == 0 and summ[0] == len(text) and got == bytes([POISON8]) * ROOM_BYTES and gb[:500] == begins and ge[:500] == ends
    for cap in (len(text) - 1, len(text) - 17, 100, 1):
        rc, summ, got, gb, ge, _ = run(fx, words, kind, cap=cap)                 # nothing at or beyond out_cap is written, total is returned
        assert rc == 0 and summ[0] == len(text) and got[:cap] == text[:cap] and got[cap:] == bytes([POISON8]) * ROOM_BYTES, cap
        assert gb[:500] == begins and ge[:500] == ends
    check(fx, words, kind, with_begin=False)
    check(fx, words, kind, with_end=False)
    check(fx, words, kind, with_begin=False, with_end=False)


def test_refusals_leave_everything_poisoned(fx):
    words = fc.int_words()[:300]

    def refused(want, **kw):
        kw.setdefault("cap", 64)
        rc, summ, got, gb, ge, _ = run(fx, words, kw.pop("kind", fc.INT64), **kw)
        assert (rc, summ[7]) == (-2, REFUSALS[want]), (want, rc, summ)
        assert set(got) <= {POISON8} and set(gb) == {POISON} and set(ge) == {POISON}, want

    refused("kind", kind=3)
    refused("kind", kind=-1)
    for flags in (1, 2, 4, 0x80000000):
        refused("flags", flags=flags)
    refused("fill", fill=256)
    refused("fill", fill=-1)
    refused("sums", gap=1 << 42, cap=64)
    refused("sums", lead=1 << 62, cap=64)
    refused("sums", gap=(1 << 54), cap=64)
    refused("out_align", out_shift=8, cap=64)
    refused("table_align", table_shift=4, cap=64)
    refused("null", value_null=True, cap=64)
    refused("too_many", n_values=1 << 31)                      # (refused before anything is read)
    refused("too_many", n_values=1 << 40)
    # a bad index: the call is refused by its first kernel -- no byte, no table row -- and names the FIRST bad row
    for indices, first in (([0, 1, 300, 2, 999], 2), ([5] * 700 + [1 << 40] + [5, 300], 700), ([NONE], 0)):
        rc, summ, got, gb, ge, _ = run(fx, words, fc.INT64, indices=indices, cap=64)
        assert rc == 0 and summ[1] == first, (summ, first)
        assert set(got) <= {POISON8} and set(gb) == {POISON} and set(ge) == {POISON}


# ------------------------------------------------------------------------------------------------ the table
def test_the_power_table_is_what_the_generator_writes(fx):
    spec = importlib.util.spec_from_file_location("gen_pow10_table", os.path.join(ROOT, "tools", "gen_pow10_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    words = (ctypes.c_uint64 * 1234)()
    assert fx.fe_table(words, 1234) == 617 == gen.ENTRIES and constants(fx)[1:3] == [617, gen.K_MIN]
    table = gen.table()
    assert [int(x) for x in words] == [w for entry in table for w in entry]
    for k, (hi, lo) in zip(range(gen.K_MIN, gen.K_MAX + 1), table):      # from the definition: (g - 1) 2^r <= 10^k < g 2^r, 2^127 <= g < 2^128
        g = hi << 64 | lo
        assert 1 << 127 <= g < 1 << 128, k
        num, den = (10 ** k, 1) if k >= 0 else (1, 10 ** -k)             # 10^k = num / den
        r = (num.bit_length() - 1 if k >= 0 else -den.bit_length()) - 127
        two_r_num, two_r_den = (1 << r, 1) if r >= 0 else (1, 1 << -r)
        assert (g - 1) * two_r_num * den <= num * two_r_den < g * two_r_num * den, k
    with open(os.path.join(ROOT, "rejit_amd", "csrc", "pow10_table.h")) as fh:
        assert fh.read() == gen.header_text()


def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: named and seeded values of every kind, every power of two, against std::to_chars' shortest digits, rows whole
    and piecewise, and the call over allocations that are exact in their last byte.  (The sanitizers' runtimes are linked
    statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("format_exec", DEPS)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"format_exec: 72888 cases" in r.stdout
