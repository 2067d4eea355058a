"""What the tests of RJ_PARSE_WIDE share (tests/test_record_parse_wide.py on the CPU, tests/test_gpu_record_parse_wide.py on the
GPU): the MEANING of a row under the flag, written in Python independently of rejit_amd/csrc/record_parse.h -- there is no
Eisel-Lemire product in this file --, and the rows both suites ask about.

    grammar, TRIM, EMPTY, MALFORMED, the integer kinds     parse_cases.meaning's: the flag is inert there
    S, q      decimal.Decimal of the mantissa: S its digits from the first non-zero one to the last, value = int(S) x 10^q
    decided   int(S) <= 2^64 - 1: the bits of float() of the whole row, RANGE when that is infinite
    bracket   else P, the longest prefix of S that fits 64 bits, r = len(S) - len(P): float() of P x 10^(q + r) and of
              (P + 1) x 10^(q + r); equal -> OK with it (and it IS float(row): asserted), both infinite -> RANGE, else -- and
              when P = 2^64 - 1 -- INEXACT"""
import decimal
import functools
import random
import struct

import parse_cases as pc
from parse_cases import EMPTY, FLOAT64, INEXACT, MALFORMED, MASK, OK, RANGE

TRIM, WIDE = 1, 4
INF = 0x7FF0000000000000
SIGN = 1 << 63


def bits_of(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def float_of(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def significant(mantissa, exponent):
    """-> (S as a str of digits, '' for zero; q): the value of a grammar's mantissa (bytes) x 10^exponent is int(S) x 10^q"""
    _, digits, e = decimal.Decimal(mantissa.decode("ascii")).as_tuple()
    text = "".join(map(str, digits)).lstrip("0")
    kept = text.rstrip("0")
    return kept, e + exponent + len(text) - len(kept)


def wide_meaning(row, kind, trim):
    """-> (status, the 64 bits of the value; 0 unless status is OK) under RJ_PARSE_WIDE"""
    if kind != FLOAT64:
        return pc.meaning(row, kind, trim)
    s = row.strip(b" \t") if trim else row
    if not s:
        return EMPTY, 0
    mt = pc._FLOAT.fullmatch(s)
    if not mt:
        return MALFORMED, 0
    sign, mantissa, exponent = mt.groups()
    S, q = significant(mantissa, int(exponent or b"0"))
    negative = SIGN if sign == b"-" else 0
    if not S:
        return OK, negative
    if len(S) <= 20 and int(S) <= MASK:                                      # decided
        bits = bits_of(float(s)) & ~SIGN
        return (RANGE, 0) if bits == INF else (OK, bits | negative)
    P = S[:20] if int(S[:20]) <= MASK else S[:19]
    r = len(S) - len(P)
    assert r >= 1 and int(P) <= MASK < int(S[:len(P) + 1])
    if int(P) == MASK:
        return INEXACT, 0
    low, high = bits_of(float("%se%d" % (P, q + r))), bits_of(float("%de%d" % (int(P) + 1, q + r)))
    if low != high:
        return INEXACT, 0
    if low == INF:
        return RANGE, 0
    assert low == bits_of(float(s)) & ~SIGN, row[:80]
    return OK, low | negative


meaning_of = functools.lru_cache(maxsize=None)(wide_meaning)


# ------------------------------------------------------------------------------------------------ the rows
def window_edge_rows():
    """what was just outside the old window: MANTISSAS x q in {-23, -22, 22, 23}, and four rows everybody meets"""
    rows = [b"%de%d" % (m, q) for m in pc.MANTISSAS for q in (-23, -22, 22, 23)]
    return rows + [b"1e23", b"0.1e-22", b"9007199254740993", b"0.30000000000000004"]


def range_rows():
    """the overflow and the subnormal edges"""
    return [b"1.7976931348623157e308", b"1.7976931348623158e308", b"1.7976931348623159e308", b"1e308", b"1e309", b"1e999999999999999999999",
            b"2.2250738585072014e-308", b"2.2250738585072011e-308", b"4.9406564584124654e-324", b"2.4703282292062327e-324",
            b"2.4703282292062328e-324", b"1e-400", b"-1e-400", b"5e-324", b"2e-324", b"3e-324", b"-1e309", b"-1.7976931348623159e308"]


def random_bits(count, seed):
    """uniformly random FINITE bit patterns"""
    rng, out = random.Random(seed), []
    while len(out) < count:
        b = rng.getrandbits(64)
        if (b >> 52) & 0x7FF != 0x7FF:
            out.append(b)
    return out


def repr_rows(count, seed):
    """repr() of random doubles -> (rows, their bits)"""
    bits = random_bits(count, seed)
    return [repr(float_of(b)).encode("ascii") for b in bits], bits


def spell(rng, digits, q):
    """the value int(digits) x 10^q in a random spelling: the point moved, zeros in front and behind, an exponent with leading
    zeros or none, a sign"""
    sign = rng.choice((b"", b"", b"-", b"+"))
    lead = b"0" * rng.choice((0, 0, 1, 3))
    shape = rng.randrange(4)
    if shape == 0:                                                           # digits e q
        return sign + lead + digits + b"e%d" % q
    if shape == 1:                                                           # the point inside the digits
        at = rng.randrange(len(digits) + 1)
        return sign + lead + digits[:at] + b"." + digits[at:] + b"E%+d" % (q + len(digits) - at)
    if shape == 2:                                                           # trailing zeros, an exponent with leading zeros
        z = rng.randrange(1, 5)
        e = q - z
        return sign + lead + digits + b"0" * z + b"e" + (b"-" if e < 0 else rng.choice((b"", b"+"))) + b"0" * rng.randrange(3) + b"%d" % abs(e)
    if -40 <= q <= 0:                                                        # no exponent at all: 0.000digits / dig.its000
        if -q >= len(digits):
            return sign + lead + b"0." + b"0" * (-q - len(digits)) + digits
        return sign + lead + digits[:len(digits) + q] + b"." + digits[len(digits) + q:] + b"0" * rng.randrange(3)
    if 0 < q <= 40:
        return sign + lead + digits + b"0" * q + rng.choice((b"", b".", b".00"))
    return sign + b"." + digits + b"e%d" % (q + len(digits))


def short_rows(count, seed):
    """random mantissas of 1 to 19 digits, q over [-345, 309], each in a random spelling"""
    rng, rows = random.Random(seed), []
    for _ in range(count):
        n = rng.randrange(1, 20)
        digits = b"%d" % rng.randrange(10 ** (n - 1), 10 ** n)
        rows.append(spell(rng, digits, rng.randrange(-345, 310)))
    return rows


def tie_rows(count, seed):
    """the exact decimals of (2 mant + 1) x 2^(e - 1) -- halfway between two neighbouring doubles -- for random 53-bit mant and
    the e at which the decimal fits 64 bits, and their neighbours +-1 in the last digit"""
    rng, rows = random.Random(seed), []
    while len(rows) < count:
        mant, e = rng.randrange(1 << 52, 1 << 53), rng.randrange(-9, 11)
        with decimal.localcontext() as ctx:
            ctx.prec = 80                                                    # (exact: 54 bits x 2^+-10 has far fewer digits)
            _, digits, exp10 = (decimal.Decimal(2 * mant + 1) * decimal.Decimal(2) ** (e - 1)).as_tuple()
        m = int("".join(map(str, digits)))
        if m + 1 > MASK:
            continue
        for x in (m - 1, m, m + 1):
            rows.append(b"%de%d" % (x, exp10) if rng.randrange(2) else spell(rng, b"%d" % x, exp10))
    return rows[:count]


def long_rows(count, seed):
    """random mantissas of 20 to 40 significant digits (the last one non-zero), q such that the value is a finite normal"""
    rng, rows = random.Random(seed), []
    for _ in range(count):
        n = rng.randrange(20, 41)
        digits = b"%d" % (rng.randrange(10 ** (n - 1), 10 ** n) | 1)
        rows.append(spell(rng, digits, rng.randrange(-300, 300 - n)))
    return rows


TENTH_EXACT = b"0.1000000000000000055511151231257827021181583404541015625"      # the double nearest 0.1, written out: 55 digits


def long_named_rows():
    return [TENTH_EXACT, b"1" + b"0" * 18 + b"5", b"18446744073709551615", b"18446744073709551616", b"184467440737095516155",
            b"9007199254740993" + b"." + b"0" * 19 + b"1", b"18446744073709551614" + b"9" * 30, b"1" + b"0" * 25 + b"5e-400", b"1" + b"0" * 25 + b"5e300",
            b"-1" + b"0" * 30 + b"1", b"123456789012345678901234567890e-20", b"1" + b"0" * 19 + b"1", b"1." + b"0" * 19 + b"1"]


def placed_wide_rows():
    """parse_cases.PLACES with 17- and 25-digit mantissas: the last digit that fits, the first one dropped and the end of the
    number at bytes 15 .. 33 of a row, behind zeros, blanks and a point"""
    rows = []
    for p in pc.PLACES:
        for digits in (b"12345678901234567", b"1234567890123456789012345", b"1844674407370955161" + b"7" * 6):
            n = len(digits)
            rows += [b"0" * p + digits, b" " * p + digits, b"0" * max(p - n, 0) + digits + b"e5", b"0" * max(p - n + 3, 0) + digits[:n - 3] + b"." + digits[n - 3:],
                     b"." + b"0" * (p - 1) + digits, digits[:5] + b"0" * p + digits[5:], b"-" + b"0" * (p - 1) + digits + b"E-30", digits + b"0" * p + b"x",
                     digits + b"0" * p, b"\t" * (p - 3) + b"+0." + digits + b"e+7 "]
    return rows


@functools.lru_cache(maxsize=None)
def mixed_rows():
    """the GPU test's pool, about 3000 rows: every family above and parse_cases' own"""
    rows = (pc.all_case_rows() + window_edge_rows() + range_rows() + long_named_rows() + placed_wide_rows() + repr_rows(500, 11)[0] + short_rows(500, 12)
            + tie_rows(300, 13) + long_rows(500, 14) + pc.random_rows(300, 15))
    random.Random(16).shuffle(rows)
    return tuple(rows)


def inexact_share(rows):
    """the share of INEXACT rows, by the meaning alone"""
    return sum(1 for r in rows if meaning_of(r, FLOAT64, False)[0] == INEXACT) / max(len(rows), 1)

