"""What the tests of rj_scan_records_parse share (tests/test_record_parse.py on the CPU, tests/test_gpu_record_parse.py on the
GPU): the MEANING of a row, written in Python independently of rejit_amd/csrc/record_parse.h, and the rows both suites ask
about.

    grammar   re.fullmatch of the three grammars over the row's bytes (trimmed of spaces and tabs first under TRIM)
    integers  int() of the row, and the type's range
    doubles   decimal.Decimal of the mantissa, its trailing zeros stripped, for (m, q); OK exactly when m == 0 or
              (m <= 2^53 and -22 <= q <= 22), and then the bits of Python's float() -- the correctly rounded value"""
import decimal
import random
import re
import struct

INT64, UINT64, FLOAT64 = 0, 1, 2
KINDS = (INT64, UINT64, FLOAT64)
KIND_NAMES = {INT64: "int64", UINT64: "uint64", FLOAT64: "float64"}
OK, EMPTY, MALFORMED, RANGE, INEXACT = range(5)
MASK = (1 << 64) - 1

_INT = re.compile(rb"[+-]?[0-9]+")
_UINT = re.compile(rb"\+?[0-9]+")
_FLOAT = re.compile(rb"([+-]?)([0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE]([+-]?[0-9]+))?")


HUGE = 10 ** 30      # decimal_value's m for a mantissa of more than 30 digits that count: far beyond every window and range


def decimal_value(mantissa, exponent):
    """the exact value mantissa x 10^exponent of a grammar's mantissa (bytes) as (m, q), m not divisible by 10 (0 for zero;
    HUGE stands for any m of more than 30 digits)"""
    _, digits, e = decimal.Decimal(mantissa.decode("ascii")).as_tuple()
    text = "".join(map(str, digits)).lstrip("0")
    kept = text.rstrip("0")
    q = e + exponent + len(text) - len(kept)
    return (int(kept) if len(kept) <= 30 else HUGE) if kept else 0, q


def meaning(row, kind, trim):
    """-> (status, the 64 bits of the value; 0 unless status is OK)"""
    s = row.strip(b" \t") if trim else row
    if not s:
        return EMPTY, 0
    if kind != FLOAT64:
        if not (_INT if kind == INT64 else _UINT).fullmatch(s):
            return MALFORMED, 0
        digits = s.lstrip(b"+-").lstrip(b"0")            # (int() has a limit of its own on the digits it reads: leading zeros go first)
        if len(digits) > 30:
            return RANGE, 0
        v = int(s[:1].strip(b"0123456789") + (digits or b"0"))
        lo, hi = (-(1 << 63), (1 << 63) - 1) if kind == INT64 else (0, MASK)
        return (OK, v & MASK) if lo <= v <= hi else (RANGE, 0)
    mt = _FLOAT.fullmatch(s)
    if not mt:
        return MALFORMED, 0
    sign, mantissa, exponent = mt.groups()
    m, q = decimal_value(mantissa, int(exponent or b"0"))
    if m == 0:
        return OK, (1 << 63) if sign == b"-" else 0
    if m <= (1 << 53) and -22 <= q <= 22:
        return OK, struct.unpack("<Q", struct.pack("<d", float(s)))[0]
    return INEXACT, 0


def lay(rows, lead=b"", sep_of=lambda i: b"|" * (i % 4), tail=b""):
    """the rows laid out one after another -> (text, records)"""
    text, records = bytearray(lead), []
    for i, s in enumerate(rows):
        text += sep_of(i)
        records.append((len(text), len(text) + len(s)))
        text += s
    return bytes(text + tail), records


# ------------------------------------------------------------------------------------------------ the rows
PLACES = (15, 16, 17, 31, 32, 33)
MANTISSAS = ((1 << 53) - 1, 1 << 53, (1 << 53) + 1)


def status_rows():
    """rows that between them have every status under every kind"""
    return [b"", b"0", b"7", b"-7", b"+7", b"x", b"-", b"+", b"1.5", b".", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808",
            b"-9223372036854775809", b"18446744073709551615", b"18446744073709551616", b"123456789012345678901234567890", b"1e23", b"1e22", b"1e-23",
            b"0.1", b"9007199254740993", b"-0", b"-0.0", b"3.14159", b"6.02e23", b"1e", b" ", b"\t", b" 5 "]


def placed_rows():
    """the sign, the point, the e, the exponent's sign, the first and the last digit at bytes 15, 16, 17, 31, 32, 33 of a row"""
    rows = []
    for p in PLACES:
        rows += [b" " * p + b"-12",                          # the sign (under TRIM)
                 b"\t" * p + b"42",                          # the first digit
                 b"0" * (p - 1) + b"7" + b".5",              # the point
                 b"0" * (p - 1) + b"7" + b"e5",              # the e
                 b"0" * (p - 2) + b"7E" + b"-3",             # the exponent's sign
                 b"0" * p + b"9",                            # the last digit
                 b"0" * (p - 3) + b"7e1" + b"2",             # the exponent's last digit
                 b"0" * (p - 2) + b"1." + b"5",              # the fraction's last digit
                 b"0" * p + b"x",                            # a bad byte there
                 b"1" * p + b"5"]                            # p + 1 digits that count
    return rows


def zero_rows():
    rows = []
    for z in range(41):
        rows += [b"0" * z + b"123", b"-" + b"0" * z + b"9223372036854775808", b"0" * z + b"18446744073709551615", b"0" * z + b".5", b"0" * z,
                 b"1" + b"0" * z, b"1." + b"0" * z, b"0." + b"0" * z + b"25"]
    return rows


def edge_rows():
    rows = []
    for edge in (-(1 << 63), (1 << 63) - 1, 0, (1 << 64) - 1):
        rows += [b"%d" % (edge + d) for d in (-1, 0, 1)]
        rows += [b"+%d" % (edge + d) for d in (0, 1) if edge + d >= 0]
    for digits in (19, 20, 21):
        rows += [b"9" * digits, b"-" + b"9" * digits, b"1" + b"0" * (digits - 1), b"-1" + b"0" * (digits - 1), b"18" + b"4" * (digits - 2),
                 b"1" * digits + b".0", b"1" * digits + b"e-3"]
    return rows


def window_rows():
    """m in {2^53 - 1, 2^53, 2^53 + 1} x q in {-23, -22, 22, 23}, in several spellings"""
    rows = []
    for m in MANTISSAS:
        for q in (-23, -22, 22, 23):
            rows += [b"%de%d" % (m, q), b"-%dE%+d" % (m, q), b"%d0e%d" % (m, q - 1), b"%d.%de%d" % (m // 10, m % 10, q + 1)]
        rows += [b"%d" % m, b"%d.0" % m, b"0.%d" % m, b"%d" % m + b"0" * 22, b"%d" % m + b"0" * 23]
    return rows


def boundary_table():
    """every q in [-22, 22] x the boundary mantissas and a few more: the rows that decide the division"""
    rng = random.Random(53)
    mantissas = list(MANTISSAS) + [1, 3, 7, 9, 123456789, (1 << 52) + 1, (1 << 53) - 3] + [rng.randrange(1 << 52, 1 << 53) | 1 for _ in range(12)]
    mantissas = [m if m % 10 else m + 1 for m in mantissas]
    return [b"%de%d" % (m, q) for q in range(-22, 23) for m in mantissas]


def spelling_rows():
    """one value, (15, -1), in many spellings -- and zeros with huge exponents, and exponents of 30 digits"""
    return [b"1.5", b"1.50", b"15e-1", b"0.0015e3", b"150e-2", b"1.5e0", b"1.5E+0", b"+1.5", b"01.5", b".15e1", b"0.15e+1", b"15.e-1", b"1500000e-6",
            b"0.00000000000000000000015e22", b"1500000000000000000000000e-24", b"1.5000000000000000000000000000000000000", b"-1.5", b"-15E-1",
            b"0e999", b"-0e999", b"0.000e-99999", b"00e+9999999999", b"-.0e5", b"0.e1", b"-0.0e-0", b"0e" + b"9" * 30, b"-0.00e-" + b"9" * 30,
            b"1e+" + b"1" * 30, b"1e-" + b"1" * 30, b"1e" + b"0" * 29 + b"5", b"25e-" + b"0" * 28 + b"03", b"1e" + b"9" * 30, b"1e4611686018427387904",
            b"1e-4611686018427387904", b"1e4611686018427387903", b"1e18446744073709551616", b"1e9223372036854775808"]


def blank_rows():
    return [b" 12", b"12 ", b" 12 ", b"\t12\t", b" \t 12 \t ", b"1 2", b"+ 1", b"- 1", b"1. 5", b"1 .5", b"1e 5", b"1 e5", b"1e+ 5", b" ", b"", b"  \t ",
            b"12\n", b"12\r", b"\n12", b"12\x0b", b"12\x0c", b" +1.5e3 ", b" . ", b" - ", b"1 \t", b"\t\t+0"]


def byte_rows():
    return [b"12\0", b"\0", b"\x0012", b"1\xff2", b"\xb1\xb2", b"\xef\xbc\x91", b"1\x80", b"\xff", b"12\0\0\0\0", b" \0 ", b"inf", b"nan", b"-inf",
            b"Infinity", b"NaN", b"0x10", b"1_000", b"1,5", b"++1", b"+-1", b"--1", b"1e", b"1e+", b"1e-", b"e5", b".", b"+.", b"-.", b"-", b"+", b"1.2.3",
            b"1e5e5", b"1e5.0", b"1-", b"1+1", b"1e5-", b".e1", b"1f", b"1d0", b"1L", b"0b1", b"1/2", b"$1", b"1%", b":", b"/", b"09", b"-09", b"\xd9\xa3"]


def random_rows(count, seed):
    """a seeded mix: numbers of every shape, some damaged, some nonsense"""
    rng = random.Random(seed)
    any_byte = b"0123456789+-.eE \t\0x_,"
    rows = []
    for _ in range(count):
        shape = rng.randrange(8)
        if shape == 0:
            rows.append(bytes(rng.choice(any_byte) for _ in range(rng.randrange(24))))
            continue
        s = bytearray()
        if rng.randrange(4) == 0:
            s += rng.choice(b" \t").to_bytes(1, "little") * rng.randrange(3)
        if rng.randrange(3) == 0:
            s += rng.choice((b"-", b"+"))
        if rng.randrange(4) == 0:
            s += b"0" * rng.randrange(40)
        s += bytes(rng.choice(b"0123456789") for _ in range(rng.randrange(8 if shape < 4 else 22)))
        if shape >= 5:
            if rng.randrange(3):
                s += b"." + bytes(rng.choice(b"0123456789") for _ in range(rng.randrange(8)))
                if rng.randrange(3) == 0:
                    s += b"0" * rng.randrange(20)
            if rng.randrange(3) == 0:
                s += rng.choice((b"e", b"E")) + rng.choice((b"", b"", b"-", b"+"))
                s += bytes(rng.choice(b"0123456789") for _ in range(1 + rng.randrange(2) if rng.randrange(4) else rng.randrange(30)))
        if rng.randrange(4) == 0:
            s += b" " * rng.randrange(3)
        if s and rng.randrange(16) == 0:
            s[rng.randrange(len(s))] = rng.choice(any_byte)
        rows.append(bytes(s))
    return rows


def all_case_rows():
    """every named family above, once"""
    return (status_rows() + placed_rows() + zero_rows() + edge_rows() + window_rows() + spelling_rows() + blank_rows() + byte_rows())
