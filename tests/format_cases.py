"""The meaning of rj_scan_records_format in Python, independent of rejit_amd/csrc/record_format.h: str(int), repr(float), the
layout arithmetic of a pack and the status rule -- nothing else -- and the value sets the CPU and the GPU tests share.  A
value is always the 64-BIT WORD the call reads (an int in [0, 2^64)): an int64 by two's complement, a uint64, a double's bits."""
import random
import struct

INT64, UINT64, FLOAT64 = 0, 1, 2
KINDS = (INT64, UINT64, FLOAT64)
KIND_NAMES = {INT64: "int64", UINT64: "uint64", FLOAT64: "float64"}
OK = 0                       # RJ_PARSE_OK: every other status makes the row empty
NOT_OK = (1, 2, 3, 4)        # RJ_PARSE_EMPTY, _MALFORMED, _RANGE, _INEXACT
MAX_ROW_BYTES = 24
MASK = (1 << 64) - 1
SIGN = 1 << 63
EXP_MASK = 0x7FF << 52


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def float_of(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def finite(bits: int) -> bool:
    return bits & EXP_MASK != EXP_MASK


def text_of(word: int, kind: int) -> bytes:
    """T(j): what Python writes for the value"""
    if kind == INT64:
        return str(word - (1 << 64) if word & SIGN else word).encode()
    if kind == UINT64:
        return str(word).encode()
    return repr(float_of(word)).encode()


def layout(words, kind, status=None, indices=None, fill=10, lead=0, gap=1):
    """-> (text, begins, ends) of the call over the column `words`"""
    rows = range(len(words)) if indices is None else indices
    out, begins, ends = bytearray(bytes([fill]) * lead), [], []
    for r in rows:
        t = text_of(words[r], kind) if status is None or status[r] == OK else b""
        begins.append(len(out))
        out += t
        ends.append(len(out))
        out += bytes([fill]) * gap
    return bytes(out), begins, ends


# ------------------------------------------------------------------------------------------------------------------ values
def int_words(seed=71, per_length=50):
    """0, +-1, 10^d - 1 / 10^d / 10^d + 1 for d in 1..19, the ends of both types, `per_length` random values of every bit length"""
    rng = random.Random(seed)
    vals = [0, 1, -1, -(1 << 63), (1 << 63) - 1, 1 << 63, (1 << 64) - 1]
    for d in range(1, 20):
        vals += [10 ** d - 1, 10 ** d, 10 ** d + 1, -(10 ** d - 1), -(10 ** d), -(10 ** d + 1)]
    vals += [10 ** 19 - 1 + (1 << 63)]
    for length in range(1, 65):
        for _ in range(per_length):
            vals.append(rng.getrandbits(length) | 1 << (length - 1))
    return [v & MASK for v in vals if -(1 << 63) <= v < (1 << 64)]


NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF4000000000123, 0x7FF00000DEADBEEF]
FORM_EDGES = [1e16, 9999999999999998.0, 1e-4, 9.999999999999999e-05, 123456789012345680.0, float(2 ** 53 - 1), float(2 ** 53), float(2 ** 53 + 2), 0.1 + 0.2,
              1e22, 1e23, 1000000000000000.5, 1.2345678901234568e+17, 5e-324, 1e-05, 0.0001, -2.9205048131065683e-196, 1.5, 100.0, 0.001, 123456.789]


def special_words():
    return [0, SIGN, 1, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000] + NANS + \
           [bits_of(x) for x in FORM_EDGES] + [bits_of(-x) for x in FORM_EDGES]


def power_of_two_words():
    """every 2^e, -1074 <= e <= 1023: the values whose lower neighbour is half as far as the upper one (for e > -1022)"""
    return [1 << (e + 1074) for e in range(-1074, -1022)] + [(e + 1023) << 52 for e in range(-1022, 1024)]


def power_of_ten_words():
    """every 1eN, -323 <= N <= 308, with both float neighbours"""
    words = []
    for n in range(-323, 309):
        b = bits_of(float("1e%d" % n))
        words += [b - 1, b, b + 1]
    return words


def random_bit_words(count=3000, seed=72):
    rng = random.Random(seed)
    return [rng.getrandbits(64) for _ in range(count)]


def decimal_words(count=3000, seed=73):
    """decimals of 1..17 random digits and a random exponent, through float()"""
    rng = random.Random(seed)
    words = []
    while len(words) < count:
        digits = str(rng.randrange(1, 10)) + "".join(str(rng.randrange(10)) for _ in range(rng.randrange(17)))
        x = float("%s%se%d" % (rng.choice(["", "-"]), digits, rng.randrange(-340, 310 - len(digits))))
        if x == x and abs(x) != float("inf"):
            words.append(bits_of(x))
    return words


def float_words():
    return special_words() + power_of_two_words() + power_of_ten_words() + random_bit_words() + decimal_words()


def words_of(kind):
    return float_words() if kind == FLOAT64 else int_words()


def gpu_words(kind, count=3000, seed=74):
    """about `count` DISTINCT values of the kind for the device tests: the named ones first, a seeded sample of the rest"""
    if kind != FLOAT64:
        return sorted(set(int_words(per_length=45)))[:count] if kind == UINT64 else sorted(set(int_words(seed=75, per_length=45)))[:count]
    named = special_words() + power_of_ten_words()[::7]
    rest = power_of_two_words() + random_bit_words(1200) + decimal_words(1200)
    rng = random.Random(seed)
    rng.shuffle(rest)
    seen, out = set(), []
    for w in named + rest:
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out[:count]


def status_column(n, seed=76):
    """a status per value: mostly OK, every non-OK code among the rest"""
    rng = random.Random(seed)
    return [OK if rng.randrange(4) else NOT_OK[rng.randrange(4)] for _ in range(n)]
