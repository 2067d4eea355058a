"""CPU tests of rj_scan_records_zip's arithmetic (rejit_amd/csrc/record_zip.h): the rows of several record tables put side by
side into lines, laid out as a pack.

The header is compiled with g++ into the test-only driver tests/support/zip_exec.cc, which walks a call as the kernels do (the
resolve, the plan unit by unit, the emit chunk by chunk through an image of the chunk and the streamed groups), checks every
access against its range and every byte and row against a second write, and makes rows again at every possible cut.  The
expectation is tests/zip_cases.py: sep.join of rjust / ljust and the layout arithmetic, independent of the header.  All
comparisons are exact."""
import ctypes
import random
import subprocess

import pytest

import zip_cases as zc
from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_zip.h", "record_rows.h", "record_pack.h", "record_group.h"), ("checked_text.h", "checked_table.h"))
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 3          # spare table rows
ROOM_BYTES = 37   # spare output bytes
CODES = {name: i for i, name in enumerate(("fine", "null", "columns", "row_counts", "sep", "width", "reserved", "flags", "pad", "fill", "table_align",
                                           "out_align", "sums", "too_many"))}


class Column(ctypes.Structure):
    _fields_ = [("text", ctypes.c_void_p), ("n", ctypes.c_uint64), ("rec_begin", ctypes.c_void_p), ("rec_end", ctypes.c_void_p), ("n_records", ctypes.c_uint64),
                ("indices", ctypes.c_void_p), ("n_indices", ctypes.c_uint64), ("width", ctypes.c_int32), ("reserved", ctypes.c_int32)]


@pytest.fixture(scope="module")
def zx():
    lib = shared_driver("zip_exec", DEPS)
    u64, ci, cu, vp = ctypes.c_uint64, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p
    lib.ze_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.ze_bad_word_before.argtypes = [u64, ctypes.c_uint32, u64, ctypes.c_uint32]
    lib.ze_zip.restype = ctypes.c_long
    lib.ze_zip.argtypes = [vp, ci, vp, u64, ci, cu, ci, u64, u64, u64, u64, vp, u64, vp, vp, ctypes.POINTER(u64), ctypes.c_char_p]
    lib.ze_row_cuts.restype = ctypes.c_long
    lib.ze_row_cuts.argtypes = [vp, ci, vp, u64, ci, u64, vp, u64]
    return lib


def aligned_bytes(n, align=16, shift=0):
    raw = (ctypes.c_uint8 * (n + 2 * align))(*([POISON8] * (n + 2 * align)))
    base = ctypes.addressof(raw)
    return raw, (base + align - 1) // align * align + shift


class Call:
    """columns: a list of (text, begins, ends) or (text, begins, ends, indices) in Python values -> the driver's arguments, kept alive"""

    def __init__(self, columns, widths=None, reserved=None, table_shift=None, text_null=None, table_null=None, n_override=None):
        self.columns = [tuple(c) for c in columns]
        self.widths = [0] * len(columns) if widths is None else list(widths)
        self.keep = []
        self.cols = (Column * max(len(columns), 1))()
        shared = {}
        for c, col in enumerate(self.columns):
            text, begins, ends = col[:3]
            indices = col[3] if len(col) == 4 else None
            key = id(text)
            if key not in shared:
                t = (ctypes.c_uint8 * max(len(text), 1))(*text)
                shared[key] = (t, _arr(begins), _arr(ends))
                self.keep.append(shared[key])
            t, b, e = shared[key]
            idx = None if indices is None else _arr(indices)
            self.keep.append(idx)
            shift = table_shift if table_shift is not None and table_shift[0] == c else None
            self.cols[c] = Column(None if text_null == c else ctypes.addressof(t), len(text) if n_override is None else n_override[c],
                                  None if table_null == c else ctypes.addressof(b) + (shift[1] if shift else 0), None if table_null == c else ctypes.addressof(e),
                                  len(begins), None if idx is None else ctypes.addressof(idx), 0 if indices is None else len(indices), self.widths[c],
                                  0 if reserved is None else reserved[c])

    def meaning(self, sep, pad):
        cols = [zc.pieces(c[0], c[1], c[2], c[3] if len(c) == 4 else None) for c in self.columns]
        return zc.lines(cols, sep, self.widths, pad)


def run(lib, call, sep=b"", pad=32, fill=10, lead=0, gap=1, unit=256, chunk=4096, cap=None, flags=0, with_begin=True, with_end=True, out_shift=0,
        n_cols=None, sep_len=None, sep_null=False, k=None, out_table_shift=0):
    """-> (rc, summary, message, out bytes with the spare ones, begins, ends with the spare rows)"""
    n_cols = len(call.columns) if n_cols is None else n_cols
    if k is None:
        k = len(call.meaning(sep, pad)) if call.columns else 0
    if cap is None:
        cap = len(zc.layout(call.meaning(sep, pad), fill, lead, gap)[0])
    keep, out = aligned_bytes(cap + ROOM_BYTES, 16, out_shift)
    begins, ends = _arr([POISON] * (k + ROOM + 1)), _arr([POISON] * (k + ROOM + 1))
    summ = (ctypes.c_uint64 * 8)()
    msg = ctypes.create_string_buffer(320)
    sep_buf = ctypes.create_string_buffer(bytes(sep), max(len(sep), 1))
    rc = lib.ze_zip(ctypes.addressof(call.cols), n_cols, None if sep_null else ctypes.addressof(sep_buf), len(sep) if sep_len is None else sep_len, pad, flags,
                    fill, lead, gap, unit, chunk, out if cap or out_shift else None, cap,
                    ctypes.addressof(begins) + out_table_shift if with_begin else None, ctypes.addressof(ends) if with_end else None, summ, msg)
    got = bytes((ctypes.c_uint8 * (cap + ROOM_BYTES)).from_address(out))
    return rc, [int(x) for x in summ], msg.value.decode(), got, list(begins), list(ends), keep


def check(lib, columns, widths=None, sep=b"", pad=32, fill=10, lead=0, gap=1, **kw):
    call = Call(columns, widths)
    text, begins, ends = zc.layout(call.meaning(sep, pad), fill, lead, gap)
    rc, summ, msg, got, gb, ge, _ = run(lib, call, sep, pad, fill, lead, gap, **kw)
    ctx = (len(columns), widths, sep, pad, fill, lead, gap, kw)
    assert rc == 0, ("an access left its range, or a byte or a row was written twice", rc, ctx, msg)
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


def cuts(lib, columns, widths, sep, pad, j):
    call = Call(columns, widths)
    want = call.meaning(sep, pad)[j]
    buf = (ctypes.c_uint8 * (len(want) + 1))()
    sep_buf = ctypes.create_string_buffer(bytes(sep), max(len(sep), 1))
    n = lib.ze_row_cuts(ctypes.addressof(call.cols), len(columns), ctypes.addressof(sep_buf), len(sep), pad, j, ctypes.addressof(buf), len(want) + 1)
    assert n == len(want) and bytes(buf[:n]) == want, ("a row made at a cut differs from the whole (-3), or left its range (-1)", n, len(want), widths, sep, j)


def random_table(k, lengths, seed):
    rng = random.Random(seed)
    return zc.table([rng.choice(lengths) for _ in range(k)], seed + 100)


# ------------------------------------------------------------------------------------------------ the meaning itself
def test_the_python_meaning_on_lines_known_by_hand():
    words, counts, sums = [b"/a", b"/bb", b""], [b"12", b"3", b"12345678"], [b"-4", b"0.5", b"7"]
    assert zc.lines([counts, words, sums], b" ", [7, 0, 0]) == [b"     12 /a -4", b"      3 /bb 0.5", b"12345678  7"]
    assert zc.lines([words, counts], b"::", [-4, 3], pad=0x2E) == [b"/a..::.12", b"/bb.::..3", b"....::12345678"]
    assert zc.layout([b"ab", b"", b"c"], 10, 2, 1) == (b"\n\nab\n\nc\n", [2, 5, 6], [4, 5, 7])
    text, begins, ends = zc.table([3, 0, 5], 1)
    assert [e - b for b, e in zip(begins, ends)] == [3, 0, 5] and ends[-1] <= len(text)
    segs = zc.segments([[b"ab"], [b"c"]], b"-", [4, -2], 32, 1, 2)
    assert segs == [("pad", 1, 3), ("piece", 3, 5), ("sep", 5, 6), ("piece", 6, 7), ("pad", 7, 8), ("row", 1, 8), ("gap", 8, 10)]


def test_the_constants_and_the_bad_word(zx):
    out = (ctypes.c_int64 * 7)()
    zx.ze_constants(out)
    assert [int(x) for x in out] == [16, 64, 4096, zc.STREAM_BYTES, zc.EMIT_CHUNK, 64, 16] and ctypes.sizeof(Column) == 64
    # the largest word is the first (j, c): the smallest j, and at that j the smallest c
    order = [(0, 0), (0, 1), (0, 15), (1, 0), (1, 15), (2, 0), (255, 3), (256, 0), (1 << 20, 7), ((1 << 31) - 1, 14), ((1 << 31) - 1, 15)]
    for a, b in zip(order, order[1:]):
        assert zx.ze_bad_word_before(a[0], a[1], b[0], b[1]) == 1 and zx.ze_bad_word_before(b[0], b[1], a[0], a[1]) == 0


# ------------------------------------------------------------------------------------------------ the call
@pytest.mark.parametrize("n_cols", [1, 2, 3, 16])
def test_column_counts_and_piece_lengths(zx, n_cols):
    lengths = (0, 1, 15, 16, 17, 33, zc.STREAM_BYTES - 1, zc.STREAM_BYTES, zc.STREAM_BYTES + 1)
    k = 150
    columns = [random_table(k, lengths, 10 * n_cols + c) for c in range(n_cols)]
    widths = [(7, 0, -7, 1, -1)[c % 5] for c in range(n_cols)]
    for sep in (b"", b",", bytes(range(0x41, 0x41 + 64))):
        for lead, gap, chunk in ((0, 1, 4096), (5, 0, 64), (3, 3, 256), (0, 40, 16)):
            summ = check(zx, columns, widths, sep, lead=lead, gap=gap, chunk=chunk, unit=64)
            assert summ[5] > 0 and summ[6] > 0      # both tiers were taken
    check(zx, columns, None, b" ")


def test_widths_against_pieces_shorter_equal_and_longer(zx):
    lengths = (0, 1, 6, 7, 8, 100, 4095, 4096, 4097)
    k = len(lengths) * 3
    a = zc.table([lengths[j % len(lengths)] for j in range(k)], 3)
    b = zc.table([lengths[(j // 3) % len(lengths)] for j in range(k)], 4)
    for widths in ((0, 0), (1, -1), (-1, 1), (7, -7), (-7, 7), (4096, -4096), (-4096, 4096)):
        check(zx, [a, b], widths, b"|", pad=0x2E, chunk=4096)
        check(zx, [a, b], widths, b"", pad=0x30, gap=0, chunk=256)
        for j in (0, 3, 4, 7, 8, k - 1):
            cuts(zx, [a, b], widths, b"|", 0x2E, j)


def test_rows_made_again_at_every_cut(zx):
    lengths = (0, 1, 15, 16, 17, 33, 31, 32, 47, 48, 49, 64, 65)
    columns = [random_table(40, lengths, 30 + c) for c in range(3)]
    for widths, sep in (((7, 0, 0), b" "), ((0, -40, 33), b""), ((-1, 1, 0), bytes(range(0x61, 0x61 + 64))), ((0, 0, 0), b"ab")):
        for j in range(40):
            cuts(zx, columns, widths, sep, 32, j)


def test_all_empty_rows_share_one_begin(zx):
    empty = zc.table([0] * 700, 5)
    for n_cols in (1, 3):
        for lead in (0, 5):
            summ = check(zx, [empty] * n_cols, None, b"", lead=lead, gap=0, chunk=64)
            assert summ[0] == lead
    mixed = zc.table([0] * 300 + [5] + [0] * 299 + [40] + [0] * 99, 6)
    check(zx, [mixed, empty], None, b"", gap=0, chunk=64, unit=64)
    check(zx, [empty, mixed], (0, 3), b"", gap=0, chunk=16)


def test_same_text_different_texts_and_index_lists(zx):
    k = 300
    one = random_table(k, (0, 3, 8, 20, 50), 40)
    others = [random_table(k, (1, 2, 9, 70), 41 + c) for c in range(2)]
    rng = random.Random(9)
    perm = list(range(k))
    rng.shuffle(perm)
    repeats = [rng.randrange(k) for _ in range(k)]
    check(zx, [one, one], None, b" ")                                                            # the same column twice
    check(zx, [one + (perm,), one + (list(reversed(range(k))),)], (5, -5), b"\t", chunk=256)     # one text, two orders
    check(zx, [one + (repeats,), others[0], others[1] + (perm,)], (7, 0, 0), b" ", unit=64)      # three texts
    check(zx, [one + ([7] * 50,), others[0] + ([299, 0] * 25,)], None, b"--", gap=0)             # k from the lists, not the tables
    check(zx, [one + ([],), others[0] + ([],)], None, b" ", lead=4)                              # non-NULL lists with count 0: no rows
    for unit_k in (1, 255, 256, 257):
        check(zx, [one + (list(range(unit_k)),), others[0] + (perm[:unit_k],)], (7, 0), b" ")


def test_the_size_query_a_short_output_and_missing_tables(zx):
    columns = [random_table(400, (0, 2, 9, 40), 50 + c) for c in range(3)]
    call = Call(columns, (7, 0, 0))
    text, begins, ends = zc.layout(call.meaning(b" ", 32))
    rc, summ, msg, got, gb, ge, _ = run(zx, call, b" ", cap=0)                      # the size query: the tables are still written
    assert rc == 0 and summ[0] == len(text) and got == bytes([POISON8]) * ROOM_BYTES and gb[:400] == begins and ge[:400] == ends
    for cap in (len(text) - 1, len(text) - 17, 100, 1):
        rc, summ, msg, got, gb, ge, _ = run(zx, call, b" ", cap=cap, chunk=256)     # nothing at or beyond out_cap, total is returned
        assert rc == 0 and summ[0] == len(text) and got[:cap] == text[:cap] and got[cap:] == bytes([POISON8]) * ROOM_BYTES, cap
        assert gb[:400] == begins and ge[:400] == ends
    for kw in ({"with_begin": False}, {"with_end": False}, {"with_begin": False, "with_end": False}):
        check(zx, columns, (7, 0, 0), b" ", **kw)


def test_one_column_is_the_pack(zx):
    """C = 1, width 0, any sep: the pack's bytes and rows -- against pack_exec's driver of record_pack.h's own functions"""
    pk = shared_driver("pack_exec", headers(("record_pack.h",), ("checked_text.h",)))
    text, begins, ends = random_table(500, (0, 1, 15, 16, 17, 33, 90), 60)
    rng = random.Random(61)
    for indices, lead, gap in ((None, 0, 1), ([rng.randrange(500) for _ in range(333)], 5, 0), (list(reversed(range(500))), 3, 7)):
        col = (text, begins, ends) if indices is None else (text, begins, ends, indices)
        want_text, want_b, want_e = zc.layout(zc.pieces(text, begins, ends, indices), 0x2C, lead, gap)
        for sep in (b"", b"::"):
            check(zx, [col], None, sep, fill=0x2C, lead=lead, gap=gap, chunk=256)
        # ... and the pack's own header functions give the same text
        k = len(want_b)
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        pk.pe_pack.restype = ctypes.c_long
        pk.pe_pack.argtypes = [vp, u64, vp, vp, u64, vp, u64, ctypes.c_uint32, u64, u64, u64, u64, u64, vp, u64, u64, u64, vp, vp, vp]
        t = (ctypes.c_uint8 * len(text))(*text)
        out = (ctypes.c_uint8 * (len(want_text) + 16))()
        tb, te, ob, oe, summ = _arr(begins), _arr(ends), _arr([0] * k), _arr([0] * k), (ctypes.c_uint64 * 8)()
        idx = None if indices is None else _arr(indices)
        n_chunks = (len(want_text) + 255) // 256
        rc = pk.pe_pack(ctypes.addressof(t), len(text), ctypes.addressof(tb), ctypes.addressof(te), 500, None if idx is None else ctypes.addressof(idx),
                        0 if indices is None else k, 0x2C, lead, gap, 256, 256, 1024, ctypes.addressof(out), len(want_text), 0, n_chunks,
                        ctypes.addressof(ob), ctypes.addressof(oe), summ)
        assert rc == 0 and bytes(out[:len(want_text)]) == want_text and list(ob) == want_b and list(oe) == want_e


def test_refusals_leave_everything_poisoned(zx):
    k = 300
    a, b, c = (random_table(k, (0, 3, 9), 70 + i) for i in range(3))
    short = random_table(k - 1, (1, 2), 75)

    def refused(want, word, columns=(a, b, c), call_kw=None, **kw):
        call = Call(list(columns), **(call_kw or {}))
        kw.setdefault("cap", 64)
        kw.setdefault("k", k)
        rc, summ, msg, got, gb, ge, _ = run(zx, call, kw.pop("sep", b" "), **kw)
        assert (rc, summ[3]) == (-2, CODES[want]) and word in msg and msg.startswith("rj_scan_records_zip: "), (want, rc, summ, msg)
        assert set(got) <= {POISON8} and set(gb) == {POISON} and set(ge) == {POISON}, want

    refused("columns", "0 columns", n_cols=0)
    refused("columns", "17 columns", columns=[a] * 17, n_cols=17)
    refused("columns", "-1 columns", n_cols=-1)
    refused("row_counts", "column 0 and column 2", columns=(a, b, short))
    refused("row_counts", "column 0 and column 1", columns=(a, b + ([1, 2],), c))
    refused("null", "null", sep_null=True, sep_len=1)
    refused("sep", "sep_len 65", sep=b"x" * 65)
    refused("width", "column 1: width 4097", call_kw={"widths": (0, 4097, 0)})
    refused("width", "column 2: width -4097", call_kw={"widths": (0, 0, -4097)})
    refused("width", "column 0: width -2147483648", call_kw={"widths": (-(1 << 31), 0, 0)})
    refused("reserved", "column 1: reserved is 5", call_kw={"reserved": (0, 5, 0)})
    for flags in (1, 2, 4, 0x80000000):
        refused("flags", "flags %#x" % flags, flags=flags)
    refused("pad", "pad 256", pad=256)
    refused("pad", "pad -1", pad=-1)
    refused("fill", "fill 256", fill=256)
    refused("fill", "fill -1", fill=-1)
    refused("null", "null", call_kw={"text_null": 1})
    refused("null", "null", call_kw={"table_null": 2})
    refused("table_align", "column 1", call_kw={"table_shift": (1, 4)})
    refused("table_align", "d_out_begin", out_table_shift=4)
    refused("out_align", "16-byte aligned", out_shift=8)
    refused("sums", "2^42", gap=1 << 42)
    refused("sums", "2^62", lead=1 << 62)
    refused("sums", "2^42", call_kw={"n_override": ((1 << 42), len(b[0]), len(c[0]))})
    refused("sums", "2^62", gap=1 << 54)
    big = (a[0], a[1], a[2])
    call = Call([big])
    call.cols[0].n_records = 1 << 31                            # (refused before anything is read)
    rc, summ, msg, got, gb, ge, _ = run(zx, call, b"", cap=64, k=4)
    assert (rc, summ[3]) == (-2, CODES["too_many"]) and "2^31" in msg and set(got) <= {POISON8}


def test_a_null_output_with_a_capacity_is_refused(zx):
    a = random_table(10, (1, 2), 80)
    call = Call([a])
    summ, msg = (ctypes.c_uint64 * 8)(), ctypes.create_string_buffer(320)
    assert zx.ze_zip(ctypes.addressof(call.cols), 1, None, 0, 32, 0, 10, 0, 1, 256, 4096, None, 64, None, None, summ, msg) == -2
    assert int(summ[3]) == CODES["null"] and b"null argument" in msg.value


def test_the_first_bad_row_and_column_is_named(zx):
    k = 700
    a, b, c = (random_table(k, (0, 3, 9), 90 + i) for i in range(3))
    good = list(range(k))

    def first_bad(columns, want_row, want_col, **kw):
        call = Call(columns, **kw)
        rc, summ, msg, got, gb, ge, _ = run(zx, call, b" ", cap=64, k=k, unit=64)
        assert rc == 0 and (summ[1], summ[2]) == (want_row, want_col), (summ, want_row, want_col)
        assert "row %d column %d " % (want_row, want_col) in msg, msg
        assert set(got) <= {POISON8} and set(gb) == {POISON} and set(ge) == {POISON}      # no byte, no table row

    bad_at = lambda at, value=k: good[:at] + [value] + good[at + 1:]
    first_bad([a + (bad_at(500),), b, c], 500, 0)
    first_bad([a, b, c + (bad_at(699, NONE),)], 699, 2)
    first_bad([a + (bad_at(400),), b, c + (bad_at(399),)], 399, 2)      # a later column at an earlier row wins over column 0
    first_bad([a + (bad_at(400),), b + (bad_at(400),), c], 400, 0)      # the same row: the smallest column
    first_bad([a, b + (bad_at(0, 1 << 40),), c], 0, 1)
    # a bad ROW: begin > end, and end > n
    text, begins, ends = b
    swapped = (text, begins[:50] + [ends[50] + 1] + begins[51:], ends[:50] + [ends[50]] + ends[51:])
    first_bad([a, swapped, c], 50, 1)
    beyond = (text, begins, ends[:-1] + [len(text) + 1])
    first_bad([a, beyond, c], k - 1, 1)


def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a child
    process: 1, 2, 3 and 16 columns, piece lengths around a group and the tier threshold, widths to +-4096, separators of 0 to 64
    bytes, index lists, every layout, over allocations that are exact in their last byte, and rows made again at every cut.
    (The sanitizers' runtimes are linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("zip_exec", DEPS)], capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"zip_exec: " in r.stdout and b" cases" in r.stdout
