"""CPU tests of rj_scan_records_translate's arithmetic (rejit_amd/csrc/record_translate.h): the rows of a record table through a
byte map and a drop set, laid out as a pack.

The header is compiled with g++ into the test-only driver tests/support/translate_exec.cc, which walks a call as the kernels do
(the rows' plan, the count unit by unit and slab by slab or the layout, the emit turn by turn through an image), checks every
text read against its range and every byte and row against a second write and against a hole, with the slab size, the image
size and the unit cap as parameters so that every seam can be forced on tiny texts.  The expectation is
tests/translate_cases.py: bytes.translate per row and the layout arithmetic, independent of the header.  All comparisons are
exact."""
import ctypes
import random
import subprocess

import pytest

import translate_cases as tc
from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_translate.h", "record_rows.h", "record_pack.h", "record_group.h"), ("checked_text.h", "checked_table.h"))
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 3          # spare table rows
ROOM_BYTES = 37   # spare output bytes
CODES = {name: i for i, name in enumerate(("fine", "null", "fill", "out_align", "table_align", "sums"))}


@pytest.fixture(scope="module")
def tx():
    lib = shared_driver("translate_exec", DEPS)
    u64, ci, vp = ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p
    lib.te_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.te_translate.restype = ctypes.c_long
    lib.te_translate.argtypes = [vp, u64, vp, vp, u64, vp, u64, vp, vp, ci, u64, u64, u64, u64, u64, u64, ci, vp, u64, vp, vp, ctypes.POINTER(u64)]
    return lib


def aligned_bytes(n, align=16, shift=0, init=None):
    raw = (ctypes.c_uint8 * (n + 2 * align))(*([POISON8] * (n + 2 * align)))
    at = (ctypes.addressof(raw) + align - 1) // align * align + shift
    if init is not None:
        ctypes.memmove(at, bytes(init), len(init))
    return raw, at


def run(lib, text, begins, ends, indices=None, table=None, delete=b"", fill=10, lead=0, gap=1, unit_rows=256, slab=4096, image=4096, unit_cap=1 << 20,
        want_stats=False, cap=None, with_begin=True, with_end=True, text_shift=0, out_shift=0, table_shift=0, text_null=False, n=None):
    """-> (rc, summary, out bytes with the spare ones, begins, ends with the spare rows)"""
    rows = tc.rows_of(text, begins, ends, indices) if n is None else []
    k = len(begins) if indices is None else len(indices)
    if cap is None:
        cap = len(tc.layout(tc.translate(rows, table, delete), fill, lead, gap)[0])
    keep_text, text_at = aligned_bytes(len(text), 16, text_shift, text)
    keep_out, out = aligned_bytes(cap + ROOM_BYTES, 16, out_shift)
    b, e = _arr(begins), _arr(ends)
    idx = None if indices is None else _arr(indices)
    ob, oe = _arr([POISON] * (k + ROOM + 1)), _arr([POISON] * (k + ROOM + 1))
    summ = (ctypes.c_uint64 * 13)()
    drop = tc.drop_bits(delete) if delete else None
    rc = lib.te_translate(None if text_null else text_at, len(text) if n is None else n, ctypes.addressof(b) + table_shift, ctypes.addressof(e), len(begins),
                          None if idx is None else ctypes.addressof(idx), 0 if indices is None else len(indices), table, drop, fill, lead, gap, unit_rows, slab,
                          image, unit_cap, int(want_stats), out if cap or out_shift else None, cap, ctypes.addressof(ob) if with_begin else None,
                          ctypes.addressof(oe) if with_end else None, summ)
    got = bytes((ctypes.c_uint8 * (cap + ROOM_BYTES)).from_address(out))
    return rc, [int(x) for x in summ], got, list(ob), list(oe)


def check(lib, text, begins, ends, indices=None, table=None, delete=b"", fill=10, lead=0, gap=1, **kw):
    rows = tc.rows_of(text, begins, ends, indices)
    want, wb, we = tc.layout(tc.translate(rows, table, delete), fill, lead, gap)
    rc, summ, got, gb, ge = run(lib, text, begins, ends, indices, table, delete, fill, lead, gap, **kw)
    ctx = (len(rows), table is not None, delete, fill, lead, gap, kw)
    assert rc == 0, ("an access left its range, a byte or a row was written twice, or one was left out", rc, ctx, summ)
    k = len(rows)
    assert summ[0] == len(want) and summ[1] == NONE, (ctx, summ, len(want))
    cap = kw.get("cap")
    shown = len(want) if cap is None else min(cap, len(want))
    assert got[:shown] == want[:shown], (ctx, next(i for i in range(shown) if got[i] != want[i]))
    assert got[shown:] == bytes([POISON8]) * (len(got) - shown), ctx
    assert gb == (wb + [POISON] * (ROOM + 1) if kw.get("with_begin", True) else [POISON] * (k + ROOM + 1)), ctx
    assert ge == (we + [POISON] * (ROOM + 1) if kw.get("with_end", True) else [POISON] * (k + ROOM + 1)), ctx
    st = tc.stats(rows, table, delete)
    assert summ[7] == st["bytes_in"] and summ[8] == st["bytes_dropped"], (ctx, summ, st)
    if summ[12]:
        assert summ[9] == st["bytes_changed"], (ctx, summ, st)
    return summ


def test_constants_mirror_the_header(tx):
    c = (ctypes.c_int64 * 4)()
    tx.te_constants(c)
    assert (c[0], c[1], c[2], c[3]) == (tc.SLAB, tc.IMAGE, tc.GROUP, 256 + 32)


def test_meaning_all_byte_values(tx):
    text = bytes(range(256))
    for seed in range(20):
        rng = random.Random(seed)
        perm = list(range(256))
        rng.shuffle(perm)
        delete = bytes(rng.sample(range(256), rng.randrange(0, 200)))
        check(tx, text, [0], [256], table=bytes(perm), delete=delete, slab=64, image=32, want_stats=True)
    for table, delete in ((None, b""), (tc.LOWER, b""), (tc.UPPER, b""), (None, b"\r\x00,"), (tc.LOWER, b"a"), (tc.LOWER, b"A")):
        check(tx, text, [0], [256], table=table, delete=delete, want_stats=True)
        check(tx, text, [0], [256], table=table, delete=delete)


@pytest.mark.parametrize("slab,image", [(16, 16), (32, 16), (16, 48), (64, 32)])
def test_every_row_cut_against_every_seam(tx, slab, image):
    """rows of every length 0..2 slabs + 1 behind every lead 0..slab + image: every begin and every end meets every phase of the
    slab seams, the turn seams and the 16-byte groups"""
    alphabet = b"abXY,."
    for length in list(range(0, 2 * slab + 2)):
        text, begins, ends = tc.table([3, length, 0, 5], 100 + length, junk=2, alphabet=alphabet)
        for lead in (0, 1, length % 16, 15, 16, image - 1, image + 1):
            for delete in (b"", b",", b"abXY,."):
                check(tx, text, begins, ends, table=tc.LOWER, delete=delete, lead=lead, gap=1, slab=slab, image=image)


def test_every_alignment_of_text_and_output(tx):
    rng = random.Random(5)
    lengths = [rng.choice((0, 1, 15, 16, 17, 33, 70)) for _ in range(40)]
    text, begins, ends = tc.table(lengths, 6, alphabet=b"abcXYZ,\r")
    for shift in range(16):
        for lead in range(16):
            check(tx, text, begins, ends, table=tc.UPPER, delete=b"\r," if (shift + lead) % 2 else b"", lead=lead, gap=(shift + lead) % 3, text_shift=shift,
                  slab=64, image=64)


@pytest.mark.parametrize("gap", [0, 1, 2, 100])
def test_gaps_and_the_image(tx, gap):
    """gap 100 is more than the image of 64 bytes: turns of pure fill between two rows"""
    rng = random.Random(gap)
    lengths = [rng.choice((0, 0, 1, 7, 16, 40)) for _ in range(60)]
    text, begins, ends = tc.table(lengths, 9, alphabet=b"ab,")
    for delete in (b"", b",", b"ab,"):
        summ = check(tx, text, begins, ends, delete=delete, gap=gap, lead=3, slab=32, image=64, fill=0x2E)
        if gap == 100:
            assert summ[6] > len(lengths) * gap // 64       # the turns go with the output


def test_drop_everything_and_empty_tables(tx):
    text = b",,,,ab,,,,,,,,,,,,,,,,,,,,,,,,,,,,,,,,,,cd"
    begins, ends = [0, 4, 6, 6, 40], [4, 6, 6, 40, 42]
    for gap in (0, 1, 3):
        check(tx, text, begins, ends, delete=b",", gap=gap, slab=16, image=16)
        check(tx, text, begins, ends, delete=b",abcd", gap=gap, slab=16, image=16)
    for k in (1, 2, 17, 100):     # empty rows alone: the terminators are all there is
        for gap in (0, 1, 5):
            check(tx, b"xyz", [1] * k, [1] * k, delete=b"x", gap=gap, lead=2, slab=16, image=32)
            check(tx, b"", [0] * k, [0] * k, gap=gap, slab=16, image=32)


def test_indices_with_repeats_and_units_of_several_slabs(tx):
    rng = random.Random(11)
    lengths = [rng.randrange(0, 50) for _ in range(30)]
    text, begins, ends = tc.table(lengths, 12, alphabet=b"abc,")
    indices = [rng.randrange(30) for _ in range(200)]
    for unit_cap in (1, 3, 1 << 20):
        for delete in (b"", b","):
            summ = check(tx, text, begins, ends, indices=indices, table=tc.UPPER, delete=delete, slab=32, image=32, unit_cap=unit_cap, unit_rows=16,
                         want_stats=True)
            assert summ[4] <= unit_cap and (unit_cap > 3 or summ[5] > 1)
    check(tx, text, begins, ends, indices=[], slab=32, image=32, lead=7)
    check(tx, text, begins, ends, indices=[29, 29, 0], with_begin=False, delete=b"a", slab=32, image=32)
    check(tx, text, begins, ends, indices=[29, 29, 0], with_end=False, delete=b"a", slab=32, image=32)


def test_no_rows_is_the_lead(tx):
    for lead in (0, 1, 16, 100):
        check(tx, b"abc", [], [], lead=lead, slab=16, image=16)
        check(tx, b"abc", [0], [3], indices=[], lead=lead, delete=b"a", slab=16, image=16)


def test_capacity(tx):
    rng = random.Random(13)
    lengths = [rng.randrange(0, 60) for _ in range(25)]
    text, begins, ends = tc.table(lengths, 14, alphabet=b"ab,")
    for delete in (b"", b","):
        total = len(tc.layout(tc.translate(tc.rows_of(text, begins, ends), None, delete))[0])
        for cap in (0, 1, 16, total - 1, total, total + 53):
            check(tx, text, begins, ends, delete=delete, cap=cap, slab=32, image=48)


def test_bad_rows_are_named_and_nothing_is_written(tx):
    text, begins, ends = tc.table([5] * 40, 15)
    for bad_at in (0, 17, 39):
        for kind in ("index", "order", "end"):
            b, e, idx = list(begins), list(ends), list(range(40))
            if kind == "index":
                idx[bad_at] = 40
            elif kind == "order":
                b[bad_at], e[bad_at] = e[bad_at], b[bad_at]
            else:
                e[bad_at] = len(text) + 1
            idx[39 if bad_at != 39 else 38] = 1 << 40      # a later (or earlier-checked) bad row does not change the name
            first = min(bad_at, 39 if bad_at != 39 else 38)
            rc, summ, got, gb, ge = run(tx, text, b, e, idx, delete=b"a", unit_rows=16, slab=32, image=32, cap=64, n=len(text))
            assert rc == 0 and summ[1] == first, (bad_at, kind, summ)
            assert got == bytes([POISON8]) * len(got) and gb == [POISON] * len(gb) and ge == [POISON] * len(ge)


def test_refusals_by_code(tx):
    text, begins, ends = tc.table([5] * 4, 16)
    code = lambda **kw: (lambda r: (r[0], r[1][2], r[2], r[3], r[4]))(run(tx, text, begins, ends, cap=kw.pop("cap", 64), **kw))
    for kw, name in (({"text_null": True}, "null"), ({"fill": -1}, "fill"), ({"fill": 256}, "fill"), ({"out_shift": 8}, "out_align"),
                     ({"table_shift": 4}, "table_align"), ({"gap": 1 << 42}, "sums"), ({"lead": 1 << 62}, "sums"), ({"n": 1 << 42, "text_null": False}, "sums")):
        rc, why, got, gb, ge = code(**kw)
        assert rc == -2 and why == CODES[name], (kw, name, why)
        assert got == bytes([POISON8]) * len(got) and gb == [POISON] * len(gb) and ge == [POISON] * len(ge)


def test_standalone_program_under_sanitizers():
    exe = sanitized_program("translate_exec", DEPS)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "translate_exec:" in done.stdout
