"""CPU tests of rj_scan_records_format_csv's arithmetic (rejit_amd/csrc/record_csv_format.h): the rows of several record tables
written as quoted CSV lines, laid out as a pack.

The header is compiled with g++ into the test-only driver tests/support/csv_format_exec.cc, which walks a call as the kernels
do (the classify by lane and by wave, the plan unit by unit, the emit chunk by chunk through an image of the chunk, the expand
walk and the streamed groups), checks every access against its range and every byte and row against a second write, and makes
rows again at every possible cut.  The expectation is tests/csv_format_cases.py: the rule in plain Python over bytes,
independent of the header -- and Python's csv.writer where the issue claims agreement.  All comparisons are exact."""
import ctypes
import random
import subprocess

import pytest

import csv_cases as cc
import csv_format_cases as fc
from exec_build import _arr, headers, sanitized_program, shared_driver

DEPS = headers(("record_csv_format.h", "record_csv.h", "record_zip.h", "record_rows.h", "record_pack.h", "record_group.h"), ("checked_text.h", "checked_table.h"))
NONE = (1 << 64) - 1
POISON = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 3          # spare table rows
ROOM_BYTES = 37   # spare output bytes
CODES = {name: i for i, name in enumerate(("fine", "null", "columns", "row_counts", "width", "reserved", "flags", "fill", "delimiter", "quote", "line_break",
                                           "same", "mask", "table_align", "out_align", "sums", "too_many"))}
CALL = "rj_scan_records_format_csv: "


class Column(ctypes.Structure):
    _fields_ = [("text", ctypes.c_void_p), ("n", ctypes.c_uint64), ("rec_begin", ctypes.c_void_p), ("rec_end", ctypes.c_void_p), ("n_records", ctypes.c_uint64),
                ("indices", ctypes.c_void_p), ("n_indices", ctypes.c_uint64), ("width", ctypes.c_int32), ("reserved", ctypes.c_int32)]


@pytest.fixture(scope="module")
def fx():
    lib = shared_driver("csv_format_exec", DEPS)
    u64, u32, ci, cu, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p
    lib.cfe_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.cfe_stage_round_trip.argtypes = [u64, u64, u64, ci]
    lib.cfe_format.restype = ctypes.c_long
    lib.cfe_format.argtypes = [vp, ci, ci, ci, u32, u32, cu, ci, u64, u64, u64, u64, vp, u64, vp, vp, ctypes.POINTER(u64), ctypes.c_char_p]
    lib.cfe_row_cuts.restype = ctypes.c_long
    lib.cfe_row_cuts.argtypes = [vp, ci, ci, ci, u32, u32, u64, vp, u64]
    return lib


def aligned_bytes(n, align=16, shift=0):
    raw = (ctypes.c_uint8 * (n + 2 * align))(*([POISON8] * (n + 2 * align)))
    base = ctypes.addressof(raw)
    return raw, (base + align - 1) // align * align + shift


def mask_of(listed):
    return sum(1 << c for c in set(listed))


class Call:
    """columns: a list of (text, begins, ends) or (text, begins, ends, indices) in Python values -> the driver's arguments, kept alive"""

    def __init__(self, columns, widths=None, reserved=None, table_shift=None, text_null=None, table_null=None, n_override=None):
        self.columns = [tuple(c) for c in columns]
        self.keep = []
        self.cols = (Column * max(len(columns), 1))()
        shared = {}
        for c, col in enumerate(self.columns):
            text, begins, ends = col[:3]
            indices = col[3] if len(col) == 4 else None
            key = id(text)
            if key not in shared:
                t = (ctypes.c_uint8 * max(len(text), 1)).from_buffer_copy(bytes(text) or b"\0")
                shared[key] = (t, _arr(begins), _arr(ends))
                self.keep.append(shared[key])
            t, b, e = shared[key]
            idx = None if indices is None else _arr(indices)
            self.keep.append(idx)
            shift = table_shift if table_shift is not None and table_shift[0] == c else None
            self.cols[c] = Column(None if text_null == c else ctypes.addressof(t), len(text) if n_override is None else n_override[c],
                                  None if table_null == c else ctypes.addressof(b) + (shift[1] if shift else 0), None if table_null == c else ctypes.addressof(e),
                                  len(begins), None if idx is None else ctypes.addressof(idx), 0 if indices is None else len(indices),
                                  0 if widths is None else widths[c], 0 if reserved is None else reserved[c])

    def pieces(self):
        return [fc.pieces(c[0], c[1], c[2], c[3] if len(c) == 4 else None) for c in self.columns]


def run(lib, call, d=44, q=34, always=(), raw=(), fill=10, lead=0, gap=1, unit=256, chunk=4096, cap=None, flags=0, with_begin=True, with_end=True,
        out_shift=0, n_cols=None, k=None, out_table_shift=0, always_mask=None, raw_mask=None):
    """-> (rc, summary, message, out bytes with the spare ones, begins, ends with the spare rows)"""
    n_cols = len(call.columns) if n_cols is None else n_cols
    if k is None or cap is None:
        want = fc.lines(call.pieces(), d, q, always, raw) if call.columns else []
        k = len(want) if k is None else k
        cap = len(fc.layout(want, fill, lead, gap)[0]) if cap is None else cap
    keep, out = aligned_bytes(cap + ROOM_BYTES, 16, out_shift)
    begins, ends = _arr([POISON] * (k + ROOM + 1)), _arr([POISON] * (k + ROOM + 1))
    summ = (ctypes.c_uint64 * 13)()
    msg = ctypes.create_string_buffer(320)
    rc = lib.cfe_format(ctypes.addressof(call.cols), n_cols, d, q, mask_of(always) if always_mask is None else always_mask,
                        mask_of(raw) if raw_mask is None else raw_mask, flags, fill, lead, gap, unit, chunk, out if cap or out_shift else None, cap,
                        ctypes.addressof(begins) + out_table_shift if with_begin else None, ctypes.addressof(ends) if with_end else None, summ, msg)
    got = bytes((ctypes.c_uint8 * (cap + ROOM_BYTES)).from_address(out))
    return rc, [int(x) for x in summ], msg.value.decode(), got, list(begins), list(ends), keep


def check(lib, columns, d=44, q=34, always=(), raw=(), fill=10, lead=0, gap=1, want_lines=None, **kw):
    call = Call(columns)
    rows = fc.lines(call.pieces(), d, q, always, raw)
    if want_lines is not None:
        assert rows == want_lines
    text, begins, ends = fc.layout(rows, fill, lead, gap)
    rc, summ, msg, got, gb, ge, _ = run(lib, call, d, q, always, raw, fill, lead, gap, **kw)
    ctx = (len(columns), d, q, always, raw, fill, lead, gap, kw)
    assert rc == 0, ("an access left its range, or a byte or a row was written twice", rc, ctx, msg)
    k = len(begins)
    assert summ[0] == len(text) and summ[1] == NONE, (ctx, summ)
    assert got[:len(text)] == text, (ctx, next(i for i in range(len(text)) if got[i] != text[i]))
    assert got[len(text):] == bytes([POISON8]) * ROOM_BYTES, ctx
    assert (summ[8], summ[9]) == fc.stats(call.pieces(), d, q, always, raw), ctx
    for given, table, want in ((kw.get("with_begin", True), gb, begins), (kw.get("with_end", True), ge, ends)):
        if given:
            assert table[:k] == want and table[k:] == [POISON] * (ROOM + 1), ctx
        else:
            assert table == [POISON] * (k + ROOM + 1), ctx
    return summ


def cuts(lib, columns, d, q, always, raw, j):
    call = Call(columns)
    want = fc.lines(call.pieces(), d, q, always, raw)[j]
    buf = (ctypes.c_uint8 * (len(want) + 1))()
    n = lib.cfe_row_cuts(ctypes.addressof(call.cols), len(columns), d, q, mask_of(always), mask_of(raw), j, ctypes.addressof(buf), len(want) + 1)
    assert n == len(want) and bytes(buf[:n]) == want, ("a row made at a cut differs from the whole (-3), or left its range (-1)", n, len(want), j)


def columns_of(cols, seed=0):
    return [fc.column_of(col, seed + c) for c, col in enumerate(cols)]


# ------------------------------------------------------------------------------------------------ the meaning itself
def test_the_python_meaning_on_lines_known_by_hand():
    assert fc.lines([[b"a", b'say "hi"', b""], [b"b,c", b"x\ny", b""]]) == [b'a,"b,c"', b'"say ""hi""","x\ny"', b","]
    assert fc.lines([[b"", b"a"]]) == [b'""', b"a"]                                         # the lone empty field
    assert fc.lines([[b"a;b", b"it's"], [b"", b"\r"]], d=59, q=39) == [b"'a;b';", b"'it''s';'\r'"]
    assert fc.lines([[b"a"], [b'b""c', b'']], always=(0,), raw=(1,)) == [b'"a","b""c"'] and fc.lines([[b'b""c']], raw=(0,)) == [b'"b""c"']
    assert fc.lines([[b"p"], [b'q"']], always=(1,), raw=(1,)) == [b'p,"q""']               # a column in both masks: raw wins on doubling
    assert fc.stats([[b"a", b'""'], [b",", b""]]) == (2, 2)
    assert fc.python_lines([[b"a", b'say "hi"', b""], [b"b,c", b"x\ny", b""]]) == [b'a,"b,c"', b'"say ""hi""","x\ny"', b","]


def test_the_constants_and_the_staged_piece(fx):
    out = (ctypes.c_int64 * 9)()
    fx.cfe_constants(out)
    assert [int(x) for x in out] == [16, fc.STREAM_BYTES, fc.EMIT_CHUNK, fc.WAVE_STEP, fc.WAVE_BYTES, fc.MAX_EXPAND, 64, 16, fc.CHECKPOINT_BYTES] and ctypes.sizeof(Column) == 64
    top = (1 << 42) - 1
    for src, length, quotes in ((0, 0, 0), (top, top, top), (1, top, 0), (top, 1, 1), (12345, 1 << 22, (1 << 22) - 1), (5, 1 << 41, 1 << 22), (0, top, (1 << 22) + 1)):
        for need in (0, 1):
            assert fx.cfe_stage_round_trip(src, length, quotes, need) == 1, (src, length, quotes, need)


# ------------------------------------------------------------------------------------------------ agreement with csv.writer
@pytest.mark.parametrize("d,q", [(44, 34), (59, 39), (9, 34)])
def test_agreement_with_csv_writer_on_random_rows_without_nul(fx, d, q):
    for n_cols in (1, 2, 3, 4):
        cols = fc.random_rows(400, n_cols, 100 * n_cols + d, d, q)
        every = tuple(range(n_cols))
        assert fc.lines(cols, d, q) == fc.python_lines(cols, d, q)
        assert fc.lines(cols, d, q, always=every) == fc.python_lines(cols, d, q, quote_all=True)
        tables = columns_of(cols, n_cols)
        check(fx, tables, d, q, want_lines=fc.python_lines(cols, d, q), chunk=256, unit=64)
        check(fx, tables, d, q, always=every, want_lines=fc.python_lines(cols, d, q, quote_all=True), gap=2, lead=3, chunk=64)


def test_the_independent_rule_with_nul_and_high_bytes(fx):
    for n_cols, d, q in ((1, 44, 34), (3, 0, 34), (2, 44, 0), (4, 0xE9, 0xFF)):
        cols = fc.random_rows(300, n_cols, 7 * n_cols + q, d, q, nul=True)
        cols[0][:3] = [b"\0", b"\0\0" + bytes([q]), bytes([0xFF, 0xE9, 0])]
        check(fx, columns_of(cols, 5), d, q, chunk=256)
        check(fx, columns_of(cols, 6), d, q, always=(0,), fill=0, gap=2)


def test_always_and_raw_masks(fx):
    cols = fc.random_rows(300, 4, 21)
    tables = columns_of(cols, 9)
    for always, raw in (((), (0,)), ((1, 3), ()), ((0, 1, 2, 3), (0, 1, 2, 3)), ((2,), (2, 3)), ((3,), (0,))):
        check(fx, tables, always=always, raw=raw, chunk=256, unit=64)
    for j in range(0, 300, 11):
        cuts(fx, tables, 44, 34, (1,), (2,), j)


def test_the_lone_empty_field(fx):
    one = fc.column_of([b"", b"a", b"", b"", b'"', b""], 3)
    summ = check(fx, [one], want_lines=[b'""', b"a", b'""', b'""', b'""""', b'""'])
    assert summ[8] == 5
    check(fx, [one, one], want_lines=[b",", b"a,a", b",", b",", b'"""",""""', b","])      # two columns: an empty field stays empty
    check(fx, [one], raw=(0,), gap=0, chunk=16)
    check(fx, [fc.column_of([b""], 1)], lead=2)                                             # k = 1 with an empty piece


def test_one_column_without_a_special_byte_is_the_pack(fx):
    """C = 1 and no piece that needs quotes: the pack's bytes and rows -- against pack_exec's driver of record_pack.h's own functions"""
    pk = shared_driver("pack_exec", headers(("record_pack.h",), ("checked_text.h",)))
    lengths = (1, 15, 16, 17, 33, 90, 1030)
    rng = random.Random(60)
    text, begins, ends = fc.table([rng.choice(lengths) for _ in range(300)], 60, alphabet=bytes(range(0x30, 0x7B)))
    for indices, lead, gap in ((None, 0, 1), ([rng.randrange(300) for _ in range(211)], 5, 0), (list(reversed(range(300))), 3, 7)):
        col = (text, begins, ends) if indices is None else (text, begins, ends, indices)
        want_text, want_b, want_e = fc.layout(fc.pieces(text, begins, ends, indices), 0x2C, lead, gap)
        summ = check(fx, [col], d=9, fill=0x2C, lead=lead, gap=gap, chunk=256)
        assert summ[8] == 0 and summ[0] == len(want_text)
        k = len(want_b)
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        pk.pe_pack.restype = ctypes.c_long
        pk.pe_pack.argtypes = [vp, u64, vp, vp, u64, vp, u64, ctypes.c_uint32, u64, u64, u64, u64, u64, vp, u64, u64, u64, vp, vp, vp]
        t = (ctypes.c_uint8 * len(text))(*text)
        out = (ctypes.c_uint8 * (len(want_text) + 16))()
        tb, te, ob, oe, psum = _arr(begins), _arr(ends), _arr([0] * k), _arr([0] * k), (ctypes.c_uint64 * 8)()
        idx = None if indices is None else _arr(indices)
        n_chunks = (len(want_text) + 255) // 256
        rc = pk.pe_pack(ctypes.addressof(t), len(text), ctypes.addressof(tb), ctypes.addressof(te), 300, None if idx is None else ctypes.addressof(idx),
                        0 if indices is None else k, 0x2C, lead, gap, 256, 256, 1024, ctypes.addressof(out), len(want_text), 0, n_chunks,
                        ctypes.addressof(ob), ctypes.addressof(oe), psum)
        assert rc == 0 and bytes(out[:len(want_text)]) == want_text and list(ob) == want_b and list(oe) == want_e


def test_raw_and_value_agree_on_the_fields_of_well_formed_texts(fx):
    """a field of rj_scan_records_csv without a MALFORMED flag: its interior written as a raw column equals its unescaped value
    written as a value column"""
    texts = [cc.generated(40, seed, n_cols=4, d=b",", final_break=seed % 2 == 0)[0] for seed in (1, 2, 3)]
    texts += [t for t in cc.random_texts(200, 5) if not any(f & cc.MALFORMED for f in cc.tables(t)["field_flags"])]
    for text in texts:
        tb = cc.tables(text)
        if not tb["field_begin"]:
            continue
        assert not any(f & cc.MALFORMED for f in tb["field_flags"])
        fields = list(zip(tb["field_begin"], tb["field_end"], tb["field_flags"]))
        values = [cc.value(text, f) for f in fields]
        raw_col = (text, tb["field_begin"], tb["field_end"])
        for n_cols in (1, 2):     # (one column: the lone empty field on both sides)
            want = fc.lines([values] * n_cols)
            check(fx, [raw_col] * n_cols, raw=tuple(range(n_cols)), want_lines=want, chunk=64)
            check(fx, [fc.column_of(values, 4)] * n_cols, want_lines=want, chunk=64)


# ------------------------------------------------------------------------------------------------ tiers and seams
def test_tier_thresholds_as_value_and_as_raw_columns(fx):
    pieces = fc.tier_pieces()
    table = fc.column_of(pieces, 8)
    short = fc.column_of([b"k%d" % (i % 7) for i in range(len(pieces))], 9)
    for raw in ((), (0,)):
        summ = check(fx, [table, short], raw=raw, chunk=4096)
        assert summ[5] > 0 and summ[6] > 0 and summ[10] > 0 and (summ[7] > 0) == (not raw)
        check(fx, [short, table], raw=tuple(1 - c for c in raw), lead=7, gap=0, chunk=256, unit=64)
    for j in range(0, len(pieces), 5):
        if len(pieces[j]) <= 65:
            cuts(fx, [table, short], 44, 34, (), (), j)
            cuts(fx, [short, table], 44, 34, (0,), (1,), j)


def test_seams_of_chunks_and_groups(fx):
    for boundary, chunk in ((4096, 4096), (4096 + 16, 4096), (256, 256)):
        for name, cols, lead in fc.seam_cases(boundary):
            check(fx, columns_of(cols, 2), lead=lead, chunk=chunk)


def test_long_expanding_pieces(fx):
    quotes = fc.column_of([b'"' * 5000], 1)
    summ = check(fx, [quotes], want_lines=[b'"' * 10002], chunk=4096)
    assert summ[4] == 3 and summ[7] == 3 and summ[11] > 0 and summ[12] == 0      # below CHECKPOINT_BYTES: the later chunks count from the piece's begin
    check(fx, [quotes, quotes], lead=9, chunk=4096)
    body = bytearray(b"m" * 9000)
    for at in (15, 16, 1023, 1024, 8999):
        body[at] = 34
    for lead in (0, 1, 4096 - 17):
        summ = check(fx, [fc.column_of([bytes(body), b"tail"], 2), fc.column_of([b"x", bytes(body)], 3)], lead=lead, chunk=4096)
        assert summ[12] == 2 * 9 and summ[11] == 0                                  # every piece is walked once, no chunk counts again


def test_checkpoints_bound_the_walk_of_a_piece_that_spans_many_chunks(fx):
    """a piece of 64 KiB with a quote byte every 61 bytes, and one of quote bytes only: 17 and 33 chunks begin inside them.  The
    walk between the plan and the emit takes every step once, and no chunk's walk begins in front of its checkpoint: the emit
    takes no step that only counts, and at most two steps more per chunk than the chunk's bytes need"""
    spread = bytearray(b"s" * 65536)
    spread[::61] = b'"' * len(spread[::61])
    for piece, lead in ((bytes(spread), 0), (bytes(spread), 4095), (b'"' * 65536, 3), (b'"' * fc.CHECKPOINT_BYTES, 0), (b'x"' + b"y" * (fc.CHECKPOINT_BYTES - 2), 4090)):
        cols = [fc.column_of([b"head", piece, b"mid"], 1), fc.column_of([piece, b"", piece], 2)]
        summ = check(fx, cols, lead=lead, chunk=4096)
        steps = 3 * (len(piece) // fc.WAVE_STEP)
        assert summ[12] == steps and summ[11] == 0, (lead, summ)
        cap = 3 * 4096 + 5                                                            # a short output: no checkpoint behind out_cap
        text = fc.layout(fc.lines(Call(cols).pieces(), raw=(0,)), 10, lead, 1)[0]
        rc, short, msg, got, _, _, _ = run(fx, Call(cols), raw=(0,), lead=lead, chunk=4096, cap=cap)
        assert rc == 0 and short[0] == len(text) and got[:cap] == text[:cap] and got[cap:] == bytes([POISON8]) * ROOM_BYTES and short[12] <= cap // fc.WAVE_STEP + 1, (lead, short)
    below = b'"' + b"z" * (fc.CHECKPOINT_BYTES - 2)
    summ = check(fx, [fc.column_of([below], 1)], lead=4000, chunk=4096)
    assert summ[12] == 0 and summ[11] > 0                                             # one byte shorter: walked from its begin


def test_rows_made_again_at_every_cut(fx):
    cols = fc.random_rows(60, 3, 33, upto=70)
    tables = columns_of(cols, 12)
    for always, raw in (((), ()), ((0, 2), (1,))):
        for j in range(60):
            cuts(fx, tables, 44, 34, always, raw, j)


# ------------------------------------------------------------------------------------------------ the call
def test_index_lists_shared_texts_and_no_rows(fx):
    k = 300
    cols = fc.random_rows(k, 2, 44, upto=40)
    one, other = columns_of(cols, 13)
    rng = random.Random(9)
    perm = list(range(k))
    rng.shuffle(perm)
    repeats = [rng.randrange(k) for _ in range(k)]
    check(fx, [one] * 16, chunk=4096)                                                      # 16 columns sharing one text
    check(fx, [one + (perm,), one + (repeats,), other], always=(1,), chunk=256, unit=64)
    check(fx, [one + ([],), other + ([],)], lead=4)                                        # non-NULL lists with count 0: no rows
    for unit_k in (1, 255, 256, 257):
        check(fx, [one + (list(range(unit_k)),), other + (perm[:unit_k],)], unit=256)


def test_the_size_query_a_short_output_and_missing_tables(fx):
    cols = fc.random_rows(300, 3, 50, upto=30)
    tables = columns_of(cols, 14)
    call = Call(tables)
    text, begins, ends = fc.layout(fc.lines(cols))
    rc, summ, msg, got, gb, ge, _ = run(fx, call, cap=0)                                   # the size query: the tables are still written
    assert rc == 0 and summ[0] == len(text) and got == bytes([POISON8]) * ROOM_BYTES and gb[:300] == begins and ge[:300] == ends
    for cap in (len(text) - 1, len(text) - 17, 100, 1):
        rc, summ, msg, got, gb, ge, _ = run(fx, call, cap=cap, chunk=256)                  # nothing at or beyond out_cap, total is returned
        assert rc == 0 and summ[0] == len(text) and got[:cap] == text[:cap] and got[cap:] == bytes([POISON8]) * ROOM_BYTES, cap
        assert gb[:300] == begins and ge[:300] == ends
    for kw in ({"with_begin": False}, {"with_end": False}, {"with_begin": False, "with_end": False}):
        check(fx, tables, **kw)


def test_refusals_leave_everything_poisoned(fx):
    k = 100
    a, b, c = columns_of(fc.random_rows(k, 3, 70), 15)
    short = fc.column_of([b"x"] * (k - 1), 1)

    def refused(want, word, columns=(a, b, c), call_kw=None, **kw):
        call = Call(list(columns), **(call_kw or {}))
        kw.setdefault("cap", 64)
        kw.setdefault("k", k)
        rc, summ, msg, got, gb, ge, _ = run(fx, call, **kw)
        assert (rc, summ[3]) == (-2, CODES[want]) and word in msg and msg.startswith(CALL), (want, rc, summ, msg)
        assert set(got) <= {POISON8} and set(gb) == {POISON} and set(ge) == {POISON}, want

    refused("columns", "0 columns", n_cols=0)
    refused("columns", "17 columns", columns=[a] * 17, n_cols=17)
    refused("columns", "-1 columns", n_cols=-1)
    refused("row_counts", "column 0 and column 2", columns=(a, b, short))
    refused("row_counts", "column 0 and column 1", columns=(a, b + ([1, 2],), c))
    refused("width", "column 1: width is 7", call_kw={"widths": (0, 7, 0)})
    refused("width", "column 2: width is -1", call_kw={"widths": (0, 0, -1)})
    refused("reserved", "column 1: reserved is 5", call_kw={"reserved": (0, 5, 0)})
    for flags in (1, 2, 0x80000000):
        refused("flags", "flags %#x" % flags, flags=flags)
    refused("fill", "fill 256", fill=256)
    refused("fill", "fill -1", fill=-1)
    refused("delimiter", "delimiter 256", d=256)
    refused("delimiter", "delimiter -1", d=-1)
    refused("quote", "quote 256", q=256)
    refused("quote", "quote -1", q=-1)                                 # no quoting at all is the zip's
    for d, q in ((10, 34), (13, 34), (44, 10), (44, 13)):
        refused("line_break", "line break", d=d, q=q)
    refused("same", "the same byte 44", d=44, q=44)
    refused("mask", "always_mask 0x8 ", always_mask=8)
    refused("mask", "raw_mask 0x80000001 ", raw_mask=0x80000001)
    refused("mask", "always_mask 0x10000 ", columns=[a] * 16, always_mask=1 << 16)
    refused("null", "null", call_kw={"text_null": 1})
    refused("null", "null", call_kw={"table_null": 2})
    refused("table_align", "column 1", call_kw={"table_shift": (1, 4)})
    refused("table_align", "d_out_begin", out_table_shift=4)
    refused("out_align", "16-byte aligned", out_shift=8)
    refused("sums", "2^42", gap=1 << 42)
    refused("sums", "2^62", lead=1 << 62)
    refused("sums", "2^42", call_kw={"n_override": ((1 << 41), len(b[0]), len(c[0]))})          # 2 n + 2 reaches 2^42
    refused("sums", "2^62", gap=1 << 56 >> 2)
    call = Call([a])
    call.cols[0].n_records = 1 << 31                                   # (refused before anything is read)
    rc, summ, msg, got, gb, ge, _ = run(fx, call, cap=64, k=4)
    assert (rc, summ[3]) == (-2, CODES["too_many"]) and "2^31" in msg and set(got) <= {POISON8}
    summ, msg = (ctypes.c_uint64 * 13)(), ctypes.create_string_buffer(320)
    assert fx.cfe_format(ctypes.addressof(Call([a]).cols), 1, 44, 34, 0, 0, 0, 10, 0, 1, 256, 4096, None, 64, None, None, summ, msg) == -2
    assert int(summ[3]) == CODES["null"] and b"null argument" in msg.value


def test_the_first_bad_row_and_column_is_named(fx):
    k = 700
    a, b, c = columns_of(fc.random_rows(k, 3, 90), 16)
    good = list(range(k))

    def first_bad(columns, want_row, want_col):
        rc, summ, msg, got, gb, ge, _ = run(fx, Call(columns), cap=64, k=k, unit=64)
        assert rc == 0 and (summ[1], summ[2]) == (want_row, want_col), (summ, want_row, want_col)
        assert msg.startswith(CALL) and "row %d column %d " % (want_row, want_col) in msg, msg
        assert set(got) <= {POISON8} and set(gb) == {POISON} and set(ge) == {POISON}      # no byte, no table row

    bad_at = lambda at, value=k: good[:at] + [value] + good[at + 1:]
    first_bad([a + (bad_at(500),), b, c], 500, 0)
    first_bad([a + (bad_at(400),), b, c + (bad_at(399),)], 399, 2)      # a later column at an earlier row wins over column 0
    first_bad([a + (bad_at(400),), b + (bad_at(400),), c], 400, 0)      # the same row: the smallest column
    text, begins, ends = b
    first_bad([a, (text, begins[:50] + [ends[50] + 1] + begins[51:], ends), c], 50, 1)
    first_bad([a, (text, begins, ends[:-1] + [len(text) + 1]), c], k - 1, 1)


def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a child
    process: 1, 2, 3 and 16 columns, piece lengths around a group, the tier threshold and the wave step, every mask layout, index
    lists, over allocations that are exact in their last byte, and rows made again at every cut.  (The sanitizers' runtimes are
    linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("csv_format_exec", DEPS)], capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"csv_format_exec: " in r.stdout and b" cases" in r.stdout
