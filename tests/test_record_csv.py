"""CPU tests of rj_scan_records_csv's arithmetic (rejit_amd/csrc/record_csv.h): the rows and fields of a CSV text with quoted
fields.

The header is compiled with g++ into the test-only driver tests/support/csv_exec.cc, which walks a call as the kernels do (the
summarise span by span, step by step and lane by lane, the resolve, the clear, the emit with its halo), checks every text read
against its range and every table entry against a second write, its cap, the counts and a hole, with the unit, the lanes of a
wave, the waves of the grid and the lanes of the resolve as parameters so that every seam can be forced on tiny texts.  The
expectation is tests/csv_cases.py: the rule byte by byte, independent of the header, and Python's csv.  All comparisons are
exact."""
import ctypes
import random
import subprocess

import pytest

import csv_cases as cc
from exec_build import headers, sanitized_program, shared_driver

DEPS = headers(("record_csv.h", "record_pack.h"), ("checked_text.h",))
POISON = 0xA5A5A5A5A5A5A5A5
POISON32 = 0xA5A5A5A5
ROOM = 3
CODES = {name: i for i, name in enumerate(("fine", "null", "stats", "table_align", "flags_align", "delimiter", "quote", "line_break", "same", "too_long"))}
# (unit, lanes of a wave, waves of the grid, lanes of the resolve): units of 16 and 32 bytes, every group and unit a seam
GEOMETRIES = ((16, 1, 1 << 20, 64), (16, 1, 2, 3), (32, 2, 3, 1), (32, 1, 1 << 20, 2))


@pytest.fixture(scope="module")
def cx():
    lib = shared_driver("csv_exec", DEPS)
    u64, u32, ci, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p
    lib.ce_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.ce_summary.argtypes = [vp, u64, ci, ci, u32, ctypes.POINTER(u64)]
    lib.ce_compose.argtypes = [ctypes.POINTER(u64)] * 3
    lib.ce_csv.restype = ctypes.c_long
    lib.ce_csv.argtypes = [vp, u64, ci, ci, u64, u32, u64, u32, vp, vp, vp, u64, vp, vp, vp, u64, vp, ctypes.POINTER(u64)]
    return lib


def run(lib, text, d=44, q=34, unit=16, lanes=1, wave_cap=1 << 20, resolve_lanes=64, row_cap=None, field_cap=None, query=False, with_stats=True,
        text_null=False, n=None, shift=None):
    """-> (rc, info, stats, tables with their spare entries as lists); the caps default to the counts of csv_cases"""
    want = cc.tables(text, d, q) if n is None else None
    if row_cap is None:
        row_cap = want["stats"]["n_rows"]
    if field_cap is None:
        field_cap = want["stats"]["n_fields"]
    buf = ctypes.create_string_buffer(bytes(text), max(len(text), 1))
    u64s = lambda k: (ctypes.c_uint64 * (k + ROOM + 1))(*([POISON] * (k + ROOM + 1)))
    t = {"row_first": u64s(row_cap + 1), "row_begin": u64s(row_cap), "row_end": u64s(row_cap), "field_begin": u64s(field_cap), "field_end": u64s(field_cap),
         "field_flags": (ctypes.c_uint32 * (field_cap + ROOM + 1))(*([POISON32] * (field_cap + ROOM + 1)))}
    addr = lambda name: None if query else ctypes.addressof(t[name]) + (shift.get(name, 0) if shift else 0)
    stats = (ctypes.c_uint64 * 9)(*([POISON] * 9))
    info = (ctypes.c_uint64 * 4)()
    rc = lib.ce_csv(None if text_null else ctypes.addressof(buf), len(text) if n is None else n, d, -1 if q is None else q, unit, lanes, wave_cap, resolve_lanes,
                    addr("row_first"), addr("row_begin"), addr("row_end"), 0 if query else row_cap, addr("field_begin"), addr("field_end"), addr("field_flags"),
                    0 if query else field_cap, ctypes.addressof(stats) if with_stats else None, info)
    return rc, [int(x) for x in info], [int(x) for x in stats], {k: [int(x) for x in v] for k, v in t.items()}


def check(lib, text, d=44, q=34, **kw):
    want = cc.tables(text, d, q)
    rc, info, stats, got = run(lib, text, d, q, **kw)
    ctx = (bytes(text), d, q, kw)
    assert rc == want["stats"]["n_fields"], ("an access left its range, an entry was written twice or beyond the counts, or one was left out", rc, ctx)
    assert stats == [want["stats"][k] for k in cc.STATS], (ctx, stats, want["stats"])
    rows, fields = want["stats"]["n_rows"], want["stats"]["n_fields"]
    row_cap, field_cap = kw.get("row_cap", rows), kw.get("field_cap", fields)
    for name, count, cap, poison in (("row_first", rows + 1, row_cap + 1, POISON), ("row_begin", rows, row_cap, POISON), ("row_end", rows, row_cap, POISON),
                                     ("field_begin", fields, field_cap, POISON), ("field_end", fields, field_cap, POISON), ("field_flags", fields, field_cap, POISON32)):
        shown = min(count, cap)
        assert got[name][:shown] == want[name][:shown], (ctx, name, got[name], want[name])
        assert got[name][shown:] == [poison] * (len(got[name]) - shown), (ctx, name, "written at or beyond the cap or the counts")
    return want


def test_constants_mirror_the_header(cx):
    c = (ctypes.c_int64 * 8)()
    cx.ce_constants(c)
    assert list(c) == [16, 64, 1024, 4096, 2048, 4, 40, 24]


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_every_small_text_against_the_rule(cx, geometry):
    unit, lanes, wave_cap, resolve_lanes = geometry
    for text in cc.small_texts(upto=6):
        check(cx, text, unit=unit, lanes=lanes, wave_cap=wave_cap, resolve_lanes=resolve_lanes)


def test_every_small_text_over_every_seam(cx):
    """the short texts behind every padding 0..33: each of their bytes meets the seams of the groups and of the units of 16 and 32"""
    texts = [t for t in cc.small_texts(upto=4)]
    for i, text in enumerate(texts):
        pad = i % 34
        for unit, lanes, wave_cap, resolve_lanes in GEOMETRIES[1:3]:
            check(cx, b"x" * pad + text + b"\nzz", unit=unit, lanes=lanes, wave_cap=wave_cap, resolve_lanes=resolve_lanes)
            check(cx, b'"' + b"x" * pad + text, unit=unit, lanes=lanes, wave_cap=wave_cap, resolve_lanes=resolve_lanes)


def test_random_texts_against_the_rule_and_python(cx):
    rng = random.Random(3)
    for i, text in enumerate(cc.random_texts(4000, 1, lo=8, hi=90)):
        unit, lanes, wave_cap, resolve_lanes = GEOMETRIES[i % len(GEOMETRIES)]
        want = check(cx, text, d=9, unit=unit, lanes=lanes, wave_cap=1 + rng.randrange(6) if i % 2 else wave_cap, resolve_lanes=resolve_lanes)
        cc.check_against_python(text, want, d=9)


def test_python_csv_agrees_on_every_small_text():
    """claims (a) and (b) of the header for the rule itself (the driver equals the rule: the tests above)"""
    for text in cc.small_texts(upto=6):
        cc.check_against_python(text, cc.tables(text))


def test_without_a_quote_the_fields_are_split(cx):
    """claim (c): quote == -1 and no \\r outside \\r\\n -> line.split(delimiter)"""
    texts = [(t, 44) for t in cc.small_texts(upto=5)] + [(t, 9) for t in cc.random_texts(1500, 2)]
    for text, d in texts:
        want = check(cx, text, d=d, q=None, unit=32, lanes=2, wave_cap=3, resolve_lanes=2)
        assert want["stats"]["n_quoted"] == 0 and want["stats"]["open_at_end"] == 0
        unified = text.replace(b"\r\n", b"\n")
        if b"\r" in unified:
            continue
        lines = unified.split(b"\n")
        if lines[-1] == b"":
            lines.pop()
        got = [[text[b:e] for b, e, _ in row] for row in cc.rows_of(want)]
        assert got == [line.split(bytes([d])) for line in lines], text


def test_generated_text_full_wave(cx):
    """a well-formed text with every kind of field at the kernels' own geometry, against the rule, numpy's rule and Python"""
    text, vals = cc.generated(60, 7)
    for unit, wave_cap in ((1024, 1 << 20), (4096, 2), (2048, 1)):
        want = check(cx, text, unit=unit, lanes=64, wave_cap=wave_cap)
    assert not any(f & cc.MALFORMED for f in want["field_flags"])
    assert [[v.encode("latin-1") for v in row] for row in cc.values(text, want)] == vals
    cc.check_against_python(text, want)
    fast = cc.tables_numpy(text)
    for name in fast:
        assert [int(x) for x in fast[name]] == want[name], name
    text2, _ = cc.generated(25, 8, final_break=False, d=b"\t")
    fast = cc.tables_numpy(text2, d=9)
    want = check(cx, text2, d=9, unit=1024, lanes=64)
    for name in fast:
        assert [int(x) for x in fast[name]] == want[name], name


def test_composition_is_associative(cx):
    u64 = ctypes.c_uint64
    rng = random.Random(4)
    compose = lambda a, b: (lambda o: (cx.ce_compose((u64 * 5)(*a), (u64 * 5)(*b), o), tuple(o))[1])((u64 * 5)())

    def summary(t, lanes):
        o = (u64 * 5)()
        buf = ctypes.create_string_buffer(t, max(len(t), 1))
        cx.ce_summary(ctypes.addressof(buf), len(t), 44, 34, lanes, o)
        return tuple(o)
    for _ in range(300):
        a, b, c = (tuple([rng.randrange(2)] + [rng.randrange(1 << 40) for _ in range(4)]) for _ in range(3))
        assert compose(compose(a, b), c) == compose(a, compose(b, c))
    for text in cc.random_texts(600, 5, alphabet=b'a",\n', lo=0, hi=80):
        whole = summary(text, 1)
        assert whole == summary(text, 3) == summary(text, 64)
        cut = rng.randrange(len(text) + 1) // 16 * 16      # (a summary is cut at a group's seam)
        assert compose(summary(text[:cut], 2), summary(text[cut:], 1)) == whole
        want = cc.tables(text)["stats"]
        tail = 1 if text and not (text.endswith(b"\n") and whole[0] == 0) else 0
        assert (whole[1] + tail, whole[3] + tail, whole[0]) == (want["n_fields"], want["n_rows"], want["open_at_end"])


def test_resolve_over_any_split(cx):
    text, _ = cc.generated(40, 9)
    for wave_cap in (1, 2, 3, 7, 64, 1000):
        for resolve_lanes in (1, 2, 5, 64):
            check(cx, text, unit=32, lanes=2, wave_cap=wave_cap, resolve_lanes=resolve_lanes)


def test_caps_and_size_query(cx):
    for text in (cc.generated(9, 10)[0], b'a,"b\n",c\r\n\r\nlast', b",", b"\n", b"a"):
        want = cc.tables(text)
        rows, fields = want["stats"]["n_rows"], want["stats"]["n_fields"]
        for row_cap in (rows - 1, rows, rows + 5):
            for field_cap in (fields - 1, fields, fields + 5):
                check(cx, text, row_cap=max(row_cap, 0), field_cap=max(field_cap, 0), unit=16, lanes=1, wave_cap=3)
        rc, _info, stats, got = run(cx, text, query=True)
        assert rc == fields and stats == [want["stats"][k] for k in cc.STATS]
        assert all(v == [POISON32 if k == "field_flags" else POISON] * len(v) for k, v in got.items())


def test_malformed_events_and_first_bad(cx):
    for text, flag, at in ((b'ab"c,d\n', cc.BAD_QUOTE, 2), (b'"ab"c,d\n', cc.BAD_CLOSE, 3), (b"a\rb,c\n", cc.BARE_CR, 1), (b'a,"bc\nd', cc.OPEN, 7),
                           (b'x,"a""b",y\n', cc.ESCAPED, None), (b'"a"\r\nb\r', cc.BARE_CR, 6), (b'"a"\r\n"b"\r', cc.BAD_CLOSE, 7)):
        want = check(cx, text, unit=16, lanes=1)
        assert any(f & flag for f in want["field_flags"]), text
        assert want["stats"]["first_bad"] == (cc.NONE if at is None else at), text


def test_refusals_by_code(cx):
    text = b"a,b\n"
    for kw, name in (({"text_null": True}, "null"), ({"with_stats": False}, "stats"), ({"shift": {"row_first": 4}}, "table_align"),
                     ({"shift": {"field_end": 2}}, "table_align"), ({"shift": {"field_flags": 2}}, "flags_align"), ({"d": -1}, "delimiter"), ({"d": 256}, "delimiter"),
                     ({"q": -2}, "quote"), ({"q": 256}, "quote"), ({"d": 10}, "line_break"), ({"d": 13}, "line_break"), ({"q": 10}, "line_break"),
                     ({"q": 13}, "line_break"), ({"d": 34}, "same"), ({"n": 1 << 42}, "too_long")):
        kw = dict(kw)
        rc, info, stats, got = run(cx, text, row_cap=2, field_cap=3, **({"n": len(text)} | kw))
        assert rc == -2 and info[0] == CODES[name], (kw, name, info)
        assert stats == [POISON] * 9
        assert all(v == [POISON32 if k == "field_flags" else POISON] * len(v) for k, v in got.items()), kw


def test_standalone_program_under_sanitizers():
    exe = sanitized_program("csv_exec", DEPS)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "csv_exec:" in done.stdout
