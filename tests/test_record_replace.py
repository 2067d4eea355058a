"""CPU tests of the record replace (rejit_amd/csrc/record_replace.h): the arithmetic of rj_scan_records_replace -- the pack of
record_pack.h in which every packed record has its own matches (spans[first[r] : first[r] + count[r]] of the scan's list)
replaced by `with`.

The header is compiled with g++ into the test-only driver tests/support/replace_exec.cc, which walks the table and the plan
unit by unit and the copy chunk by chunk as record_replace.hip's kernels do, every access checked against its range.  The
expectation is a brute-force splice per record in Python, straight from the meaning:
    R(r) = text[rb:re] with each of r's matches replaced by `with`, left to right (an empty match inserts `with`);
    ob(0) = lead, ob(j + 1) = ob(j) + len(R(r(j))) + gap, total = ob(k); out[ob(j) : ...] = R(r(j)); the rest = fill.
counts / first come from the join rule of record_join.h written out in Python.  Units of 1, 3 and 256, chunks of 16, 48 and 4096
bytes, a stage of 0, 1, 7 and 1024 rows; the output and the tables are poisoned with 0xA5 first."""
import bisect
import ctypes
import random
import subprocess

import pytest

import test_record_pack as the_pack
from exec_build import _arr, headers, sanitized_program, shared_driver
from test_record_pack import px  # noqa: F401  (the fixture: the pack's driver, pack_exec.cc)

DEPS = headers(("record_replace.h", "record_pack.h"), ("checked_text.h", "checked_table.h"))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)
NONE = (1 << 64) - 1
SAT = (1 << 32) - 1
CHUNKS = (16, 48, 4096)
CAPS = (0, 1, 7, 1024)
UNITS = (1, 3, 256)
WITHS = (0, 1, 15, 16, 17, 40)
POISON = 0xA5
FILL = 0x7C
OK, BAD_INDEX, BAD_ROW, SATURATED, BAD_RANGE, BEGINS_BEFORE, CROSSES = range(7)      # replace::Kind


@pytest.fixture(scope="module")
def rx():
    lib = shared_driver("replace_exec", DEPS)
    u64 = ctypes.c_uint64
    lib.re_replace.restype = ctypes.c_long
    lib.re_replace.argtypes = [ctypes.c_char_p, u64, _u64p, _u64p, u64, _u32p, _u64p, _u64p, u64, _u64p, ctypes.c_int, u64, ctypes.c_char_p, u64,
                               ctypes.c_uint32, u64, u64, u64, u64, u64, u64, _u8p, u64, _u64p, _u64p, _u64p]
    lib.re_sums_fit.argtypes = [u64] * 6
    return lib


def join(records, spans):
    """record_join.h's rule -> (counts, first): first[i] = lb(rec_begin[i]), count[i] = lb(min(rec_end[i] + 1, rec_begin[i + 1])) - first[i]"""
    begins = [b for b, _ in spans]
    counts, first = [], []
    for i, (rb, re_) in enumerate(records):
        key = re_ + 1 if i + 1 == len(records) else min(re_ + 1, records[i + 1][0])
        f = bisect.bisect_left(begins, rb)
        first.append(f)
        counts.append(max(bisect.bisect_left(begins, key) - f, 0))
    return counts, first


def splice(text, rb, re_, own, repl):
    out, pos = bytearray(), rb
    for b, e in own:
        out += text[pos:b] + repl
        pos = e
    return bytes(out + text[pos:re_])


def brute(text, records, spans, counts, first, indices, repl, lead, gap, fill=FILL):
    """The meaning, literally -> (out bytes, out_begin, out_end)"""
    rows = range(len(records)) if indices is None else indices
    out = bytearray(bytes([fill]) * lead)
    ob, oe = [], []
    for r in rows:
        ob.append(len(out))
        out += splice(text, records[r][0], records[r][1], spans[first[r]:first[r] + counts[r]], repl)
        oe.append(len(out))
        out += bytes([fill]) * gap
    return bytes(out), ob, oe


def run(lib, text, n, records, spans, counts, first, indices, repl, lead, gap, unit, chunk, cap, out_cap=None, room=None, tables=True, fill=FILL,
        table_unit=None):
    """-> (rc, total, first bad row or None, its kind, out bytes (the whole poisoned buffer), out_begin, out_end, summary)"""
    k = len(records) if indices is None else len(indices)
    rb, re_ = _arr([b for b, _ in records]), _arr([e for _, e in records])
    flat = _arr([x for s in spans for x in s])
    idx = None if indices is None else _arr(indices)
    if room is None:
        room = (out_cap if out_cap is not None else 0) + 32
    if out_cap is None:
        out_cap = room - 32
    out = (ctypes.c_uint8 * room)(*([POISON] * room))
    ob = (ctypes.c_uint64 * max(k, 1))(*([NONE] * max(k, 1))) if tables else None
    oe = (ctypes.c_uint64 * max(k, 1))(*([NONE] * max(k, 1))) if tables else None
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.re_replace(text, n, rb, re_, len(records), _arr(counts, ctypes.c_uint32), _arr(first), flat, len(spans), idx, int(indices is not None),
                        0 if indices is None else len(indices), repl, len(repl), fill, lead, gap, unit if table_unit is None else table_unit, unit,
                        chunk, cap, out, out_cap, ob, oe, summ)
    bad = None if summ[1] == NONE else int(summ[1])
    return rc, int(summ[0]), bad, int(summ[2]), bytes(out), (list(ob)[:k] if tables else None), (list(oe)[:k] if tables else None), [int(x) for x in summ]


def check(lib, text, records, spans, repl, indices=None, lead=0, gap=1, units=UNITS, chunks=CHUNKS, caps=CAPS, out_caps=(None,), joined=None):
    counts, first = joined if joined is not None else join(records, spans)
    want, w_ob, w_oe = brute(text, records, spans, counts, first, indices, repl, lead, gap)
    seen = [0] * 8
    for unit in units:
        for chunk in chunks:
            for cap in caps:
                for out_cap in out_caps:
                    oc = len(want) + 40 if out_cap is None else out_cap
                    rc, total, bad, _, out, ob, oe, summ = run(lib, text, len(text), records, spans, counts, first, indices, repl, lead, gap, unit, chunk,
                                                               cap, out_cap=oc)
                    ctx = (unit, chunk, cap, out_cap, lead, gap, len(repl), records[:6], None if indices is None else indices[:6])
                    assert rc == 0, ("an access left its range", ctx)
                    assert bad is None and total == len(want), ctx        # the total comes back whatever out_cap is
                    limit = min(oc, len(want))
                    assert out[:limit] == want[:limit], ctx
                    assert out[limit:] == bytes([POISON]) * (len(out) - limit), ctx      # nothing at or beyond total / out_cap
                    assert ob == w_ob and oe == w_oe, ctx
                    seen = [a + b for a, b in zip(seen, summ)]
    # without the caller's tables (the copy then reads the driver's own begins) the bytes are the same
    rc, total, bad, _, out, _, _, _ = run(lib, text, len(text), records, spans, counts, first, indices, repl, lead, gap, units[-1], chunks[0], caps[-1],
                                          out_cap=len(want), tables=False)
    assert rc == 0 and total == len(want) and out[:total] == want and out[total:] == bytes([POISON]) * (len(out) - total)
    return seen


def _text(n, seed=1):
    rng = random.Random(seed)
    return bytes(rng.randrange(32, 127) for _ in range(n))


def _with(w):
    return bytes(65 + (i * 7) % 26 for i in range(w))


# the hand-made table: every kind of match and record the issue names
RECORDS = [(3, 43), (43, 59), (59, 59), (59, 60), (62, 62), (64, 64), (64, 80), (80, 120), (120, 200), (200, 200), (203, 250)]
SPANS = ([(3, 4), (10, 10), (20, 36), (36, 37), (37, 39), (42, 43),      # first byte, empty, 16 long, two adjacent ones, last byte
          (43, 59),                                                        # a record that is one match, 16 long
          (59, 60),                                                        # ... and one byte long, behind an empty record it touches
          (62, 62),                                                        # an empty record's own empty match (a gap follows)
          (64, 64), (70, 71)]                                              # an empty match where two records touch: the second one's
         + [(b, b + 1) for b in range(120, 200, 2)]                        # many, between records without any
         + [(203, 203), (250, 250)])                                       # insertions at a record's begin and end


def test_the_join_of_the_hand_made_table_is_the_rule():
    counts, first = join(RECORDS, SPANS)
    assert counts == [6, 1, 0, 1, 1, 0, 2, 0, 40, 0, 2]
    assert first[4] == 8 and first[5] == 9 and first[6] == 9            # the empty match at 64 is the SECOND touching record's


def test_every_with_length_against_every_kind_of_match(rx):
    text = _text(260)
    seen = [0] * 8
    for w in WITHS:
        for lead, gap in ((0, 0), (0, 1), (17, 1), (17, 0)):
            s = check(rx, text, RECORDS, SPANS, _with(w), lead=lead, gap=gap, units=(1, 3, 256) if w in (0, 17) else (3,))
            seen = [a + b for a, b in zip(seen, s)]
    assert all(seen[i] for i in (3, 4, 5, 6, 7)), seen       # staged and table chunks; whole-piece, fill-only and seam groups
    # deletion of a record that is one match leaves an empty record; an insertion into an empty record makes it `with`
    counts, first = join(RECORDS, SPANS)
    _, ob, oe = brute(text, RECORDS, SPANS, counts, first, None, b"", 0, 1)
    assert oe[1] - ob[1] == 0 and oe[3] - ob[3] == 0
    _, ob, oe = brute(text, RECORDS, SPANS, counts, first, None, b"xyz", 0, 1)
    assert oe[4] - ob[4] == 3 and oe[5] - ob[5] == 0 and oe[10] - ob[10] == 47 + 6


def test_one_record_with_5000_matches_among_empty_records(rx):
    n = 15000
    text = _text(n + 20, seed=5)
    lens = (1, 0, 2)
    spans = [(7 + 3 * i, 7 + 3 * i + lens[i % 3]) for i in range(5000)]
    records = [(2, 2)] * 300 + [(7, 7 + n)] + [(7 + n + 3, 7 + n + 3)] * 300
    for w in (0, 1, 17):
        for gap in (0, 1):
            check(rx, text, records, spans, _with(w), gap=gap, lead=17 * gap, units=(3, 256), chunks=(48, 4096), caps=(0, 7, 1024))


def test_indices_as_a_permutation_and_as_a_take_with_repeats(rx):
    text = _text(260)
    rng = random.Random(3)
    perm = list(range(len(RECORDS)))
    rng.shuffle(perm)
    for w in (0, 1, 40):
        check(rx, text, RECORDS, SPANS, _with(w), indices=perm, units=(3, 256), chunks=(16, 48))
        check(rx, text, RECORDS, SPANS, _with(w), indices=[8, 8, 0, 4, 8, 10, 10, 1, 4], gap=0, lead=1, chunks=(16, 48))
    check(rx, text, RECORDS, SPANS, b"#", indices=[], lead=17, chunks=(16,))
    check(rx, text, RECORDS, SPANS, b"#", indices=[], lead=0, chunks=(16,))
    check(rx, text, [], [], b"#", lead=1, chunks=(16,))
    check(rx, text, [], SPANS, b"#", lead=0, chunks=(16,))


def test_out_cap_inside_a_text_piece_a_replacement_a_gap_and_the_size_query(rx):
    text = _text(260)
    repl = _with(40)
    counts, first = join(RECORDS, SPANS)
    want, ob, oe = brute(text, RECORDS, SPANS, counts, first, None, repl, 3, 5)
    # record 0 is text[3:43) with its first byte a match: the replacement is out[3, 43), then six bytes of text
    caps = (0, 1, ob[0] + 20, ob[0] + 40, ob[0] + 43, oe[0], oe[0] + 2, ob[1], oe[8] - 1, len(want) - 6, len(want) - 1, len(want), len(want) + 50)
    check(rx, text, RECORDS, SPANS, repl, lead=3, gap=5, out_caps=caps, units=(3,), caps=(0, 1024))
    check(rx, text, RECORDS, SPANS, b"", lead=0, gap=0, out_caps=(0, 16, 41, 47, 48, 49), units=(256,), caps=(1, 1024))
    # the size query: no output at all, the tables still written
    rc, total, bad, _, out, g_ob, g_oe, _ = run(rx, text, len(text), RECORDS, SPANS, counts, first, None, repl, 3, 5, 3, 16, 7, out_cap=0, room=64)
    assert rc == 0 and bad is None and total == len(want) and g_ob == ob and g_oe == oe and out == bytes([POISON]) * 64


def test_a_foreign_match_is_copied_as_text(rx):
    """A match that begins in a gap and reaches into the next record belongs to no record: its bytes inside the record are
    text.  So are the bytes of a match the row's count leaves out."""
    text = _text(60)
    records = [(0, 10), (13, 30), (30, 50)]
    spans = [(2, 4), (11, 16), (20, 22), (35, 36), (40, 44)]
    counts, first = join(records, spans)
    assert counts == [1, 1, 2] and first == [0, 2, 3]
    check(rx, text, records, spans, b"<>", chunks=(16, 48))
    want, _, _ = brute(text, records, spans, counts, first, None, b"<>", 0, 1)
    assert text[13:16] in want
    # counts that leave a row's last match out: that match stays text
    check(rx, text, records, spans, b"<>", chunks=(16,), joined=([1, 1, 1], [0, 2, 3]))
    check(rx, text, records, spans, b"", chunks=(16,), joined=([0, 0, 1], [0, 0, 4]))


def test_random_tables_equal_the_brute_force_splice(rx):
    rng = random.Random(11)
    seen = [0] * 8
    for _ in range(60):
        k = rng.choice([1, 2, 9, 70, 300])
        records, spans, at = [], [], rng.choice([0, 1, 9])
        for _ in range(k):
            size = rng.choice([0, 0, 1, 2, 15, 16, 17, 31, 100])
            seam = rng.choice([0, 0, 1, 4])
            records.append((at, at + size))
            pos = at + rng.choice([0, 0, 1, 5])
            dense = rng.random() < 0.5
            while pos <= at + size and rng.random() < (0.95 if dense else 0.6):
                ln = min(rng.choice([0, 1, 1, 2, 16, 100]), at + size - pos)
                if spans and spans[-1] == (pos, pos):
                    break
                if ln == 0 and pos == at + size and seam == 0:
                    break       # (it would be the next record's by the rule; the next record plants its own)
                spans.append((pos, pos + ln))
                pos += ln + (rng.choice([1, 3]) if ln == 0 else rng.choice([0, 0, 1, 7]))
            at += size + seam
        text = _text(at + rng.choice([0, 3]), seed=rng.randrange(1 << 30))
        indices = None if rng.random() < 0.5 else [rng.randrange(k) for _ in range(rng.choice([0, 1, k, 2 * k]))]
        s = check(rx, text, records, spans, _with(rng.choice(WITHS)), indices=indices, lead=rng.choice([0, 1, 17]), gap=rng.choice([0, 1]),
                  units=(rng.choice(UNITS),), chunks=rng.sample(CHUNKS, 2), caps=rng.sample(CAPS, 2))
        seen = [a + b for a, b in zip(seen, s)]
    assert all(seen[i] for i in (3, 4, 5, 6, 7)), seen


def test_a_long_text_piece_reads_sixteen_bytes_at_once(rx):
    """One record of 4096 bytes with one match in its middle: all groups but a few are one load16."""
    text = _text(5000)
    for begin in (0, 5, 15):
        for w in (0, 1, 17):
            records, spans = [(begin, begin + 4096)], [(begin + 2000, begin + 2003)]
            rc, total, bad, _, out, _, _, summ = run(rx, text, len(text), records, spans, [1], [0], None, _with(w), 1, 1, 256, 4096, 1024, out_cap=5000)
            assert rc == 0 and out[:total] == brute(text, records, spans, [1], [0], None, _with(w), 1, 1)[0]
            assert summ[7] <= 6 and summ[5] >= (total + 15) // 16 - 6, (begin, w, summ)


@pytest.mark.parametrize("what,want,kind", [
    ("an index == n_records", 2, BAD_INDEX),
    ("end < begin", 1, BAD_ROW),
    ("end > n", 3, BAD_ROW),
    ("first + count > m", 2, BAD_RANGE),
    ("first > m", 0, BAD_RANGE),
    ("a saturated count", 1, SATURATED),
    ("the first match begins before the record", 2, BEGINS_BEFORE),
    ("the last match ends beyond the record", 1, CROSSES),
    ("two bad rows", 1, CROSSES),
    ("a bad row reached through the indices only at j = 4", 4, BAD_RANGE),
    ("... and not reached at all", None, OK),
])
def test_refusals_name_the_first_bad_row_and_nothing_is_copied(rx, what, want, kind):
    n = 100
    text = _text(n)
    records = [(0, 20), (20, 45), (50, 70), (70, 100)]
    spans = [(5, 6), (30, 32), (40, 45), (55, 56), (80, 90)]
    counts, first = join(records, spans)
    m = len(spans)
    indices = None
    if what == "an index == n_records":
        indices = [0, 1, 4, 2]
    elif what == "end < begin":
        records[1] = (20, 19)
    elif what == "end > n":
        records[3] = (70, 101)
    elif what == "first + count > m":
        counts[2] = m - first[2] + 1
    elif what == "first > m":
        first[0], counts[0] = m + 1, 0
    elif what == "a saturated count":
        counts[1] = SAT
    elif what == "the first match begins before the record":
        first[2] -= 1
    elif what == "the last match ends beyond the record":
        records[1] = (20, 44)
    elif what == "two bad rows":
        records[1] = (20, 44)
        counts[3] = SAT
    elif what.startswith("a bad row reached") or what.startswith("..."):
        counts[3] = 9
        indices = [0, 1, 2, 0, 3] if what.startswith("a bad row") else [0, 1, 2, 0]
    for unit in UNITS:
        for chunk in (16, 4096):
            for cap in (0, 1024):
                rc, total, bad, got_kind, out, ob, oe, _ = run(rx, text, n, records, spans, counts, first, indices, b"<repl>", 1, 1, unit, chunk, cap,
                                                               out_cap=4096)
                assert rc == 0, "an access left its range"
                assert bad == want and got_kind == kind, (what, unit, chunk, cap)
                if want is not None:
                    assert out == bytes([POISON]) * len(out)          # a refused call copies nothing


def test_with_nothing_to_replace_the_replace_is_the_pack(rx, px):  # noqa: F811
    """An empty match list (m = 0, every count 0): re_replace gives the bytes, ob / oe and the total of pe_pack through the
    other driver -- the one fact the copy frame the two kernels share (record_frame.h's copy_chunks) relies on: the two policies
    describe the same output when there is nothing to replace.  Units of 256, chunks of 64 bytes, a stage of 4 and 1024 rows."""
    rng = random.Random(23)
    seen_pack, seen_replace = [0] * 8, [0] * 8
    for k in (0, 1, 255, 256, 257):
        records, at = [], rng.choice([0, 3])
        for _ in range(k):
            size = rng.choice([0, 0, 1, 15, 16, 17, 40, 100])
            records.append((at, at + size))
            at += size + rng.choice([0, 0, 2])
        text = _text(at + 5, seed=k + 1)
        for indices in (None, [rng.randrange(k) for _ in range(k + 3)] if k else []):
            for lead in (0, 3):
                for gap in (0, 1):
                    want, w_ob, w_oe = the_pack.brute(text, records, indices, lead, gap)
                    inside = [(b + e) // 2 for b, e in zip(w_ob, w_oe) if e - b >= 2]
                    middle = inside[len(inside) // 2] if inside else len(want) // 2
                    for out_cap in (0, middle, len(want)):
                        for cap in (4, 1024):
                            ctx = (k, indices is not None, lead, gap, out_cap, cap)
                            p_rc, p_total, p_bad, p_out, p_ob, p_oe, p_summ = the_pack.run(px, text, len(text), records, indices, lead, gap, 256, 64,
                                                                                           cap, out_cap=out_cap)
                            r_rc, r_total, r_bad, _, r_out, r_ob, r_oe, r_summ = run(rx, text, len(text), records, [], [0] * len(records),
                                                                                     [0] * len(records), indices, b"xyz", lead, gap, 256, 64, cap,
                                                                                     out_cap=out_cap)
                            assert p_rc == 0 and r_rc == 0 and p_bad is None and r_bad is None, ctx
                            assert r_total == p_total == len(want), ctx
                            assert r_out == p_out and r_out[:out_cap] == want[:out_cap], ctx      # (both buffers: out_cap + 32 poisoned bytes)
                            limit = min(out_cap, len(want))
                            assert r_out[limit:] == bytes([POISON]) * (len(r_out) - limit), ctx            # nothing at or beyond total / out_cap
                            assert r_ob == p_ob == w_ob and r_oe == p_oe == w_oe, ctx
                            seen_pack = [a + b for a, b in zip(seen_pack, p_summ)]
                            seen_replace = [a + b for a, b in zip(seen_replace, r_summ)]
    # staged chunks and chunks that searched the tables, several chunks per call, in both drivers
    assert seen_pack[2] and seen_pack[3] and seen_replace[3] == seen_pack[2] and seen_replace[4] == seen_pack[3], (seen_pack, seen_replace)


def test_the_bounds_on_the_sums_at_their_edges(rx):
    f = rx.re_sums_fit                                    # (k, n, m, with_len, lead, gap)
    assert f(40 << 20, 4 << 30, 1 << 28, 16, 0, 1) == 1                           # 40 M lines of 4 GiB, 2^28 matches, 16 bytes each
    # n + (m + 1) * with_len + gap < 2^42
    assert f(1, (1 << 42) - 2, 0, 0, 0, 1) == 1 and f(1, (1 << 42) - 1, 0, 0, 0, 1) == 0
    assert f(1, 0, (1 << 32) - 1, 1 << 9, 0, (1 << 41) - 1) == 1 and f(1, 0, (1 << 32) - 1, 1 << 9, 0, 1 << 41) == 0
    assert f(1, 0, (1 << 41) - 2, 2, 0, 1) == 1 and f(1, 0, (1 << 41) - 1, 2, 0, 0) == 0
    assert f(1, 0, (1 << 63), 0, 0, 0) == 0 and f(1, 0, 5, 1 << 42, 0, 0) == 0 and f(1, 0, 1 << 41, 1 << 41, 0, 0) == 0
    # lead + k * that < 2^62
    assert f(1 << 20, (1 << 42) - 1, 0, 0, (1 << 20) - 1, 0) == 1 and f(1 << 20, (1 << 42) - 1, 0, 0, 1 << 20, 0) == 0      # 2^62 - 1 / 2^62
    assert f((1 << 30) - 1, 0, (1 << 16) - 1, 1 << 16, (1 << 32) - 1, 0) == 1 and f((1 << 30) - 1, 0, (1 << 16) - 1, 1 << 16, 1 << 32, 0) == 0
    assert f(1 << 30, 0, (1 << 16) - 1, 1 << 16, 0, 0) == 0                                                              # 2^30 * 2^32
    assert f(0, 0, 0, 0, (1 << 62) - 1, 0) == 1 and f(0, 0, 0, 0, 1 << 62, 0) == 0
    assert f((1 << 60) - 1, 0, 0, 0, 0, 1) == 1 and f(1 << 60, 0, 0, 0, 0, 0) == 0                # the row number shares a word with its kind


def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(), built with -fsanitize=address,undefined and run as a
    child process: a fixed set of cases against a splice written out in C++, exact allocations.  (The sanitizers' runtimes are
    linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    r = subprocess.run([sanitized_program("replace_exec", DEPS)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert b"216 cases" in r.stdout
