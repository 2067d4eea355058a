"""CPU tests of the record pack (rejit_amd/csrc/record_pack.h): the arithmetic of rj_scan_records_pack -- a list of records of
one text gathered into a new contiguous text, `gap` fill bytes behind each record and `lead` in front.

The header is compiled with g++ into the test-only driver tests/support/pack_exec.cc, which walks the plan unit by unit and the
copy chunk by chunk as record_pack.hip's kernels do (the chunk's rows from one pair of searches, staged when they fit, else
every 16-byte group searches the table).  The expectation is a brute-force pack in Python straight from the meaning:
    ob(0) = lead, ob(j + 1) = ob(j) + len(j) + gap, total = ob(k); out[ob(j) : ob(j) + len(j)] = record r(j); the rest = fill.
Chunks of 16, 48 and 4096 bytes, a stage of 0, 1, 7 and 1024 rows, units of 1, 3 and 256 rows.  The output and the tables are
poisoned first: every byte of [0, min(total, out_cap)) and every row is written, nothing behind it is touched."""
import ctypes
import random

import pytest

from exec_build import _arr, headers, shared_driver

DEPS = headers(("record_pack.h",), ("checked_text.h",))
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
NONE = (1 << 64) - 1
CHUNKS = (16, 48, 4096)
CAPS = (0, 1, 7, 1024)          # 1024: record_pack.hip's kStageRows
UNITS = (1, 3, 256)
POISON = 0xA5
FILL = 0x7C


@pytest.fixture(scope="module")
def px():
    lib = shared_driver("pack_exec", DEPS)
    u64 = ctypes.c_uint64
    lib.pe_pack.restype = ctypes.c_long
    lib.pe_pack.argtypes = [ctypes.c_char_p, u64, _u64p, _u64p, u64, _u64p, u64, ctypes.c_uint32, u64, u64, u64, u64, u64, _u8p, u64, u64, u64,
                            _u64p, _u64p, _u64p]
    lib.pe_synth.restype = ctypes.c_uint8
    lib.pe_synth.argtypes = [u64]
    lib.pe_sums_fit.argtypes = [u64, u64, u64, u64]
    return lib


def run(lib, text, n, records, indices, lead, gap, unit, chunk, cap, out_cap=None, tables=True, window=None, fill=FILL):
    """-> (rc, total, first bad row or None, out bytes (the whole poisoned buffer), out_begin, out_end, summary).
    text None: numbers only, `window` = (first chunk, chunk count); the buffer then stands for the output from that chunk on."""
    k = len(records) if indices is None else len(indices)
    rb, re_ = _arr([b for b, _ in records]), _arr([e for _, e in records])
    idx = None if indices is None else _arr(indices)
    if window is None:
        rows = range(len(records)) if indices is None else [r for r in indices if r < len(records)]
        room = (out_cap if out_cap is not None else lead + sum(max(records[r][1] - records[r][0], 0) for r in rows) + gap * k + 64) + 32
        first, count = 0, 0
    else:
        first, count = window
        room = count * chunk + 32
    if out_cap is None:
        out_cap = room - 32 if window is None else NONE >> 9
    out = (ctypes.c_uint8 * room)(*([POISON] * room))
    ob = (ctypes.c_uint64 * max(k, 1))(*([NONE] * max(k, 1))) if tables else None
    oe = (ctypes.c_uint64 * max(k, 1))(*([NONE] * max(k, 1))) if tables else None
    summ = (ctypes.c_uint64 * 8)()
    rc = lib.pe_pack(text, n, rb, re_, len(records), idx, 0 if indices is None else len(indices), fill, lead, gap, unit, chunk, cap,
                     out, out_cap, first, count, ob, oe, summ)
    bad = None if summ[1] == NONE else int(summ[1])
    return rc, int(summ[0]), bad, bytes(out), (list(ob)[:k] if tables else None), (list(oe)[:k] if tables else None), [int(x) for x in summ]


def brute(text, records, indices, lead, gap, fill=FILL):
    """The meaning, literally -> (out bytes, out_begin, out_end)"""
    rows = range(len(records)) if indices is None else indices
    out = bytearray(bytes([fill]) * lead)
    ob, oe = [], []
    for r in rows:
        b, e = records[r]
        ob.append(len(out))
        out += text[b:e]
        oe.append(len(out))
        out += bytes([fill]) * gap
    return bytes(out), ob, oe


def check(lib, text, records, indices=None, lead=0, gap=1, units=UNITS, chunks=CHUNKS, caps=CAPS, out_caps=(None,)):
    want, w_ob, w_oe = brute(text, records, indices, lead, gap)
    seen = [0] * 8
    for unit in units:
        for chunk in chunks:
            for cap in caps:
                for out_cap in out_caps:
                    rc, total, bad, out, ob, oe, summ = run(lib, text, len(text), records, indices, lead, gap, unit, chunk, cap, out_cap=out_cap)
                    ctx = (unit, chunk, cap, out_cap, lead, gap, records[:6], None if indices is None else indices[:6])
                    assert rc == 0, ("an access left its range", ctx)
                    assert bad is None and total == len(want), ctx        # the total comes back whatever out_cap is
                    limit = len(want) if out_cap is None else min(out_cap, len(want))
                    assert out[:limit] == want[:limit], ctx
                    assert out[limit:] == bytes([POISON]) * (len(out) - limit), ctx      # nothing at or beyond total / out_cap
                    assert ob == w_ob and oe == w_oe, ctx
                    seen = [a + b for a, b in zip(seen, summ)]
    # without the caller's tables (the copy then reads the driver's own begins) the bytes are the same
    rc, total, bad, out, _, _, _ = run(lib, text, len(text), records, indices, lead, gap, units[-1], chunks[0], caps[-1], tables=False)
    assert rc == 0 and total == len(want) and out[:total] == want and out[total:] == bytes([POISON]) * (len(out) - total)
    return seen


def _text(n, seed=1):
    rng = random.Random(seed)
    return bytes(rng.randrange(32, 127) for _ in range(n))


def _touching(sizes, at=0, seams=(0,)):
    """records of the given sizes, `seams[i % len]` bytes of text between them"""
    out = []
    for i, s in enumerate(sizes):
        out.append((at, at + s))
        at += s + seams[i % len(seams)]
    return out, at


def test_sizes_around_a_group_at_every_lead_and_gap(px):
    """Records of 0, 1, 15, 16 and 17 bytes in every order of two, gap 0 / 1 / 5, lead 0 / 1 / 17: every source misalignment
    against every destination misalignment comes up, and every kind of 16-byte group."""
    sizes = [a for x in (0, 1, 15, 16, 17) for y in (0, 1, 15, 16, 17) for a in (x, y)] + [40, 0, 0, 33]
    records, n = _touching(sizes, at=3, seams=(0, 2))
    text = _text(n + 5)
    seen = [0] * 8
    for lead in (0, 1, 17):
        for gap in (0, 1, 5):
            s = check(px, text, records, lead=lead, gap=gap)
            seen = [a + b for a, b in zip(seen, s)]
    assert all(seen[i] for i in (2, 3, 4, 5, 6, 7)), seen       # staged and table chunks; whole-record, fill-only and seam groups


def test_runs_of_empty_records_longer_than_a_chunk(px):
    text = _text(200)
    # 150 empty records (gap 1: 150 fill bytes, more than three chunks of 48; gap 0: 150 rows share one offset), then bytes
    records = [(5, 5)] * 150 + [(10, 60)] + [(60, 60)] * 70 + [(0, 17)]
    for gap in (0, 1, 5):
        check(px, text, records, lead=1, gap=gap, chunks=(16, 48), caps=(0, 7, 1024))
    check(px, text, [(7, 7)] * 300, gap=1, chunks=(16, 48))
    check(px, text, [(7, 7)] * 300, gap=0, lead=17, chunks=(16, 48))      # the lead is all there is
    assert brute(text, [(7, 7)] * 300, None, 0, 0)[0] == b""
    check(px, text, [(7, 7)] * 300, gap=0, lead=0, chunks=(16,))          # an empty output


def test_chunk_boundaries_on_a_first_byte_a_last_byte_and_inside_a_gap(px):
    for chunk in (16, 48, 4096):
        text = _text(3 * chunk + 200, seed=chunk)
        # a record exactly one byte longer than a chunk, from output offset 0: the boundary falls on its last byte
        check(px, text, [(3, 3 + chunk + 1), (1, 9)], lead=0, gap=1, chunks=(chunk,))
        # lead + length == chunk: the boundary falls on the next record's first byte (gap 0) / inside the gap (gap 5)
        check(px, text, [(2, 2 + chunk - 1), (40, 40 + chunk)], lead=1, gap=0, chunks=(chunk,))
        check(px, text, [(2, 2 + chunk - 3), (40, 40 + chunk)], lead=1, gap=5, chunks=(chunk,))
        # the record's last byte is the chunk's last byte; the next record begins exactly at the boundary behind a gap of 1
        check(px, text, [(9, 9 + chunk), (0, chunk - 1), (5, 6)], lead=0, gap=1, chunks=(chunk,))
        # a record longer than two chunks between empty ones
        check(px, text, [(4, 4), (1, 2 * chunk + 50), (6, 6), (0, 3)], lead=17, gap=1, chunks=(chunk,))


def test_indices_permuted_repeated_and_empty(px):
    rng = random.Random(3)
    sizes = [rng.choice([0, 1, 5, 15, 16, 17, 60]) for _ in range(40)]
    records, n = _touching(sizes, seams=(0, 0, 3))
    text = _text(n)
    perm = list(range(40))
    rng.shuffle(perm)
    check(px, text, records, indices=perm, units=(3, 256), chunks=(16, 48))
    check(px, text, records, indices=[7, 7, 7, 39, 0, 7, 12, 12], gap=0, lead=1, chunks=(16, 48))
    check(px, text, records, indices=perm[::-1] + perm + [5] * 30, gap=5, chunks=(48, 4096), units=(3,))
    check(px, text, records, indices=[], lead=17, chunks=(16,))
    check(px, text, records, indices=[], lead=0, chunks=(16,))
    check(px, text, [], lead=1, chunks=(16,))
    # overlapping and descending rows are fine for a pack (rows need not be in order with each other)
    check(px, text, [(10, 50), (0, 30), (20, 21), (0, n)], gap=1, chunks=(16, 48))


def test_out_cap_cuts_inside_a_record_inside_a_gap_and_at_zero(px):
    text = _text(300)
    records = [(0, 40), (40, 41), (41, 41), (50, 150), (150, 300)]
    _, ob, oe = brute(text, records, None, 3, 5)
    caps = (0, 1, oe[0] - 7, oe[0], oe[0] + 2, ob[1], ob[3] + 17, oe[3] + 4, oe[4] + 4, oe[4] + 5, oe[4] + 50)
    check(px, text, records, lead=3, gap=5, out_caps=caps, units=(3,), caps=(0, 1024))
    check(px, text, records, lead=0, gap=0, out_caps=(0, 16, 41, 47, 48, 49), units=(256,), caps=(1, 1024))


def test_random_packs_equal_the_brute_force_pack(px):
    rng = random.Random(11)
    seen = [0] * 8
    for _ in range(40):
        k = rng.choice([1, 2, 9, 70, 300])
        sizes = [rng.choice([0, 0, 1, 2, 15, 16, 17, 31, 100]) for _ in range(k)]
        records, n = _touching(sizes, at=rng.choice([0, 1, 9]), seams=(0, rng.choice([0, 1, 4])))
        text = _text(n + rng.choice([0, 3]), seed=rng.randrange(1 << 30))
        indices = None if rng.random() < 0.5 else [rng.randrange(k) for _ in range(rng.choice([0, 1, k, 2 * k]))]
        s = check(px, text, records, indices=indices, lead=rng.choice([0, 1, 17]), gap=rng.choice([0, 1, 5]),
                  units=(rng.choice(UNITS),), chunks=rng.sample(CHUNKS, 2), caps=rng.sample(CAPS, 2))
        seen = [a + b for a, b in zip(seen, s)]
    assert all(seen[i] for i in (2, 3, 4, 5, 6)), seen


def test_a_whole_record_group_reads_sixteen_bytes_at_once(px):
    """One record of 4096 bytes: every group but none goes byte by byte, whatever the misalignment of source and output."""
    text = _text(5000)
    for begin in range(0, 16):
        for lead in (0, 1, 15, 16):
            rc, total, bad, out, ob, oe, summ = run(px, text, len(text), [(begin, begin + 4096)], None, lead, 1, 256, 4096, 1024)
            assert rc == 0 and out[:total] == brute(text, [(begin, begin + 4096)], None, lead, 1)[0]
            groups = (total + 15) // 16
            assert summ[4] >= groups - 2 and summ[6] <= 2 and summ[7] <= 32, (begin, lead, summ)


def synth_expect(lib, records, indices, lead, gap, lo, hi, fill=FILL):
    """bytes [lo, hi) of the pack of a synthetic text (byte at s = pe_synth(s)), row by row"""
    rows = range(len(records)) if indices is None else indices
    out = bytearray()
    at = lead
    pieces = []
    for r in rows:
        b, e = records[r]
        pieces.append((at, at + (e - b), b))
        at += e - b + gap
    for p in range(lo, min(hi, at)):
        c = fill
        for ob, oe, b in pieces:
            if ob <= p < oe:
                c = lib.pe_synth(b + (p - ob))
        out.append(c)
    return bytes(out), at, [x[0] for x in pieces], [x[1] for x in pieces]


@pytest.mark.parametrize("src_base,lead", [((1 << 32) - 40, (1 << 32) - 100), ((1 << 40) + 5, (1 << 40) + 3), ((1 << 40) + 5, 7), (3, (1 << 41) + 17)])
def test_offsets_beyond_32_and_40_bits(px, src_base, lead):
    """Synthetic numbers, no text: source offsets and output offsets above 2^32 and 2^40, a window of the output produced."""
    sizes = [17, 0, 1, 300, 16, 0, 0, 15, 5000, 33]
    records, end = _touching(sizes, at=src_base, seams=(0, 9))
    n = end + 7
    for indices in (None, [8, 0, 3, 3, 9]):
        for gap in (0, 1):
            for chunk in (16, 48, 4096):
                first = lead // chunk
                count = 3 if chunk == 4096 else 40
                lo = first * chunk
                want, total, w_ob, w_oe = synth_expect(px, records, indices, lead, gap, lo, lo + count * chunk)
                for cap in (0, 7, 1024):
                    rc, got_total, bad, out, ob, oe, _ = run(px, None, n, records, indices, lead, gap, 3, chunk, cap, window=(first, count))
                    assert rc == 0 and bad is None and got_total == total, (chunk, cap, gap)
                    assert ob == w_ob and oe == w_oe
                    assert out[:len(want)] == want, (chunk, cap, gap, indices)
                    assert out[len(want):] == bytes([POISON]) * (len(out) - len(want))
    # the bounds that keep every sum inside the look-back's words: a row below 2^42, the total below 2^62
    assert px.pe_sums_fit(1 << 20, 1 << 34, 0, 1) == 1 and px.pe_sums_fit(1 << 30, 1 << 40, 0, 1) == 0
    assert px.pe_sums_fit(40 << 20, 4 << 30, 0, 1) == 1                       # 40 M lines of a 4 GiB text
    assert px.pe_sums_fit(0, 1 << 40, 1 << 61, 0) == 1 and px.pe_sums_fit(0, 0, 1 << 62, 0) == 0
    assert px.pe_sums_fit(1, 1 << 42, 0, 0) == 0 and px.pe_sums_fit(1, (1 << 42) - 2, 0, 1) == 1 and px.pe_sums_fit(1, (1 << 42) - 1, 0, 1) == 0


@pytest.mark.parametrize("records,indices,n,want", [
    ([(0, 3), (7, 5), (9, 12)], None, 30, 1),                       # end < begin
    ([(0, 3), (4, 5), (9, 31)], None, 30, 2),                       # end > n
    ([(0, 3), (31, 31)], None, 30, 1),                              # begin > n
    ([(0, 3), (4, 5), (9, 12)], [0, 2, 3, 1], 30, 2),               # an index == n_records
    ([(0, 3), (4, 5), (9, 12)], [2, 1, 0, 1 << 40], 30, 3),         # a huge index
    ([(0, 3), (7, 5), (9, 12)], [0, 2, 2, 0, 1, 2], 30, 4),         # a bad row reached through the indices only at j = 4
    ([(0, 3), (7, 5), (9, 12)], [0, 2, 2, 0], 30, None),            # ... and not reached at all: fine
    ([(0, 3)] + [(4, 4)] * 400 + [(6, 5), (9, 40)], None, 30, 401),  # the first bad row of two, deep inside the table
    ([(1 << 63, 5)], None, 30, 0),
])
def test_bad_rows_report_the_first_bad_j_and_nothing_is_copied(px, records, indices, n, want):
    text = _text(n)
    for unit in UNITS:
        for chunk in (16, 4096):
            for cap in (0, 1024):
                rc, total, bad, out, ob, oe, _ = run(px, text, n, records, indices, 1, 1, unit, chunk, cap, out_cap=4096)
                assert rc == 0, "an access left its range"
                assert bad == want, (unit, chunk, cap)
                if want is not None:
                    assert out == bytes([POISON]) * len(out)          # a refused pack copies nothing
