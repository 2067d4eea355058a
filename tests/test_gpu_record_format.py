"""GPU tests (-m gpu) of rj_scan_records_format (rejit_amd/csrc/record_format.hip; Scan.format_records): a column of int64 /
uint64 / float64 values written as decimal text on the device, laid out as a pack.

The meaning is tests/format_cases.py's, written in Python independently of the library: str(int), repr(float), the layout
arithmetic and the status rule.  Every comparison is exact.  Outputs are poisoned first, with room behind the text and the
tables that must stay poisoned.  Every distinct value stands twice in its column."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import format_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_BAD_ARGUMENT = -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON8 = 0xA5
ROOM = 7                          # spare table rows
ROOM_BYTES = 53                   # spare output bytes
UNIT_GRID_ROWS = 1024 * 256       # record_frame.h: unit_grid() workgroups of 256 rows, one pass of the check and of the plan
EMIT_GRID_BYTES = 256 * 8 * 4096  # record_format.hip: kCopyGrid workgroups, a chunk of kEmitChunk bytes each: one turn of the emit


@pytest.fixture(scope="module")
def rj():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rejit_amd
    rejit_amd.build()
    rejit_amd.load_library()
    return rejit_amd


@pytest.fixture(scope="module")
def scan(rj):
    return rj.Scan(rj.Program(b"[0-9]+"))


def dev_words(words):
    import torch
    return torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).to("cuda:0")


def dev(x, dtype=np.int64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to("cuda:0")


class Column:
    """about 3000 distinct values of a kind, each twice (entries p and R + p), on the device, with a status column"""

    def __init__(self, kind):
        distinct = fc.gpu_words(kind)
        assert len(set(distinct)) == len(distinct) >= 2500
        self.kind, self.R = kind, len(distinct)
        self.words = distinct + distinct
        self.status = fc.status_column(len(self.words))
        self.d, self.d_status = dev_words(self.words), dev(self.status, np.uint8)


@pytest.fixture(scope="module")
def columns(rj):
    return {kind: Column(kind) for kind in fc.KINDS}


def format_poisoned(rj, scan, d_value, n_values, kind, d_status=None, idx_t=None, fill=10, lead=0, gap=1, cap=0, flags=0, with_begin=True, with_end=True):
    """the raw call into poisoned buffers -> (return value, out bytes with the spare ones, begins, ends with the spare rows)"""
    import torch
    lib = rj.load_library()
    k = n_values if idx_t is None else int(idx_t.numel())
    out = torch.full((cap + ROOM_BYTES,), POISON8, dtype=torch.uint8, device="cuda:0")
    begins = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    ends = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    assert out.data_ptr() % 16 == 0
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    total = lib.rj_scan_records_format(scan._h, vp(d_value) if n_values else None, None if d_status is None else vp(d_status), n_values,
                                       None if idx_t is None else vp(idx_t), 0 if idx_t is None else k, kind, flags, fill, lead, gap,
                                       vp(out) if cap else None, cap, vp(begins) if with_begin else None, vp(ends) if with_end else None,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return int(total), out.cpu().numpy().tobytes(), begins.cpu().numpy(), ends.cpu().numpy()


def check(rj, scan, C, status=False, indices=None, fill=10, lead=0, gap=1, ctx=None):
    """size query, then the call with an exact capacity, against format_cases.layout"""
    st = C.status if status else None
    text, begins, ends = fc.layout(C.words, C.kind, st, None if indices is None else list(indices), fill, lead, gap)
    idx_t = None if indices is None else dev(indices)
    d_status = C.d_status if status else None
    k = len(begins)
    c = (ctx, C.kind, status, indices is not None, fill, lead, gap)
    total, out, gb, ge = format_poisoned(rj, scan, C.d, len(C.words), C.kind, d_status, idx_t, fill, lead, gap, cap=0)
    assert total == len(text), (c, total, rj.load_library().rj_last_error())
    assert out == bytes([POISON8]) * ROOM_BYTES and (gb[:k] == begins).all() and (ge[:k] == ends).all(), c
    total, out, gb, ge = format_poisoned(rj, scan, C.d, len(C.words), C.kind, d_status, idx_t, fill, lead, gap, cap=len(text))
    assert total == len(text), (c, total, rj.load_library().rj_last_error())
    if out[:total] != text:
        at = next(i for i in range(total) if out[i] != text[i])
        raise AssertionError((c, "first differing byte", at, out[max(at - 30, 0):at + 30], text[max(at - 30, 0):at + 30]))
    assert out[total:] == bytes([POISON8]) * ROOM_BYTES, c
    assert (gb[:k] == begins).all() and (ge[:k] == ends).all() and (gb[k:] == POISON).all() and (ge[k:] == POISON).all(), c
    return text, begins, ends


def index_list(C, count, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.permutation(2 * C.R), rng.randint(0, 2 * C.R, count)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the value sets
@pytest.mark.parametrize("kind", fc.KINDS)
def test_the_value_sets_with_and_without_an_index_list_and_a_status_column(rj, scan, columns, kind):
    """the named values, every power of two (doubles), a sample of the powers of ten with their neighbours, random bits and
    random decimals: bytes and both tables, lead / gap / fill combinations"""
    C = columns[kind]
    picked = index_list(C, 1500, 5)
    for lead, gap, fill in ((0, 1, 10), (5, 0, 0x2C), (0, 3, 0), (5, 40, 10)):
        check(rj, scan, C, False, None, fill, lead, gap, "every value")
        check(rj, scan, C, True, picked, fill, lead, gap, "index list, status")
    check(rj, scan, C, True, None, ctx="status")
    check(rj, scan, C, False, picked, ctx="index list")
    lengths = {len(fc.text_of(w, kind)) for w in C.words}
    assert max(lengths) == (24 if kind == fc.FLOAT64 else 20) and min(lengths) == (3 if kind == fc.FLOAT64 else 1)


@pytest.mark.parametrize("kind", fc.KINDS)
def test_round_trip_on_the_device(rj, scan, columns, kind):
    """parse_records(wide=True) of the formatted text returns the input's bits with status OK for every finite value; the
    non-finite rows (inf, -inf, nan) are MALFORMED there"""
    import torch
    C = columns[kind]
    name = fc.KIND_NAMES[kind]
    values = C.d.view(torch.float64) if kind == fc.FLOAT64 else C.d
    text, ob, oe = scan.format_records(values, kind=name)
    want, begins, ends = fc.layout(C.words, kind)
    assert text.cpu().numpy().tobytes() == want and ob.cpu().tolist() == begins and oe.cpu().tolist() == ends
    back, status = scan.parse_records(text, ob, oe, kind=name, wide=True)
    back = back.view(torch.int64).cpu().numpy().view(np.uint64)
    status = status.cpu().numpy()
    words = np.array(C.words, dtype=np.uint64)
    is_finite = np.array([kind != fc.FLOAT64 or fc.finite(w) for w in C.words])
    assert (status[is_finite] == rj.PARSE_OK).all() and (back[is_finite] == words[is_finite]).all()
    assert (status[~is_finite] == rj.PARSE_MALFORMED).all() and int((~is_finite).sum()) >= (2 * (2 + len(fc.NANS)) if kind == fc.FLOAT64 else 0)
    if kind != fc.FLOAT64:      # kind defaults from the dtype for int64; "uint64" takes the int64 tensor of bits
        again = scan.format_records(C.d, kind=None if kind == fc.INT64 else "uint64")[0]
        assert again.cpu().numpy().tobytes() == want
    else:
        assert scan.format_records(values)[0].cpu().numpy().tobytes() == want


# ------------------------------------------------------------------------------------------------ beyond one pass of the grids
def test_one_row_more_than_a_pass_of_the_unit_grid(rj, scan, columns):
    """262 145 rows drawn from the doubles' column: the check and the plan take their units round again.  Then one bad index in
    the second pass: the call is refused naming it, and output and tables stay poisoned."""
    C = columns[fc.FLOAT64]
    k = UNIT_GRID_ROWS + 1
    pk = np.random.RandomState(77).randint(0, 2 * C.R, k).astype(np.int64)
    texts = [fc.text_of(w, fc.FLOAT64) for w in C.words]
    lens = np.array([len(t) for t in texts], dtype=np.int64)[pk]
    begins = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    want = b"".join(texts[i] + b"\n" for i in pk)
    total, out, gb, ge = format_poisoned(rj, scan, C.d, len(C.words), fc.FLOAT64, None, dev(pk), cap=len(want))
    assert total == len(want), (total, rj.load_library().rj_last_error())
    assert out[:total] == want and out[total:] == bytes([POISON8]) * ROOM_BYTES
    assert (gb[:k] == begins).all() and (ge[:k] == begins + lens).all() and (gb[k:] == POISON).all() and (ge[k:] == POISON).all()
    bad = pk.copy()
    at = k - 1                                   # the one row of the second pass
    assert UNIT_GRID_ROWS <= at < k
    bad[at] = 2 * C.R
    total, out, gb, ge = format_poisoned(rj, scan, C.d, len(C.words), fc.FLOAT64, None, dev(bad), cap=len(want))
    msg = rj.load_library().rj_last_error().decode()
    assert total == RJ_BAD_ARGUMENT and "row %d " % at in msg, (total, msg)
    assert out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all()
    check(rj, scan, C, True, pk[:5000], ctx="behind a refusal")


def test_the_output_passes_one_turn_of_the_emit_grid(rj, scan):
    """10 000 maximum-length doubles with gap = 4096: 41 MB of output, five turns of the emit's 2048 workgroups of 4 KiB,
    most chunks without a row's begin, rows that cross a chunk's end"""
    k, gap = 10000, 4096
    assert k * (24 + gap) > 4 * EMIT_GRID_BYTES
    rng = np.random.RandomState(78)
    xs = -(1.0 + rng.randint(1, 1 << 52, k * 4) / float(1 << 52)) * 1e-196
    words = [w for w in (fc.bits_of(float(x)) for x in xs) if len(fc.text_of(w, fc.FLOAT64)) == 24][:k]
    assert len(words) == k
    total, out, gb, ge = format_poisoned(rj, scan, dev_words(words), k, fc.FLOAT64, gap=gap, cap=k * (24 + gap))
    assert total == k * (24 + gap), (total, rj.load_library().rj_last_error())
    got = np.frombuffer(out, dtype=np.uint8)
    assert (got[total:] == POISON8).all()
    rows = got[:total].reshape(k, 24 + gap)
    assert (rows[:, 24:] == 10).all()
    assert rows[:, :24].tobytes() == b"".join(fc.text_of(w, fc.FLOAT64) for w in words)
    assert (gb[:k] == np.arange(k) * (24 + gap)).all() and (ge[:k] == gb[:k] + 24).all()


# ------------------------------------------------------------------------------------------------ the chunk's seam, the row loop, the tail store
INT64_MIN_WORD = 1 << 63          # -9223372036854775808: the 20 bytes of the longest integer row


def test_every_cut_of_a_row_by_a_chunk_seam(rj, scan):
    """300 rows of 20 bytes at a pitch of 20 and of 21: for every i in 0..24 a lead that makes a row begin at 4096 - i, so the seam
    cuts a row at every one of its bytes, falls on its begin and its end, and in the gap behind it"""
    k, words = 300, [INT64_MIN_WORD] * 300
    assert fc.text_of(INT64_MIN_WORD, fc.INT64) == b"-9223372036854775808"
    d = dev_words(words)
    for gap in (0, 1):
        pitch = 20 + gap
        for i in range(25):
            lead = (4096 - i) % pitch
            text, begins, ends = fc.layout(words, fc.INT64, None, None, 0x2C, lead, gap)
            assert 4096 - i in begins and len(text) > 4096 + 24
            total, out, gb, ge = format_poisoned(rj, scan, d, k, fc.INT64, fill=0x2C, lead=lead, gap=gap, cap=len(text))
            assert total == len(text), (i, gap, total, rj.load_library().rj_last_error())
            assert out[:total] == text and out[total:] == bytes([POISON8]) * ROOM_BYTES, (i, gap, out[4096 - 48:4096 + 24])
            assert (gb[:k] == begins).all() and (ge[:k] == ends).all(), (i, gap)


def test_more_than_256_empty_rows_inside_one_chunk(rj, scan):
    """600 rows, rows 150..449 with a status that is not OK, gap 0: one chunk holds 300 empty rows and the rows around them, and
    the lanes take its rows in two trips"""
    k = 600
    words = [(j * 7919 + 1) % (1 << 40) for j in range(k)]
    status = [fc.NOT_OK[j % 4] if 150 <= j < 450 else fc.OK for j in range(k)]
    text, begins, ends = fc.layout(words, fc.INT64, status, None, 10, 0, 0)
    assert len(text) < 4096 and begins[150] == begins[450] == ends[449]
    total, out, gb, ge = format_poisoned(rj, scan, dev_words(words), k, fc.INT64, dev(status, np.uint8), gap=0, cap=len(text))
    assert total == len(text), (total, rj.load_library().rj_last_error())
    assert out[:total] == text and out[total:] == bytes([POISON8]) * ROOM_BYTES
    assert (gb[:k] == begins).all() and (ge[:k] == ends).all()


def test_the_tail_store_under_an_out_cap_sweep(rj, scan):
    """an output of two chunks and 21 bytes: below min(out_cap, total) the reference's bytes, at and beyond it the sentinel, and
    the total returned whatever out_cap is"""
    k, words = 391, [INT64_MIN_WORD] * 391
    text, begins, ends = fc.layout(words, fc.INT64, None, None, 0x2C, 2, 1)
    total = len(text)
    assert total == 2 * 4096 + 21
    d = dev_words(words)
    for cap in (1, 15, 16, 17, 4095, 4096, 4097, total - 17, total - 16, total - 1, total, total + 16):
        got, out, gb, ge = format_poisoned(rj, scan, d, k, fc.INT64, fill=0x2C, lead=2, gap=1, cap=cap)
        below = min(cap, total)
        assert got == total, (cap, got, rj.load_library().rj_last_error())
        assert out[:below] == text[:below] and out[below:] == bytes([POISON8]) * (cap + ROOM_BYTES - below), cap
        assert (gb[:k] == begins).all() and (ge[:k] == ends).all(), cap


# ------------------------------------------------------------------------------------------------ edges and refusals
def test_no_rows(rj, scan, columns):
    import torch
    C = columns[fc.INT64]
    empty = torch.zeros(1, dtype=torch.int64, device="cuda:0")[:0]
    a_list = torch.zeros(1, dtype=torch.int64, device="cuda:0")      # a non-null list, handed over with count 0
    for d_value, n_values, idx_t in ((C.d, 0, None), (C.d, len(C.words), a_list)):
        lib = rj.load_library()
        out = torch.full((64,), POISON8, dtype=torch.uint8, device="cuda:0")
        tb = torch.full((ROOM,), POISON, dtype=torch.int64, device="cuda:0")
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        total = lib.rj_scan_records_format(scan._h, vp(d_value), None, n_values, None if idx_t is None else vp(idx_t), 0, fc.INT64, 0, 0x2C, 5, 1, vp(out), 16,
                                           vp(tb), vp(tb), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert total == 5 and out.cpu().numpy().tobytes() == b"," * 5 + bytes([POISON8]) * 59 and (tb.cpu().numpy() == POISON).all()
    text, ob, oe = scan.format_records(empty)
    assert text.numel() == 0 and ob.numel() == 0 and oe.numel() == 0
    text, ob, oe = scan.format_records(C.d, indices=empty, lead=3)
    assert text.cpu().numpy().tobytes() == b"\n\n\n" and ob.numel() == 0


def test_out_too_small_and_out_given_through_the_python_api(rj, scan, columns):
    import torch
    C = columns[fc.FLOAT64]
    values = C.d.view(torch.float64)
    want, begins, ends = fc.layout(C.words, fc.FLOAT64, C.status, None, 0x2C, 2, 1)
    room = torch.full((len(want) + 64,), POISON8, dtype=torch.uint8, device="cuda:0")
    text, ob, oe = scan.format_records(values, status=C.d_status, fill=0x2C, lead=2, out=room)
    assert text.data_ptr() == room.data_ptr() and text.cpu().numpy().tobytes() == want and ob.cpu().tolist() == begins and oe.cpu().tolist() == ends
    assert (room[len(want):] == POISON8).all()
    small = torch.full((len(want) - 1,), POISON8, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(rj.RejitError) as err:
        scan.format_records(values, status=C.d_status, fill=0x2C, lead=2, out=small)
    assert "%d bytes" % len(want) in str(err.value)
    assert small.cpu().numpy().tobytes() == want[:-1]                     # nothing at or beyond out_cap was written, the rest is complete
    total, out, gb, ge = format_poisoned(rj, scan, C.d, len(C.words), fc.FLOAT64, C.d_status, None, 0x2C, 2, 1, cap=len(want) - 17)
    assert total == len(want) and out[:len(want) - 17] == want[:-17] and out[len(want) - 17:] == bytes([POISON8]) * ROOM_BYTES


def test_refusals_write_nothing(rj, scan, columns):
    import torch
    C = columns[fc.INT64]
    lib = rj.load_library()
    n = len(C.words)

    def refused(word, status=RJ_BAD_ARGUMENT, d_value=C.d, **kw):
        total, out, gb, ge = format_poisoned(rj, scan, d_value, n, kw.pop("kind", fc.INT64), cap=kw.pop("cap", 4096), **kw)
        msg = lib.rj_last_error().decode()
        assert total == status and word in msg, (word, total, msg)
        assert out == bytes([POISON8]) * len(out) and (gb == POISON).all() and (ge == POISON).all(), word

    for flags in (1, 2, 4, 0x80000000):
        refused("flags", flags=flags)
    refused("kind", kind=3)
    refused("kind", kind=-1)
    refused("fill", fill=256)
    refused("fill", fill=-1)
    refused("2^42", gap=1 << 42)
    refused("2^62", lead=1 << 62)
    refused("8-byte aligned", d_value=C.d.view(torch.uint8)[4:].view(torch.int32))
    refused("row 3 ", idx_t=dev([0, 1, 2, n, 5, n + 7]))
    with pytest.raises(rj.RejitError):
        scan.format_records(C.d, flags=1)
    with pytest.raises(ValueError):
        scan.format_records(C.d, kind="float32")
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    out = torch.full((4096 + 16,), POISON8, dtype=torch.uint8, device="cuda:0")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.rj_scan_records_format(scan._h, vp(C.d), None, n, None, 0, 0, 0, 10, 0, 1, ctypes.c_void_p(out.data_ptr() + 8), 4096, None, None, st) == RJ_BAD_ARGUMENT
    assert "16-byte aligned" in lib.rj_last_error().decode()
    assert lib.rj_scan_records_format(scan._h, None, None, n, None, 0, 0, 0, 10, 0, 1, vp(out), 4096, None, None, st) == RJ_BAD_ARGUMENT
    assert "null" in lib.rj_last_error().decode() and (out == POISON8).all()
    check(rj, scan, C, True, None, ctx="behind the refusals")


def test_the_scan_keeps_its_spans_and_stats(rj, scan, columns):
    import torch
    text = torch.from_numpy(np.frombuffer(b"ab 12 cd 345 e 6\n", dtype=np.uint8).copy()).to("cuda:0")
    assert scan.run_tensor(text) == 3
    spans, stats = scan.spans(), scan.stats()
    scan.format_records(columns[fc.FLOAT64].d.view(torch.float64))
    assert scan.spans() == spans == [(3, 5), (9, 12), (15, 16)] and scan.stats() == stats


# ------------------------------------------------------------------------------------------------ the sample
SAMPLE_LINES = [b"/a 200 0.25", b"/b 500 1e3", b"/a 200 -3.5", b"/c 404", b"/b 200 12abc", b"/a 301  5", b"/b 200 \t1.5", b"/c 200 0.30000000000000004",
                b"/a 200 -40", b"/d 200 1e999", b"/d 7 0", b"/e 200 6.02214076e23", b"/f 1 -0.125", b"/g 7 1e-400", b"/h 9 1e16", b"/h 9 9e15", b"/i 3 1e-7"]


@pytest.mark.parametrize("options", [["7|2", "-n"], ["7|2", "-n", "-v"], [" ", "-f", "1", "-u", "-a", "2"], [" ", "-f", "1", "-u", "-A", "3"],
                                     [" ", "-f", "1", "-u", "-t", "3", "-A", "3"]])
def test_linegrep_sample_numbers_as_text_from_the_device(rj, tmp_path, options):
    """-D: the line numbers / the sums are formatted on the device; the output is byte for byte the output without it"""
    path = str(tmp_path / "access.log")
    with open(path, "wb") as fh:
        fh.write(b"\n".join(SAMPLE_LINES) + b"\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    plain = subprocess.run([sys.executable, sample, path] + options, capture_output=True, timeout=300)
    device = subprocess.run([sys.executable, sample, path] + options + ["-D"], capture_output=True, timeout=300)
    assert plain.returncode == device.returncode == 0, (plain.stderr.decode()[-500:], device.stderr.decode()[-500:])
    assert device.stdout == plain.stdout and len(plain.stdout) > 10, (device.stdout, plain.stdout)
    if "-A" in options and "-t" not in options:      # a sum that needs 17 digits, exponent forms and a zero among them (every sum is exact in any order)
        assert b" /c 0.30000000000000004\n" in device.stdout and b" /a -43.25\n" in device.stdout and b" /h 1.9e+16\n" in device.stdout and b" /i 1e-07\n" in device.stdout
        assert b" /g 0.0\n" in device.stdout and b" /e 6.02214076e+23\n" in device.stdout
