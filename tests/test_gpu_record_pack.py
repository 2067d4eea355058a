"""GPU tests (-m gpu) of rj_scan_records_pack (rejit_amd/csrc/record_pack.hip; Scan.pack_records, records.offsets_records) and
of samples/linegrep_gpu.py -p.

Expected bytes come from numpy slicing of the host copy of the text, straight from the meaning: ob(0) = lead, ob(j + 1) =
ob(j) + len(j) + gap, out[ob(j) : ob(j) + len(j)] = record r(j), every other byte of [0, total) = fill.  The end-to-end tests
take their matches from checkers.Oracle.  Outputs and tables are poisoned first: the kernels write every byte of [0, total) and
every row, and nothing behind them."""
import ctypes
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from checkers import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
_u64p = ctypes.POINTER(ctypes.c_uint64)
RJ_BAD_ARGUMENT = -4
CHUNK = 16384            # record_pack.hip's kCopyChunk
POISON = 0xA5


@pytest.fixture(scope="module")
def rj():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rejit_amd
    rejit_amd.build()
    rejit_amd.load_library()
    return rejit_amd


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def scan(rj):
    return rj.Scan(rj.Program(b"the"))


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))).to("cuda:0")


def expect(t, rb, re_, rows, fill, lead, gap):
    """The meaning, row by row -> (out, out_begin, out_end) as numpy"""
    rb, re_ = np.asarray(rb, dtype=np.int64), np.asarray(re_, dtype=np.int64)
    rows = np.arange(len(rb)) if rows is None else np.asarray(rows, dtype=np.int64)
    lens = (re_ - rb)[rows] if len(rows) else np.zeros(0, dtype=np.int64)
    ob = lead + np.concatenate([[0], np.cumsum(lens + gap)[:-1]]).astype(np.int64) if len(rows) else np.zeros(0, dtype=np.int64)
    total = lead + int(lens.sum()) + gap * len(rows)
    out = np.full(total, fill, dtype=np.uint8)
    for o, r, l in zip(ob.tolist(), rows.tolist(), lens.tolist()):
        if l:
            out[o:o + l] = t[rb[r]:rb[r] + l]
    return out, ob, ob + lens


def pack_poisoned(scan, d, rb_t, re_t, want_total, indices=None, room=64, **kw):
    """pack_records into a poisoned buffer; -> (out, out_begin, out_end, the bytes behind total)"""
    import torch
    buf = torch.full((want_total + room,), POISON, dtype=torch.uint8, device=d.device)
    out, ob, oe = scan.pack_records(d, rb_t, re_t, indices=indices, out=buf, **kw)
    return out.cpu().numpy(), ob.cpu().numpy(), oe.cpu().numpy(), buf[out.numel():].cpu().numpy()


def check_pack(scan, t, d, rb, re_, rows=None, fill=0x7C, lead=0, gap=1):
    want, w_ob, w_oe = expect(t, rb, re_, rows, fill, lead, gap)
    out, ob, oe, behind = pack_poisoned(scan, d, dev(rb), dev(re_), len(want), indices=None if rows is None else dev(rows), fill=fill, lead=lead, gap=gap)
    ctx = (len(rb), None if rows is None else len(rows), fill, lead, gap)
    assert len(out) == len(want), ctx
    assert (ob == w_ob).all() and (oe == w_oe).all(), ctx
    assert (out == want).all(), (ctx, np.nonzero(out != want)[0][:8])
    assert (behind == POISON).all(), ctx
    return w_ob


# ------------------------------------------------------------------------------------------------ shapes
def _table(k, rng, rare_big):
    """k records with lengths from {0, 1, 15, 16, 17, chunk - 1, chunk, chunk + 1}, 0..3 bytes of text between them"""
    small, big = [0, 1, 15, 16, 17], [CHUNK - 1, CHUNK, CHUNK + 1]
    if rare_big:
        lens = np.where(rng.rand(k) < 0.06, rng.choice(big, k), rng.choice(small + [40, 100], k))
    else:
        lens = rng.choice(small + big, k)
    seams = rng.randint(0, 4, k)
    rb = 5 + np.concatenate([[0], np.cumsum(lens + seams)[:-1]]).astype(np.int64)
    return rb, rb + lens, int(rb[-1] + lens[-1]) + 9


@pytest.mark.parametrize("k", [255, 256, 257, 3 * 64 * 256 + 1])
def test_shapes_equal_numpy_slicing(rj, scan, k):
    """Tables of 255, 256, 257 rows and of more units than one look-back group; every length around a 16-byte group and around
    a chunk; gap 0 / 1, lead 0 / 17.  Over the four settings every source misalignment meets every destination misalignment."""
    import torch
    from rejit_amd import workloads as W
    rng = np.random.RandomState(k)
    rb, re_, n = _table(k, rng, rare_big=k > 1000)
    t = W.random_ascii_numpy(n, seed=k)
    d = torch.from_numpy(t).to("cuda:0")
    met = set()
    for gap, lead in ((0, 0), (1, 17), (1, 0), (0, 17)):
        ob = check_pack(scan, t, d, rb, re_, lead=lead, gap=gap)
        long_ = (re_ - rb) >= 48
        met |= set(zip((rb[long_] % 16).tolist(), (ob[long_] % 16).tolist()))
    if k > 1000:
        assert len(met) == 256, len(met)
    # a permutation and a take with repeats through the indices; the library's own allocation (one size query) gives the same
    perm = rng.permutation(k)[:min(k, 3000)]
    check_pack(scan, t, d, rb, re_, rows=perm, lead=1, gap=1)
    take = rng.randint(0, k, 300)
    want, w_ob, w_oe = expect(t, rb, re_, take, 0, 0, 0)
    out, ob, oe = scan.pack_records(d, dev(rb), dev(re_), indices=dev(take), fill=0, lead=0, gap=0)
    assert out.numel() == len(want) and (out.cpu().numpy() == want).all() and (ob.cpu().numpy() == w_ob).all() and (oe.cpu().numpy() == w_oe).all()


def test_no_rows_and_empty_outputs(rj, scan):
    import torch
    t = np.frombuffer(b"0123456789", dtype=np.uint8).copy()
    d = torch.from_numpy(t).to("cuda:0")
    empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
    check_pack(scan, t, d, [], [], lead=0, gap=1)
    check_pack(scan, t, d, [], [], lead=17, gap=1)
    check_pack(scan, t, d, [2, 4], [4, 9], rows=[], lead=5, gap=1)          # an empty selection is not "every record"
    check_pack(scan, t, d, [3, 3, 3], [3, 3, 3], lead=0, gap=0)             # rows, but no bytes at all
    out, ob, oe = scan.pack_records(d, empty, empty, fill=1)
    assert out.numel() == 0 and ob.numel() == 0 and oe.numel() == 0


# ------------------------------------------------------------------------------------------------ skew
def test_one_huge_record_among_empty_ones_and_a_million_empty_records(rj, scan):
    import torch
    from rejit_amd import workloads as W
    big = 64 << 20
    d = W.random_ascii_torch(big + 100, 77, torch.device("cuda:0"))
    rb = np.concatenate([np.full(50000, 5), [7], np.full(50000, big + 50)]).astype(np.int64)
    re_ = rb.copy()
    re_[50000] = 7 + big
    buf = torch.full((big + 100001 + 64,), POISON, dtype=torch.uint8, device="cuda:0")
    out, ob, oe = scan.pack_records(d, dev(rb), dev(re_), fill=0x7C, lead=0, gap=1, out=buf)
    assert out.numel() == big + 100001
    assert bool((out[:50000] == 0x7C).all()) and bool((out[50000 + big:] == 0x7C).all()) and bool((buf[out.numel():] == POISON).all())
    assert torch.equal(out[50000:50000 + big], d[7:7 + big])
    assert ob.cpu().tolist()[49999:50002] == [49999, 50000, 50001 + big] and int(oe[50000]) == 50000 + big
    # a million empty records, gap 1: a million fill bytes
    k = 1000000
    z = dev(np.full(k, 3))
    buf = torch.full((k + 64,), POISON, dtype=torch.uint8, device="cuda:0")
    out, ob, oe = scan.pack_records(d, z, z, fill=10, lead=0, gap=1, out=buf)
    assert out.numel() == k and bool((out == 10).all()) and bool((buf[k:] == POISON).all())
    assert torch.equal(ob, torch.arange(k, device="cuda:0")) and torch.equal(oe, ob)
    # ... and gap 0: nothing at all, whatever the number of rows that share offset 17
    out, ob, oe = scan.pack_records(d, z, z, fill=10, lead=17, gap=0)
    assert out.numel() == 17 and bool((out == 10).all()) and bool((ob == 17).all())


# ------------------------------------------------------------------------------------------------ capacity
def test_size_query_and_out_cap(rj, scan):
    import torch
    from rejit_amd import workloads as W
    lib = rj.load_library()
    rng = np.random.RandomState(5)
    rb, re_, n = _table(300, rng, rare_big=False)
    t = W.random_ascii_numpy(n, seed=5)
    d = torch.from_numpy(t).to("cuda:0")
    want, w_ob, w_oe = expect(t, rb, re_, None, 0x7C, 3, 2)
    rb_t, re_t = dev(rb), dev(re_)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(out, cap, ob=None, oe=None):
        return lib.rj_scan_records_pack(scan._h, vp(d), n, vp(rb_t), vp(re_t), 300, None, 0, 0x7C, 3, 2, vp(out) if out is not None else None, cap,
                                        vp(ob) if ob is not None else None, vp(oe) if oe is not None else None, st)
    # the size query: no output, the tables still written
    ob = torch.full((300,), -7, dtype=torch.int64, device="cuda:0")
    oe = torch.full((300,), -7, dtype=torch.int64, device="cuda:0")
    assert call(None, 0, ob, oe) == len(want)
    assert (ob.cpu().numpy() == w_ob).all() and (oe.cpu().numpy() == w_oe).all()
    assert call(None, 0) == len(want)
    long_row = int(np.argmax(re_ - rb))
    for cap in (int(w_ob[long_row]) + 4097,            # inside a record
                int(w_oe[long_row]) + 1,               # inside a gap
                16, 1, len(want) - 1, len(want), len(want) + 40):
        buf = torch.full((len(want) + 64,), POISON, dtype=torch.uint8, device="cuda:0")
        assert call(buf, cap) == len(want), cap        # (without the caller's tables: the scan's own begins)
        got = buf.cpu().numpy()
        lim = min(cap, len(want))
        assert (got[:lim] == want[:lim]).all() and (got[lim:] == POISON).all(), cap


# ------------------------------------------------------------------------------------------------ end to end
def _oracle_spans(oracle, rx, data):
    cap = len(data) + 2
    buf = np.empty(2 * cap, dtype=np.uint64)
    m = oracle.lib.ro_match_all_re(rx, data, len(data), buf.ctypes.data_as(_u64p), cap)
    assert 0 <= m <= cap, (rx, m)
    return buf[:2 * m].astype(np.int64).reshape(m, 2)


def test_selected_lines_round_trip(rj, oracle):
    """run_records on a line table, select_records in both senses, pack_records(indices=...) with fill 10: the output is the
    oracle-selected lines, a line break behind each; the scan's spans and its selection are untouched by the pack."""
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    t = W.log_like_numpy(1 << 20, 41)
    t[-1] = ord("z")
    t[1000:1003] = 10                        # empty lines
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = R.line_records(d)
    rb, re_ = rb_t.cpu().numpy(), re_t.cpu().numpy()
    lines = data.split(b"\n")
    assert len(lines) == len(rb)
    for rx in (b"the", b"[0-9]+", b"^$"):
        scan = rj.Scan(rj.Program(rx))
        spans = _oracle_spans(oracle, rx, data)
        has = np.zeros(len(rb), dtype=bool)
        has[np.searchsorted(rb, spans[:, 0], side="right") - 1] = True      # (none of the patterns matches across a line break)
        scan.run_records(d, rb_t, re_t)
        before = scan.spans_tensor(d.device).clone()
        assert (before.cpu().numpy() == spans).all()
        for invert in (False, True):
            idx = scan.select_records(invert=invert)
            want_rows = np.nonzero(~has if invert else has)[0]
            assert (idx.cpu().numpy() == want_rows).all() and len(want_rows) > 0, (rx, invert)
            want = b"".join(lines[i] + b"\n" for i in want_rows.tolist())
            out, ob, oe, behind = pack_poisoned(scan, d, rb_t, re_t, len(want), indices=idx, fill=10, lead=0, gap=1)
            assert out.tobytes() == want, (rx, invert)
            assert (behind == POISON).all() and (oe - ob == (re_ - rb)[want_rows]).all()
            # run -> select -> pack -> select again
            assert torch.equal(scan.spans_tensor(d.device), before)
            again = scan.select_records(invert=invert)
            assert torch.equal(again, idx) and scan.n_selected == len(want_rows)


def test_packing_makes_touching_strings_independent(rj, oracle):
    """An Arrow-layout column (offsets, strings that touch) and `ab+`: strings ending in `a` in front of strings beginning with
    `b` give matches across the seams.  Packed with the program's separator they are independent: per string the oracle's
    count and the oracle's spans."""
    import torch
    from rejit_amd import records as R
    rng = random.Random(8)
    texts = []
    for i in range(700):
        body = bytes(rng.choice(b"abbc ") for _ in range(rng.choice([0, 1, 3, 20, 90])))
        texts.append((b"b" if i % 3 == 1 else b"") + body + (b"a" if i % 3 == 0 else b""))
    rx = b"ab+"
    p = rj.Program(rx)
    assert p.batch_separator() >= 0
    scan = rj.Scan(p)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.int64)
    d = torch.from_numpy(np.frombuffer(b"".join(texts), dtype=np.uint8).copy()).to("cuda:0")
    rb_t, re_t = R.offsets_records(dev(offsets))
    assert rb_t.numel() == 700 and int(re_t[-1]) == d.numel() and rb_t.data_ptr() + 8 == re_t.data_ptr()      # views
    want = [oracle.match_all(rx, x) for x in texts]
    res = scan.run_records(d, rb_t, re_t)
    counts = res.counts.cpu().numpy().view(np.uint32).tolist()
    assert res.n_crossing > 0 and counts != [len(w) for w in want]
    out, ob, oe = scan.pack_records(d, rb_t, re_t)                  # fill = the separator, lead 0, gap 1
    assert out.numel() == d.numel() + 700 and bool((out[oe] == p.batch_separator()).all())
    res = scan.run_records(out, ob, oe)
    assert res.n_crossing == 0
    assert res.counts.cpu().numpy().view(np.uint32).tolist() == [len(w) for w in want]
    assert R.all_relative_spans(scan.spans_tensor(d.device), res, ob) == want
    # int32 offsets (Arrow's default) give the same table
    b32, e32 = R.offsets_records(dev(offsets).to(torch.int32))
    assert torch.equal(b32, rb_t) and torch.equal(e32, re_t) and b32.dtype == torch.int64


def test_records_beyond_4gib(rj, scan):
    """A text of 2^32 + 4096 bytes that is never filled; records written into its last 4 KiB and packed through indices."""
    import torch
    n = (1 << 32) + 4096
    d = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    tail = np.random.RandomState(2).randint(32, 127, 4096).astype(np.uint8)
    d[-4096:] = torch.from_numpy(tail).to("cuda:0")
    base = 1 << 32
    rel = [(0, 17), (17, 17), (20, 1000), (1001, 1016), (1016, 4096), (4090, 4096), (4096, 4096)]
    rb = np.array([0, 100] + [base + b for b, _ in rel], dtype=np.int64)       # rows 0 and 1 lie in the part nobody filled
    re_ = np.array([50, 100] + [base + e for _, e in rel], dtype=np.int64)
    rows = [8, 2, 3, 4, 5, 6, 7, 4, 8]
    want = bytearray(b"\x7c" * 17)
    w_ob, w_oe = [], []
    for r in rows:
        b, e = rel[r - 2]
        w_ob.append(len(want))
        want += tail[b:e].tobytes()
        w_oe.append(len(want))
        want += b"\x7c"
    out, ob, oe, behind = pack_poisoned(scan, d, dev(rb), dev(re_), len(want), indices=dev(rows), fill=0x7C, lead=17, gap=1)
    assert out.tobytes() == bytes(want) and ob.tolist() == w_ob and oe.tolist() == w_oe and (behind == POISON).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_row_and_the_scan_stays_usable(rj):
    import torch
    from rejit_amd import workloads as W
    lib = rj.load_library()
    t = W.log_like_numpy(1 << 16, 3)
    n = len(t)
    d = torch.from_numpy(t).to("cuda:0")
    scan = rj.Scan(rj.Program(b"the"))
    good_b = np.arange(0, n, 64, dtype=np.int64)
    good_e = np.minimum(good_b + 60, n)
    k = len(good_b)
    res0 = scan.run_records(d, dev(good_b), dev(good_e))
    sel0 = scan.select_records().clone()
    buf = torch.full((n + 2 * k + 64,), POISON, dtype=torch.uint8, device="cuda:0")
    for what, row, edit, idx in (("end < begin", 700, lambda b, e: e.__setitem__(700, int(b[700]) - 1), None),
                                 ("end > n", k - 1, lambda b, e: e.__setitem__(k - 1, n + 1), None),
                                 ("begin > n", 3, lambda b, e: (b.__setitem__(3, n + 5), e.__setitem__(3, n + 5)), None),
                                 ("two bad rows", 40, lambda b, e: (e.__setitem__(40, n + 1), e.__setitem__(900, 0)), None),
                                 ("an index == n_records", 2, lambda b, e: None, [5, 0, k, 1]),
                                 ("a negative index", 1, lambda b, e: None, [5, -1, k, 1]),
                                 ("a bad row reached through the indices", 3, lambda b, e: e.__setitem__(9, n + 1), [1, 2, 3, 9, 9])):
        b, e = good_b.copy(), good_e.copy()
        edit(b, e)
        with pytest.raises(rj.RejitError) as err:
            scan.pack_records(d, dev(b), dev(e), indices=None if idx is None else dev(idx), fill=10, out=buf)
        assert err.value.status == RJ_BAD_ARGUMENT, what
        assert ("row %d " % row) in err.value.message, (what, err.value.message)
        assert bool((buf == POISON).all()), what             # a refused pack copies nothing
    # arguments: a misaligned output, fill out of range, null tables, a pattern without a separator
    with pytest.raises(rj.RejitError) as err:
        scan.pack_records(d, dev(good_b), dev(good_e), fill=10, out=buf[8:])
    assert err.value.status == RJ_BAD_ARGUMENT and "aligned" in err.value.message
    for fill in (256, -1):
        with pytest.raises(rj.RejitError) as err:
            scan.pack_records(d, dev(good_b), dev(good_e), fill=fill)
        assert err.value.status == RJ_BAD_ARGUMENT and "fill" in err.value.message
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.rj_scan_records_pack(scan._h, ctypes.c_void_p(d.data_ptr()), n, None, None, 3, None, 0, 10, 0, 1, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    assert lib.rj_scan_records_pack(scan._h, ctypes.c_void_p(d.data_ptr()), n, None, None, 0, None, 0, 10, 0, 1, None, 64, None, None, st) == RJ_BAD_ARGUMENT
    assert lib.rj_scan_records_pack(None, ctypes.c_void_p(d.data_ptr()), n, None, None, 0, None, 0, 10, 0, 1, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    assert lib.rj_scan_records_pack(scan._h, ctypes.c_void_p(d.data_ptr()), n, None, None, 0, None, 0, 10, 9, 1, None, 0, None, None, st) == 9
    no_sep = [rx for rx in (b"[^a]+|a+", b".*|[\n\r]+") if rj.Program(rx).batch_separator() < 0]
    assert no_sep, "a pattern that consumes every byte has no separator"
    with pytest.raises(rj.RejitError) as err:
        rj.Scan(rj.Program(no_sep[0])).pack_records(d, dev(good_b), dev(good_e))
    assert err.value.status == RJ_BAD_ARGUMENT and "separator" in err.value.message
    # the scan is usable afterwards, and its last join is still the one the selection reads
    assert torch.equal(scan.select_records(), sel0)
    want, w_ob, w_oe = expect(t, good_b, good_e, None, 10, 0, 1)
    out, ob, oe = scan.pack_records(d, dev(good_b), dev(good_e), fill=10, out=buf)
    assert (out.cpu().numpy() == want).all() and (ob.cpu().numpy() == w_ob).all()
    assert scan.run_records(d, dev(good_b), dev(good_e)).n_kept == res0.n_kept


# ------------------------------------------------------------------------------------------------ samples/linegrep_gpu.py -p
def test_linegrep_sample_prints_the_lines_gnu_grep_prints(rj, tmp_path):
    grep = shutil.which("grep")
    assert grep, "GNU grep is needed for this comparison"
    rng = random.Random(45)
    words = [b"int", b"regexp", b"return", b"for (;;)", b"x = y + 1;", b"// a comment", b"regexps", b"char* s", b"", b"}", b"error 42"]
    lines = [b" ".join(rng.choice(words) for _ in range(rng.randint(0, 6))) for _ in range(5000)]
    path = str(tmp_path / "file.txt")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    for terminated, cases in ((False, (("regexps|return", ["-p"]), ("[0-9]+", ["-v", "-p"]))),
                              (True, (("regexp", ["-v", "-p"]), ("no such thing", ["-p"])))):
        with open(path, "wb") as fh:
            fh.write(b"\n".join(lines) + (b"\n" if terminated else b""))
        for pattern, opts in cases:
            g = subprocess.run([grep, "-E"] + [o for o in opts if o != "-p"] + [pattern, path], capture_output=True, timeout=120)
            assert g.returncode in (0, 1)
            r = subprocess.run([sys.executable, sample, path, pattern] + opts, capture_output=True, timeout=300)
            assert r.returncode == g.returncode, (pattern, opts, r.stderr.decode()[-500:])
            assert r.stdout == g.stdout, (pattern, opts, terminated)
