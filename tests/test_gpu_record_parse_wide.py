"""GPU tests (-m gpu) of RJ_PARSE_WIDE: rj_scan_records_parse's FLOAT64 rows beyond Clinger's window
(rejit_amd/csrc/record_parse.hip: record_parse_kernel<kFloat64, wide>; Scan.parse_records(wide=True)).

The meaning is tests/parse_wide_cases.py's, written in Python independently of the library: decimal.Decimal for the significant
digits, float() for the bits of the whole row or of the two ends of its bracket.  Every comparison is exact, bit patterns
included.  Outputs are poisoned first, with ROOM extra rows that must stay poisoned.  Every distinct row is laid into the text
twice, at different misalignments; the first row begins at offset 0 and the last one ends at the text's last byte."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import parse_cases as pc
import parse_wide_cases as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RJ_BAD_ARGUMENT = -4
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
POISON_U = 0xA5A5A5A5A5A5A5A5
POISON8 = 0xA5
ROOM = 7
STATS = ("n_ok", "n_empty", "n_malformed", "n_range", "n_inexact")      # rj_parse_stats: five uint64
F = pc.FLOAT64
WIDE_GRID_ROWS = 256 * 7 * 256     # record_parse.hip: kParseWideGrid workgroups of 256 rows, one pass of the wide kernel
CHECK_GRID_ROWS = 1024 * 256       # record_frame.h: unit_grid(), one pass of the kernel that checks the rows
SCALE_K = 2048 * 256 + 1           # one row more than a pass of kParseGrid: beyond a pass of either parse grid, two of the check's


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


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))).to("cuda:0")


class Pool:
    """R distinct rows in one text, each laid TWICE: entries p and R + p have equal bytes at different misalignments.  The
    first entry begins at offset 0, the last one laid ends at the text's last byte, and the length is no multiple of 16."""

    def __init__(self, rows, seed=1):
        import torch
        rng = random.Random(seed)
        R = len(rows)
        text, rb, re_ = bytearray(), [0] * (2 * R), [0] * (2 * R)
        for p, s in enumerate(rows):
            text += b"|" * (p % 4 if p else 0)
            rb[p], re_[p] = len(text), len(text) + len(s)
            text += s
        order = list(range(R))
        rng.shuffle(order)
        for p in order:
            last = p == order[-1]
            seam = next(z for z in range(1, 8) if (len(text) + z) % 16 != rb[p] % 16 and not (last and (len(text) + z + len(rows[p])) % 16 == 0))
            text += b"#" * seam
            rb[R + p], re_[R + p] = len(text), len(text) + len(rows[p])
            text += rows[p]
        self.rows, self.R, self.text = list(rows) + list(rows), R, bytes(text)
        self.rb, self.re = np.array(rb, dtype=np.int64), np.array(re_, dtype=np.int64)
        assert rb[0] == 0 and max(re_) == len(text) and len(text) % 16 != 0
        assert all(rb[p] % 16 != rb[R + p] % 16 for p in range(R)) and all(self.text[b:e] == s for b, e, s in zip(rb, re_, self.rows))
        self.d = torch.from_numpy(np.frombuffer(self.text, dtype=np.uint8).copy()).to("cuda:0")
        self.rb_t, self.re_t = dev(self.rb), dev(self.re)
        self._meanings = {}

    def meaning(self, kind, flags):
        """-> (status as uint8, bits as uint64) of every entry, from the Python meanings alone"""
        if (kind, flags) not in self._meanings:
            M = pw.meaning_of if flags & pw.WIDE else pc.meaning
            want = [M(s, kind, bool(flags & pw.TRIM)) for s in self.rows[:self.R]] * 2
            self._meanings[kind, flags] = (np.array([w[0] for w in want], dtype=np.uint8), np.array([w[1] for w in want], dtype=np.uint64))
        return self._meanings[kind, flags]


@pytest.fixture(scope="module")
def pool(rj):
    return Pool(pw.mixed_rows())


def parse_poisoned(rj, scan, P, idx_t, kind, flags, rb_t=None, re_t=None, want_status=True, want_stats=True):
    """rj_scan_records_parse into poisoned tables -> (return value, values as uint64, status: the whole buffers, stats or None)"""
    import torch
    lib = rj.load_library()
    rb_t, re_t = (P.rb_t, P.re_t) if rb_t is None else (rb_t, re_t)
    n_records = int(rb_t.numel())
    k = n_records if idx_t is None else int(idx_t.numel())
    values = torch.full((k + ROOM,), POISON, dtype=torch.int64, device="cuda:0")
    status = torch.full((k + ROOM,), POISON8, dtype=torch.uint8, device="cuda:0")
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    out = (ctypes.c_uint64 * 5)(*([0xA5A5] * 5))
    total = lib.rj_scan_records_parse(scan._h, vp(P.d), int(P.d.numel()), vp(rb_t), vp(re_t), n_records, None if idx_t is None else vp(idx_t),
                                      0 if idx_t is None else k, kind, flags, vp(values), vp(status) if want_status else None,
                                      ctypes.cast(out, lib.rj_scan_records_parse.argtypes[12]) if want_stats else None,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    stats = dict(zip(STATS, (int(x) for x in out))) if want_stats else None
    return int(total), values.cpu().numpy().view(np.uint64), status.cpu().numpy(), stats


def check(rj, scan, P, entries, kind, flags, idx_t=None, rb_t=None, re_t=None, ctx=None, want_status=True):
    """the raw call into poisoned tables against the meaning of the pool's `entries` (the rows of the call, in order)"""
    m_status, m_bits = P.meaning(kind, flags)
    w_status, w_bits = m_status[entries], m_bits[entries]
    w_stats = dict(zip(STATS, (int(c) for c in np.bincount(w_status, minlength=5))))
    k = len(entries)
    c = (ctx, kind, flags, k)
    total, values, status, stats = parse_poisoned(rj, scan, P, idx_t, kind, flags, rb_t, re_t, want_status)
    assert total == w_stats["n_ok"], (c, total, rj.load_library().rj_last_error())
    differ = np.nonzero(values[:k] != w_bits)[0]
    assert differ.size == 0, (c, int(differ.size), int(differ[0]), P.rows[int(entries[differ[0]])][:80], hex(int(values[differ[0]])), hex(int(w_bits[differ[0]])))
    assert (values[k:] == POISON_U).all(), c
    if want_status:
        differ = np.nonzero(status[:k] != w_status)[0]
        assert differ.size == 0, (c, int(differ[0]), P.rows[int(entries[differ[0]])][:80], int(status[differ[0]]), int(w_status[differ[0]]))
        assert (status[k:] == POISON8).all(), c
    else:
        assert (status == POISON8).all(), c
    assert stats == w_stats and sum(stats.values()) == k, (c, stats, w_stats)
    return w_status, w_bits, w_stats


def index_list(P, count, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.permutation(2 * P.R), rng.randint(0, 2 * P.R, count)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the rows under WIDE
def test_the_mixed_set_under_wide_with_and_without_an_index_list(rj, scan, pool):
    """about 3000 distinct rows -- parse_cases' families, the old window's edges, the range and subnormal edges, repr() of random
    doubles, short mantissas in many spellings, ties and their neighbours, long mantissas, saturation at the group seams -- each
    laid twice: values, statuses, n_range, n_inexact and the return value, through the C ABI and Scan.parse_records(wide=True)"""
    import torch
    every = np.arange(2 * pool.R)
    picked = index_list(pool, 1500, 5)
    idx_t = dev(picked)
    for flags in (pw.WIDE, pw.WIDE | pw.TRIM):
        _, _, w_stats = check(rj, scan, pool, every, F, flags, ctx="every record")
        assert w_stats["n_range"] > 20 and 0 < w_stats["n_inexact"] < 0.01 * len(every) and w_stats["n_malformed"] > 100, w_stats
        check(rj, scan, pool, picked, F, flags, idx_t=idx_t, ctx="index list")
    check(rj, scan, pool, every, F, pw.WIDE, ctx="no d_status", want_status=False)
    for trim in (False, True):
        flags = pw.WIDE | (pw.TRIM if trim else 0)
        m_status, m_bits = pool.meaning(F, flags)
        values, status, stats = scan.parse_records(pool.d, pool.rb_t, pool.re_t, indices=idx_t, kind="float64", trim=trim, stats=True, wide=True)
        assert values.dtype == torch.float64 and status.dtype == torch.uint8 and values.numel() == len(picked) == status.numel()
        assert (values.cpu().numpy().view(np.uint64) == m_bits[picked]).all() and (status.cpu().numpy() == m_status[picked]).all(), trim
        assert stats == dict(zip(STATS, (int(c) for c in np.bincount(m_status[picked], minlength=5)))), (trim, stats)
        assert stats["n_range"] == int((status == rj.PARSE_RANGE).sum()) > 0 and stats["n_inexact"] == int((status == rj.PARSE_INEXACT).sum())
    only = scan.parse_records(pool.d, pool.rb_t, pool.re_t, kind="float64", wide=True)
    assert len(only) == 2 and (only[0].cpu().numpy().view(np.uint64) == pool.meaning(F, pw.WIDE)[1]).all()
    # what the flag is for: rows that have no value without it
    old = pool.meaning(F, 0)[0]
    new = pool.meaning(F, pw.WIDE)[0]
    assert int(((old == pc.INEXACT) & (new == pc.OK)).sum()) > 2000 and not ((old == pc.OK) & (new != pc.OK)).any()


def test_the_same_table_without_the_flag_is_as_before(rj, scan, pool):
    """status and bits equal parse_cases.meaning: FLOAT64 outside the window is INEXACT, never RANGE"""
    every = np.arange(2 * pool.R)
    for flags in (0, pw.TRIM):
        _, _, w_stats = check(rj, scan, pool, every, F, flags, ctx="no flag")
        assert w_stats["n_range"] == 0 and w_stats["n_inexact"] > 2000
    values, status = scan.parse_records(pool.d, pool.rb_t, pool.re_t, kind="float64", trim=True)
    assert (status.cpu().numpy() == pool.meaning(F, pw.TRIM)[0]).all() and (values.cpu().numpy().view(np.uint64) == pool.meaning(F, pw.TRIM)[1]).all()


def test_the_flag_is_inert_for_the_integer_kinds(rj, scan, pool):
    every = np.arange(2 * pool.R)
    for kind in (pc.INT64, pc.UINT64):
        for trim in (0, pw.TRIM):
            without = check(rj, scan, pool, every, kind, trim, ctx="integers")
            with_flag = check(rj, scan, pool, every, kind, trim | pw.WIDE, ctx="integers, WIDE")
            assert (without[0] == with_flag[0]).all() and (without[1] == with_flag[1]).all() and without[2] == with_flag[2]
            assert without[2]["n_inexact"] == 0 and without[2]["n_range"] > 0
    values, status = scan.parse_records(pool.d, pool.rb_t, pool.re_t, kind="int64", trim=True, wide=True)
    assert (status.cpu().numpy() == pool.meaning(pc.INT64, pw.TRIM)[0]).all()
    assert (values.cpu().numpy().view(np.uint64) == pool.meaning(pc.INT64, pw.TRIM)[1]).all()


# ------------------------------------------------------------------------------------------------ beyond one pass of the grid
def test_one_row_more_than_a_pass_of_the_grid(rj, scan, pool):
    """524 289 rows drawn from the pool's entries (both copies), expectations gathered with numpy: the wide kernel's grid
    takes its units round again, a wave adds its five counts up over all of them.  As records of their own (rows alias the
    same bytes) and through an index list.  Then one bad index in the second pass: the call is refused naming it, and no
    output row is written."""
    rng = np.random.RandomState(77)
    pk = rng.randint(0, 2 * pool.R, SCALE_K).astype(np.int64)
    assert SCALE_K > WIDE_GRID_ROWS and SCALE_K > 2 * CHECK_GRID_ROWS
    flags = pw.WIDE | pw.TRIM
    _, _, w_stats = check(rj, scan, pool, pk, F, flags, rb_t=dev(pool.rb[pk]), re_t=dev(pool.re[pk]), ctx="direct")
    assert all(w_stats[s] > 0 for s in STATS), w_stats
    check(rj, scan, pool, pk, F, flags, idx_t=dev(pk), ctx="indexed")
    bad = pk.copy()
    at = WIDE_GRID_ROWS + 1000
    assert CHECK_GRID_ROWS < at < SCALE_K
    bad[at] = 2 * pool.R
    total, values, status, _ = parse_poisoned(rj, scan, pool, dev(bad), F, flags)
    msg = rj.load_library().rj_last_error().decode()
    assert total == RJ_BAD_ARGUMENT and "row %d " % at in msg, (total, msg)
    assert (values == POISON_U).all() and (status == POISON8).all()
    check(rj, scan, pool, pk[:5000], F, flags, idx_t=dev(pk[:5000]), ctx="behind a refusal")


# ------------------------------------------------------------------------------------------------ refusals
def test_unknown_flag_bits_are_refused_and_nothing_is_written(rj, scan, pool):
    lib = rj.load_library()
    for flags in (2, 3, 6):
        for kind in pc.KINDS:
            total, values, status, stats = parse_poisoned(rj, scan, pool, None, kind, flags)
            msg = lib.rj_last_error().decode()
            assert total == RJ_BAD_ARGUMENT and "flag" in msg, (flags, kind, total, msg)
            assert (values == POISON_U).all() and (status == POISON8).all() and stats == dict(zip(STATS, [0xA5A5] * 5)), flags
    check(rj, scan, pool, np.arange(2 * pool.R), F, pw.WIDE | pw.TRIM, ctx="behind a refusal")


# ------------------------------------------------------------------------------------------------ the sample
SAMPLE_LINES = [b"/a 200 0.25", b"/b 500 1e3", b"/a 200 -3.5", b"/c 404", b"/b 200 12abc", b"/a 301  5", b"/b 200 \t1.5", b"/c 200 0.30000000000000004",
                b"/a 200 +4e1", b"/d 200 1e999", b"/d 200 0", b"/e 200 6.02214076e23", b"/f 1 184467440737095516155", b"/f 1 -0.125", b"/g 7 1e-400"]


def test_linegrep_sample_sums_a_float_field_per_distinct_value_of_another(rj, tmp_path):
    """-f 1 -u -A 3: count, value of field 1, the float64 sum of field 3 over its lines, read with TRIM | WIDE; a missing,
    spoilt, infinite or INEXACT field adds 0.  (The values of a group add up exactly in any order.)"""
    path = str(tmp_path / "access.log")
    with open(path, "wb") as fh:
        fh.write(b"\n".join(SAMPLE_LINES) + b"\n")
    seen, count, total = [], {}, {}
    for ln in SAMPLE_LINES:
        parts = ln.split(b" ")
        if parts[0] not in count:
            seen.append(parts[0])
            count[parts[0]], total[parts[0]] = 0, 0.0
        count[parts[0]] += 1
        st, bits = pw.wide_meaning(parts[2] if len(parts) >= 3 else b"", F, True)
        if st == pc.OK:
            total[parts[0]] += pw.float_of(bits)
    want = b"".join(b"%7d %s %s\n" % (count[k], k, repr(total[k]).encode()) for k in seen)
    assert want == (b"      4 /a 36.75\n      3 /b 1001.5\n      2 /c 0.30000000000000004\n      2 /d 0.0\n      1 /e 6.02214076e+23\n"
                    b"      2 /f -0.125\n      1 /g 0.0\n")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    r = subprocess.run([sys.executable, sample, path, " ", "-f", "1", "-u", "-A", "3"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-500:])
    assert r.stdout == want, r.stdout
    r = subprocess.run([sys.executable, sample, path, " ", "-f", "1", "-u", "-a", "3", "-A", "3"], capture_output=True, timeout=60)
    assert r.returncode == 2 and r.stdout == b""
