"""GPU tests (-m gpu) of rj_scan_records / rj_scan_records_select (rejit_amd/csrc/record_join.hip; Scan.run_records /
Scan.select_records, rejit_amd/records.py) and of samples/linegrep_gpu.py.

Expected values come from the oracle's MatchAll over the WHOLE text (or per text, for packed batches), handed to the records
in numpy match by match, by the rule's text: a match with begin b belongs to the last record i with rec_begin[i] <= b and is
kept iff b <= rec_end[i]; a kept match that ends beyond rec_end[i] crosses."""
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


def oracle_spans(oracle, rx, data):
    """Oracle.match_all's C entry point, into a numpy array instead of a list of tuples (64 MiB texts): (m, 2) int64."""
    cap = len(data) + 2
    buf = np.empty(2 * cap, dtype=np.uint64)
    m = oracle.lib.ro_match_all_re(rx, data, len(data), buf.ctypes.data_as(_u64p), cap)
    assert 0 <= m <= cap, (rx, m)
    return buf[:2 * m].astype(np.int64).reshape(m, 2)


def attribute(spans, rb, re_):
    """The rule, match by match -> counts, first (lb(rec_begin): where a record's matches begin or would), kept, matching, crossing"""
    rb, re_ = np.asarray(rb, dtype=np.int64), np.asarray(re_, dtype=np.int64)
    counts = np.zeros(len(rb), dtype=np.int64)
    first = np.searchsorted(spans[:, 0], rb, side="left") if len(rb) else np.zeros(0, dtype=np.int64)
    if len(rb) == 0 or len(spans) == 0:
        return counts, first, 0, 0, 0
    b, e = spans[:, 0], spans[:, 1]
    rec = np.searchsorted(rb, b, side="right") - 1            # the last record that begins at or before b
    kept = (rec >= 0) & (b <= re_[np.maximum(rec, 0)])
    counts = np.bincount(rec[kept], minlength=len(rb)).astype(np.int64)
    # the first kept match of every record with one is where `first` points
    k_idx = np.nonzero(kept)[0]
    first_kept = np.full(len(rb), -1, dtype=np.int64)
    first_kept[rec[k_idx][::-1]] = k_idx[::-1]
    assert (first[counts > 0] == first_kept[counts > 0]).all()
    crossing = int((e[kept] > re_[rec[kept]]).sum())
    return counts, first, int(kept.sum()), int((counts > 0).sum()), crossing


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))).to("cuda:0")


def got_counts(res):
    return res.counts.cpu().numpy().view(np.uint32).astype(np.int64)


def check_run(scan, text_t, rb, re_, want_spans, poison=True):
    """run_records over (rb, re_) against the attribution of want_spans; returns the result.  The output tensors are poisoned
    first: the join writes every row, nothing has to be cleared."""
    import torch
    k = len(rb)
    counts = torch.full((k,), -7, dtype=torch.int32, device=text_t.device) if poison else None
    first = torch.full((k,), -7, dtype=torch.int64, device=text_t.device) if poison else None
    res = scan.run_records(text_t, dev(rb), dev(re_), counts=counts, first=first)
    w_counts, w_first, kept, matching, crossing = attribute(want_spans, rb, re_)
    assert res.n_matches == len(want_spans)
    assert (got_counts(res) == w_counts).all()
    assert (res.first.cpu().numpy() == w_first).all()
    assert (res.n_kept, res.n_matching, res.n_crossing) == (kept, matching, crossing)
    assert res.n_kept == int(w_counts.sum()) and res.n_matches >= res.n_kept
    return res


def check_select(scan, w_counts):
    for invert in (False, True):
        want = np.nonzero((w_counts == 0) if invert else (w_counts > 0))[0]
        got = scan.select_records(invert=invert)
        assert scan.n_selected == len(want), invert
        assert (got.cpu().numpy() == want).all(), invert


# ------------------------------------------------------------------------------------------------ parity with the host batch
def _layout(texts, sep, lead, gaps, rng):
    """As tests/test_gpu_batch_abi.py: `lead` separator bytes, then every text followed by 1..gaps separator bytes."""
    buf = bytearray(bytes([sep]) * lead)
    offsets, sizes = [], []
    for t in texts:
        offsets.append(len(buf))
        sizes.append(len(t))
        buf += t
        buf += bytes([sep]) * rng.randint(1, gaps)
    return bytes(buf), offsets, sizes


def test_packed_records_equal_per_text_oracle(rj, oracle):
    """The patterns and layouts of test_packed_batches_equal_per_text_oracle, the packed buffer resident on the device and the
    records equal to the texts: per text the oracle's count and the oracle's spans, nothing crossing."""
    import torch
    from rejit_amd import records as R
    rng = random.Random(5)
    alphabet = b"abcx \nregxp"
    patterns = [b"regexp", b"[a-c]+x", b"x*", b"^", b"$", b"^a.*x$", b"(ab|bc)+", b"a[^x]*x"]
    with_sep = 0
    for rx in patterns:
        p = rj.Program(rx)
        sep = p.batch_separator()
        if sep < 0:
            continue                      # (matched text by text on the host: such a pattern has no packed layout)
        assert p.info()["ring_artefact_risk"] == 0
        with_sep += 1
        scan = rj.Scan(p)
        for trial in range(4):
            k = rng.choice([1, 2, 7, 40])
            texts = []
            for _ in range(k):
                n = rng.choice([0, 0, 1, 5, 17, 300, 5000])
                texts.append(bytes(rng.choice(alphabet) for _ in range(n)).replace(bytes([sep]), b"q"))
            lead = rng.choice([0, 0, 1, 5])
            buf, offsets, sizes = _layout(texts, sep, lead, rng.choice([1, 3]), rng)
            want = [oracle.match_all(rx, t) for t in texts]
            d = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to("cuda:0")
            rb, re_ = dev(offsets), dev([o + s for o, s in zip(offsets, sizes)])
            res = scan.run_records(d, rb, re_)
            counts = got_counts(res).tolist()
            assert counts == [len(w) for w in want], (rx, trial, lead, sizes[:8])
            spans = scan.spans_tensor(d.device)
            assert R.all_relative_spans(spans, res, rb) == want, (rx, trial)
            assert R.relative_spans(spans, res, rb, k - 1).cpu().tolist() == [list(x) for x in want[-1]]
            assert res.n_crossing == 0 and res.n_kept == sum(counts) and res.n_matches >= res.n_kept
            assert res.n_matches == len(spans) and res.n_matching == sum(c > 0 for c in counts)
            check_select(scan, np.array(counts))
        # pack_records builds the same layout from the texts
        d2, rb2, re2 = R.pack_records(texts, sep, "cuda:0", lead=2, gap=2)
        res = scan.run_records(d2, rb2, re2)
        assert got_counts(res).tolist() == [len(w) for w in want] and res.n_crossing == 0
    assert with_sep >= 5


# ------------------------------------------------------------------------------------------------ lines
def _log_text(mib, seed):
    """Seeded log-like text: a last line without a line break, empty lines, and one line of a third of a MiB (more matches of
    most patterns than a tile stages, more bytes than a tile of ordinary lines spans)."""
    from rejit_amd import workloads as W
    t = W.log_like_numpy(mib << 20, seed)
    a = (mib << 20) // 3
    region = t[a:a + (1 << 20) // 3]
    region[region == 10] = 32
    t[a + 5:a + 8] = 10                  # empty lines right behind each other
    t[-1] = ord("z")
    t[0:7] = np.frombuffer(b"# first", dtype=np.uint8)
    return t


@pytest.mark.parametrize("mib", [1, 17, 64])
def test_lines_equal_the_oracle_attributed_by_the_rule(rj, oracle, mib):
    import torch
    from rejit_amd import records as R
    t = _log_text(mib, seed=100 + mib)
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = R.line_records(d)
    rb, re_ = rb_t.cpu().numpy(), re_t.cpu().numpy()
    # the line table itself: begins behind every line break, ends before the next one
    brk = np.nonzero(t == 10)[0]
    assert (rb == np.concatenate([[0], brk + 1])).all() and (re_ == np.concatenate([brk, [len(t)]])).all()
    assert (re_ - rb == 0).sum() >= 2 and (re_ - rb).max() > 300000 and re_[-1] == len(t) and t[-1] != 10
    for rx in (b"the", b"[a-z]+@[a-z]+", b"^#.*", b"x*", b"[^a]+"):
        p = rj.Program(rx)
        scan = rj.Scan(p)
        want = oracle_spans(oracle, rx, data)
        res = check_run(scan, d, rb, re_, want)
        print("lines %d MiB %-16r risk %d: %d matches, kept %d, matching %d of %d, crossing %d" % (
            mib, rx, p.info()["ring_artefact_risk"], res.n_matches, res.n_kept, res.n_matching, len(rb), res.n_crossing))
        assert (scan.spans_tensor(d.device).cpu().numpy() == want).all(), rx
        w_counts = attribute(want, rb, re_)[0]
        check_select(scan, w_counts)
        if rx == b"x*":
            assert (w_counts > 0).all()           # an empty match on every line, the empty ones included
        if rx == b"[^a]+":
            assert res.n_crossing > 0             # it runs over line breaks
        else:
            assert res.n_crossing == 0


# ------------------------------------------------------------------------------------------------ selection
def test_selection_caps_and_extremes(rj, oracle):
    import torch
    from rejit_amd import records as R
    t = _log_text(1, seed=9)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = R.line_records(d)
    k = rb_t.numel()
    scan = rj.Scan(rj.Program(b"the"))
    res = scan.run_records(d, rb_t, re_t)
    w = got_counts(res)
    want = np.nonzero(w > 0)[0]
    assert 10 < len(want) < k
    # cap smaller than the answer: the full number comes back, nothing is written beyond cap
    lib = rj.load_library()
    out = torch.full((len(want) + 8,), -5, dtype=torch.int64, device="cuda:0")
    cap = len(want) // 2
    st = torch.cuda.current_stream().cuda_stream
    total = lib.rj_scan_records_select(scan._h, 0, ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(st))
    assert total == len(want)
    o = out.cpu().numpy()
    assert (o[:cap] == want[:cap]).all() and (o[cap:] == -5).all()
    assert lib.rj_scan_records_select(scan._h, 1, None, 0, ctypes.c_void_p(st)) == k - len(want)
    got = scan.select_records(cap=3)
    assert got.cpu().tolist() == want[:3].tolist() and scan.n_selected == len(want)
    # all selected / none selected
    every = rj.Scan(rj.Program(b"$"))
    res = every.run_records(d, rb_t, re_t)
    assert res.n_matching == k
    assert every.select_records().cpu().tolist() == list(range(k)) and every.select_records(invert=True).numel() == 0
    none = rj.Scan(rj.Program(b"no such string anywhere"))
    res = none.run_records(d, rb_t, re_t)
    assert (res.n_matches, res.n_kept, res.n_matching) == (0, 0, 0) and got_counts(res).sum() == 0
    assert none.select_records().numel() == 0 and none.select_records(invert=True).cpu().tolist() == list(range(k))
    # zero records
    empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
    res = scan.run_records(d, empty, empty)
    assert (res.n_kept, res.n_matching, res.n_crossing) == (0, 0, 0) and res.n_matches == len(oracle.match_all(b"the", t.tobytes()))
    assert scan.select_records().numel() == 0 and scan.select_records(invert=True).numel() == 0 and scan.n_selected == 0


def test_select_needs_the_last_run_to_be_a_join(rj):
    import torch
    from rejit_amd import records as R
    t = _log_text(1, seed=10)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = R.line_records(d)
    for rx in (b"the", b"agggtaaa|tttaccct"):          # (the second one's count takes the one-kernel count path)
        scan = rj.Scan(rj.Program(rx))
        with pytest.raises(rj.RejitError) as e:
            scan.select_records()
        assert e.value.status == RJ_BAD_ARGUMENT
        scan.run_records(d, rb_t, re_t)
        scan.select_records()
        scan.run_tensor(d)
        with pytest.raises(rj.RejitError) as e:
            scan.select_records()
        assert e.value.status == RJ_BAD_ARGUMENT
        scan.run_records(d, rb_t, re_t)
        scan.select_records()
        scan.count_tensor(d)
        with pytest.raises(rj.RejitError) as e:
            scan.select_records(invert=True)
        assert e.value.status == RJ_BAD_ARGUMENT
        scan.run_records(d, rb_t, re_t)
        assert scan.select_records().numel() == scan.n_selected


# ------------------------------------------------------------------------------------------------ shapes
def test_shapes_that_force_both_search_branches(rj, oracle):
    import torch
    from rejit_amd import workloads as W
    n = 2 << 20
    t = W.random_ascii_numpy(n, seed=4, lo=ord("a"), hi=ord("z"))      # (no 'z')
    t[100:200000:4] = ord("z")
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    scan = rj.Scan(rj.Program(b"z"))
    want = oracle_spans(oracle, b"z", data)
    assert len(want) == 49975
    # one record holding more matches than LDS stages, between records with none and with few
    rb = [0, 64, 250000, 250001]
    re_ = [64, 250000, 250001, n]
    res = check_run(scan, d, rb, re_, want)
    assert got_counts(res)[1] > 40000
    # 2 million one-byte records against three matches
    three = np.full(n, ord("a"), dtype=np.uint8)
    three[[5, 1 << 20, n - 1]] = ord("z")
    d3 = torch.from_numpy(three).to("cuda:0")
    ones = np.arange(n, dtype=np.int64)
    res = check_run(scan, d3, ones, ones + 1, oracle_spans(oracle, b"z", three.tobytes()))
    assert res.n_kept == 3 and scan.select_records().cpu().tolist() == [5, 1 << 20, n - 1]
    assert scan.select_records(invert=True).numel() == n - 3
    # touching records with no gaps, of uneven sizes, over the dense text; empty matches on the seams go to the next record
    rng = np.random.RandomState(3)
    cuts = np.unique(np.concatenate([[0], rng.randint(0, n, 5000), np.arange(100, 200000, 4)[:300]]))
    rb, re_ = cuts, np.concatenate([cuts[1:], [n]])
    check_run(scan, d, rb, re_, want)
    # ... and empty matches exactly on the seams: `$` over lines, records that touch at every line break (and elsewhere) --
    # the match at a seam is the NEXT record's, the one at the end of the text the last record's
    lt = _log_text(1, seed=12)
    dl = torch.from_numpy(lt).to("cuda:0")
    cuts = np.unique(np.concatenate([[0], np.nonzero(lt == 10)[0], rng.randint(0, len(lt), 2000)]))
    rb, re_ = cuts, np.concatenate([cuts[1:], [len(lt)]])
    dollar = rj.Scan(rj.Program(b"$"))
    want_dollar = oracle_spans(oracle, b"$", lt.tobytes())
    res = check_run(dollar, dl, rb, re_, want_dollar)
    assert res.n_kept == res.n_matches == int((lt == 10).sum()) + 1    # no gaps: every match has a record
    w = attribute(want_dollar, rb, re_)[0]
    assert w[0] == 0 and w[-1] >= 1
    check_select(dollar, w)


def test_records_beyond_4gib(rj):
    """4.5 GiB of device text, occurrences planted on both sides of 2^32 (as test_planted_literal_beyond_4gib), cut into
    records of 1 MiB: counts and first against Python."""
    import torch
    from rejit_amd import workloads as W
    dev0 = torch.device("cuda:0")
    n = (9 << 29) + 12345
    t = W.random_ascii_torch(n, 0xBEEF, dev0)
    offs = sorted(set(W.plant_offsets(n, 6, 300, seed=5, boundaries=[1 << 32, (1 << 32) + 1024, 1 << 31, n // 2])
                      + [(1 << 32) - 3, (1 << 32) - 6, (1 << 32), (1 << 32) + 7, n - 6]))
    keep, last = [], -10
    for o in offs:
        if o >= last + 6 and o + 6 <= n:
            keep.append(o)
            last = o
    W.plant(t, keep, b"regexp")
    scan = rj.Scan(rj.Program(b"regexp"))
    rb = np.arange(0, n, 1 << 20, dtype=np.int64)
    re_ = np.minimum(rb + (1 << 20), n)
    res = scan.run_records(t, dev(rb), dev(re_))
    spans = scan.spans_tensor(dev0).cpu().numpy()
    assert set(keep) <= set(spans[:, 0].tolist()) and (spans[:, 0] >= (1 << 32)).sum() >= 5
    w_counts, w_first, kept, matching, crossing = attribute(spans, rb, re_)
    assert (got_counts(res) == w_counts).all() and (res.first.cpu().numpy() == w_first).all()
    assert (res.n_kept, res.n_matching, res.n_crossing, res.n_matches) == (kept, matching, crossing, len(spans))
    assert kept == len(spans) and crossing >= 1        # (a planted occurrence straddles the record seam at 2^31)
    assert w_counts[4096:].sum() >= 5 and w_first[4096] > 0
    check_select(scan, w_counts)


# ------------------------------------------------------------------------------------------------ reuse
def test_one_scan_interleaves_joins_runs_and_counts(rj, oracle):
    import torch
    from rejit_amd import records as R
    ta, tb = _log_text(1, seed=21), _log_text(2, seed=22)
    da, db = torch.from_numpy(ta).to("cuda:0"), torch.from_numpy(tb).to("cuda:0")
    for rx in (b"the", b"[a-z]+@[a-z]+", b"#.*"):
        wa, wb = oracle_spans(oracle, rx, ta.tobytes()), oracle_spans(oracle, rx, tb.tobytes())
        scan = rj.Scan(rj.Program(rx))
        la = [x.cpu().numpy() for x in R.line_records(da)]
        check_run(scan, da, la[0], la[1], wa)
        assert scan.run_tensor(db) == len(wb) and (scan.spans_tensor(db.device).cpu().numpy() == wb).all()
        blocks = np.arange(0, len(tb), 4096, dtype=np.int64)
        check_run(scan, db, blocks, np.minimum(blocks + 4000, len(tb)), wb)           # gaps of 96 bytes
        check_select(scan, attribute(wb, blocks, np.minimum(blocks + 4000, len(tb)))[0])
        assert scan.count_tensor(da) == len(wa)
        check_run(scan, da, [7, 100, 5000], [90, 100, len(ta)], wa)
        check_run(scan, db, [], [], wb)
        check_run(scan, da, la[0], la[1], wa)
        # stats() are the whole-text run's: a fresh scan's run_records against a fresh scan's plain run of the same text, the
        # times apart (a REUSED scan may route its next run by what it met before: tests/test_gpu_sequences.py)
        joined, plain = rj.Scan(rj.Program(rx)), rj.Scan(rj.Program(rx))
        res = check_run(joined, da, la[0], la[1], wa)
        assert plain.run_tensor(da) == res.n_matches
        drop = lambda s: {k: v for k, v in s.items() if not k.endswith("_ms")}
        assert drop(joined.stats()) == drop(plain.stats()), rx
        assert joined.spans() == plain.spans() and joined.device_spans_ptr() != 0


def test_bad_tables_are_refused_and_the_scan_stays_usable(rj, oracle):
    import torch
    t = _log_text(1, seed=30)
    d = torch.from_numpy(t).to("cuda:0")
    n = len(t)
    want = oracle_spans(oracle, b"the", t.tobytes())
    scan = rj.Scan(rj.Program(b"the"))
    lib = rj.load_library()
    good = np.arange(0, n, 512, dtype=np.int64)
    for what, row, edit in (("descending", 699, lambda b, e: b.__setitem__(700, 5)),
                            ("end < begin", 3, lambda b, e: e.__setitem__(3, int(b[3]) - 1)),
                            ("end > n", len(good) - 1, lambda b, e: e.__setitem__(len(good) - 1, n + 1)),
                            ("two bad rows", 40, lambda b, e: (e.__setitem__(40, int(b[41]) + 1), e.__setitem__(1500, n + 9)))):
        b, e = good.copy(), np.minimum(good + 500, n)
        edit(b, e)
        with pytest.raises(rj.RejitError) as err:
            scan.run_records(d, dev(b), dev(e))
        assert err.value.status == RJ_BAD_ARGUMENT, what
        assert ("row %d " % row) in lib.rj_last_error().decode(), (what, lib.rj_last_error())
        with pytest.raises(rj.RejitError):
            scan.select_records()                          # (a refused join leaves nothing to select from)
        check_run(scan, d, good, np.minimum(good + 500, n), want)
    # null tables with records, a null text
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.rj_scan_records(scan._h, ctypes.c_void_p(d.data_ptr()), n, None, None, 3, None, None, None, st) == RJ_BAD_ARGUMENT
    assert lib.rj_scan_records(scan._h, None, n, None, None, 0, None, None, None, st) == RJ_BAD_ARGUMENT
    # no outputs wanted at all: the summary alone, and the selection from the scan's own counts
    from rejit_amd.api import _RecordStats
    rs = _RecordStats()
    gb, ge = dev(good), dev(np.minimum(good + 500, n))
    kept = lib.rj_scan_records(scan._h, ctypes.c_void_p(d.data_ptr()), n, ctypes.c_void_p(gb.data_ptr()), ctypes.c_void_p(ge.data_ptr()),
                               len(good), None, None, ctypes.byref(rs), st)
    w_counts, _, w_kept, w_matching, w_crossing = attribute(want, good, np.minimum(good + 500, n))
    assert kept == w_kept and (rs.n_kept, rs.n_matching, rs.n_crossing, rs.n_matches) == (w_kept, w_matching, w_crossing, len(want))
    out = torch.empty(len(good), dtype=torch.int64, device="cuda:0")
    k = lib.rj_scan_records_select(scan._h, 0, ctypes.c_void_p(out.data_ptr()), len(good), st)
    assert k == w_matching and (out[:k].cpu().numpy() == np.nonzero(w_counts)[0]).all()


# ------------------------------------------------------------------------------------------------ samples/linegrep_gpu.py
def test_linegrep_sample_equals_gnu_grep(rj, tmp_path):
    grep = shutil.which("grep")
    assert grep, "GNU grep is needed for this comparison"
    rng = random.Random(44)
    words = [b"int", b"regexp", b"return", b"for (;;)", b"x = y + 1;", b"// a comment", b"regexps", b"char* s", b"", b"}", b"error 42"]
    lines = [b" ".join(rng.choice(words) for _ in range(rng.randint(0, 6))) for _ in range(20000)]
    path = str(tmp_path / "file.txt")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    # a last line without a line break: three patterns, the three forms; a terminated file: a pattern without a match (exit status 1)
    for terminated, patterns, forms in ((False, ("regexp", "regexps|return", "[0-9]+"), (["-c"], ["-v", "-c"], ["-n"])),
                                        (True, ("no such thing",), (["-c"], ["-v", "-c"]))):
        with open(path, "wb") as fh:
            fh.write(b"\n".join(lines) + (b"\n" if terminated else b""))
        for pattern in patterns:
            for opts in forms:
                g = subprocess.run([grep, "-E"] + opts + [pattern, path], capture_output=True, timeout=120)
                assert g.returncode in (0, 1)
                want = g.stdout
                if opts == ["-n"]:
                    want = b"".join(l.split(b":", 1)[0] + b"\n" for l in g.stdout.splitlines())     # grep -n | cut -d: -f1
                r = subprocess.run([sys.executable, sample, path, pattern] + opts, capture_output=True, timeout=300)
                assert r.returncode == g.returncode, (pattern, opts, r.stderr.decode()[-500:])
                assert r.stdout == want, (pattern, opts, terminated)
