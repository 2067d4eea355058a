"""GPU tests (-m gpu) of rj_scan_records_replace (rejit_amd/csrc/record_replace.hip; Scan.replace_records) and of
samples/linegrep_gpu.py -s.

The meaning: R(r) = the record's bytes with each of its own matches (spans[first[r] : first[r] + count[r]]) replaced by `with`,
left to right; ob(0) = lead, ob(j + 1) = ob(j) + len(R(r(j))) + gap; out[ob(j) : ...] = R(r(j)), every other byte of [0, total) =
fill.  The shape tests plant a literal at chosen offsets of a text that holds it nowhere else, so the expected bytes are Python's
bytes.replace of each record's host copy; the end-to-end tests splice by checkers.Oracle's spans, handed to the lines by the
join rule in numpy.  Outputs are poisoned first: every byte of [0, total) is written and nothing behind it."""
import ctypes
import os
import random
import re
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
CHUNK = 16384            # record_replace.hip's kCopyChunk
POISON = 0xA5
LIT = b"@#"              # the planted literal; the texts around it are lower-case letters
SETTINGS = ((0, 0), (1, 17), (1, 0), (0, 17))      # (gap, lead)
WITHS = (b"", b"X", b"0123456789abcdef", b"0123456789abcdefg", b"<" + b"0123456789" * 3 + b"abcdefgh>")


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
    return rj.Scan(rj.Program(LIT))


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))).to("cuda:0")


def letters(n, seed):
    return np.random.RandomState(seed).randint(ord("a"), ord("z") + 1, n).astype(np.uint8)


def expect(pieces, rows, repl, fill, lead, gap):
    """pieces[r]: the text pieces of record r around its matches -> (out bytes, out_begin, out_end)"""
    out = bytearray(bytes([fill]) * lead)
    ob, oe = [], []
    for r in rows:
        ob.append(len(out))
        out += repl.join(pieces[r])
        oe.append(len(out))
        out += bytes([fill]) * gap
    return bytes(out), np.array(ob, dtype=np.int64), np.array(oe, dtype=np.int64)


def replace_poisoned(scan, d, rb_t, re_t, res, repl, want_total, indices=None, room=64, **kw):
    """replace_records into a poisoned buffer; -> (out, out_begin, out_end, the bytes behind total)"""
    import torch
    buf = torch.full((want_total + room,), POISON, dtype=torch.uint8, device=d.device)
    out, ob, oe = scan.replace_records(d, rb_t, re_t, res, repl, indices=indices, out=buf, **kw)
    return out.cpu().numpy(), ob.cpu().numpy(), oe.cpu().numpy(), buf[out.numel():].cpu().numpy()


def check(scan, d, rb_t, re_t, res, pieces, repl, rows=None, fill=0x7C, lead=0, gap=1):
    n_rows = range(len(pieces)) if rows is None else rows
    want, w_ob, w_oe = expect(pieces, n_rows, repl, fill, lead, gap)
    out, ob, oe, behind = replace_poisoned(scan, d, rb_t, re_t, res, repl, len(want), indices=None if rows is None else dev(rows), fill=fill, lead=lead,
                                           gap=gap)
    ctx = (len(pieces), None if rows is None else len(rows), len(repl), fill, lead, gap)
    assert len(out) == len(want), (ctx, len(out), len(want))
    assert (ob == w_ob).all() and (oe == w_oe).all(), ctx
    got = out.tobytes()
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError((ctx, at, got[max(at - 20, 0):at + 20], want[max(at - 20, 0):at + 20]))
    assert (behind == POISON).all(), ctx


# ------------------------------------------------------------------------------------------------ shapes
def _planted(k, rng, rare_big):
    """k records with lengths from {0, 1, 15, 16, 17, chunk - 1, chunk, chunk + 1}, 0..3 bytes of text between them, and 0, 1, 2
    or 300 copies of LIT planted inside each where they fit: one anywhere; two at the record's first and last bytes; 300 evenly.
    -> (text, rec_begin, rec_end, the number of matches)"""
    small, big = [0, 1, 15, 16, 17], [CHUNK - 1, CHUNK, CHUNK + 1]
    if rare_big:
        lens = np.where(rng.rand(k) < 0.06, rng.choice(big, k), rng.choice(small + [40, 100], k))
    else:
        lens = rng.choice(small + big, k)
    seams = rng.randint(0, 4, k)
    rb = 5 + np.concatenate([[0], np.cumsum(lens + seams)[:-1]]).astype(np.int64)
    n = int(rb[-1] + lens[-1]) + 9
    t = letters(n, k)
    m = 0
    for b, ln, c in zip(rb.tolist(), lens.tolist(), rng.choice([0, 1, 2, 300], k).tolist()):
        if c == 300 and ln < 600:
            c = 2
        if c == 2 and ln < 4:
            c = 1
        if c == 1 and ln < 2:
            c = 0
        at = [] if c == 0 else [rng.randint(0, ln - 1)] if c == 1 else [0, ln - 2] if c == 2 else [i * (ln // 300) for i in range(300)]
        for a in at:
            t[b + a], t[b + a + 1] = LIT[0], LIT[1]
        m += c
    return t, rb, rb + lens, m


@pytest.mark.parametrize("k", [255, 256, 257, 3 * 64 * 256 + 1])
def test_shapes_equal_the_meaning(rj, scan, k):
    """Tables of 255, 256, 257 rows and of more units than one look-back group; every record length around a 16-byte group and
    around a chunk; 0, 1, 2 and 300 matches in a record; with_len 0, 1, 16, 17 and 40 at gap 0 / 1 and lead 0 / 17."""
    import torch
    rng = np.random.RandomState(k)
    t, rb, re_, m = _planted(k, rng, rare_big=k > 1000)
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matches == m == res.n_kept and res.n_crossing == 0
    pieces = [data[b:e].split(LIT) for b, e in zip(rb.tolist(), re_.tolist())]
    # every with_len at every setting for the small tables; for the large one each with_len once, the four settings among them
    combos = [(w, s) for w in WITHS for s in SETTINGS] if k < 1000 else [(w, SETTINGS[i % 4]) for i, w in enumerate(WITHS)]
    for repl, (gap, lead) in combos:
        check(scan, d, rb_t, re_t, res, pieces, repl, lead=lead, gap=gap)
    # a permutation and a take with repeats through the indices; the library's own allocation (one size query) gives the same
    perm = rng.permutation(k)[:min(k, 3000)]
    check(scan, d, rb_t, re_t, res, pieces, b"<>", rows=perm.tolist(), lead=1, gap=1)
    take = rng.randint(0, k, 300).tolist()
    want, w_ob, w_oe = expect(pieces, take, b"<>", 0, 0, 0)
    out, ob, oe = scan.replace_records(d, rb_t, re_t, res, b"<>", indices=dev(take), fill=0, lead=0, gap=0)
    assert out.cpu().numpy().tobytes() == want and (ob.cpu().numpy() == w_ob).all() and (oe.cpu().numpy() == w_oe).all()


def test_a_list_that_crosses_a_look_back_group_of_the_table_kernel(rj, scan):
    """64 * 256 + 1 matches: the table kernel's 65th unit begins a second look-back group."""
    import torch
    m = 64 * 256 + 1
    t = letters(5 * m + 995, 3)
    at = 5 * np.arange(m) + 1
    t[at], t[at + 1] = LIT[0], LIT[1]
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    rb = np.arange(0, len(t), 1000, dtype=np.int64)              # records of 1000 bytes that touch; no match lies on a seam
    re_ = np.minimum(rb + 1000, len(t))
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matches == m and res.n_crossing == 0
    pieces = [data[b:e].split(LIT) for b, e in zip(rb.tolist(), re_.tolist())]
    for repl in (b"", b"0123456789abcdefg"):
        check(scan, d, rb_t, re_t, res, pieces, repl)
    check(scan, d, rb_t, re_t, res, pieces, b"X", rows=[len(rb) - 1, 0, 33, 33], gap=0, lead=17)


def test_no_rows_and_empty_outputs(rj, scan):
    import torch
    t = np.frombuffer(b"01@#456@#9", dtype=np.uint8).copy()
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev([2, 4]), dev([4, 9])
    res = scan.run_records(d, rb_t, re_t)
    pieces = [[b"", b""], [b"456", b""]]
    check(scan, d, rb_t, re_t, res, pieces, b"", lead=0, gap=0)                 # deleting a record that is one match
    check(scan, d, rb_t, re_t, res, pieces, b"", rows=[0, 0, 0], lead=0, gap=0)  # rows, but no bytes at all
    check(scan, d, rb_t, re_t, res, pieces, b"xy", rows=[], lead=5, gap=1)      # an empty selection is not "every record"
    empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
    res0 = scan.run_records(d, empty, empty)
    out, ob, oe = scan.replace_records(d, empty, empty, res0, b"xy", fill=1)
    assert out.numel() == 0 and ob.numel() == 0 and oe.numel() == 0


@pytest.mark.parametrize("k", [1, 257, 64 * 256 + 1])
def test_without_a_match_the_replace_is_the_pack(rj, scan, k):
    """A pattern that matches nowhere in the text: replace_records is pack_records, byte for byte and row for row -- the two
    policies of the one copy kernel frame (record_frame.h's copy_chunks) describe the same output.  One row, 257 rows and one
    look-back group plus one unit; lead 3, gap 1; out_cap whole and cutting a record."""
    import torch
    lib = rj.load_library()
    rng = np.random.RandomState(k)
    lens = rng.choice([0, 1, 15, 16, 17, 40, 100], k)
    cut_row = k // 2
    lens[cut_row] = 40
    rb = 5 + np.concatenate([[0], np.cumsum(lens + rng.randint(0, 3, k))[:-1]]).astype(np.int64)
    re_ = rb + lens
    t = letters(int(re_[-1]) + 9, k)
    data, n = t.tobytes(), len(t)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matches == 0 and res.n_kept == 0
    want, w_ob, w_oe = expect([[data[b:e]] for b, e in zip(rb.tolist(), re_.tolist())], range(k), b"xyz", 0x7C, 3, 1)
    want = np.frombuffer(want, dtype=np.uint8)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    for cap in (int(w_ob[cut_row]) + 20, len(want)):
        got = []
        for replace in (False, True):
            buf = torch.full((len(want) + 64,), POISON, dtype=torch.uint8, device="cuda:0")
            ob = torch.full((k,), -7, dtype=torch.int64, device="cuda:0")
            oe = torch.full((k,), -7, dtype=torch.int64, device="cuda:0")
            if replace:
                total = lib.rj_scan_records_replace(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), None, 0, b"xyz", 3, 0x7C, 3, 1,
                                                    vp(buf), cap, vp(ob), vp(oe), st)
            else:
                total = lib.rj_scan_records_pack(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, None, 0, 0x7C, 3, 1, vp(buf), cap, vp(ob), vp(oe), st)
            assert total == len(want), (k, cap, replace, total)
            got.append((buf.cpu().numpy(), ob.cpu().numpy(), oe.cpu().numpy()))
        (p_out, p_ob, p_oe), (r_out, r_ob, r_oe) = got
        assert (r_out == p_out).all() and (r_ob == p_ob).all() and (r_oe == p_oe).all(), (k, cap)
        assert (p_out[:cap] == want[:cap]).all() and (p_out[cap:] == POISON).all(), (k, cap)
        assert (p_ob == w_ob).all() and (p_oe == w_oe).all(), (k, cap)


# ------------------------------------------------------------------------------------------------ skew
def test_one_record_with_a_million_matches_and_a_million_records_with_one(rj, scan):
    """16 MiB with LIT in every block of 16 bytes: as ONE record among 50 000 empty ones, and as 2^20 records of 16 bytes.
    Expected with torch ops on the device: every block becomes its five bytes before LIT, `with`, its nine bytes behind."""
    import torch
    big = 16 << 20
    blocks = big // 16
    g = torch.Generator(device="cuda:0").manual_seed(9)
    d = torch.randint(ord("a"), ord("z") + 1, (big + 16,), dtype=torch.uint8, device="cuda:0", generator=g)
    body = d[8:8 + big].view(blocks, 16)
    body[:, 5], body[:, 6] = LIT[0], LIT[1]
    repl = b"XYZ"
    w = torch.tensor(list(repl), dtype=torch.uint8, device="cuda:0")
    new_blocks = torch.cat([body[:, :5], w.expand(blocks, 3), body[:, 7:]], dim=1)           # (blocks, 17)
    # one record
    rb = np.concatenate([np.full(25000, 2), [8], np.full(25000, big + 12)]).astype(np.int64)
    re_ = rb.copy()
    re_[25000] = 8 + big
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matches == blocks == res.n_kept and res.n_matching == 1
    total = 17 * blocks + 50001
    buf = torch.full((total + 64,), POISON, dtype=torch.uint8, device="cuda:0")
    out, ob, oe = scan.replace_records(d, rb_t, re_t, res, repl, fill=0x7C, lead=0, gap=1, out=buf)
    assert out.numel() == total
    assert bool((out[:25000] == 0x7C).all()) and bool((out[25000 + 17 * blocks:] == 0x7C).all()) and bool((buf[total:] == POISON).all())
    assert torch.equal(out[25000:25000 + 17 * blocks], new_blocks.reshape(-1))
    assert ob.cpu().tolist()[24999:25002] == [24999, 25000, 25001 + 17 * blocks] and int(oe[25000]) == 25000 + 17 * blocks
    # a record per block
    rb_t = torch.arange(8, 8 + big, 16, device="cuda:0")
    re_t = rb_t + 16
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matching == blocks and res.n_crossing == 0
    buf = torch.full((18 * blocks + 64,), POISON, dtype=torch.uint8, device="cuda:0")
    out, ob, oe = scan.replace_records(d, rb_t, re_t, res, repl, fill=10, lead=0, gap=1, out=buf)
    assert out.numel() == 18 * blocks and bool((buf[out.numel():] == POISON).all())
    rows = out.view(blocks, 18)
    assert torch.equal(rows[:, :17], new_blocks) and bool((rows[:, 17] == 10).all())
    assert torch.equal(ob, 18 * torch.arange(blocks, device="cuda:0")) and torch.equal(oe, ob + 17)


# ------------------------------------------------------------------------------------------------ end to end
def _oracle_spans(oracle, rx, data):
    cap = len(data) + 2
    buf = np.empty(2 * cap, dtype=np.uint64)
    m = oracle.lib.ro_match_all_re(rx, data, len(data), buf.ctypes.data_as(_u64p), cap)
    assert 0 <= m <= cap, (rx, m)
    return buf[:2 * m].astype(np.int64).reshape(m, 2)


def _join(rb, re_, spans):
    """the join rule in numpy -> (first, count, the number of kept matches that end beyond their record)"""
    begins = spans[:, 0]
    key = np.minimum(re_ + 1, np.concatenate([rb[1:], [np.iinfo(np.int64).max]]))
    first = np.searchsorted(begins, rb, side="left")
    count = np.maximum(np.searchsorted(begins, key, side="left") - first, 0)
    has = count > 0
    last_end = spans[(first + count - 1)[has], 1]
    return first, count, int((last_end > re_[has]).sum())


def _line_pieces(data, rb, re_, spans, first, count):
    out = []
    sp = spans.tolist()
    for b, e, f, c in zip(rb.tolist(), re_.tolist(), first.tolist(), count.tolist()):
        own = sp[f:f + c]
        out.append([data[x:y] for x, y in zip([b] + [o[1] for o in own], [o[0] for o in own] + [e])])
    return out


def test_lines_replaced_end_to_end_against_the_oracle(rj, oracle):
    """1 MiB of log-like text cut into its lines; `the`, `[0-9]+` and ` *` (empty matches everywhere) replaced by nothing, by one
    byte and by ten, in every line and in the lines select_records lists in both senses.  The scan's spans and its selection
    are what they were before the call."""
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
    assert len(data.split(b"\n")) == len(rb)
    for rx in (b"the", b"[0-9]+", b" *"):
        spans = _oracle_spans(oracle, rx, data)
        first, count, n_crossing = _join(rb, re_, spans)
        assert n_crossing == 0 and int(count.sum()) == len(spans), rx        # the reference alone: no match crosses a line break
        pieces = _line_pieces(data, rb, re_, spans, first, count)
        scan = rj.Scan(rj.Program(rx))
        res = scan.run_records(d, rb_t, re_t)
        before = scan.spans_tensor(d.device).clone()
        assert (before.cpu().numpy() == spans).all() and res.n_crossing == 0
        for invert in (None, False, True):
            idx = None if invert is None else scan.select_records(invert=invert)
            rows = range(len(rb)) if invert is None else np.nonzero((count == 0) if invert else (count > 0))[0].tolist()
            if invert is not None:
                assert idx.cpu().tolist() == rows, (rx, invert)          # (` *` matches in every line: no row without)
            for repl in (b"", b"#", b"<<number>>"):
                want, w_ob, w_oe = expect(pieces, rows, repl, 10, 0, 1)
                out, ob, oe, behind = replace_poisoned(scan, d, rb_t, re_t, res, repl, len(want), indices=idx, fill=10, lead=0, gap=1)
                assert out.tobytes() == want, (rx, invert, repl)
                assert (behind == POISON).all() and (ob == w_ob).all() and (oe == w_oe).all()
            assert torch.equal(scan.spans_tensor(d.device), before)
            if invert is not None:
                assert torch.equal(scan.select_records(invert=invert), idx) and scan.n_selected == len(rows)


# ------------------------------------------------------------------------------------------------ samples/linegrep_gpu.py -s
def test_linegrep_sample_prints_what_sed_prints(rj, tmp_path):
    sed, grep = shutil.which("sed"), shutil.which("grep")
    rng = random.Random(45)
    words = [b"int", b"regexp", b"return", b"for (;;)", b"x = y + 1;", b"// a comment", b"regexps", b"char* s", b"", b"}", b"error 42"]
    lines = [b" ".join(rng.choice(words) for _ in range(rng.randint(0, 6))) for _ in range(5000)]
    path = str(tmp_path / "file.txt")
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    for terminated, cases in ((False, (("regexps|return", "FOO", []), ("[0-9]+", "", ["-p"]))),
                              (True, (("regexp", "<<word>>", ["-p"]), ("int|char", "T", [])))):
        with open(path, "wb") as fh:
            fh.write(b"\n".join(lines) + (b"\n" if terminated else b""))
        for pattern, repl, opts in cases:
            r = subprocess.run([sys.executable, sample, path, pattern, "-s", repl] + opts, capture_output=True, timeout=300)
            assert r.returncode == 0, (pattern, opts, r.stderr.decode()[-500:])
            assert r.stdout.count(b"\n") > 500
            if not sed or (opts and not grep):
                continue                     # (the comparison needs the system's sed; the sample has run)
            script = "s/%s/%s/g" % (pattern, repl)
            if opts:
                g = subprocess.run([grep, "-E", pattern, path], capture_output=True, timeout=120)
                s = subprocess.run([sed, "-E", script], input=g.stdout, capture_output=True, timeout=120)
            else:
                s = subprocess.run([sed, "-E", script, path], capture_output=True, timeout=120)
            assert s.returncode == 0
            assert r.stdout == s.stdout, (pattern, repl, opts, terminated)


# ------------------------------------------------------------------------------------------------ crossing
def test_crossing_matches_are_refused_and_packing_first_makes_the_strings_independent(rj, oracle):
    """The Arrow-layout `ab+` column of test_gpu_record_pack.py: on the touching strings replace_records names the first row
    with a match that runs into the next string; packed with the separator, every string is the oracle's matches spliced."""
    import torch
    from rejit_amd import records as R
    rng = random.Random(8)
    texts = []
    for i in range(700):
        body = bytes(rng.choice(b"abbc ") for _ in range(rng.choice([0, 1, 3, 20, 90])))
        texts.append((b"b" if i % 3 == 1 else b"") + body + (b"a" if i % 3 == 0 else b""))
    rx = b"ab+"
    p = rj.Program(rx)
    scan = rj.Scan(p)
    whole = b"".join(texts)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.int64)
    d = torch.from_numpy(np.frombuffer(whole, dtype=np.uint8).copy()).to("cuda:0")
    rb_t, re_t = R.offsets_records(dev(offsets))
    spans = np.array(oracle.match_all(rx, whole), dtype=np.int64).reshape(-1, 2)
    first, count, n_crossing = _join(offsets[:-1], offsets[1:], spans)
    has = count > 0
    crossing_rows = np.nonzero(has)[0][spans[(first + count - 1)[has], 1] > offsets[1:][has]]
    assert n_crossing > 0 and len(crossing_rows) == n_crossing
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_crossing == n_crossing
    buf = torch.full((d.numel() + 64,), POISON, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(rj.RejitError) as err:
        scan.replace_records(d, rb_t, re_t, res, b"X", fill=0, lead=0, gap=0, out=buf)
    assert err.value.status == RJ_BAD_ARGUMENT and ("row %d " % crossing_rows[0]) in err.value.message, err.value.message
    assert "rj_scan_records_pack" in err.value.message and "independent" in err.value.message
    assert bool((buf == POISON).all())
    # through the indices: the first crossing row at j = 2
    clean = np.nonzero(~np.isin(np.arange(700), crossing_rows))[0]
    with pytest.raises(rj.RejitError) as err:
        scan.replace_records(d, rb_t, re_t, res, b"X", indices=dev([clean[0], clean[1], crossing_rows[3], crossing_rows[0]]), fill=0, out=buf)
    assert err.value.status == RJ_BAD_ARGUMENT and "row 2 " in err.value.message
    # ... and the rows without a crossing match alone are fine
    scan.replace_records(d, rb_t, re_t, res, b"X", indices=dev(clean), fill=0)
    # packed with the separator: independent
    packed, ob, oe = scan.pack_records(d, rb_t, re_t)
    res = scan.run_records(packed, ob, oe)
    assert res.n_crossing == 0
    for repl in (b"", b"<ab>"):
        out, nb, ne = scan.replace_records(packed, ob, oe, res, repl, fill=0, lead=0, gap=0)
        want = []
        for x in texts:
            pos, parts = 0, []
            for b, e in oracle.match_all(rx, x):
                parts.append(x[pos:b])
                pos = e
            want.append(repl.join(parts + [x[pos:]]))
        assert out.cpu().numpy().tobytes() == b"".join(want)
        nb, ne = nb.cpu().numpy(), ne.cpu().numpy()
        assert nb[0] == 0 and (ne[:-1] == nb[1:]).all() and (ne - nb == [len(x) for x in want]).all() and ne[-1] == out.numel()


# ------------------------------------------------------------------------------------------------ capacity and refusals
def test_size_query_and_out_cap(rj, scan):
    import torch
    lib = rj.load_library()
    rng = np.random.RandomState(5)
    t, rb, re_, m = _planted(300, rng, rare_big=False)
    data = t.tobytes()
    n = len(t)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    repl = WITHS[4]
    pieces = [data[b:e].split(LIT) for b, e in zip(rb.tolist(), re_.tolist())]
    want, w_ob, w_oe = expect(pieces, range(300), repl, 0x7C, 3, 2)
    want = np.frombuffer(want, dtype=np.uint8)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(out, cap, ob=None, oe=None):
        return lib.rj_scan_records_replace(scan._h, vp(d), n, vp(rb_t), vp(re_t), 300, vp(res.counts), vp(res.first), None, 0, repl, len(repl), 0x7C, 3, 2,
                                           vp(out) if out is not None else None, cap, vp(ob) if ob is not None else None,
                                           vp(oe) if oe is not None else None, st)
    # the size query: no output, the tables still written
    ob = torch.full((300,), -7, dtype=torch.int64, device="cuda:0")
    oe = torch.full((300,), -7, dtype=torch.int64, device="cuda:0")
    assert call(None, 0, ob, oe) == len(want)
    assert (ob.cpu().numpy() == w_ob).all() and (oe.cpu().numpy() == w_oe).all()
    assert call(None, 0) == len(want)
    dense = int(np.argmax([len(p) for p in pieces]))        # a record with 300 matches
    assert len(pieces[dense]) == 301 and len(pieces[dense][0]) == 0
    plain = int(np.argmax([len(p[0]) for p in pieces]))     # ... and one with a long stretch of text at its begin
    for cap in (int(w_ob[dense]) + 17,                 # inside a replacement (the record begins with one, 40 bytes long)
                int(w_ob[plain]) + 4097,               # inside a text piece
                int(w_oe[dense]) + 1,                  # inside a gap
                16, 1, len(want) - 1, len(want), len(want) + 40):
        buf = torch.full((len(want) + 64,), POISON, dtype=torch.uint8, device="cuda:0")
        assert call(buf, cap) == len(want), cap        # (without the caller's tables: the scan's own begins)
        got = buf.cpu().numpy()
        lim = min(cap, len(want))
        assert (got[:lim] == want[:lim]).all() and (got[lim:] == POISON).all(), cap


def test_refusals_and_the_scan_stays_usable(rj):
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    lib = rj.load_library()
    t = W.log_like_numpy(1 << 17, 3)
    t[100:108] = np.frombuffer(b"agggtaaa", dtype=np.uint8)
    n = len(t)
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    scan = rj.Scan(rj.Program(b"[0-9]+"))
    rb_t, re_t = R.line_records(d)                         # lines: `[0-9]+` crosses none
    rb, re_ = rb_t.cpu().numpy(), re_t.cpu().numpy()
    k = len(rb)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_crossing == 0 and res.n_matching > 20 and k > 100
    sel0 = scan.select_records().clone()
    spans0 = scan.spans_tensor(d.device).clone()
    buf = torch.full((2 * n + 64,), POISON, dtype=torch.uint8, device="cuda:0")
    # the pack's own refusals, naming the row
    for what, row, edit, idx in (("end < begin", k // 2, lambda b, e: e.__setitem__(k // 2, int(b[k // 2]) - 1), None),
                                 ("end > n", k - 1, lambda b, e: e.__setitem__(k - 1, n + 1), None),
                                 ("an index == n_records", 2, lambda b, e: None, [5, 0, k, 1]),
                                 ("a negative index", 1, lambda b, e: None, [5, -1, k, 1])):
        b, e = rb.copy(), re_.copy()
        edit(b, e)
        with pytest.raises(rj.RejitError) as err:
            scan.replace_records(d, dev(b), dev(e), res, b"THE", indices=None if idx is None else dev(idx), fill=10, out=buf)
        assert err.value.status == RJ_BAD_ARGUMENT and ("row %d " % row) in err.value.message, (what, err.value.message)
        assert bool((buf == POISON).all()), what
    # a record cut short under its last match: that match now ends beyond it
    has = np.nonzero(res.counts.cpu().numpy() > 0)[0]
    row = int(has[5])
    last = int(res.first[row]) + int(res.counts[row]) - 1
    e = re_.copy()
    e[row] = int(spans0[last, 1]) - 1
    with pytest.raises(rj.RejitError) as err:
        scan.replace_records(d, rb_t, dev(e), res, b"THE", fill=10, out=buf)
    assert err.value.status == RJ_BAD_ARGUMENT and ("row %d " % row) in err.value.message and "independent" in err.value.message
    # ... and one that begins behind its first match
    b = rb.copy()
    b[row] = int(spans0[int(res.first[row]), 0]) + 1
    with pytest.raises(rj.RejitError) as err:
        scan.replace_records(d, dev(b), re_t, res, b"THE", fill=10, out=buf)
    assert err.value.status == RJ_BAD_ARGUMENT and ("row %d " % row) in err.value.message and "begins before" in err.value.message
    # stale counts / first: those of a run of another pattern (many more matches: first + count leaves this scan's list)
    other = rj.Scan(rj.Program(b"[a-z]"))
    stale = other.run_records(d, rb_t, re_t)
    assert stale.n_matches > 4 * res.n_matches
    with pytest.raises(rj.RejitError) as err:
        scan.replace_records(d, rb_t, re_t, stale, b"THE", fill=10, out=buf)
    assert err.value.status == RJ_BAD_ARGUMENT and "row " in err.value.message
    assert bool((buf == POISON).all())
    # a counts-only last run: there is no list
    dna = rj.Scan(rj.Program(b"agggtaaa|tttaccct"))
    dna_res = dna.run_records(d, rb_t, re_t)
    assert dna.count_tensor(d) == dna_res.n_matches >= 1 and dna.stats()["count_path"] == 1
    with pytest.raises(rj.RejitError) as err:
        dna.replace_records(d, rb_t, re_t, dna_res, b"THE", fill=10, out=buf)
    assert err.value.status == RJ_BAD_ARGUMENT and "counts-only" in err.value.message and "no span list" in err.value.message
    dna_res = dna.run_records(d, rb_t, re_t)               # usable afterwards
    row = int(np.searchsorted(rb, 100, side="right")) - 1
    out, _, _ = dna.replace_records(d, rb_t, re_t, dna_res, b"", indices=dev([row]), fill=10, gap=0)
    assert out.cpu().numpy().tobytes() == data[rb[row]:re_[row]].replace(b"agggtaaa", b"") and b"agggtaaa" in data[rb[row]:re_[row]]
    # arguments: a misaligned output, fill out of range, null tables, `with` missing, a pattern without a separator
    with pytest.raises(rj.RejitError) as err:
        scan.replace_records(d, rb_t, re_t, res, b"THE", fill=10, out=buf[8:])
    assert err.value.status == RJ_BAD_ARGUMENT and "aligned" in err.value.message
    for fill in (256, -1):
        with pytest.raises(rj.RejitError) as err:
            scan.replace_records(d, rb_t, re_t, res, b"THE", fill=fill)
        assert err.value.status == RJ_BAD_ARGUMENT and "fill" in err.value.message
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    f = lib.rj_scan_records_replace
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, None, vp(res.first), None, 0, b"x", 1, 10, 0, 1, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, vp(res.counts), None, None, 0, b"x", 1, 10, 0, 1, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), None, 0, None, 1, 10, 0, 1, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, None, None, 3, None, None, None, 0, b"x", 1, 10, 0, 1, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    assert f(None, vp(d), n, None, None, 0, None, None, None, 0, b"x", 1, 10, 0, 1, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, vp(d), n, None, None, 0, None, None, None, 0, b"x", 1, 10, 9, 1, None, 0, None, None, st) == 9
    assert f(scan._h, vp(d), n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), None, 0, b"x", 1 << 41, 10, 0, 1, None, 0, None, None, st) == RJ_BAD_ARGUMENT
    no_sep = [rx for rx in (b"[^a]+|a+", b".*|[\n\r]+") if rj.Program(rx).batch_separator() < 0]
    assert no_sep, "a pattern that consumes every byte has no separator"
    with pytest.raises(rj.RejitError) as err:
        rj.Scan(rj.Program(no_sep[0])).replace_records(d, rb_t, re_t, res, b"x")
    assert err.value.status == RJ_BAD_ARGUMENT and "separator" in err.value.message
    # the scan is usable afterwards: its list and its last join are what they were, and the call itself works
    assert torch.equal(scan.spans_tensor(d.device), spans0) and torch.equal(scan.select_records(), sel0)
    pieces = [re.split(b"[0-9]+", data[b:e]) for b, e in zip(rb.tolist(), re_.tolist())]
    check(scan, d, rb_t, re_t, res, pieces, b"THE", fill=10)
    assert scan.run_records(d, rb_t, re_t).n_kept == res.n_kept


# ------------------------------------------------------------------------------------------------ beyond 4 GiB
def test_records_and_matches_beyond_4gib(rj, scan):
    """A text of 2^32 + 4096 bytes that is never filled; records and planted matches in its last 4 KiB, rows taken through
    indices: offsets and bytes are exact."""
    import torch
    n = (1 << 32) + 4096
    d = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    tail = letters(4096, 2)
    for a in (0, 15, 30, 500, 502, 998, 1001, 1014, 2000, 4088, 4094):
        tail[a], tail[a + 1] = LIT[0], LIT[1]
    d[-4096:] = torch.from_numpy(tail).to("cuda:0")
    d[-4200:-4096] = ord("a")                                  # (no match of the part nobody filled runs into the tail)
    base = 1 << 32
    rel = [(0, 17), (17, 17), (20, 1000), (1001, 1016), (1016, 4096), (4096, 4096)]
    rb = np.array([0, 100] + [base + b for b, _ in rel], dtype=np.int64)       # rows 0 and 1 lie in the part nobody filled
    re_ = np.array([50, 100] + [base + e for _, e in rel], dtype=np.int64)
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    assert res.counts.cpu().tolist()[2:] == [2, 0, 4, 2, 3, 0]
    rows = [7, 2, 3, 4, 5, 6, 4, 7]
    data = tail.tobytes()
    pieces = [None, None] + [data[b:e].split(LIT) for b, e in rel]
    for repl in (b"", b"0123456789abcdefg"):
        want, w_ob, w_oe = expect(pieces, rows, repl, 0x7C, 17, 1)
        out, ob, oe, behind = replace_poisoned(scan, d, rb_t, re_t, res, repl, len(want), indices=dev(rows), fill=0x7C, lead=17, gap=1)
        assert out.tobytes() == want and ob.tolist() == w_ob.tolist() and oe.tolist() == w_oe.tolist() and (behind == POISON).all()
