"""GPU tests (-m gpu) of rj_scan_records_split (rejit_amd/csrc/record_split.hip; Scan.split_records), of records.field_records /
nonempty_pieces and of samples/linegrep_gpu.py -o / -f.

The meaning: with record r(j) = [rb, re) and its own matches (b_t, e_t) = spans[first[r] + t], t < c = count[r],
    between: row j has c + 1 pieces, piece t = [t == 0 ? rb : e_{t-1}, t == c ? re : b_t)
    matches: row j has c pieces,     piece t = [b_t, e_t)
    piece_first[0] = 0, piece_first[j + 1] = piece_first[j] + (pieces of row j), P = piece_first[k].
The shape tests plant a literal at chosen offsets of a text that holds it nowhere else, so the expected pieces follow from the
planted offsets and the fields are Python's bytes.split of each record's host copy; the end-to-end tests take checkers.Oracle's
spans, handed to the lines by the join rule in numpy.  Outputs are poisoned first: every row of [0, P) and of piece_first[0..k]
is written and nothing behind them."""
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
CHUNK = 512              # record_split.hip's kEmitChunk (pieces)
POISON = -0x5A5A5A5A5A5A5A5B      # 0xA5 in every byte, as int64
LIT = b"@#"              # the planted literal; the texts around it are lower-case letters
BETWEEN, MATCHES = 0, 1
WHATS = ((BETWEEN, "between"), (MATCHES, "matches"))


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


def meaning(rb, re_, own, rows, what):
    """own[r]: record r's own matches [(b, e), ...] -> (pieces as an (P, 2) array, piece_first)"""
    pieces, pf = [], []
    for r in rows:
        pf.append(len(pieces))
        if what == MATCHES:
            pieces += own[r]
        else:
            pos = int(rb[r])
            for b, e in own[r]:
                pieces.append((pos, b))
                pos = e
            pieces.append((pos, int(re_[r])))
    return np.array(pieces, dtype=np.int64).reshape(-1, 2), np.array(pf + [len(pieces)], dtype=np.int64)


def split_poisoned(rj, scan, n, rb_t, re_t, res, what, indices=None, piece_cap=None, want_total=0, room=7, offsets=True):
    """rj_scan_records_split into poisoned tables -> (P, piece_begin, piece_end, piece_first): the whole buffers as numpy"""
    import torch
    lib = rj.load_library()
    k = int(rb_t.numel()) if indices is None else int(indices.numel())
    cap = want_total if piece_cap is None else piece_cap
    pb = torch.full((max(cap, want_total) + room,), POISON, dtype=torch.int64, device="cuda:0")
    pe = torch.full((max(cap, want_total) + room,), POISON, dtype=torch.int64, device="cuda:0")
    pf = torch.full((k + 1 + room,), POISON, dtype=torch.int64, device="cuda:0")
    keep = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = None if indices is None else (indices if k else keep)
    total = lib.rj_scan_records_split(scan._h, n, vp(rb_t), vp(re_t), int(rb_t.numel()), vp(res.counts), vp(res.first),
                                      ctypes.c_void_p(idx.data_ptr()) if idx is not None else None, k, what, vp(pf) if offsets else None,
                                      vp(pb) if cap else None, vp(pe) if cap else None, cap, st)
    return int(total), pb.cpu().numpy(), pe.cpu().numpy(), pf.cpu().numpy()


def check(rj, scan, n, rb_t, re_t, res, rb, re_, own, rows=None):
    """both values of `what`: the raw call into poisoned tables, and Scan.split_records (one size query, exact tables)"""
    k = len(rb) if rows is None else len(rows)
    idx = None if rows is None else dev(rows)
    for what, name in WHATS:
        want, w_pf = meaning(rb, re_, own, range(len(rb)) if rows is None else rows, what)
        P = len(want)
        total, pb, pe, pf = split_poisoned(rj, scan, n, rb_t, re_t, res, what, indices=idx, want_total=P)
        ctx = (len(rb), None if rows is None else len(rows), name)
        assert total == P, (ctx, total, P)
        assert (pf[:k + 1] == w_pf).all() and (pf[k + 1:] == POISON).all(), ctx
        assert (pb[:P] == want[:, 0]).all() and (pe[:P] == want[:, 1]).all(), ctx
        assert (pb[P:] == POISON).all() and (pe[P:] == POISON).all(), ctx
        g_pb, g_pe, g_pf = scan.split_records(rb_t, re_t, res, n, indices=idx, what=name)
        assert g_pb.numel() == P == g_pe.numel() and g_pf.numel() == k + 1
        assert (g_pb.cpu().numpy() == want[:, 0]).all() and (g_pe.cpu().numpy() == want[:, 1]).all() and (g_pf.cpu().numpy() == w_pf).all(), ctx


# ------------------------------------------------------------------------------------------------ shapes
def _planted(k, rng):
    """k records with lengths from {0, 1, 15, 16, 17, 40, 700}, 0..3 bytes of text between them, and 0, 1, 2 or 300 copies of LIT
    planted inside each where they fit: one anywhere; two at the record's first and last bytes; 300 evenly.
    -> (text, rec_begin, rec_end, own: each record's matches)"""
    lens = np.where(rng.rand(k) < 0.04, 700, rng.choice([0, 1, 15, 16, 17, 40], k))
    seams = rng.randint(0, 4, k)
    rb = 5 + np.concatenate([[0], np.cumsum(lens + seams)[:-1]]).astype(np.int64)
    n = int(rb[-1] + lens[-1]) + 9
    t = letters(n, k)
    own = []
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
        own.append([(b + a, b + a + 2) for a in at])
    return t, rb, rb + lens, own


@pytest.mark.parametrize("k", [255, 256, 257, 64 * 256 + 1])
def test_shapes_equal_the_meaning(rj, scan, k):
    """Tables of 255, 256, 257 rows and of more units than one look-back group (the plan has k + 1 rows: 256 fills a unit and
    the closing row opens the next); record lengths 0, 1, 15, 16, 17; 0, 1, 2 and 300 matches in a record; both values of
    `what`, all rows, a permutation and a take with repeats."""
    import torch
    rng = np.random.RandomState(k)
    t, rb, re_, own = _planted(k, rng)
    data, n = t.tobytes(), len(t)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matches == sum(len(o) for o in own) == res.n_kept and res.n_crossing == 0
    # the planted offsets are what bytes.split sees
    fields, _ = meaning(rb, re_, own, range(k), BETWEEN)
    at = 0
    for b, e in zip(rb.tolist()[:2000], re_.tolist()[:2000]):
        parts = data[b:e].split(LIT)
        assert [data[x:y] for x, y in fields[at:at + len(parts)].tolist()] == parts
        at += len(parts)
    check(rj, scan, n, rb_t, re_t, res, rb, re_, own)
    check(rj, scan, n, rb_t, re_t, res, rb, re_, own, rows=rng.permutation(k)[:min(k, 3000)].tolist())
    check(rj, scan, n, rb_t, re_t, res, rb, re_, own, rows=rng.randint(0, k, 300).tolist())


@pytest.mark.parametrize("c", [CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1])
def test_piece_counts_around_the_chunk_size(rj, scan, c):
    """One record with c matches among empty ones: between has c + 1 pieces plus one per empty record, matches c -- totals of one
    less than a chunk of the emit, a chunk, and one more, in both tables."""
    import torch
    t = letters(3 * c + 40, c)
    at = 10 + 3 * np.arange(c)
    t[at], t[at + 1] = LIT[0], LIT[1]
    n = len(t)
    d = torch.from_numpy(t).to("cuda:0")
    for extra in (0, 1):                      # (extra empty records: between gets one piece each, matches none)
        rb = np.array([2] * extra + [8], dtype=np.int64)
        re_ = np.array([2] * extra + [n - 5], dtype=np.int64)
        own = [[]] * extra + [[(int(a), int(a) + 2) for a in at]]
        rb_t, re_t = dev(rb), dev(re_)
        res = scan.run_records(d, rb_t, re_t)
        assert res.n_kept == c
        check(rj, scan, n, rb_t, re_t, res, rb, re_, own)


def test_both_paths_of_the_emit(rj, scan):
    """A chunk stages its rows when fewer than 640 touch it, else every lane searches piece_first in memory.  Staged: 3000 rows
    with 0..2 matches each, in both tables (between gives every row a piece, so a chunk of 512 pieces touches at most 512 rows
    and ALWAYS stages: the constants make the other path unreachable for between).  Not staged: matches over 2000 rows without
    a match in front of one row with 700, 2000 more behind it and a row with one match at the end -- the first chunk's rows run
    from row 0 to the long row, the second chunk's from the long row to the last."""
    import torch
    rng = np.random.RandomState(12)
    t, rb, re_, own = _planted(3000, rng)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    check(rj, scan, len(t), rb_t, re_t, res, rb, re_, own)
    t = letters(2000 * 5 + 2100 + 2000 * 5 + 30, 13)
    long_b = 3 + 2000 * 5
    at = long_b + 3 * np.arange(700)
    last_b = long_b + 2100 + 2000 * 5
    t[at], t[at + 1] = LIT[0], LIT[1]
    t[last_b + 1], t[last_b + 2] = LIT[0], LIT[1]
    rb = np.concatenate([3 + 5 * np.arange(2000), [long_b], long_b + 2100 + 5 * np.arange(2000), [last_b]]).astype(np.int64)
    re_ = np.concatenate([rb[:2000] + 4, [long_b + 2100], rb[2001:4001] + 5, [last_b + 9]]).astype(np.int64)
    own = [[]] * 2000 + [[(int(a), int(a) + 2) for a in at]] + [[]] * 2000 + [[(last_b + 1, last_b + 3)]]
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_kept == 701 and res.n_matching == 2
    check(rj, scan, len(t), rb_t, re_t, res, rb, re_, own)
    check(rj, scan, len(t), rb_t, re_t, res, rb, re_, own, rows=list(range(4001, -1, -1)))


# ------------------------------------------------------------------------------------------------ skew
def test_one_row_with_a_million_matches_and_a_million_rows_with_one(rj, scan):
    """4 MiB with LIT in every block of 4 bytes: as ONE record among 50 000 empty ones, and as 2^20 records of 4 bytes.  Both
    give the piece tables of the meaning, written out with torch ops on the device; neither loops over a row's matches or over
    a run of rows without one (each would take minutes, not milliseconds)."""
    import torch
    big = 4 << 20
    blocks = big // 4
    g = torch.Generator(device="cuda:0").manual_seed(9)
    d = torch.randint(ord("a"), ord("z") + 1, (big + 16,), dtype=torch.uint8, device="cuda:0", generator=g)
    body = d[8:8 + big].view(blocks, 4)
    body[:, 1], body[:, 2] = LIT[0], LIT[1]
    n = int(d.numel())
    mb = 8 + 4 * torch.arange(blocks, device="cuda:0") + 1            # the matches' begins
    # one record
    rb = np.concatenate([np.full(25000, 2), [8], np.full(25000, big + 12)]).astype(np.int64)
    re_ = rb.copy()
    re_[25000] = 8 + big
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matches == blocks == res.n_kept and res.n_matching == 1
    pb, pe, pf = scan.split_records(rb_t, re_t, res, n, what="matches")
    assert torch.equal(pb, mb) and torch.equal(pe, mb + 2)
    assert torch.equal(pf, torch.cat([torch.zeros(25001, dtype=torch.int64), torch.full((25001,), blocks, dtype=torch.int64)]).to("cuda:0"))
    pb, pe, pf = scan.split_records(rb_t, re_t, res, n, what="between")
    assert pb.numel() == blocks + 1 + 50000
    row = slice(25000, 25000 + blocks + 1)
    assert torch.equal(pb[row], torch.cat([dev([8]), mb + 2])) and torch.equal(pe[row], torch.cat([mb, dev([8 + big])]))
    assert bool((pb[:25000] == 2).all()) and bool((pe[:25000] == 2).all()) and bool((pb[25001 + blocks:] == big + 12).all())
    ar = torch.arange(25001, device="cuda:0")
    assert torch.equal(pf, torch.cat([ar, 25001 + blocks + ar]))
    # a record per block
    rb_t = torch.arange(8, 8 + big, 4, device="cuda:0")
    re_t = rb_t + 4
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_matching == blocks and res.n_crossing == 0
    pb, pe, pf = scan.split_records(rb_t, re_t, res, n, what="matches")
    assert torch.equal(pb, mb) and torch.equal(pe, mb + 2) and torch.equal(pf, torch.arange(blocks + 1, device="cuda:0"))
    pb, pe, pf = scan.split_records(rb_t, re_t, res, n, what="between")
    assert torch.equal(pb.view(blocks, 2), torch.stack([rb_t, mb + 2], dim=1)) and torch.equal(pe.view(blocks, 2), torch.stack([mb, re_t], dim=1))
    assert torch.equal(pf, 2 * torch.arange(blocks + 1, device="cuda:0"))


# ------------------------------------------------------------------------------------------------ end to end
def _oracle_spans(oracle, rx, data):
    cap = len(data) + 2
    buf = np.empty(2 * cap, dtype=np.uint64)
    m = oracle.lib.ro_match_all_re(rx, data, len(data), buf.ctypes.data_as(_u64p), cap)
    assert 0 <= m <= cap, (rx, m)
    return buf[:2 * m].astype(np.int64).reshape(m, 2)


def _join(rb, re_, spans):
    """the join rule in numpy -> (first, count)"""
    begins = spans[:, 0]
    key = np.minimum(re_ + 1, np.concatenate([rb[1:], [np.iinfo(np.int64).max]]))
    first = np.searchsorted(begins, rb, side="left")
    count = np.maximum(np.searchsorted(begins, key, side="left") - first, 0)
    return first, count


def _own(spans, first, count):
    sp = spans.tolist()
    return [[tuple(x) for x in sp[f:f + c]] for f, c in zip(first.tolist(), count.tolist())]


@pytest.fixture(scope="module")
def log_lines(rj):
    """256 KiB of log-like text with commas and tabs planted, cut into its lines -> (data, d, rb_t, re_t, rb, re_)"""
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    t = W.log_like_numpy(1 << 18, 41)
    rng = np.random.RandomState(4)
    spots = rng.choice(len(t), 6000, replace=False)
    spots = spots[(t[spots] != 10) & (t[spots] != 13)]
    t[spots[:4000]] = ord(",")
    t[spots[4000:]] = 9
    t[-1] = ord("z")
    t[1000:1003] = 10                        # empty lines
    data = t.tobytes()
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = R.line_records(d)
    rb, re_ = rb_t.cpu().numpy(), re_t.cpu().numpy()
    assert 2000 < len(rb) == len(re.split(b"[\n\r]", data))
    return data, d, rb_t, re_t, rb, re_


@pytest.mark.parametrize("rx", [b"[ \t]+", b",", b"[0-9]+", b"x*", b"QQQQ"])
def test_fields_and_matches_of_lines_against_the_oracle(rj, oracle, log_lines, rx):
    """checkers.Oracle's spans, handed to the lines by the join rule in numpy: the fields and the matches of every line, and of
    the lines select_records lists, equal split_records'; field 2 of every line (records.field_records), packed, equals the
    Python list byte for byte.  `x*` matches the empty string everywhere; QQQQ matches nowhere."""
    import torch
    from rejit_amd import records as R
    data, d, rb_t, re_t, rb, re_ = log_lines
    n = len(data)
    spans = _oracle_spans(oracle, rx, data)
    first, count = _join(rb, re_, spans)
    assert int(count.sum()) == len(spans), rx          # the reference alone: every match is some line's
    own = _own(spans, first, count)
    s = rj.Scan(rj.Program(rx))
    res = s.run_records(d, rb_t, re_t)
    assert res.n_crossing == 0 and (s.spans_tensor(d.device).cpu().numpy() == spans).all()
    check(rj, s, n, rb_t, re_t, res, rb, re_, own)
    if rx != b"QQQQ":
        sel = s.select_records()
        check(rj, s, n, rb_t, re_t, res, rb, re_, own, rows=sel.cpu().tolist())
    else:
        assert len(spans) == 0
    # field 2 (the third) of every line; negative: the last field
    pb, pe, pf = s.split_records(rb_t, re_t, res, n)
    fields, w_pf = meaning(rb, re_, own, range(len(rb)), BETWEEN)
    for f in (2, -1, 0):
        fb, fe, present = R.field_records(pb, pe, pf, f)
        packed, _, _ = s.pack_records(d, fb, fe, fill=10, lead=0, gap=1)
        want, has = [], []
        for j in range(len(rb)):
            row = fields[w_pf[j]:w_pf[j + 1]].tolist()
            ok = -len(row) <= f < len(row)
            has.append(ok)
            want.append(data[row[f][0]:row[f][1]] if ok else b"")
        assert present.cpu().tolist() == has, (rx, f)
        assert packed.cpu().numpy().tobytes() == b"".join(w + b"\n" for w in want), (rx, f)
        absent = ~present
        if bool(absent.any()):                         # the empty record at the row's last piece's end
            assert torch.equal(fb[absent], fe[absent]) and torch.equal(fb[absent], pe[pf[1:][absent] - 1])
    keep = R.nonempty_pieces(pb, pe)
    assert keep.cpu().tolist() == [i for i, (b, e) in enumerate(fields.tolist()) if e > b]


def test_the_field_table_is_a_record_table_and_joins_to_the_replace(rj, oracle, log_lines):
    """The between table of all lines is ascending and not overlapping: run_records of a second pattern accepts it and counts
    that pattern per FIELD as numpy's join over the same table does; and repl.join(a row's fields) is what replace_records
    writes for the same rows."""
    import torch
    data, d, rb_t, re_t, rb, re_ = log_lines
    n = len(data)
    s = rj.Scan(rj.Program(b"[ \t]+"))
    res = s.run_records(d, rb_t, re_t)
    pb, pe, pf = s.split_records(rb_t, re_t, res, n)
    fb, fe = pb.cpu().numpy(), pe.cpu().numpy()
    assert (fb <= fe).all() and (fe[:-1] <= fb[1:]).all()
    second = rj.Scan(rj.Program(b"[a-z]+"))
    per_field = second.run_records(d, pb, pe)
    spans2 = _oracle_spans(oracle, b"[a-z]+", data)
    _, count2 = _join(fb, fe, spans2)
    assert (per_field.counts.cpu().numpy() == count2).all() and per_field.n_kept == int(count2.sum()) > 1000
    # the join against the replace: all rows, and a take
    w_pf = pf.cpu().numpy()
    for rows in (None, [5, 5, 1000, 7, len(rb) - 1]):
        idx = None if rows is None else dev(rows)
        qb, qe, qf = s.split_records(rb_t, re_t, res, n, indices=idx)
        qb, qe, qf = qb.cpu().tolist(), qe.cpu().tolist(), qf.cpu().tolist()
        for repl in (b"", b"<sep>"):
            out, ob, oe = s.replace_records(d, rb_t, re_t, res, repl, indices=idx, fill=10, lead=0, gap=1)
            got = out.cpu().numpy().tobytes()
            want = b"".join(repl.join(data[qb[p]:qe[p]] for p in range(qf[j], qf[j + 1])) + b"\n" for j in range(len(qf) - 1))
            assert got == want, (rows, repl)
    assert w_pf[-1] == len(fb)


# ------------------------------------------------------------------------------------------------ capacity
def test_size_query_piece_cap_and_no_rows(rj, scan):
    import torch
    rng = np.random.RandomState(5)
    t, rb, re_, own = _planted(300, rng)
    n = len(t)
    d = torch.from_numpy(t).to("cuda:0")
    rb_t, re_t = dev(rb), dev(re_)
    res = scan.run_records(d, rb_t, re_t)
    dense = next(r for r in range(300) if len(own[r]) == 300)
    for what, _ in WHATS:
        want, w_pf = meaning(rb, re_, own, range(300), what)
        P = len(want)
        # the size query: no piece row, the offsets still written; and without the offsets
        total, pb, pe, pf = split_poisoned(rj, scan, n, rb_t, re_t, res, what, piece_cap=0)
        assert total == P and (pb == POISON).all() and (pe == POISON).all() and (pf[:301] == w_pf).all() and (pf[301:] == POISON).all()
        total, _, _, pf = split_poisoned(rj, scan, n, rb_t, re_t, res, what, piece_cap=0, offsets=False)
        assert total == P and (pf == POISON).all()
        # piece_cap inside a row, at a row's boundary, one piece, everything, more than everything; the scan's own offsets
        for cap in (int(w_pf[dense]) + 150, int(w_pf[dense]), int(w_pf[dense + 1]), 1, P - 1, P, P + 40):
            total, pb, pe, pf = split_poisoned(rj, scan, n, rb_t, re_t, res, what, piece_cap=cap, want_total=P, offsets=cap % 2 == 0)
            lim = min(cap, P)
            assert total == P, (what, cap)
            assert (pb[:lim] == want[:lim, 0]).all() and (pe[:lim] == want[:lim, 1]).all(), (what, cap)
            assert (pb[lim:] == POISON).all() and (pe[lim:] == POISON).all(), (what, cap)
        # no rows: an empty selection is not "every record"; piece_first[0] = 0 is written
        total, pb, pe, pf = split_poisoned(rj, scan, n, rb_t, re_t, res, what, indices=dev([]), piece_cap=5)
        assert total == 0 and (pb == POISON).all() and (pe == POISON).all() and pf[0] == 0 and (pf[1:] == POISON).all()
        g_pb, g_pe, g_pf = scan.split_records(rb_t, re_t, res, n, indices=dev([]), what="between" if what == BETWEEN else "matches")
        assert g_pb.numel() == 0 and g_pe.numel() == 0 and g_pf.cpu().tolist() == [0]
    empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
    res0 = scan.run_records(d, empty, empty)
    pb, pe, pf = scan.split_records(empty, empty, res0, n)
    assert pb.numel() == 0 and pe.numel() == 0 and pf.cpu().tolist() == [0]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_the_scans_state_stays(rj):
    import torch
    from rejit_amd import records as R
    from rejit_amd import workloads as W
    lib = rj.load_library()
    t = W.log_like_numpy(1 << 17, 3)
    t[100:108] = np.frombuffer(b"agggtaaa", dtype=np.uint8)
    n = len(t)
    d = torch.from_numpy(t).to("cuda:0")
    scan = rj.Scan(rj.Program(b"[0-9]+"))
    rb_t, re_t = R.line_records(d)                         # lines: `[0-9]+` crosses none
    rb, re_ = rb_t.cpu().numpy(), re_t.cpu().numpy()
    k = len(rb)
    res = scan.run_records(d, rb_t, re_t)
    assert res.n_crossing == 0 and res.n_matching > 20 and k > 100
    sel0 = scan.select_records().clone()
    spans0 = scan.spans_tensor(d.device).clone()
    stats0 = scan.stats()
    own = _own(spans0.cpu().numpy(), res.first.cpu().numpy(), res.counts.cpu().numpy())
    P = k + len(spans0)

    def good():
        check(rj, scan, n, rb_t, re_t, res, rb, re_, own, rows=list(range(0, k, 3)))

    def refused(why, row, word, b_t=rb_t, e_t=re_t, r=res, idx=None, s=scan):
        for what, name in WHATS:
            total, pb, pe, _ = split_poisoned(rj, s, n, b_t, e_t, r, what, indices=idx, piece_cap=P + 10)
            msg = lib.rj_last_error().decode()
            assert total == RJ_BAD_ARGUMENT, (why, name, total)
            assert (row is None or ("row %d " % row) in msg) and word in msg, (why, name, msg)
            assert word != "independent" or "rj_scan_records_pack" in msg      # the message about independent records names the pack
            assert (pb == POISON).all() and (pe == POISON).all(), (why, name)
            with pytest.raises(rj.RejitError) as err:
                s.split_records(b_t, e_t, r, n, indices=idx, what=name)
            assert err.value.status == RJ_BAD_ARGUMENT and word in err.value.message
        if s is scan:
            good()                                         # the same scan answers a good call afterwards

    # a bad index, a bad row
    refused("an index == n_records", 2, "names no record", idx=dev([5, 0, k, 1]))
    refused("a negative index", 1, "names no record", idx=dev([5, -1, k, 1]))
    e = re_.copy()
    e[k // 2] = int(rb[k // 2]) - 1
    refused("end < begin", k // 2, "names no record", e_t=dev(e))
    e = re_.copy()
    e[k - 1] = n + 1
    refused("end > n", k - 1, "outside the text", e_t=dev(e))
    # a saturated count; first + count > m
    has = np.nonzero(res.counts.cpu().numpy() > 0)[0]
    row = int(has[5])
    c = res.counts.clone()
    c[row] = -1
    refused("a saturated count", row, "saturated", r=rj.api.RecordsResult(rj.api._RecordStats(), c, res.first, k))
    c = res.counts.clone()
    c[row] = len(spans0) - int(res.first[row]) + 1
    refused("first + count > m", row, "beyond the scan's list", r=rj.api.RecordsResult(rj.api._RecordStats(), c, res.first, k))
    # a record cut short under its last match; one that begins behind its first match
    last = int(res.first[row]) + int(res.counts[row]) - 1
    e = re_.copy()
    e[row] = int(spans0[last, 1]) - 1
    refused("the last match ends beyond the record", row, "independent", e_t=dev(e))
    b = rb.copy()
    b[row] = int(spans0[int(res.first[row]), 0]) + 1
    refused("the first match begins before the record", row, "begins before", b_t=dev(b))
    # two bad rows: the first is named
    e = re_.copy()
    e[row] = int(spans0[last, 1]) - 1
    e[int(has[2])] = n + 5
    refused("two bad rows", int(has[2]), "outside the text", e_t=dev(e))
    # a stale result: that of a run of another pattern (many more matches: first + count leaves this scan's list)
    other = rj.Scan(rj.Program(b"[a-z]"))
    stale = other.run_records(d, rb_t, re_t)
    assert stale.n_matches > 4 * res.n_matches
    refused("a stale result", None, "row ", r=stale)
    # a counts-only last run: there is no list
    dna = rj.Scan(rj.Program(b"agggtaaa|tttaccct"))
    dna_res = dna.run_records(d, rb_t, re_t)
    assert dna.count_tensor(d) == dna_res.n_matches >= 1 and dna.stats()["count_path"] == 1
    refused("a counts-only last run", None, "counts-only", r=dna_res, s=dna)
    dna_res = dna.run_records(d, rb_t, re_t)               # usable afterwards
    row100 = int(np.searchsorted(rb, 100, side="right")) - 1
    pb, pe, pf = dna.split_records(rb_t, re_t, dna_res, n, indices=dev([row100]), what="matches")
    assert pb.cpu().tolist() == [100] and pe.cpu().tolist() == [108] and pf.cpu().tolist() == [0, 1]
    # arguments
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    f = lib.rj_scan_records_split
    out = torch.full((P + 10,), POISON, dtype=torch.int64, device="cuda:0")
    out2 = out.clone()
    assert f(scan._h, n, vp(rb_t), vp(re_t), k, None, vp(res.first), None, 0, 0, None, None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, n, vp(rb_t), vp(re_t), k, vp(res.counts), None, None, 0, 0, None, None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, n, None, None, 3, None, None, None, 0, 0, None, None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(None, n, None, None, 0, None, None, None, 0, 0, None, None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), None, 0, 0, None, vp(out), None, 5, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), None, 0, 0, None, None, vp(out), 5, st) == RJ_BAD_ARGUMENT
    for what in (2, -1):
        assert f(scan._h, n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), None, 0, what, None, vp(out), vp(out2), P, st) == RJ_BAD_ARGUMENT
        assert "what" in lib.rj_last_error().decode()
    assert f(scan._h, n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), None, 0, 0, None, ctypes.c_void_p(out.data_ptr() + 4), vp(out2), P,
             st) == RJ_BAD_ARGUMENT
    assert "aligned" in lib.rj_last_error().decode()
    assert f(scan._h, n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), vp(rb_t), 1 << 60, 0, None, None, None, 0, st) == RJ_BAD_ARGUMENT
    assert f(scan._h, n, vp(rb_t), vp(re_t), k, vp(res.counts), vp(res.first), vp(rb_t), 1 << 59, 0, None, None, None, 0, st) == RJ_BAD_ARGUMENT
    assert "2^62" in lib.rj_last_error().decode()
    assert f(scan._h, n, None, None, 0, None, None, None, 0, 1, None, None, None, 0, st) == 0
    assert bool((out == POISON).all()) and bool((out2 == POISON).all())
    with pytest.raises(ValueError):
        scan.split_records(rb_t, re_t, res, n, what="fields")
    # the scan's state stays: its list, its stats and its last join are what they were, and the call itself works
    good()
    assert torch.equal(scan.spans_tensor(d.device), spans0) and torch.equal(scan.select_records(), sel0) and scan.stats() == stats0
    assert scan.run_records(d, rb_t, re_t).n_kept == res.n_kept


# ------------------------------------------------------------------------------------------------ samples/linegrep_gpu.py -o / -f
@pytest.fixture(scope="module")
def sample_files(tmp_path_factory):
    """5000 lines, once without a line break behind the last line and once with one -> (lines, {terminated: path})"""
    rng = random.Random(46)
    words = [b"int", b"regexp", b"return", b"for (;;)", b"x = y + 1;", b"key: value", b"a,b,,c", b"regexps", b"char*\ts", b"", b"}", b"error: 42", b"k:v"]
    lines = [b" ".join(rng.choice(words) for _ in range(rng.randint(0, 6))) for _ in range(4999)] + [b"the end: of, the file"]
    paths = {}
    for terminated in (False, True):
        paths[terminated] = str(tmp_path_factory.mktemp("linegrep") / "file.txt")
        with open(paths[terminated], "wb") as fh:
            fh.write(b"\n".join(lines) + (b"\n" if terminated else b""))
    return lines, paths


def _field(pattern, ln, f):
    return (re.split(pattern.encode(), ln) + [b""] * f)[f - 1]


# (options, pattern, the file ends in a line break, the lines grep selects, what is printed per selected line, the exit status)
SAMPLE_CASES = [
    (["-o"], "regexps|return", True, None, lambda p, ln: re.findall(p.encode(), ln), 0),
    (["-o"], "[a-z]+", False, None, lambda p, ln: re.findall(p.encode(), ln), 0),
    (["-p", "-o"], "[0-9]+", True, [], lambda p, ln: re.findall(p.encode(), ln), 0),
    (["-v", "-f", "2"], ",", True, ["-v"], lambda p, ln: [_field(p, ln, 2)], 0),
    (["-p", "-f", "2"], ": *", False, [], lambda p, ln: [_field(p, ln, 2)], 0),
    (["-f", "1"], "[ \t]+", True, None, lambda p, ln: [_field(p, ln, 1)], 0),
    (["-f", "3"], ",", False, None, lambda p, ln: [_field(p, ln, 3)], 0),
    (["-f", "9"], ": *", True, None, lambda p, ln: [_field(p, ln, 9)], 0),          # more fields than any line has: empty lines
    (["-o"], "QQQQ", True, [], lambda p, ln: [], 1),                                 # nothing selected: 1, nothing printed
    (["-p", "-f", "1"], "QQQQ", True, [], lambda p, ln: [], 1),
    (["-f", "1"], "QQQQ", False, None, lambda p, ln: [ln], 0),                       # every line is printed whatever matches
]


@pytest.mark.parametrize("opts,pattern,terminated,grep_opts,printed,status", SAMPLE_CASES,
                         ids=[" ".join(c[0] + [c[1]]) + ("" if c[2] else " (no last line break)") for c in SAMPLE_CASES])
def test_linegrep_sample_prints_matches_like_grep_o_and_fields_like_awk(rj, sample_files, opts, pattern, terminated, grep_opts, printed, status):
    """-o against `grep -E -o`; -f N against Python's re.split per line (separators for which leftmost-longest and Python's
    leftmost-first agree, none of which matches the empty string or a line break); with -p / -v over the lines grep selects."""
    lines, paths = sample_files
    path = paths[terminated]
    sample = os.path.join(ROOT, "samples", "linegrep_gpu.py")
    r = subprocess.run([sys.executable, sample, path, pattern] + opts, capture_output=True, timeout=300)
    assert r.returncode == status, (r.returncode, r.stderr.decode()[-500:])
    chosen = lines
    if grep_opts is not None:
        inverted = grep_opts == ["-v"]
        chosen = [ln for ln in lines if (re.search(pattern.encode(), ln) is None) == inverted]
    grep = shutil.which("grep")
    if grep and grep_opts is not None:
        g = subprocess.run([grep, "-E"] + grep_opts + [pattern, path], capture_output=True, timeout=120)
        assert g.stdout == b"".join(ln + b"\n" for ln in chosen)
    want = b"".join(x + b"\n" for ln in chosen for x in printed(pattern, ln))
    assert r.stdout == want
    assert status == 1 or len(want) > 1000
    if grep and opts[-1] == "-o":
        g = subprocess.run([grep, "-E", "-o", pattern, path], capture_output=True, timeout=120)
        assert g.returncode == status and r.stdout == g.stdout


def test_linegrep_sample_refuses_a_field_number_below_one(sample_files):
    _, paths = sample_files
    r = subprocess.run([sys.executable, os.path.join(ROOT, "samples", "linegrep_gpu.py"), paths[True], ",", "-f", "0"], capture_output=True, timeout=60)
    assert r.returncode == 2 and r.stdout == b""
