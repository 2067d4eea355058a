"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against

* every golden vector (the reference's own test.cc cases incl. the 33-alignment sweeps,
  hand-picked semantics probes, 2500 random regex/text pairs) -- bit-exact offsets;
* the oracle on seeded inputs at sizes it finishes in seconds;
* size-independent properties at larger sizes (planted-literal recovery, shard + carry
  composition == single run, idempotence of the sink).
"""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from checkers import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rj():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rejit_amd
    rejit_amd.build()
    lib = rejit_amd.load_library()
    assert rejit_amd.device_count() >= 1
    return rejit_amd


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


_programs = {}


def prog(rj, rx: bytes):
    p = _programs.get(rx)
    if p is None:
        if len(_programs) > 64:
            _programs.clear()
        p = _programs[rx] = rj.Program(rx)
    return p


def test_golden_vectors(rj, oracle):
    """Bit-exact with the real reference (use_fast_forward=0) on every golden vector --
    including the 19 random vectors that exercise the reference's ring artefact Q8, which
    the engine reproduces through its one-lane exact kernel."""
    n = 0
    for rx, tx, exp_all, exp_full in V.all_matchall_cases():
        p = prog(rj, rx)
        got = p.match_all(tx)
        assert got == exp_all, (rx, tx, got, exp_all)
        assert p.count(tx) == len(got)
        assert p.match_full(tx) == bool(exp_full), (rx, tx)
        n += 1
    assert n > 2500


def test_high_byte_vectors(rj):
    """The HIP path on bytes >= 0x80 (half the byte range was unpinned): the 1900 high-byte vectors with the
    real reference's outputs -- signed bracket ranges around 0x7f / 0x80, `.` / \\S / \\D / negated classes over Latin-1
    and UTF-8 text, literal windows of high bytes (nibble filter, 2-bit codes: they alias ASCII bytes there), texts of up
    to 5000 bytes so that the window and dense scans run, not only the small-text kernel."""
    n = high = 0
    for rx, tx, exp_all, exp_full in V.highbyte_cases():
        p = prog(rj, rx)
        got = p.match_all(tx)
        assert got == exp_all, (rx, tx[:80], got[:5])
        assert p.match_full(tx) == bool(exp_full), (rx, tx[:80])
        high += any(c >= 0x80 for c in rx + tx)
        n += 1
    assert n >= 1800 and high >= 400


def test_high_byte_vectors_device_text(rj):
    """The same vectors through the device-text entry points with the small-text kernel OFF (texts >= 200 bytes): the
    general pipeline -- window scans with the nibble filter, dense kernels, verify tails -- on high bytes."""
    import torch
    n = 0
    for rx, tx, exp_all, exp_full in V.highbyte_cases():
        if len(tx) < 200:
            continue
        sc = rj.Scan(prog(rj, rx))
        t = torch.frombuffer(bytearray(tx), dtype=torch.uint8).cuda()
        k = sc.run_tensor(t)
        got = sc.spans()
        assert got == exp_all and k == len(got), (rx, tx[:60], got[:5])
        n += 1
    assert n >= 400


def test_ring_artefact_vectors(rj):
    """The engine against the REAL reference's outputs where its ring artefact applies (263 of these 840 vectors
    differ from the documented semantics): host-text calls, i.e. the small-text kernel handing over to the
    general pipeline and the exact replay."""
    n = 0
    for rx, tx, exp_all, exp_full in V.artefact_cases():
        p = prog(rj, rx)
        assert p.match_all(tx) == exp_all, (rx, tx)
        assert p.match_full(tx) == bool(exp_full), (rx, tx)
        n += 1
    assert n >= 800


def test_fresh_random_vs_oracle(rj, oracle):
    """Seeds that are NOT in the committed fixtures, longer texts (more adjacent matches):
    the GPU result must equal the strict restatement of the reference bit for bit."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import RegexGen, ALPHABETS, ALPHABETS_HI
    rng = random.Random(4242)
    checked = exact = 0
    for it in range(2100):
        alphabet = rng.choice(ALPHABETS if it < 1500 else [a.replace("\x00", "") for a in ALPHABETS_HI])   # (then: bytes >= 0x80)
        rx = RegexGen(rng, alphabet).alt(2).encode("latin1")
        text = "".join(rng.choice(alphabet) for _ in range(rng.choice([5, 40, 150, 400]))).encode("latin1")
        want = oracle.match_all(rx, text)
        if isinstance(want, int):
            continue
        got = prog(rj, rx).match_all(text)
        assert got == want, (rx, text)
        exact += want != oracle.match_all_spec(rx, text)
        checked += 1
    assert checked > 2000
    assert exact > 0   # the artefact does occur in this sample, and is reproduced


def test_fresh_random_multi_chunk_vs_oracle(rj, oracle):
    """The same generator over texts of several 1-KiB chunks, so that the full-chunk fast paths
    (register pre-steps, pipelined scan loop, halos, wave edges, walker refill) are compared with
    the oracle on arbitrary patterns, not only the guarded tail chunk.  (tools/fuzz_large.py runs
    thousands of these; a lost pair of matches at every chunk edge was found that way.)"""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import RegexGen, ALPHABETS, ALPHABETS_HI
    rng = random.Random(90125)
    checked = 0
    for it in range(800):
        alphabet = rng.choice(ALPHABETS if it < 500 else [a.replace("\x00", "") for a in ALPHABETS_HI])   # (then: bytes >= 0x80)
        rx = RegexGen(rng, alphabet).alt(2).encode("latin1")
        n = rng.choice([1500, 2047, 2048, 2053, 3100, 4096, 5000])
        text = "".join(rng.choice(alphabet) for _ in range(n)).encode("latin1")
        want = oracle.match_all(rx, text)
        if isinstance(want, int):
            continue
        assert prog(rj, rx).match_all(text) == want, (rx, n)
        checked += 1
    assert checked > 720


def test_testcc_expectations(rj):
    """The expectations written in the reference's test.cc, for every match type."""
    for v in V.testcc():
        rx, tx = V.b(v["regex"]), V.b(v["text"])
        p = prog(rj, rx)
        if v["macro"] == "TEST":
            if v["match_type"] == "kMatchAll":
                assert p.count(tx) == v["expected"], v
            else:
                assert (p.match_first(tx) is not None) == bool(v["expected"]), v
        elif v["macro"] == "TEST_Full":
            assert p.match_full(tx) == bool(v["expected_full"]), v
            if v["expected_full"]:
                assert p.match_first(tx) is not None and p.count(tx) == 1, v
        else:
            assert p.count(tx) == v["expected_count"], v
            assert p.match_anywhere(tx) == bool(v["expected_count"]), v
            first = p.match_first(tx)
            if v["expected_count"]:
                assert list(first) == v["expected_first"], v
            else:
                assert first is None, v


def test_parse_errors(rj):
    for e in V.semantics()["errors"]:
        with pytest.raises(rj.RejitError):
            rj.Program(V.b(e["regex"]))


def _digest(ms):
    h = hashlib.sha256()
    for b_, e_ in ms:
        h.update(int(b_).to_bytes(8, "little"))
        h.update(int(e_).to_bytes(8, "little"))
    return h.hexdigest()


def test_bench_regexes(rj):
    from rejit_amd import workloads as W
    for v in V.bench()["bench"]:
        text = W.random_ascii_numpy(v["n"], v["seed"], ord(v["low"]), ord(v["high"]))
        for k, o in enumerate(v["plant_offsets"]):
            pl = V.b(v["plants"][k % len(v["plants"])])
            text[o:o + len(pl)] = np.frombuffer(pl, dtype=np.uint8)
        assert prog(rj, V.b(v["regex"])).match_all(text.tobytes()) == V.tup(v["ref_all"]), v["regex"]


@pytest.mark.parametrize("nf", [1000, 50000])
def test_regexdna(rj, nf):
    from rejit_amd import workloads as W
    g = V.bench()["regexdna"][str(nf)]
    raw = W.fasta_raw_numpy(nf).tobytes()
    stripped = W.fasta_stripped_numpy(nf).tobytes()
    strip = prog(rj, V.b(g["strip"]["regex"])).match_all(raw)
    assert len(strip) == g["strip"]["count"] and _digest(strip) == g["strip"]["digest"]
    for p in g["patterns"]:
        ms = prog(rj, V.b(p["regex"])).match_all(stripped)
        assert len(ms) == p["count"] and _digest(ms) == p["digest"], p["regex"]


def test_fasta_device_generator(rj):
    import torch
    from rejit_amd import workloads as W
    a = W.fasta_stripped_numpy(3000)
    b_ = W.fasta_stripped_torch(3000, torch.device("cuda:0"), chunk=4096).cpu().numpy()
    assert (a == b_).all()
    x = W.random_ascii_numpy(100000, 5, start=12345)
    y = W.random_ascii_torch(100000, 5, torch.device("cuda:0"), start=12345, chunk=30000).cpu().numpy()
    assert (x == y).all()


@pytest.mark.parametrize("n", [0, 1, 5, 6, 7, 15, 16, 17, 1023, 1024, 1025, 1030, 2048, 4099, 70000, (1 << 20) + 3])
def test_literal_scan_sizes(rj, oracle, n):
    """Every tail / chunk-edge shape of the fast-forward scan vs the oracle."""
    from rejit_amd import workloads as W
    t = W.random_ascii_numpy(n, seed=n + 1) if n else np.zeros(0, dtype=np.uint8)
    if n >= 6:
        offs = W.plant_offsets(n, 6, min(30, max(1, n // 12)), seed=n, boundaries=[16, 1024, 2048, 65536])
        W.plant(t, offs, b"regexp")
    tb = t.tobytes()
    assert prog(rj, b"regexp").match_all(tb) == oracle.match_all(b"regexp", tb)


def test_dense_and_unbounded_vs_oracle(rj, oracle):
    rng = random.Random(5)
    cases = [b"x*", b"a+", b"[ab]+c", b"^", b"$", b"^a|b$", b"(ab)*c", b".*b", b"a.*", b"(a|b)+", b"\\d+",
             b"[^a]+", b"a{2,4}", b"(ab|ba){2,}", b">.*\n|\n"]
    for rx in cases:
        for n in (0, 1, 17, 200, 3000, 70000):
            text = bytes(rng.choice(b"ab\nc>1x") for _ in range(n))
            want = oracle.match_all(rx, text)
            got = prog(rj, rx).match_all(text)
            assert got == want, (rx, n)


def test_dense_walk_kernel_shapes(rj, oracle):
    """The fused dense kernel: 1, 2 and 4 state words, with and without assertions, region overflow
    (every position matches), starts decided by the register pre-steps vs walked, chunk and wave
    edges (texts of a few chunks so that the last lane's positions and the tail chunk are hit)."""
    rng = random.Random(11)
    A, B = b"abcdefgh", b"ijklmnop"
    cases = [
        (b"[a-h][i-p]", A + B),                      # 1 word, everything decided by the pre-steps
        (b"[a-h]+[i-p]", A + B),                     # loops: long walks
        (b"[a-h][i-p]?[a-h]", A + B),                # skip positions
        (b"([a-h][i-p]){17}", A + B),                # 34 positions: 2 words
        (b"[a-h]{70}", A + b"i"),                    # 70 positions: 4 words (3 used)
        (b"^[a-h]+$", A + b"\n"),                    # assertions: context tables
        (b"[a-h]+$", A + b"q\n"),
        (b"[a-p]", A + B),                           # every position matches: regions overflow and grow
        (b"[a-p]+", A + B + b"z"),
        (b"([a-h]|[i-p][i-p])+[a-h]", A + B),        # general follow rows
        (b"[a-h][ ]?", A),                           # every start decided by the pre-steps except the wave's last two
        (b"[^ ]{1,2}", A),
    ]
    n_dense = 0
    for rx, alphabet in cases:
        n_dense += prog(rj, rx).info()["scan_mode"] == 0
        for n in (1, 15, 16, 17, 1023, 1024, 1025, 1027, 1028, 2049, 5000, 70001, 300000):
            text = bytes(rng.choice(alphabet) for _ in range(n))
            want = oracle.match_all(rx, text)
            got = prog(rj, rx).match_all(text)
            assert got == want, (rx, n)
    assert n_dense >= 8, "these patterns are meant to run in dense mode"


def test_match_first_and_anywhere_early_exit(rj, oracle):
    """kMatchFirst / kMatchAnywhere look at growing prefixes of the start positions and upload only
    what those can reach: same answers as MatchAll[0] wherever the first match lies (block edges at
    256 KiB and 2 MiB + 256 KiB, bounded and unbounded patterns, `$` at a false text end)."""
    import time
    from rejit_amd import workloads as W
    n = 6 << 20
    base = W.random_ascii_numpy(n, seed=77)
    for rx, needle in ((b"regexp", b"regexp"), (b"reg+exp$", b"reggggexp\n"), (b"re[a-g]+xp|abc$", b"regexp"),
                       (b"q[0-9]*regexp", b"q123regexp")):
        p = prog(rj, rx)
        for where in (None, 0, 100, (256 << 10) - 3, (256 << 10), (256 << 10) + 1, (2 << 20) + (256 << 10) - 2, n - len(needle)):
            t = base.copy()
            if where is not None:
                W.plant(t, [where], needle)
            tb = t.tobytes()
            all_ = p.match_all(tb)
            first = p.match_first(tb)
            assert first == (all_[0] if all_ else None), (rx, where)
            assert p.match_anywhere(tb) == bool(all_), (rx, where)
    # an early hit must not pay for the whole buffer
    t = base.copy()
    W.plant(t, [1000], b"regexp")
    tb = t.tobytes()
    p = prog(rj, b"regexp")
    p.match_first(tb)
    early, full = [], []
    for _ in range(5):   # (wall clock on a shared host: the best of five each -- one descheduled call failed this once in ten suite runs)
        t0 = time.perf_counter(); p.match_first(tb); early.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); p.match_all(tb); full.append(time.perf_counter() - t0)
    assert min(early) < min(full) / 2, (early, full)
    # small texts vs the oracle (all block logic collapses to one run)
    rng = random.Random(3)
    for rx in (b"a+b", b"^b", b"b$", b"x*", b"(ab|ba)+"):
        for _ in range(20):
            text = bytes(rng.choice(b"ab\n") for _ in range(rng.randrange(0, 40)))
            want = oracle.match_all(rx, text)
            assert prog(rj, rx).match_first(text) == (want[0] if want else None), (rx, text)


def test_match_all_batch_vs_per_text_oracle(rj, oracle):
    """rj_match_all_batch (many files, one device pass) == the oracle run on every text alone:
    empty texts, texts ending in a match, empty matches at text ends, ^ / $ at text boundaries,
    patterns that can consume a newline (other separator or the text-by-text fallback)."""
    rng = random.Random(21)
    patterns = [b"ab+", b"^a", b"a$", b"^$", b"x*", b"(ab|ba)+", b"[^a]+", b"a\nb|b", b"\\s+", b"[ab]{2,3}",
                b".*b", b"^[ab]+$", b"regexp"]
    for rx in patterns:
        for alphabet in (b"ab\n", b"abx \r\n"):
            texts = [bytes(rng.choice(alphabet) for _ in range(rng.choice((0, 0, 1, 2, 5, 17, 64, 300)))) for _ in range(40)]
            texts += [b"", b"ab", b"b" * 20, b"regexp", b"xregexp\n", b"\n"]
            want = [oracle.match_all(rx, t) for t in texts]
            got = prog(rj, rx).match_all_batch(texts)
            assert got == want, rx
    # larger batch: 2000 "files" of a few KiB with planted needles, counts per file
    from rejit_amd import workloads as W
    files = []
    for i in range(2000):
        n = rng.randrange(0, 6000)
        t = W.random_ascii_numpy(n, seed=1000 + i) if n else np.zeros(0, dtype=np.uint8)
        if n > 40 and i % 3 == 0:
            W.plant(t, [rng.randrange(0, n - 6) for _ in range(i % 4 + 1)], b"regexp")
        files.append(t.tobytes())
    got = prog(rj, b"regexp").match_all_batch(files)
    for t, g in zip(files, got):
        assert g == oracle.match_all(b"regexp", t)


def test_fused_multi_pattern_equals_single_runs(rj):
    """rj_multi: the nine regexdna patterns in one pass over the text give the spans of nine single
    runs (SURVEY 8f-4 "fused vs unfused results identical"); a set with a pattern that cannot be
    fused runs pattern by pattern; region overflow inside the fused kernel grows and reruns."""
    import torch
    from rejit_amd import workloads as W
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    progs = [rj.Program(rx) for rx in W.REGEXDNA_PATTERNS]
    multi = rj.MultiScan(progs)
    singles = [rj.Scan(p) for p in progs]
    texts = [W.fasta_stripped_torch(50000, dev), W.fasta_stripped_torch(3000000, dev)]
    # a text made of hits only: every region overflows its first capacity
    dense = torch.from_numpy(np.frombuffer(b"agggtaaatttaccct" * 40000, dtype=np.uint8).copy()).to(dev)
    texts.append(dense)
    for t in texts:
        n = int(t.numel())
        counts = multi.run(t.data_ptr(), n, stream=st)
        assert multi.fused
        for i, sc in enumerate(singles):
            c = sc.run(t.data_ptr(), n, stream=st)
            assert counts[i] == c, (i, counts[i], c)
            assert multi.scan(i).spans() == sc.spans(), i
    assert multi.run(texts[0].data_ptr(), int(texts[0].numel()), stream=st) == [3, 12, 43, 27, 58, 16, 15, 18, 20]
    # tiny and ragged sizes
    for n in (0, 1, 15, 16, 17, 1023, 1025, 4099):
        t = texts[1][1000:1000 + max(n, 1)].clone()
        counts = multi.run(t.data_ptr(), n, stream=st)
        assert counts == [sc.run(t.data_ptr(), n, stream=st) for sc in singles], n
    # mode 4: the scan kernel classifies its own candidates (plane_scan_classify); the text made of hits only overflows
    # its LDS candidate slots and falls back to the two kernels
    one = rj.MultiScan(progs)
    one.set_mode(4)
    t = texts[1]
    for lo, hi in ((0, 1000000), (999999, 2000001), (1234567, int(t.numel()) + 1)):
        counts = one.run(t.data_ptr(), int(t.numel()), stream=st, own_begin=lo, own_end=hi)
        assert counts == [sc.run(t.data_ptr(), int(t.numel()), own_begin=lo, own_end=hi, stream=st) for sc in singles], (lo, hi)
    for t in [texts[0], texts[1], texts[1][784:784 + 100001].clone(), texts[1][16:16 + 2047].clone(), texts[2], texts[0]]:
        n = int(t.numel())
        for _ in range(2):
            counts = one.run(t.data_ptr(), n, stream=st)
            assert one.fused
            for i, sc in enumerate(singles):
                assert counts[i] == sc.run(t.data_ptr(), n, stream=st), i
                assert one.scan(i).spans() == sc.spans(), i
    # the same nine patterns with separate scan kernels and batched tails (mode 1)
    sep = rj.MultiScan(progs)
    sep.set_mode(1)
    il = rj.MultiScan(progs)
    il.set_mode(2)                  # ... and with the scan kernels on two alternating streams
    for t in texts:
        n = int(t.numel())
        for ms in (sep, il):
            counts = ms.run(t.data_ptr(), n, stream=st)
            assert ms.how == 2
            for i, sc in enumerate(singles):
                assert counts[i] == sc.run(t.data_ptr(), n, stream=st)
                assert ms.scan(i).spans() == sc.spans(), i
    # shards: matches that begin in [own_begin, own_end) of a text with its halo (multi-GPU ranks)
    t = texts[1]
    n = int(t.numel())
    for lo, hi in ((0, 1000000), (999999, 2000001), (1234567, n + 1), (5, 6)):
        for ms in (multi, sep):
            counts = ms.run(t.data_ptr(), n, stream=st, own_begin=lo, own_end=hi)
            for i, sc in enumerate(singles):
                assert counts[i] == sc.run(t.data_ptr(), n, own_begin=lo, own_end=hi, stream=st), (lo, hi, i)
                assert ms.scan(i).spans() == sc.spans()
    # a set that cannot be fused but can be batched (large alphabet, one window, 4-byte window) ...
    t = texts[0]
    n = int(t.numel())
    batch = [rj.Program(b"agggtaaa|tttaccct"), rj.Program(b"gggt"), rj.Program(b"regexp"), rj.Program(b"ag[ct]g")]
    m2 = rj.MultiScan(batch)
    counts = m2.run(t.data_ptr(), n, stream=st)
    assert m2.how == 2
    assert counts == [rj.Scan(p).run(t.data_ptr(), n, stream=st) for p in batch]
    # ... and one that has to run pattern by pattern (a dense pattern in the set)
    mixed = [rj.Program(b"agggtaaa|tttaccct"), rj.Program(b"[cgt]+a"), rj.Program(b"regexp")]
    m3 = rj.MultiScan(mixed)
    counts = m3.run(t.data_ptr(), n, stream=st)
    assert m3.how == 0 and not m3.fused
    assert counts == [rj.Scan(p).run(t.data_ptr(), n, stream=st) for p in mixed]


def test_general_one_pass_pattern_sets(rj, oracle):
    """The general one-pass plan (plane_scan_general + classify_shared_general, round 4): pattern sets that are NOT the
    regexdna shape -- literal alternations of the reference's benchmark regexes with windows at differing offsets and of
    7 / 8 bytes, four 6-mers over [a-z] (codes alias), windows with a class byte (one code may differ) -- run in ONE pass
    (how == 1) and give the spans of single runs and of the oracle; a set the plan refuses runs as separate scans."""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    rng = random.Random(77)
    sets = [
        ([b"alternation|strings", b"prefix abcd|prefix 1234"], [b"alternation", b"strings", b"prefix abcd", b"prefix 1234", b"alternatiom", b"refix abcd"], 1),
        ([b"qwerty", b"zxcvbn", b"plmokn", b"ijbuhv"], [b"qwerty", b"zxcvbn", b"plmokn", b"ijbuhv", b"qwertz", b"ijbuhw", b"uaivzr"], 1),
        ([b"abc[de]fgh", b"abcdfgh[xy]", b"abcefgh"], [b"abcdfgh", b"abcefgh", b"abcdfghx", b"abcdfghz", b"abcffgh"], 1),
        # (round 6: a window with ONE class position becomes a base of its own under tolerance 1 -- this set ran as separate scans until then)
        ([b"x[0-9]regexp", b"regexpyz", b"abcd suffix|1234 suffix"], [b"x7regexp", b"regexpyz", b"abcd suffix", b"1234 suffix", b"xxregexp"], 1),
        # two class positions inside the compared bytes: no base within one byte -- refused, separate scans + batched tails
        ([b"ab[cd][ef]ghij", b"klmnopqr"], [b"abceghij", b"abdfghij", b"abcgghij", b"klmnopqr", b"klmnopqs"], 2),
        # nine 6-mers over [a-z]: nine bases (the scan loops over them; VERDICT r03's example)
        ([b"qwerty", b"zxcvbn", b"plmokn", b"ijbuhv", b"ygctfx", b"rdzesw", b"aqmnbv", b"lkjhgf", b"poiuyt"],
         [b"qwerty", b"zxcvbn", b"plmokn", b"ijbuhv", b"ygctfx", b"rdzesw", b"aqmnbv", b"lkjhgf", b"poiuyt", b"qwertz", b"poiuyr"], 1),
    ]
    for patterns, needles, how in sets:
        progs = [rj.Program(rx) for rx in patterns]
        multi = rj.MultiScan(progs)
        singles = [rj.Scan(p) for p in progs]
        for n, alphabet in ((300_000, b"abcdefghijklmnopqrstuvwxyz 0123456789"), (2_000_000, b"abcdefghijklmnopqrstuvwxyz 0123456789"),
                            (100_000, b"abcdefgh"), (40_000, b"qwertyzxcvbnplmokijuh"), (17, b"ab"), (5000, b"a")):
            body = bytearray(rng.choices(alphabet, k=n))
            for _ in range(n // 900):
                nd = rng.choice(needles)
                at = rng.randrange(0, max(1, n - len(nd)))
                body[at:at + len(nd)] = nd
            for nd in needles[:2]:                       # at the very beginning and end, and across 1-KiB / 2-KiB edges
                if n > 4096:
                    body[0:len(nd)] = nd
                    body[n - len(nd):n] = nd
                    body[1024 - 3:1024 - 3 + len(nd)] = nd
                    body[2048 - 2:2048 - 2 + len(nd)] = nd
            text = bytes(body)
            t = torch.frombuffer(bytearray(text + bytes(16)), dtype=torch.uint8).to(dev)
            counts = multi.run(t.data_ptr(), n, stream=st)
            if n >= 16:
                assert multi.how == how, (patterns, n, multi.how)
            for i, sc in enumerate(singles):
                want = oracle.match_all(patterns[i], text)
                assert counts[i] == len(want), (patterns[i], n, counts[i], len(want))
                assert multi.scan(i).spans() == want, (patterns[i], n)
                assert sc.run(t.data_ptr(), n, stream=st) == len(want)
            # a shard's own range
            if n >= 100_000:
                lo, hi = n // 3 + 1, 2 * n // 3
                counts = multi.run(t.data_ptr(), n, stream=st, own_begin=lo, own_end=hi)
                for i in range(len(patterns)):
                    want = [m for m in oracle.match_all(patterns[i], text) if lo <= m[0] < hi]
                    assert multi.scan(i).spans() == want, (patterns[i], n, "range")


def test_concurrent_match_all_on_one_program(rj, oracle):
    """A compiled pattern is shared by worker threads that call MatchAll concurrently (jrep -j,
    sample/jrep.cc:461-493): scratch is per thread, results are those of serial calls."""
    from concurrent.futures import ThreadPoolExecutor
    rng = random.Random(17)
    texts = [bytes(rng.choice(b"abc \n") for _ in range(rng.choice([0, 10, 3000, 70000]))) for _ in range(48)]
    for rx in (b"ab+c", b"^a.*c$", b"[ab]{3}", b"abc"):
        p = prog(rj, rx)
        want = [oracle.match_all(rx, t) for t in texts]
        with ThreadPoolExecutor(max_workers=6) as pool:
            got = list(pool.map(p.match_all, texts))
        assert got == want, rx
        with ThreadPoolExecutor(max_workers=6) as pool:
            firsts = list(pool.map(p.match_first, texts))
        assert firsts == [w[0] if w else None for w in want], rx


def test_dense_output_gather_paths(rj, oracle):
    """Many matches per hit region: the first call sizes the regions (overflow + retry) and copies
    inside the offsets kernel, the second call -- the scan remembers the density -- takes the
    two-launch gather with a wave per region.  Both must equal the oracle, also when the candidates
    overlap (selection path) and across several sizes."""
    rng = random.Random(23)
    for rx, alphabet in ((b"^", b"ab\n"), (b"x", b"xy"), (b"[ab]+", b"abc"), (b"(ab|ba)+", b"ab"), (b"[ab][ab]", b"ab"),
                         (b"a*", b"ab")):
        for n in (5000, 70000, 400000):
            text = bytes(rng.choice(alphabet) for _ in range(n))
            want = oracle.match_all(rx, text)
            p = rj.Program(rx)          # a fresh program: its scan starts without any hint
            for call in range(3):
                assert p.match_all(text) == want, (rx, n, call)


def test_scan_start_finish_equals_run(rj):
    """rj_scan_start / rj_scan_finish with several scans in flight (all started, then all finished)
    give the results of rj_scan_run -- for patterns the overlapped tail takes (fixed windows) and for
    those that fall back to the synchronous pipeline (dense, floating, Q8-risk, overlapping
    candidates, a region overflow on the first call)."""
    import torch
    from rejit_amd import workloads as W
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    pats = W.REGEXDNA_PATTERNS + ["[cgt]+a", "(ag|ga)+", "a.{0,2}g", "agggtaaa", "ttt", "[acgt]{2,9}tttaccct"]
    progs = [rj.Program(p) for p in pats]
    for t in (W.fasta_stripped_torch(50000, dev), W.fasta_stripped_torch(2000000, dev),
              torch.from_numpy(np.frombuffer(b"agggtaaatttaccct" * 30000, dtype=np.uint8).copy()).to(dev)):
        n = int(t.numel())
        a = [rj.Scan(p) for p in progs]
        b = [rj.Scan(p) for p in progs]
        for rounds in range(2):            # second round: hints are warm
            for sc in a:
                sc.start(t.data_ptr(), n, stream=st)
            got = [sc.finish() for sc in a]
            want = [sc.run(t.data_ptr(), n, stream=st) for sc in b]
            assert got == want
            for x, y, p in zip(a, b, pats):
                assert x.spans() == y.spans(), p
    with pytest.raises(rj.RejitError):
        a[0].finish()                      # nothing started
    a[0].start(t.data_ptr(), n, stream=st)
    with pytest.raises(rj.RejitError):
        a[0].start(t.data_ptr(), n, stream=st)
    a[0].finish()


def test_many_matches_large_path(rj, oracle):
    """More candidates than the LDS finalize holds: the rocPRIM sort path."""
    rng = random.Random(9)
    text = bytes(rng.choice(b"xxxy") for _ in range(50000))
    for rx in (b"x", b"xx", b"x+", b"xy|yx", b"(x|y)y"):
        want = oracle.match_all(rx, text)
        assert len(want) > 2048
        got = prog(rj, rx).match_all(text)
        assert got == want, rx


def test_long_literal_wave_automaton(rj, oracle):
    lit = b"0123456789" * 100
    text = b"ab" + lit + b"cd" + lit[:-1] + b"X" + lit
    assert prog(rj, lit).match_all(text) == oracle.match_all(lit, text)
    assert prog(rj, lit).match_full(lit) and not prog(rj, lit).match_full(lit + b"X")


def test_device_scan_shards_and_carry(rj, oracle):
    """Sharding the owned range with a carried selection state reproduces the single run
    (what the multi-GPU driver relies on)."""
    import torch
    from rejit_amd import workloads as W
    n = 300000
    t = W.random_ascii_numpy(n, seed=3, lo=ord("a"), hi=ord("e"))
    d = torch.from_numpy(t).cuda()
    for rx in (b"abc", b"aa", b"(ab|ba)+", b"a[bc]d?a", b"x*"):
        want = oracle.match_all(rx, t.tobytes())   # (patterns at risk of the ring artefact: ranges own whole segments, exact_replay.hip)
        scan = rj.Scan(prog(rj, rx))
        assert scan.run_tensor(d) == len(want)
        assert scan.spans() == want
        cuts = [0, 99999, 100000, 200001, n + 1]
        got, cur, prev_end, have = [], 0, 0, False
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            scan.run_tensor(d, own_begin=lo, own_end=hi, carry_cur=cur, carry_prev_end=prev_end, have_prev=have)
            part = scan.spans()
            got += part
            if part:
                b_, e_ = part[-1]
                cur, prev_end, have = (e_ if e_ > b_ else b_ + 1), e_, True
        assert got == want, rx


def test_planted_literal_large(rj):
    """256 MiB device-generated text: every planted occurrence is found, every reported
    match is a true occurrence (checked with plain torch), and the count agrees with an
    independent torch sliding compare."""
    import torch
    from rejit_amd import workloads as W
    dev = torch.device("cuda:0")
    n = 1 << 28
    d = W.random_ascii_torch(n, 11, dev)
    offs = W.plant_offsets(n, 6, 500, seed=11, boundaries=[16, 1024, 1 << 20, 1 << 27])
    W.plant(d, offs, b"regexp")
    scan = rj.Scan(rj.Program("regexp"))
    count = scan.run_tensor(d)
    spans = scan.spans()
    needle = torch.tensor(list(b"regexp"), dtype=torch.uint8, device=dev)
    hit = torch.ones(n - 5, dtype=torch.bool, device=dev)
    for k in range(6):
        hit &= d[k:n - 5 + k] == needle[k]
    truth = torch.nonzero(hit).flatten().cpu().tolist()
    assert count == len(truth) and [b_ for b_, _ in spans] == truth
    assert all(e_ - b_ == 6 for b_, e_ in spans)
    assert set(offs) <= set(truth)
    st = scan.stats()
    assert st["n_matches"] == count and st["scan_ms"] > 0


@pytest.mark.parametrize("needle", [b"qz", b"qzv", b"qzvwx", b"regexpqz"])
def test_literal_across_every_lane_and_chunk_edge(rj, needle):
    """The streaming loop of scan_windows takes the bytes behind a lane's 16 from the lane above and, for lane 63, from the
    NEXT chunk's buffer (round 6: no halo load).  A needle planted at every offset around 16-byte lane edges, 1-KiB chunk
    edges and the edges of the waves' spans of a 64 MiB device text (steady loop, the loop's last three chunks, the plain
    loop, the guarded tail): exactly the planted occurrences come back (checked with a torch sliding compare)."""
    import torch
    dev = torch.device("cuda:0")
    n = (64 << 20) + 777
    g = torch.Generator(device="cpu").manual_seed(len(needle))
    d = torch.randint(ord("a"), ord("p"), (n,), dtype=torch.uint8, generator=g).to(dev)   # (no q, z, r ... in the filler)
    L = len(needle)
    offs = []
    for base in list(range(1 << 20, n - (2 << 20), (5 << 20) + 1024 * 37)) + [0, n - 4096]:
        k = base // 1024 * 1024
        for edge in (k + 1024, k + 2048 + 16 * 17, k + 5 * 1024 + 16 * 63, k + 9 * 1024):
            offs.append(edge - L - 1 + (len(offs) % (L + 3)))     # ends before, on and behind the edge in turn
    offs += [n - L, n - L - 1024, 16 - L // 2]
    offs = sorted(set(o for o in offs if 0 <= o <= n - L))
    kept, last = [], -100
    for o in offs:                                              # (apart: no planted needle overwrites another)
        if o >= last + L + 1:
            kept.append(o)
            last = o
    nd = torch.tensor(list(needle), dtype=torch.uint8, device=dev)
    for o in kept:
        d[o:o + L] = nd
    scan = rj.Scan(rj.Program(needle.decode()))
    count = scan.run_tensor(d)
    hit = torch.ones(n - L + 1, dtype=torch.bool, device=dev)
    for j in range(L):
        hit &= d[j:n - L + 1 + j] == nd[j]
    truth = torch.nonzero(hit).flatten().cpu().tolist()
    assert truth == kept
    assert count == len(truth) and [b_ for b_, _ in scan.spans()] == truth


def _splice(text: bytes, spans, repl: bytes) -> bytes:
    out, p = bytearray(), 0
    for b_, e_ in spans:
        out += text[p:b_] + repl
        p = e_
    out += text[p:]
    return bytes(out)


def test_replace_all_vs_oracle(rj, oracle):
    """rj_replace_all (MatchAll + the device replace_gather) == the reference's Replace
    (src/rejit.cc:97-112) applied to the oracle's matches."""
    from rejit_amd import workloads as W
    rng = random.Random(17)
    cases = [(b"regexp", b"X"), (b"a", b""), (b"ab|ba", b"<->"), (b"x*", b"-"), (b"\n", b""), (b">.*\n|\n", b""),
             (b"[0-9]+", b"#"), (b"^", b"> "), (b"zzzz", b"never")]
    for rx, repl in cases:
        for n in (0, 1, 50, 3000, 200000):
            text = bytes(rng.choice(b"ab\nx>1regexp z") for _ in range(n))
            want_spans = oracle.match_all(rx, text)
            m, got = prog(rj, rx).replace_all(text, repl)
            assert m == len(want_spans) and got == _splice(text, want_spans, repl), (rx, n)
    # long gaps (copied by the whole grid) and the regexdna pipeline sizes
    big = W.random_ascii_numpy(3_000_000, 3)
    offs = W.plant_offsets(len(big), 6, 5, seed=5)
    W.plant(big, offs, b"regexp")
    tb = big.tobytes()
    m, got = prog(rj, b"regexp").replace_all(tb, b"<<literal>>")
    assert got == tb.replace(b"regexp", b"<<literal>>") and m == tb.count(b"regexp")
    g = V.bench()["regexdna"]["50000"]
    raw = W.fasta_raw_numpy(50000).tobytes()
    m, stripped = prog(rj, V.b(g["strip"]["regex"])).replace_all(raw, b"")
    assert m == g["strip"]["count"] and hashlib.sha256(stripped).hexdigest() == g["stripped_sha256"]
    text = stripped
    for code, repl in W.REGEXDNA_IUB:
        _, text = prog(rj, code.encode()).replace_all(text, repl.encode())
    assert len(text) == g["replaced_size"] and hashlib.sha256(text).hexdigest() == g["replaced_sha256"]


def test_replace_all_in_two_steps_and_large(rj, oracle):
    """rj_replace_all_begin / _fetch (round 6: Regej::ReplaceAll takes the new text straight into its own string) and the
    library's own staging of large downloads (host_api.hip: staged_download, >= 32 MiB): the same bytes as rj_replace_all and
    as the reference's Replace on the oracle's matches; growing, shrinking and unchanged texts; a buffer that is too small is
    refused and a fetch without begin too."""
    from rejit_amd import workloads as W
    rng = random.Random(19)
    for rx, repl in [(b"regexp", b"<<literal>>"), (b"\n", b""), (b"[0-9]+", b"#"), (b"zzzz", b"never")]:
        text = bytes(rng.choice(b"ab\nx>1regexp z0") for _ in range(150000))
        want = _splice(text, oracle.match_all(rx, text), repl)
        p = prog(rj, rx)
        dst = bytearray(len(want) + 100)
        m, new_len = p.replace_all_into(text, repl, dst)
        assert new_len == len(want) and bytes(dst[:new_len]) == want and m == len(oracle.match_all(rx, text)), rx
        with pytest.raises(rj.RejitError):
            p.replace_all_into(text, repl, bytearray(max(len(want) - 1, 0)))
    lib = rj.load_library()
    assert lib.rj_replace_all_fetch(prog(rj, b"never begun")._h, None, 0) < 0
    # 100 MB: four slices of the pinned ring each way round, matches across slice boundaries
    n = 100_000_000
    big = W.random_ascii_numpy(n, 9)
    offs = W.plant_offsets(n, 6, 2000, seed=9, boundaries=[16 << 20, 32 << 20, 48 << 20, (16 << 20) * 5])
    W.plant(big, offs, b"regexp")
    tb = big.tobytes()
    want = tb.replace(b"regexp", b"<<regular expression>>")
    m, got = prog(rj, b"regexp").replace_all(tb, b"<<regular expression>>")
    assert m == tb.count(b"regexp") and got == want
    dst = bytearray(len(want))
    m2, new_len = prog(rj, b"regexp").replace_all_into(tb, b"<<regular expression>>", dst)
    assert (m2, new_len) == (m, len(want)) and bytes(dst) == want
    m3, shrunk = prog(rj, b"regexp").replace_all(tb, b"")
    assert m3 == m and shrunk == tb.replace(b"regexp", b"")


def test_device_replace_keeps_text_in_hbm(rj):
    import torch
    from rejit_amd import workloads as W
    dev = torch.device("cuda:0")
    raw = torch.from_numpy(W.fasta_raw_numpy(20000)).to(dev)
    scan = rj.Scan(rj.Program(W.REGEXDNA_STRIP))
    n = raw.numel()
    m = scan.run_tensor(raw)
    out = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    new_len = scan.replace(raw.data_ptr(), n, b"", out.data_ptr(), out.numel())
    assert new_len == 200000 and m == n - new_len - (len(b"".join(W.HEADERS)) - 3)
    assert (out[:new_len].cpu().numpy() == W.fasta_stripped_numpy(20000)).all()


def test_complex_regex_floating_windows_large(rj, oracle):
    """BASELINE configs[3] shape: the complex benchmark regex over device-resident random text
    with planted strings of its language and `abcdefgh` decoys.  The scan plan is the floating
    window `abcdefgh` (2..42 bytes after the match start); every reported match must be a true
    left-most-longest match (checked with the oracle on a window around it) and every planted
    string must be covered by one."""
    import torch
    from rejit_amd import workloads as W
    rx = W.BENCH_REGEXES[3][0].encode()
    p = rj.Program(rx)
    info = p.info()
    assert info["scan_mode"] == 1
    dev = torch.device("cuda:0")
    n = 1 << 27
    d = W.random_ascii_torch(n, 23, dev)
    rng = random.Random(23)
    planted = []
    offs = W.plant_offsets(n, 80, 400, seed=23, boundaries=[1024, 1 << 20, 1 << 26])
    for k, o in enumerate(offs):
        sample = W.complex_regex_sample(rng) if k % 4 else b"abcdefgh"      # every 4th is a decoy
        W.plant(d, [o + 4], sample)
        if k % 4:
            planted.append((o + 4, o + 4 + len(sample)))
    scan = rj.Scan(p)
    count = scan.run_tensor(d)
    spans = scan.spans()
    assert count == len(spans) and count >= len(planted)
    host = d.cpu().numpy()
    for b_, e_ in spans:      # each reported match, re-derived by the oracle on its neighbourhood
        lo, hi = max(0, b_ - 64), min(n, e_ + 64)
        local = oracle.match_all(rx, host[lo:hi].tobytes())
        assert (b_ - lo, e_ - lo) in local, (b_, e_)
    got = set(spans)
    for b_, e_ in planted:    # a planted string is matched (possibly extended to the left by the repetition)
        assert any(gb <= b_ and ge == e_ for gb, ge in got if gb >= b_ - 48 and ge == e_), (b_, e_)


def test_planted_literal_beyond_4gib(rj):
    """64-bit offsets in a pytest (round 1 only checked them inside bench.py): 4.5 GiB of device text,
    occurrences planted on both sides of 2^32, the result compared with an independent torch compare
    of the six bytes around every planted position and of a window across the 4 GiB line."""
    import torch
    from rejit_amd import workloads as W
    dev = torch.device("cuda:0")
    n = (9 << 29) + 12345          # 4.5 GiB and a ragged tail
    t = W.random_ascii_torch(n, 0xBEEF, dev)
    offs = sorted(set(W.plant_offsets(n, 6, 300, seed=5, boundaries=[1 << 32, (1 << 32) + 1024, 1 << 31, n // 2])
                      + [(1 << 32) - 3, (1 << 32) - 6, (1 << 32), (1 << 32) + 7, n - 6]))
    keep, last = [], -10
    for o in offs:                 # planted occurrences must not overlap
        if o >= last + 6 and o + 6 <= n:
            keep.append(o)
            last = o
    W.plant(t, keep, b"regexp")
    sc = rj.Scan(rj.Program(b"regexp"))
    cnt = sc.run_tensor(t)
    spans = sc.spans()
    found = [b for b, _ in spans]
    assert all(e - b == 6 for b, e in spans) and found == sorted(found) and cnt == len(spans)
    assert set(keep) <= set(found)
    assert sum(1 for b in found if b >= (1 << 32)) >= 5 and max(found) == n - 6
    # independent check of the natural occurrences: a sliding compare over a 256 MiB window across 2^32
    lo, hi = (1 << 32) - (128 << 20), (1 << 32) + (128 << 20)
    w = t[lo:hi]
    pat = torch.tensor(list(b"regexp"), dtype=torch.uint8, device=dev)
    m = torch.ones(w.numel() - 5, dtype=torch.bool, device=dev)
    for k in range(6):
        m &= w[k:w.numel() - 5 + k] == pat[k]
    want = (torch.nonzero(m).flatten() + lo).tolist()
    assert [b for b in found if lo <= b < hi - 5] == want


def test_random_patterns_through_the_general_pipeline():
    """Texts of a few KiB take the one-workgroup kernel (match_small), so the random-pattern tests above no
    longer reach the kernels large texts run on.  tools/fuzz_large.py with RJ_NO_SMALL=1 (read once per
    process, hence the subprocess) sends the same kind of random patterns over texts of 1.5..9 KiB through
    the general pipeline -- window scans, the dense kernel with its lane-packed pre-steps, verification,
    gather, selection, the exact replay -- and compares every result with the oracle."""
    import subprocess
    import sys
    env = dict(os.environ, RJ_NO_SMALL="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_large.py"), "700", "4711"], env=env, capture_output=True,
                       timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    last = out.strip().splitlines()[-1]
    assert last.startswith("checked 700") and last.endswith("mismatches 0"), out[-2000:]


@pytest.mark.gpu
def test_multi_start_finish_two_in_flight():
    """rj_multi_start / rj_multi_finish: two rj_multi objects of the nine regexdna patterns used alternately over two
    different texts give, step by step, the counts of rj_multi_run; a second start before finish is refused; ranges."""
    import torch
    import rejit_amd
    from rejit_amd import workloads as W
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    progs = [rejit_amd.Program(rx) for rx in W.REGEXDNA_PATTERNS]
    texts = [torch.from_numpy(W.fasta_stripped_numpy(n).copy()).to(dev) for n in (30000, 47000)]
    ref = rejit_amd.MultiScan(progs)
    want = [ref.run(t.data_ptr(), t.numel(), stream=st) for t in texts]
    a, b = rejit_amd.MultiScan(progs), rejit_amd.MultiScan(progs)
    objs, got = [a, b], []
    a.start(texts[0].data_ptr(), texts[0].numel(), stream=st)          # step 0
    with pytest.raises(rejit_amd.RejitError):
        a.start(texts[0].data_ptr(), texts[0].numel(), stream=st)
    for k in range(1, 9):                                               # step k runs on object k % 2 over text k % 2
        objs[k % 2].start(texts[k % 2].data_ptr(), texts[k % 2].numel(), stream=st)
        got.append(objs[(k - 1) % 2].finish())                          # ... while step k - 1 is collected
    got.append(objs[8 % 2].finish())
    assert got == [want[k % 2] for k in range(9)]
    # a shard's own range
    n = texts[1].numel()
    lo, hi = n // 3, 2 * n // 3
    want_r = ref.run(texts[1].data_ptr(), n, stream=st, own_begin=lo, own_end=hi)
    a.start(texts[1].data_ptr(), n, stream=st, own_begin=lo, own_end=hi)
    assert a.finish() == want_r
    with pytest.raises(rejit_amd.RejitError):
        a.finish()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "mode4", "mode1", "tail_stream", "general"])
def test_multi_finish_after_overflowed_regions(variant):
    """rj_multi_finish after a run whose regions overflowed: the first attempt was enqueued by rj_multi_start, the larger
    ones run inside rj_multi_finish.  Two objects in flight over a text made of hits only (every region overflows its first
    capacity; in mode 4 the scan kernel's LDS slots) and a sparse one, each object seeing dense, sparse, dense: step by step
    the counts, the return value and every pattern's spans of rj_multi_run on a fresh object; the first dense step of each
    object reports its retries, the second one needs none."""
    import torch
    import rejit_amd
    from rejit_amd import workloads as W
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    if variant == "general":
        patterns = [b"qwerty", b"zxcvbn", b"plmokn", b"ijbuhv"]
        rng = random.Random(78)
        sparse = bytearray(rng.choices(b"abcdefghijklmnopqrstuvwxyz 0123456789", k=30000))
        for k in range(30):
            sparse[1000 * k + 17:1000 * k + 23] = patterns[k % 4]
        datas = [b"qwertyzxcvbnplmoknijbuhv" * 27000, bytes(sparse)]
    else:
        patterns = W.REGEXDNA_PATTERNS
        datas = [b"agggtaaatttaccct" * 40000, W.fasta_stripped_numpy(30000).tobytes()]
    progs = [rejit_amd.Program(rx) for rx in patterns]
    texts = [torch.from_numpy(np.frombuffer(d + bytes(16), dtype=np.uint8).copy()).to(dev) for d in datas]

    def make():
        m = rejit_amd.MultiScan(progs)
        if variant == "mode4":
            m.set_mode(4)
        elif variant == "mode1":
            m.set_mode(1)
        elif variant == "tail_stream":
            m.set_tail_stream(True)
        return m

    want = []
    for d, t in zip(datas, texts):
        ref = make()                                                    # (a fresh object per text: its first capacities)
        counts = ref.run(t.data_ptr(), len(d), stream=st)
        want.append((counts, ref.how, [ref.scan(i).spans() for i in range(len(progs))]))
    objs = [make(), make()]
    order = [0, 0, 1, 1, 0, 0]                                          # step k: object k % 2 over text order[k]

    def collect(k):
        m = objs[k % 2]
        got = (m.finish(), m.how, [m.scan(i).spans() for i in range(len(progs))])
        assert got == want[order[k]], (variant, k)
        retries = max(m.scan(i).stats()["retries"] for i in range(len(progs)))
        if k < 2:
            assert retries >= 1, (variant, k)                           # the path under test was taken
        elif k >= 4:
            assert retries == 0, (variant, k)                           # the same text again: the capacities hold

    for k in range(len(order)):
        objs[k % 2].start(texts[order[k]].data_ptr(), len(datas[order[k]]), stream=st)
        if k >= 1:
            collect(k - 1)
    collect(len(order) - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["tails_on_own_streams", "stream_per_object"])
def test_multi_two_in_flight_on_tail_streams(variant):
    """The two other ways to keep two steps in flight (bench.py's headline loop and its extras): every run's tails on a
    stream of the object's own behind the scan's end event (rj_multi_set_tail_stream), and an object per stream with the
    scans ordered by rj_multi_order_after -- step by step the counts and the spans of rj_multi_run, on texts of
    different sizes so that a run that overtook its predecessor would show."""
    import torch
    import rejit_amd
    from rejit_amd import workloads as W
    dev = torch.device("cuda:0")
    main = torch.cuda.current_stream(dev).cuda_stream
    second = torch.cuda.Stream(dev)
    progs = [rejit_amd.Program(rx) for rx in W.REGEXDNA_PATTERNS]
    texts = [torch.from_numpy(W.fasta_stripped_numpy(n).copy()).to(dev) for n in (30000, 470000, 2000000)]
    ref = rejit_amd.MultiScan(progs)
    want, want_spans = [], []
    for t in texts:
        want.append(ref.run(t.data_ptr(), t.numel(), stream=main))
        want_spans.append([ref.scan(i).spans() for i in range(len(progs))])
    objs = [rejit_amd.MultiScan(progs), rejit_amd.MultiScan(progs)]
    streams = [main, main]
    if variant == "tails_on_own_streams":
        for m in objs:
            m.set_tail_stream(True)
    else:
        streams = [main, second.cuda_stream]
        objs[0].order_after(objs[1]); objs[1].order_after(objs[0])
    steps, got = 13, []
    for k in range(steps):
        j = k & 1
        if k >= 2:
            got.append(objs[j].finish())
            assert [objs[j].scan(i).spans() for i in range(len(progs))] == want_spans[(k - 2) % 3], (variant, k)
        objs[j].start(texts[k % 3].data_ptr(), texts[k % 3].numel(), stream=streams[j])
    for k in (steps - 2, steps - 1):
        got.append(objs[k & 1].finish())
    assert got == [want[k % 3] for k in range(steps)], variant
    for m in objs:                       # (the raw pointers of order_after must not outlive their targets)
        m.order_after(None)
