"""GPU tests (-m gpu) of the counts path's scan_ms (rj_multi_set_timing on the one-kernel MatchAllCount,
rejit_amd/csrc/plane_count.hip): the kernel's workgroups stamp their entry and exit with the device's wall clock,
plane_count_finish hands the first entry and the last exit to the host, and no start event is put on the stream.

For every shape of the kernel that ends in rows -- the regexdna nine (ExactShape<2>), a one-base set (ExactShape<1>), a set
of literals of other lengths (GeneralShape) -- and for texts of
  16 bytes        one workgroup, the smallest text the path takes,
  2049 bytes      one block plus one byte: the guarded end-of-text path,
  35 000 bytes    18 blocks of 2 KiB, two per workgroup: 9 workgroups, one more than plane_count_finish has groups (the rows are
                  dealt out two per group: four groups with two rows, one with one, three with none),
  3 MiB           256 workgroups,
  64 MiB          512 workgroups; the bandwidth bound below,
counts and bounds are the oracle's and the same with timing on and off; scan_ms() is 0 with timing off and, with timing on,
positive and below the host's time around the synchronous call (unconverted ticks, a wrapped difference, or a duration far
beyond the call's would miss that).  At 64 MiB the duration must put the scan between 0.2 and 8.0 TB/s: no correct duration
beats the HBM peak, and one workgroup's exit taken for the last one's would.
"""
import random
import time

import numpy as np
import pytest

from checkers import Oracle
from test_gpu_counts import device_text, regexdna_strings

pytestmark = pytest.mark.gpu

MIB = 1 << 20
ASCII_BG = bytes(range(ord("0"), ord("z")))
# (one exact window, `agggtaaa`, the others within one byte of it: one base, three symbols)
ONE_BASE = [b"agggtaaa", b"[cgt]gggtaaa", b"agggtaa[cgt]", b"ag[act]gtaaa"]
GENERAL = [b"alternation|strings", b"prefix abcd|prefix 1234"]
GENERAL_STRINGS = [b"alternation", b"strings", b"prefix abcd", b"prefix 1234", b"alternatio", b"prefix abc4", b"string", b"prefix 123"]
SIZES = [16, 2049, 35000, 3 * MIB]


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
def sets(rj):
    """name -> (patterns, programs, strings to plant, background alphabet, a filler byte that no match consists of)"""
    from rejit_amd import workloads as W
    dna = [rx.encode() for rx in W.REGEXDNA_PATTERNS]
    return {
        "regexdna": (dna, [rj.Program(rx) for rx in dna], regexdna_strings(), b"acgt", b"c"),
        "one_base": (ONE_BASE, [rj.Program(rx) for rx in ONE_BASE], regexdna_strings()[:33], b"acgt", b"c"),
        "general": (GENERAL, [rj.Program(rx) for rx in GENERAL], GENERAL_STRINGS, ASCII_BG, b"#"),
    }


def make_text(name, n, strings, alphabet):
    """random bytes of the alphabet, one of the strings planted per 512-byte slot, a match at either end of the text"""
    seed = sum(name.encode()) * 1000003 + n
    rng = random.Random(seed)
    t = bytearray(np.random.default_rng(seed).choice(np.frombuffer(alphabet, dtype=np.uint8), n).tobytes())
    for slot in range(0, n - 512, 512):    # (at least 16 bytes apart: the plants' matches do not overlap each other)
        s = rng.choice(strings)
        p = slot + rng.randrange(0, 512 - 32)
        t[p:p + len(s)] = s
    first, last = strings[0], strings[1]
    if n >= len(last):
        t[n - len(last):n] = last
    if n >= len(first) + len(last):
        t[0:len(first)] = first
    return bytes(t)


def oracle_answer(oracle, rxs, data, own=None, repeat=1):
    """(counts, bounds as MultiScan.bounds() gives them) by the oracle; own: match begins in [own[0], own[1]) only.
    repeat k: the answer for `data` k times in a row, for a text no match of which touches its first or last 16 bytes."""
    counts, bounds = [], []
    for rx in rxs:
        sp = oracle.match_all(rx, data)
        if own is not None:
            sp = [m for m in sp if own[0] <= m[0] < own[1]]
        counts.append(len(sp) * repeat)
        shift = (repeat - 1) * len(data)
        bounds.append((sp[0][0], sp[0][1], sp[-1][0] + shift, sp[-1][1] + shift) if sp else None)
    return counts, bounds


def timed_run(m, ptr, n, **kw):
    """(counts, how, bounds, scan_ms, the host's milliseconds around the synchronous call)"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = m.run(ptr, n, **kw)
    wall = (time.perf_counter() - t0) * 1e3
    return c, m.how, m.bounds(), m.scan_ms(), wall


def check_both(rj, progs, t, n, want, label, **kw):
    """one object: timing off, then on -- the same (the oracle's) counts and bounds; returns the timed run's scan_ms"""
    m = rj.MultiScan(progs)
    assert m.set_counts_only(True), label
    m.set_timing(False)
    c0, how0, b0, ms0, _ = timed_run(m, t.data_ptr(), n, **kw)
    m.set_timing(True)
    c1, how1, b1, ms1, wall = timed_run(m, t.data_ptr(), n, **kw)
    print("%s: n = %d, scan_ms %.5f (timing off: %.5f), call %.5f ms" % (label, n, ms1, ms0, wall))
    assert how0 == 3 and how1 == 3, (label, how0, how1)
    assert (c0, b0) == want, (label, c0, want[0])
    assert (c1, b1) == want, (label, c1, want[0])
    assert ms0 == 0.0, (label, ms0)
    assert 0.0 < ms1 < wall, (label, ms1, wall)
    return ms1


@pytest.mark.parametrize("name", ["regexdna", "one_base", "general"])
def test_scan_ms_by_the_device_clock(rj, oracle, sets, name):
    rxs, progs, strings, alphabet, _ = sets[name]
    for n in SIZES:
        data = make_text(name, n, strings, alphabet)
        want = oracle_answer(oracle, rxs, data)
        assert sum(want[0]) > 0, (name, n)
        check_both(rj, progs, device_text(data), n, want, name)


@pytest.mark.parametrize("name", ["regexdna", "one_base", "general"])
def test_duration_of_64_mib_is_a_possible_one(rj, oracle, sets, name):
    """A tile of 2 MiB, checked by the oracle, 32 times in a row.  The tile begins and ends with 16 bytes of a filler, and no
    match is longer than 16 bytes: one across a seam would lie inside the 32 filler bytes, and filler alone matches nothing.
    The oracle's selection (a match that begins inside the one before it is dropped) reaches no further than a match: every
    copy holds the tile's matches."""
    rxs, progs, strings, alphabet, filler = sets[name]
    tile = bytearray(make_text(name, 2 * MIB, strings, alphabet))
    tile[:16] = filler * 16
    tile[-16:] = filler * 16
    tile = bytes(tile)
    want = oracle_answer(oracle, rxs, tile, repeat=32)
    assert sum(want[0]) > 0
    n = 64 * MIB
    t = device_text(tile * 32)
    ms = check_both(rj, progs, t, n, want, name)
    tbps = n / (ms * 1e-3) / 1e12
    print("%s: 64 MiB in %.5f ms = %.3f TB/s" % (name, ms, tbps))
    assert 0.2 < tbps < 8.0, (name, ms, tbps)


def test_timing_toggled_between_calls(rj, oracle, sets):
    """The first call of a fresh object (it allocates and clears the buffers of the counts path on the stream first) with timing
    on, then off, on, on, off on the same object."""
    rxs, progs, strings, alphabet, _ = sets["regexdna"]
    n = 200001
    data = make_text("toggle", n, strings, alphabet)
    want = oracle_answer(oracle, rxs, data)
    t = device_text(data)
    m = rj.MultiScan(progs)
    assert m.set_counts_only(True)
    for on in (True, False, True, True, False):
        m.set_timing(on)
        c, how, b, ms, wall = timed_run(m, t.data_ptr(), n)
        assert how == 3 and (c, b) == want, (on, how, c)
        assert (0.0 < ms < wall) if on else ms == 0.0, (on, ms, wall)


def test_two_timed_objects_in_flight_on_one_stream(rj, oracle, sets):
    import torch
    rxs, progs, strings, alphabet, _ = sets["regexdna"]
    texts = [make_text("flight%d" % k, n, strings, alphabet) for k, n in enumerate((300000, 2 * MIB + 77))]
    wants = [oracle_answer(oracle, rxs, d) for d in texts]
    ts = [device_text(d) for d in texts]
    st = torch.cuda.current_stream().cuda_stream
    ms = [rj.MultiScan(progs) for _ in range(2)]
    for m in ms:
        assert m.set_counts_only(True)
        m.set_timing(True)
    for _ in range(2):   # (the second round: both objects' buffers exist)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for m, t, d in zip(ms, ts, texts):
            m.start(t.data_ptr(), len(d), stream=st)
        got = [(m.finish(), m.how, m.bounds(), m.scan_ms()) for m in ms]
        wall = (time.perf_counter() - t0) * 1e3
        for (c, how, b, dur), want in zip(got, wants):
            assert how == 3 and (c, b) == want, (how, c, want[0])
            assert 0.0 < dur < wall, (dur, wall)


def test_own_range(rj, oracle, sets):
    rxs, progs, strings, alphabet, _ = sets["regexdna"]
    n = 150000
    data = make_text("own", n, strings, alphabet)
    t = device_text(data)
    for own in ((12345, 99999), (2048, 4096), (70000, n + 1)):
        want = oracle_answer(oracle, rxs, data, own=own)
        check_both(rj, progs, t, n, want, "own %r" % (own,), own_begin=own[0], own_end=own[1])
    # ... and for the general shape, whose windows have offsets of their own
    rxs, progs, strings, alphabet, _ = sets["general"]
    data = make_text("own general", n, strings, alphabet)
    want = oracle_answer(oracle, rxs, data, own=(12345, 99999))
    check_both(rj, progs, device_text(data), n, want, "general own", own_begin=12345, own_end=99999)


def test_a_void_run_reports_the_span_pipelines_time(rj, oracle, sets):
    """`agggtaaa` back to back overfills a wave's ring: THAT run is void and the span pipeline answers, with its own (event-based)
    scan_ms; the next call on a clean text takes the kernel again, with the clock's duration.
    (The oracle's counts: the copies match pattern 0 once each and nothing else -- checked at 5000 copies; the copies' matches do
    not overlap, so 400 000 copies hold 400 000.  The oracle needs minutes for that text.)"""
    rxs, progs, strings, alphabet, _ = sets["regexdna"]
    clean = b"agggtaaa" * 5000 + b"acgt" * 1000
    want_clean = oracle_answer(oracle, rxs, clean)
    assert want_clean[0] == [5000] + [0] * 8
    void = b"agggtaaa" * 400000 + b"acgt" * 1000
    tv, tc = device_text(void), device_text(clean)
    m = rj.MultiScan(progs)
    assert m.set_counts_only(True)
    m.set_timing(True)
    c, how, b, ms, wall = timed_run(m, tv.data_ptr(), len(void))
    assert c == [400000] + [0] * 8 and how != 3, (how, c)
    assert b[0] == (0, 8, 8 * 399999, 8 * 400000) and b[1:] == [None] * 8, b
    assert ms >= 0.0, ms
    c, how, b, ms, wall = timed_run(m, tc.data_ptr(), len(clean))
    assert how == 3 and (c, b) == want_clean, (how, c)
    assert 0.0 < ms < wall, (ms, wall)
