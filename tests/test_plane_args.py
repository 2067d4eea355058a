"""CPU test of the pure launch-argument builders of the plane kernels (rejit_amd/csrc/plane_args.h, used by
multi_pattern.hip for plane_scan / plane_list / plane_count and their general forms): the three encodings of a plan's base
windows against ONE definition of the 2-bit symbol code, the window positions and 2-KiB blocks of a range of starts and their
split over the regions against brute force, a pattern's own window range, and the chunk range engine.hip's run_range scans
(chunk_range) against the window sweep's restatement of it.  The driver (tests/support/plane_args_exec.cc)
is loaded through ctypes, and once more built as a stand-alone program under the address and undefined sanitizers."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import window_sweep as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "support", "plane_args_exec.cc")
DEPS = [SRC, os.path.join(ROOT, "rejit_amd", "csrc", "plane_args.h")]
SO = os.path.join(HERE, "support", "libplane_args_exec.so")
EXE = os.path.join(HERE, "support", "plane_args_exec_asan")
ROWS = 12           # kPlaneMaxBases (rejit_amd/csrc/kernels.h)
U64 = ctypes.c_uint64
U32 = ctypes.c_uint32


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def pa():
    if _stale(SO):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO, SRC])
    lib = ctypes.CDLL(SO)
    u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(U32), ctypes.POINTER(U64)
    lib.pa_encodings.restype = None
    lib.pa_encodings.argtypes = [u8p, U32, U32, U32, u32p, u32p, u32p, u32p]
    lib.pa_blocks.restype = None
    lib.pa_blocks.argtypes = [U64, U64, U64, U32, U32, U32, u64p]
    lib.pa_split.restype = None
    lib.pa_split.argtypes = [U64, U64, U32, u64p]
    lib.pa_window_range.restype = None
    lib.pa_window_range.argtypes = [U64, U64, U64, U32, U32, u64p]
    lib.pa_chunk_range.restype = None
    lib.pa_chunk_range.argtypes = [U64, U64, U64, ctypes.c_int, U32, U32, U32, ctypes.c_int, u64p]
    return lib


def code(byte, shift):
    """THE definition: a byte's 2-bit symbol code under a plan's shift."""
    return (byte >> shift) & 3


def test_the_three_encodings_of_the_bases_agree(pa):
    rng = random.Random(31)
    for n_bases in range(1, ROWS + 1):
        for shift in range(0, 7):                  # plan_plane / plan_plane_general try the shifts 0..6
            for n_cmp in range(4, 9):
                base = (ctypes.c_uint8 * (ROWS * 8))(*[rng.randrange(256) for _ in range(ROWS * 8)])
                lo, hi, idx = (U32 * (ROWS * 8))(), (U32 * (ROWS * 8))(), (U32 * (ROWS * 8))()
                bits = U32()
                pa.pa_encodings(base, n_bases, shift, n_cmp, lo, hi, ctypes.byref(bits), idx)
                for b in range(ROWS):
                    src = b if b < n_bases else 0                                      # bases beyond n_bases repeat base 0
                    for i in range(8):
                        c = code(base[8 * src + i], shift)
                        ctx = (n_bases, shift, n_cmp, b, i)
                        assert lo[8 * b + i] in (0, 0xFFFFFFFF) and hi[8 * b + i] in (0, 0xFFFFFFFF), ctx
                        assert (lo[8 * b + i] == 0xFFFFFFFF) == (c & 1 == 0), ctx
                        assert (hi[8 * b + i] == 0xFFFFFFFF) == (c & 2 == 0), ctx
                        if b < 2:                                                      # mask_bits: the two bases of the exact plan
                            assert bool(bits.value >> (16 * b + 2 * i) & 1) == (c & 1 == 0), ctx
                            assert bool(bits.value >> (16 * b + 2 * i + 1) & 1) == (c & 2 == 0), ctx
                        assert idx[8 * b + i] == (c if i < n_cmp else 4), ctx


def _starts(n):
    return sorted({x for x in (0, 1, 2047, 2048, 2049, 4095, 4096, 4097, n - 1, n, n + 1) if 0 <= x <= n + 1})


def test_window_positions_blocks_and_split_against_brute_force(pa):
    out, sp = (U64 * 4)(), (U64 * 3)()
    checked = empty = 0
    for n in (0, 7, 8, 15, 16, 2047, 2048, 2049, 4096 + 5, 10 ** 6):
        at = _starts(n)
        for sb in at:
            for se in [e for e in at if e > sb] + [sb + 1]:                           # (an empty [sb, se) never reaches the builders)
                if se > n + 1:
                    continue
                for lo_off in (0, 3, 7):
                    for hi_off in (0, 3, 7):
                        for n_cmp in (4, 8):
                            if hi_off < lo_off:
                                continue
                            pa.pa_blocks(n, sb, se, lo_off, hi_off, n_cmp, out)
                            wlo, whi, first, end = out[0], out[1], out[2], out[3]
                            # brute force: w = s + off for a start s in [sb, se) and an offset of the set, n_cmp bytes of text behind it
                            w = np.arange(sb + lo_off, se + hi_off, dtype=np.int64)
                            w = w[w + n_cmp <= n]
                            ctx = (n, sb, se, lo_off, hi_off, n_cmp)
                            if len(w):
                                assert (wlo, whi) == (w[0], w[-1] + 1), ctx
                                assert list(range(first, end)) == np.flatnonzero(np.bincount(w >> 11)).tolist(), ctx
                            else:
                                empty += 1
                                assert whi <= wlo and end == first, ctx
                            for n_regions in (1, 2, 7, 64):
                                pa.pa_split(first, end, n_regions, sp)
                                assert sum(sp[0] + (1 if r < sp[1] else 0) for r in range(n_regions)) == end - first, ctx
                                assert sp[1] < n_regions and sp[2] == max(-(-(end - first) // n_regions), 1), ctx
                            checked += 1
    assert checked > 2000 and empty > 100


def test_a_patterns_own_window_range(pa):
    out = (U64 * 2)()
    for n in (0, 7, 8, 15, 16, 2047, 2049, 4096 + 5):
        for sb in _starts(n):
            for se in _starts(n):
                for off in (0, 3, 7):
                    for length in (4, 5, 8):
                        pa.pa_window_range(n, sb, se, off, length, out)
                        w = [s + off for s in range(sb, se) if s + off + length <= n]
                        assert out[1] >= out[0] == sb + off, (n, sb, se, off, length)
                        assert out[1] - out[0] == len(w), (n, sb, se, off, length)


def test_the_engines_chunk_range_on_the_window_sweeps_geometries(pa):
    """chunk_range is what run_range scans; tests/window_sweep.py plans its texts from window_range, its own statement of the
    same four values.  Every plan of the sweep -- whole texts of every family, own ranges, the tails with the window behind an
    unbounded prefix -- must get the same (wlo, whi, first_chunk, end_chunk) from both; a sweep that plans nothing fails."""
    out = (U64 * 4)()
    checked = {False: 0, True: 0}
    for sweep in list(W.FAMILIES) + ["own"] + list(W.TAILS):
        behind = bool(W.TAILS[sweep]["behind"]) if sweep in W.TAILS else False
        for grid in W.GRIDS:
            for case in W.cases_of(sweep, grid):
                plan = case.plan
                offset, length = plan.window
                pa.pa_chunk_range(plan.n, plan.sb, plan.se, 1, offset, offset, length, int(behind), out)
                assert tuple(out) == (plan.wlo, plan.whi, plan.first_chunk, plan.end_chunk), (case.label, tuple(out))
                assert tuple(out) == W.window_range(plan.n, plan.sb, plan.se, offset, length, behind), case.label
                checked[behind] += 1
    assert checked[False] > 500 and checked[True] > 0, checked      # fixed windows (own ranges among them) and behind


def test_chunk_range_floating_and_dense(pa):
    """The two forms the sweep does not plan: floating windows (w in [s + float_min, s + float_max]) are the fixed form with the
    two offsets apart, dense mode walks the chunks of the starts themselves."""
    out = (U64 * 4)()
    checked = 0
    for n in (0, 7, 1023, 1024, 1025, 4096 + 5, 10 ** 5):
        for sb in _starts(n):
            for se in [e for e in _starts(n) if e > sb]:
                pa.pa_chunk_range(n, sb, se, 0, 3, 7, 4, 0, out)
                assert tuple(out) == (0, 0, sb // 1024, (se + 1023) // 1024), (n, sb, se)
                for fmin, fmax in ((0, 3), (2, 7), (5, 5)):
                    pa.pa_chunk_range(n, sb, se, 1, fmin, fmax, 4, 0, out)
                    w = np.arange(sb + fmin, se + fmax, dtype=np.int64)                       # brute force, as for the blocks above
                    w = w[w + 4 <= n]
                    want = (w[0], w[-1] + 1) if len(w) else (sb + fmin, sb + fmin)
                    assert (out[0], out[1]) == want, (n, sb, se, fmin, fmax)
                    assert (out[2], out[3]) == (out[0] // 1024, (out[1] + 1023) // 1024), (n, sb, se, fmin, fmax)
                    checked += 1
    assert checked > 300


def test_the_driver_is_clean_under_the_address_and_undefined_sanitizers():
    """The same driver as a stand-alone program with its own main(): the sweeps above on small texts, written out in C++.
    (The sanitizers' runtimes are linked statically: nothing is preloaded, and nothing is loaded into Python.)"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-DPLANE_ARGS_EXEC_MAIN", "-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    assert r.stdout.decode().strip().endswith("cases")
