"""GPU tests (-m gpu): the filter of the plane kernels (rejit_amd/csrc/plane_count.hip) behind its three-input network.

"At most one of the window's eight codes differs from a base" is a network of nine v_bitop3_b32 per base (plane_network.h), the
planes it reads are formed from whole words, and a block's codes are joined by one hand-written statement.  What such a change
can break is a FALSE NEGATIVE of the filter: a window one code off a base that no longer becomes a candidate, and then is not
counted.  So the plants are the whole set of strings within one byte of a base -- all 50 of regexdna's two bases (ExactShape<2>,
ListShape<2>), the 25 of `agggtaaa` (ExactShape<1>, ListShape<1>) --, not a rotation of it, and EVERY one of them stands, in
every geometry, with its window starting
  A    inside a lane's piece A,                              B    inside a lane's piece B,
  LA   1..7 bytes before the end of a lane's piece A,        LB   ... of a lane's piece B (the window reads the lane above),
  AB   1..7 bytes before the end of lane 63's piece A (followed by lane 0's piece B),
  BN   1..7 bytes before the end of lane 63's piece B, the next block a fast block of the same span,
  BH   1..7 bytes before the end of a span's last fast block (followed by the `behind` stand-in),
  G    in a guarded block (the `test<true>` call).
The distance to the boundary rotates over 1..7 with the slot and the text.  A fast block holds twelve plants; the four BH places of
a text take four strings per text, so a group runs ceil(strings / 4) texts.  One general family with tolerance (`one_base`:
GeneralShape<1, 8, true>, GeneralListShape<true>) goes through the same placements for general_test.

Counts, bounds and span lists are compared with the plain-C oracle by tests/seam_sweep.py's driver, which requires the counts path
(return value 3).  The means are those of tests/test_gpu_stash_ring.py: RJ_SCAN_GRID=1 (four waves), texts of 64 blocks less 1000
bytes (spans of 16 blocks; the last wave: 14 fast blocks, a guarded full block, a partial one) and of 60 blocks (spans of 15: the
loop's odd-block arm; one guarded block that ends with the text), one child process per group, one child at a time.

  python tests/test_gpu_plane_network.py GROUP     the child"""
import os
import subprocess
import sys
import time

import pytest

import seam_sweep as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 30
BLOCK, PIECE = S.BLOCK, S.PIECE
N_EVEN = 64 * BLOCK - 1000
N_ODD = 60 * BLOCK
CLASSES = ("A", "B", "LA", "LB", "AB", "BN", "BH", "G")
GROUPS = ["%s_%s" % (f, g) for f in ("dna9", "dna1", "one_base") for g in ("even", "odd")]


def strings_of(family):
    if family == "dna9":
        return S._one_off([b"agggtaaa", b"tttaccct"], b"acgt")
    if family == "dna1":
        return S._one_off([b"agggtaaa"], b"acgt")
    return list(S.FAMILIES[family]["plants"])


def slots_of(plan, n):
    """{class: [(block base, offset of the boundary or of the window inside the block, crossing)]} in text order; crossing: the
    window starts 1..7 bytes BEFORE the offset, else 0..7 bytes behind it (inside one lane's piece: 16 L + 0..7 + 8 <= 16 L + 16)"""
    out = {c: [] for c in CLASSES}
    for w in plan.waves:
        for c in range(w.c0, w.fast_end):
            base = c * BLOCK
            for lane in (2, 10, 18):
                out["A"].append((base, 16 * lane, False))
            for lane in (6, 14, 22):
                out["B"].append((base, PIECE + 16 * lane, False))
            for lane in (30, 40):
                out["LA"].append((base, 16 * (lane + 1), True))
            for lane in (34, 44):
                out["LB"].append((base, PIECE + 16 * (lane + 1), True))
            out["AB"].append((base, PIECE, True))
            out["BN" if c + 1 < w.fast_end else "BH"].append((base, BLOCK, True))
        for c in range(w.fast_end, w.c1):
            base = c * BLOCK
            for at in range(40, BLOCK, 40):   # (the block's first bytes may end a window that began in the block before)
                if base + at + 16 <= n:
                    out["G"].append((base, at, False))
    return out


def text_of(family, n, plan, strings, r):
    """Text r of a group: class by class the slots take the strings in turn (BH: four per text, continued from text to text)."""
    bg = S.pick_background(strings, 8)[0]
    text = bytearray([bg]) * n
    plants, seen = [], {}
    for cls, slots in slots_of(plan, n).items():
        first = r * len(slots) if cls == "BH" else r
        for i, (base, at, crossing) in enumerate(slots):
            k = (first + i) % len(strings)
            d = 1 + (i + r) % 7
            start = base + at - d if crossing else base + at + (i + r) % 8
            s = strings[k]
            assert start >= 0 and start + len(s) <= n and bytes(text[start:start + len(s)]) == bytes([bg]) * len(s), (cls, start)
            text[start:start + len(s)] = s
            plants.append((start, s, (cls,), base + at))
            seen.setdefault(cls, set()).add(k)
    plants.sort()
    return S.Case("%s n=%d text %d" % (family, n, r), plan, bytes(text), plants, expect_how=3), seen


def group_cases(group):
    """-> (patterns, cases) of one child; every string stands in every class (checked here, not assumed)"""
    family, _, geometry = group.rpartition("_")
    n = N_ODD if geometry == "odd" else N_EVEN
    plan = S.Plan(n, None, 1, 0, 0, 8)
    strings = strings_of(family)
    n_bh = len(slots_of(plan, n)["BH"])
    assert n_bh == 4, n_bh   # (three spans that end inside the text, and the last span's last fast block before its guarded one)
    cases, covered = [], {}
    for r in range((len(strings) + n_bh - 1) // n_bh):
        case, seen = text_of(family, n, plan, strings, r)
        cases.append(case)
        for cls, ks in seen.items():
            covered.setdefault(cls, set()).update(ks)
    for cls in CLASSES:
        assert covered.get(cls) == set(range(len(strings))), (group, cls, sorted(set(range(len(strings))) - covered.get(cls, set())))
    return S.FAMILIES[family]["rx"], cases


def child(group):
    assert os.environ.get("RJ_SCAN_GRID") == "1", "RJ_SCAN_GRID=1 must be set"
    sys.path.insert(0, HERE)
    from checkers import Oracle
    oracle = Oracle()
    rep = S.Report("plane_network:" + group, 1)
    be = S.GpuBackend()
    rxs, cases = group_cases(group)
    S.check_multi(rep, be, oracle, rxs, cases, window=(0, 0, 8))
    rep.done()


@pytest.mark.parametrize("group", GROUPS)
def test_plane_network(group):
    env = dict(os.environ)
    for k in ("RJ_COUNT_BATCH", "RJ_NO_SMALL"):
        env.pop(k, None)
    env["RJ_SCAN_GRID"] = "1"
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=env, capture_output=True, timeout=TIMEOUT)
    out = r.stdout.decode(errors="replace")
    print("%s: %.1f s\n%s" % (group, time.time() - t0, out[-3000:]))
    assert r.returncode == 0, (out[-3000:], r.stderr.decode(errors="replace")[-2000:])
    last = out.strip().splitlines()[-1]
    assert last.startswith("checked ") and last.endswith("mismatches 0") and not last.startswith("checked 0 "), out[-2000:]


if __name__ == "__main__":
    child(sys.argv[1])
