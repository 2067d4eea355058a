"""GPU tests (-m gpu): the capture stash of the exact count kernels (rejit_amd/csrc/plane_count.hip) as ONE ring of 4 KiB.

A candidate takes its 8 bytes from the wave's stash of the last two blocks; the bytes behind a block are the head of the other
slot -- written there by the stash of the block that follows or, where that block is not stashed (behind the span's last fast
block, behind a guarded block), by a stand-in of 8 bytes.  A window that crosses such a place is right only if the FOLLOWER'S
BYTES arrived: every placement below is run twice, once with a regexdna string across the boundary (it must count) and once
with one byte of the string's part BEHIND the boundary replaced by a byte of the same 2-bit code (`A` for `a`: still a
candidate of the scan, no match of any pattern; it must not count).  Counts, bounds and span lists are compared with the
plain-C oracle by tests/seam_sweep.py's driver.

The means are those of tests/test_gpu_seams.py: RJ_SCAN_GRID=1 and texts of about 128 KiB (spans of 16 and of 15 blocks, so
that the loop leaves both through `c + 2 == fast_end` and through its odd-block arm, with spans that begin at even and at odd
blocks), one child process per group (the library reads the variable once), one child at a time, 20 s each.

  python tests/test_gpu_stash_ring.py GROUP     the child"""
import os
import subprocess
import sys
import time

import pytest

import seam_sweep as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 20
BLOCK = S.BLOCK

# 16 blocks per wave; the last wave: 14 fast blocks, the last full block (guarded), a partial block of 1048 bytes
N_EVEN = 64 * BLOCK - 1000
# 15 blocks per wave (spans begin at blocks 0, 15, 30, 45): waves 0..2 leave through the odd-block arm into `behind`; the last
# wave: 14 fast blocks and a guarded full block that ends with the text
N_ODD = 60 * BLOCK
OFFSETS = range(-7, 1)          # the string's start relative to the boundary: 7 ... 1 bytes before it, and at it
CROSSED = ("B01", "B12", "BH1", "BH2", "SW", "SG", "GF", "GG", "P", "GE")
DNA1_RX = S.FAMILIES["dna1"]["rx"]
# (a group = one child: a kind of placement and a geometry, `even` or `odd`; own_end: the own range's end before / behind the boundary)
GROUPS = ["%s_%s" % (k, g) for k in ("dna9", "dna1", "single", "two_in_lane", "pair7") for g in ("even", "odd")] + ["own_end_before", "own_end_behind"]


def alias(s, j):
    """byte j in upper case: the same 2-bit code under the scan's shift, another byte"""
    assert s[j:j + 1].islower()
    return s[:j] + s[j:j + 1].upper() + s[j + 1:]


def seams_of(plan, tags=CROSSED):
    return [(pos, t) for pos, t in plan.seams() if set(t) & set(tags)]


def placed(n, grid_plan, strings, d, variant, lead=0, seams=None, own=None, expect_how=3, label=""):
    """One string at every boundary, its window of interest starting at boundary + d (lead: bytes of the string before that
    window); variant None: all exact, 0 / 1: the plants of that parity carry an alias byte behind the boundary."""
    bg = S.pick_background(S.FAMILIES["dna9"]["plants"], 8)[0]
    text = bytearray([bg]) * n
    plants = []
    for i, (pos, tags) in enumerate(seams if seams is not None else seams_of(grid_plan)):
        s = strings[(i + d) % len(strings)]
        at_end = tags == ("GE",)
        start = (n - len(s) + d) if at_end else pos + d - lead
        if start < 0 or start + len(s) > n:
            continue
        if variant is not None and i % 2 == variant:
            first_behind = len(s) - 1 if at_end else lead - d      # the first byte of the string at or behind the boundary
            s = alias(s, first_behind if i % 4 < 2 else len(s) - 1)
        text[start:start + len(s)] = s
        plants.append((start, s, tags, pos))
    return S.Case("%s n=%d d=%d variant=%s" % (label, n, d, variant), grid_plan, bytes(text), plants, own=own, expect_how=expect_how)


def group_cases(group):
    """-> (patterns, cases) of one child"""
    dna9 = S.FAMILIES["dna9"]["plants"]
    dna1 = S.FAMILIES["dna1"]["plants"]
    cases = []
    group, _, geometry = group.rpartition("_")
    n = N_ODD if geometry == "odd" else N_EVEN
    plan = S.Plan(n, None, 1, 0, 0, 8)
    if group == "dna9":
        for d in OFFSETS:
            for variant in (None, 0, 1):
                cases.append(placed(n, plan, dna9, d, variant, label=group))
        return S.DNA9, cases
    if group in ("dna1", "single"):       # ExactShape<1>: the `agggtaaa` halves of the nine / `agggtaaa` alone
        strings = dna1 if group == "dna1" else [b"agggtaaa"]
        for d in OFFSETS:
            for variant in (None, d & 1):
                cases.append(placed(n, plan, strings, d, variant, label=group))
        return (DNA1_RX if group == "dna1" else [b"agggtaaa"]), cases
    if group == "two_in_lane":
        # 16 bytes = two matches 8 apart; the second begins at boundary + d, so for d < 0 both begin in ONE 16-byte piece (lane
        # 63's, or the last lane's of piece A) and the second crosses; the alias byte lies in the second
        strings = [b"agggtaaatttaccct", b"tttaccctagggtaaa", b"cgggtaaatttacccg"]
        for d in OFFSETS:
            for variant in (None, d & 1):
                cases.append(placed(n, plan, strings, d, variant, lead=8, label=group))
        return S.DNA9, cases
    if group == "pair7":
        # two candidates 7 bytes apart that share a pattern (the second is dropped: the ring's ORDER decides which), the first
        # at boundary + d - 4: before, across and -- its partner -- behind the boundary.  Across a span seam the documented
        # answer is a void run that the span pipeline answers: those placements only compare the counts.
        strings = [b"agggtaaagggtaaa", b"tttaccctttaccct"]
        inner = [s for s in seams_of(plan) if not (set(s[1]) & {"SW", "SG", "GE"})]
        outer = [s for s in seams_of(plan) if set(s[1]) & {"SW", "SG"}]
        for d in OFFSETS:
            cases.append(placed(n, plan, strings, d, None, lead=4, seams=inner, label=group))
            cases.append(placed(n, plan, strings, d, None, lead=4, seams=outer, expect_how=None, label=group + " at span seams"))
        return S.DNA9, cases
    if group == "own_end":
        # an own range that ends inside the crossing window: 3 bytes before the boundary behind a span's last fast block (the
        # starts at boundary - 7 ... - 4 count, the others do not), and 2 bytes behind it (the block behind the boundary is a
        # span block with two window positions)
        edge = 20 * BLOCK
        own = (0, edge - 3 if geometry == "before" else edge + 2)
        seams = [s for s in seams_of(plan) if s[0] <= edge + BLOCK]
        for d in OFFSETS:
            for variant in (None, d & 1):
                cases.append(placed(n, S.Plan(n, own, 1, 0, 0, 8), dna9, d, variant, seams=seams, own=own, label="%s %s" % (group, own)))
        return S.DNA9, cases
    raise KeyError(group)


def child(group):
    assert os.environ.get("RJ_SCAN_GRID") == "1", "RJ_SCAN_GRID=1 must be set"
    sys.path.insert(0, HERE)
    from checkers import Oracle
    oracle = Oracle()
    rep = S.Report("stash_ring:" + group, 1)
    be = S.GpuBackend()
    rxs, cases = group_cases(group)
    S.check_multi(rep, be, oracle, rxs, cases, window=(0, 0, 8))
    rep.done()


@pytest.mark.parametrize("group", GROUPS)
def test_stash_ring(group):
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
