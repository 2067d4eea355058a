"""GPU tests (-m gpu): the seams of the plane kernels' streaming loop (rejit_amd/csrc/plane_count.hip), swept on small texts.

scan_geometry() gives every text below 2 MiB one 2-KiB block per wave, so the tests of tests/test_gpu_counts.py run the
kernel's prologue and its odd-block arm and nothing else.  RJ_SCAN_GRID forces the workgroup count: with a grid of 1 a
128-KiB text is dealt out as 16 blocks per wave, the production span length of every text from 32 MiB up, and the plain-C
oracle answers in milliseconds.  tests/seam_sweep.py plans the texts (one planted string across every seam of every class,
at every offset; tests/test_seam_plan.py asserts that coverage without a GPU) and, as a child process -- the library
reads the variable once --, compares the counts-only run, its bounds and the span lists of a default run with the oracle.
One child at a time; nothing is launched in this process.

A failing seam has an address: the child prints family, n, grid, seam class, offset, pattern, got and want."""
import os
import subprocess
import sys
import time

import pytest

import seam_sweep as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWEEP = os.path.join(HERE, "seam_sweep.py")
# a child's limit: about five times the slowest case measured on an MI355X (pairs, grid 3: 3.5 s with process start,
# library load, planning and oracle)
TIMEOUT = 20

SWEEPS = list(S.FAMILIES) + ["own", "busy", "busy7", "pairs", "pairs_general", "void", "single"]


def run_child(family, grid):
    env = dict(os.environ)
    for k in ("RJ_SCAN_GRID", "RJ_COUNT_BATCH", "RJ_NO_SMALL"):
        env.pop(k, None)
    if grid is not None:
        env["RJ_SCAN_GRID"] = str(grid)
    if family == "busy7":
        env["RJ_COUNT_BATCH"] = "7"     # partial batches arrive mid-span: the prev_rel / ends[] carry at every batch edge
    if family == "single":
        env["RJ_NO_SMALL"] = "1"        # (texts this small would take the one-workgroup kernel)
    t0 = time.time()
    r = subprocess.run([sys.executable, SWEEP, family], env=env, capture_output=True, timeout=TIMEOUT)
    out = r.stdout.decode(errors="replace")
    print("%s grid %s: %.1f s\n%s" % (family, grid, time.time() - t0, out[-3000:]))
    assert r.returncode == 0, (out[-3000:], r.stderr.decode(errors="replace")[-2000:])
    last = out.strip().splitlines()[-1]
    assert last.startswith("checked ") and last.endswith("mismatches 0") and not last.startswith("checked 0 "), out[-2000:]


@pytest.mark.parametrize("grid", S.GRIDS)
@pytest.mark.parametrize("family", SWEEPS)
def test_seams(family, grid):
    run_child(family, grid)


def test_anchor_at_the_production_geometry():
    """No override: a text of ~34 MiB gets its 16- and 17-block spans from scan_geometry itself.  regexdna strings across
    the P, B01, B12, BH and S seams the planner computes for that geometry, checked against a sliding compare in torch:
    the forced grid reproduces the production loop, it does not replace it."""
    run_child("anchor", None)
