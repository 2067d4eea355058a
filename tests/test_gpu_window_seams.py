"""GPU tests (-m gpu): the seams of the window scan's streaming loop (rejit_amd/csrc/scan_windows.hip), swept on small texts.

scan_geometry() gives every text below 1 MiB one 1-KiB chunk per wave, so the suite's small texts never enter the kernel's
four-buffer pipeline, its epilogue or the plain loop behind it.  RJ_SCAN_GRID forces the workgroup count: under a grid of 1 to 3
a text of at most 140 KiB is dealt out in spans of up to 35 chunks, and RJ_NO_SMALL keeps the one-workgroup kernel out of the
way.  tests/window_sweep.py plans the texts (one planted string across every seam of every class at every offset, for every
kernel variant and K class; tests/test_window_sweep_plan.py asserts that coverage without a GPU) and, as a child process -- the
library reads the variables once --, compares Scan.run + spans(), the return count and Scan.count with the oracle, exactly.
One child at a time; nothing is launched in this process.

A failing seam has an address: the child prints family, pattern, n, grid, seam class, role, offset, got and want."""
import os
import subprocess
import sys
import time

import pytest

import window_sweep as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWEEP = os.path.join(HERE, "window_sweep.py")
# a child's limit, the value of tests/test_gpu_seams.py: about six times the slowest case measured on an MI355X (own, grid 3:
# 3.4 s with process start, library load, planning and oracle; a family's child takes 2.0 - 3.0 s)
TIMEOUT = 20
FAULT_STATUS = (134, 139, -6, -11, 124, 137)
_faulted = []       # the first child that ended by time-out or with a fault's status: nothing more is started on the GPU


def run_child(sweep, grid, want_texts):
    assert not _faulted, "not run: an earlier child faulted (%s)" % _faulted[0]
    env = dict(os.environ)
    for k in ("RJ_SCAN_GRID", "RJ_COUNT_BATCH", "RJ_NO_SMALL"):
        env.pop(k, None)
    if grid is not None:
        env["RJ_SCAN_GRID"] = str(grid)
        env["RJ_NO_SMALL"] = "1"        # (texts this small would take the one-workgroup kernel)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, SWEEP, sweep], env=env, capture_output=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _faulted.append("%s grid %s: time-out" % (sweep, grid))
        raise
    out = r.stdout.decode(errors="replace")
    print("%s grid %s: %.1f s\n%s" % (sweep, grid, time.time() - t0, out[-3000:]))
    if r.returncode in FAULT_STATUS:
        _faulted.append("%s grid %s: status %d" % (sweep, grid, r.returncode))
    assert r.returncode == 0, (r.returncode, out[-3000:], r.stderr.decode(errors="replace")[-2000:])
    last = out.strip().splitlines()[-1]
    assert last == "checked %d texts, mismatches 0" % want_texts, out[-2000:]


@pytest.mark.parametrize("grid", W.GRIDS)
@pytest.mark.parametrize("sweep", W.SWEEPS)
def test_window_seams(sweep, grid):
    want = W.text_count(sweep, grid)
    assert want > 0
    run_child(sweep, grid, want)


def test_anchor_at_the_production_geometry():
    """No override: a text of 34 MiB gets its spans of 32 chunks from scan_geometry itself (the child asserts that).  Three
    patterns -- nibble, two-level, one dword -- across the pipeline, epilogue and span seams the planner computes for that
    geometry, checked against a sliding compare in torch: the forced grid reproduces the production loop, it does not replace it."""
    run_child("anchor", None, 1)
