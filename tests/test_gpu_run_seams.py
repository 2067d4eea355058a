"""GPU tests (-m gpu): the seams and the resolve levels of the run and pair kernels (rejit_amd/csrc/run_scan.hip), swept on small texts.

The suite's other texts leave most of these kernels' geometry alone: a text below 8 MiB has at most 1024 tiles, so every thread of the
one-level resolve owns one tile; the two-level resolve and the 32-KiB tile need texts of 32 MiB and 256 MiB.  RJ_RUN_TILE_KB forces
the tile length (2 KiB: one iteration, no prefetch; 4 and 8 KiB; 32 KiB: sixteen iterations) and RJ_RUN_TWO_LEVELS the two-level
resolve in blocks of that many tiles; RJ_NO_SMALL keeps the one-workgroup kernel out of the way and RJ_RUNS_FIRST sends the run
shapes to the run kernels first.  tests/run_sweep.py plans the texts -- a motif across every seam of every class at every offset,
own ranges and carries cut at the seams, sequences of tile kinds across every class of resolve seam (tests/test_run_sweep_plan.py
asserts that coverage without a GPU) -- and, as a child process (the library reads the variables once), compares Scan.run + spans(),
the return count and Scan.count with the oracle, exactly, and the library's own geometry with the planner's.  One child at a time;
nothing is launched in this process.

A failing seam has an address: the child prints configuration, family, pattern, n, seam class and offset (or the tile and its
neighbours' kinds), got and want."""
import os
import subprocess
import sys
import time

import pytest

import run_sweep as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWEEP = os.path.join(HERE, "run_sweep.py")
# a child's limit, the value of tests/test_gpu_seams.py and tests/test_gpu_window_seams.py: more than five times the slowest child measured
# on an MI355X (level:runsA under blocks of 300 tiles: 3.7 s with process start, library load, planning and oracle; the smallest child takes
# 2.1 s, the anchor 3.4 s; all 50 children 149 s).  A child that grows beyond 4 s is split (run_sweep.INTRA_GROUPS / OWN_GROUPS /
# LEVEL_GROUPS / LEVEL_SPLIT), the limit stays.
TIMEOUT = 20
FAULT_STATUS = (134, 139, -6, -11, 124, 137)
_faulted = []       # the first child that ended by time-out or with a fault's status: nothing more is started on the GPU


def run_child(sweep, config, want_texts):
    assert not _faulted, "not run: an earlier child faulted (%s)" % _faulted[0]
    env = dict(os.environ)
    for k in (R.ENV_TILE, R.ENV_LEVELS, "RJ_NO_SMALL", "RJ_RUNS_FIRST", "RJ_NO_PAIRS", "RJ_NO_WINDOW_RUNS", "RJ_BOL_DENSE_GENERAL", "RJ_SCAN_GRID"):
        env.pop(k, None)
    env.update(R.config_env(config))
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, SWEEP, sweep, config], env=env, capture_output=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _faulted.append("%s %s: time-out" % (sweep, config))
        raise
    out = r.stdout.decode(errors="replace")
    print("%s %s: %.1f s\n%s" % (sweep, config, time.time() - t0, out[-3000:]))
    if r.returncode in FAULT_STATUS:
        _faulted.append("%s %s: status %d" % (sweep, config, r.returncode))
    assert r.returncode == 0, (r.returncode, out[-3000:], r.stderr.decode(errors="replace")[-2000:])
    last = out.strip().splitlines()[-1]
    assert last == "checked %d texts, mismatches 0" % want_texts, out[-2000:]


@pytest.mark.parametrize("sweep,config", R.sweeps())
def test_run_seams(sweep, config):
    want = R.text_count(sweep, config)
    assert want > 0
    run_child(sweep, config, want)


def test_anchor_at_the_production_geometry():
    """No override: a text just above 32 MiB has more than 4096 tiles of 8 KiB and gets the two-level resolve with blocks of 1024
    tiles from launch_run_resolve / launch_pair_resolve themselves (the child asserts that through the library's accessor).  Tile
    kinds across the block seams, and across chunk and workgroup seams spread over the text, one run pattern and one pair pattern
    against the oracle: the forced configurations reproduce the production path, they do not replace it."""
    run_child("anchor", "anchor", len(R.ANCHOR_FAMILIES))
