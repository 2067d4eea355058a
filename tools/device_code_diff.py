#!/usr/bin/env python3
"""Is the device code of two source trees the same?  Compiles every .hip unit of api.SOURCES in both trees to gfx950
assembly (the build's own flags + --cuda-device-only -S; no GPU needed), drops the lines that name __hip_cuid_ (a hash of
the unit's source text: the one difference a pure refactor leaves) and compares.  Prints `identical` or the first
differing lines per unit; exit status 1 when any unit differs.
usage: device_code_diff.py <tree before> [<tree after> = this tree] [unit.hip ...]"""
import difflib, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from rejit_amd import api

args = sys.argv[1:]
if not args:
    sys.exit(__doc__)
units = [a for a in args if a.endswith(".hip")]
trees = [os.path.abspath(a) for a in args if not a.endswith(".hip")]
if len(trees) == 1:
    trees.append(root)
units = units or [s for s in api.SOURCES if s.endswith(".hip")]
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def assembly(job):
    tree, unit, out = job
    src = os.path.join(tree, "rejit_amd", "csrc", unit)
    r = subprocess.run([hipcc] + api.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        return "compile failed: " + r.stderr[-2000:]
    with open(out) as fh:
        return [line for line in fh if "__hip_cuid_" not in line]


with tempfile.TemporaryDirectory() as tmp:
    jobs = [(t, u, os.path.join(tmp, f"{i}_{u}.s")) for u in units for i, t in enumerate(trees)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        listings = list(pool.map(assembly, jobs))
different = 0
for k, unit in enumerate(units):
    before, after = listings[2 * k], listings[2 * k + 1]
    if isinstance(before, str) or isinstance(after, str):
        different += 1
        print(f"{unit:28s} {before if isinstance(before, str) else after}")
    elif before == after:
        print(f"{unit:28s} identical ({len(after)} lines)")
    else:
        different += 1
        delta = [d for d in difflib.unified_diff(before, after, "before", "after", n=0) if not d.startswith(("---", "+++"))]
        print(f"{unit:28s} DIFFERENT ({len(before)} / {len(after)} lines); the first differences:")
        sys.stdout.writelines("    " + d for d in delta[:12])
sys.exit(1 if different else 0)
