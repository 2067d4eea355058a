#!/usr/bin/env python3
"""CPU only: the instruction mix along ONE PATH through a kernel's loop, from the compiler's assembly (hipcc -S, gfx950).
tools/isa_blocks.py counts per labelled block; a block that holds an early exit mixes two paths.  This walks the instructions
from the loop's header label back to it, taking (T) or not taking (N) every conditional branch it meets as the decision string
says, follows s_branch, and prints the branches met -- read them against the source to see that the path is the one meant --
and the classes: VALU (v_*), SALU (s_*, waits and nops included), LDS (ds_*), VMEM (global / buffer / flat / scratch).
usage: isa_path.py <file.s> <substring of the kernel's mangled name> <header label> <decisions, e.g. NTTNNNTTN> [q = no trace]
       e.g. isa_path.py pc.s plane_countINS_10ExactShapeILi2 .LBB3_20 NTTNNNTTN"""
import re, sys

if len(sys.argv) < 5:
    sys.exit(__doc__)
text = open(sys.argv[1]).read().split("\n")
want, header, dec = sys.argv[2], sys.argv[3], sys.argv[4]
quiet = len(sys.argv) > 5
start = next(i for i, l in enumerate(text) if re.match(r"^_Z\w+:", l) and want in l)
end = start
while "s_endpgm" not in text[end]:
    end += 1
body = text[start:end + 1]
label = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
pc, k, steps, trace = label[header], 0, 0, []
count = {"VALU": 0, "SALU": 0, "LDS": 0, "VMEM": 0}
while True:
    line = body[pc].split(";")[0].strip()
    pc += 1
    steps += 1
    if steps > 20000:
        sys.exit("the path does not return to " + header)
    if not line or line.startswith(".") or line.endswith(":"):
        if line.startswith(header + ":") and steps > 1:
            break
        continue
    op = line.split()[0]
    if op.startswith("v_"): count["VALU"] += 1
    elif op.startswith("s_"): count["SALU"] += 1
    elif op.startswith("ds_"): count["LDS"] += 1
    elif op.split("_")[0] in ("global", "buffer", "flat", "scratch"): count["VMEM"] += 1
    if op.startswith("s_cbranch"):
        if k >= len(dec):
            print("\n".join(trace))
            sys.exit("more conditional branches than decisions; the next one: " + line)
        trace.append("%s %s -> %s" % (op, line.split()[1], "taken" if dec[k] == "T" else "not taken"))
        k += 1
        if dec[k - 1] == "T":
            if line.split()[1] == header:
                break
            pc = label[line.split()[1]]
    elif op == "s_branch":
        trace.append("s_branch " + line.split()[1])
        if line.split()[1] == header:
            break
        pc = label[line.split()[1]]
if not quiet:
    print("\n".join(trace))
print("VALU %d  SALU %d  LDS %d  VMEM %d  total %d  (%d of %d decisions used)" % (count["VALU"], count["SALU"], count["LDS"], count["VMEM"], sum(count.values()), k, len(dec)))
