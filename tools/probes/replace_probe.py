"""What rj_scan_records_replace costs next to the whole-text replace it stands beside and next to the ceiling, in ONE run on one
box: log-like text (rejit_amd/workloads.py: log_like_torch) cut into its lines.  Per case, median and min..max of the repeats after
the warm-up calls, host clock around calls that end in a synchronise; the ways alternate inside a repeat, so that all see the
same machine:
  records  Scan.replace_records of every line into a buffer of the caller's (ONE call: table, plan and copy kernels)
  whole    Scan.replace (rj_scan_replace, replace_gather) of the same text and pattern -- the comparison
  copy     a device-to-device copy of the records' output size (Tensor.copy_: hipMemcpyAsync) -- the ceiling
Cases:
  a  a sparse pattern: `the` -> `THE`
  b  a dense pattern: `[0-9]+` -> `#`
  c  one record with 10^6 matches: 16 MB with `@#` every 16 bytes, -> `XYZ` (no `whole` beside it: records and copy only)
    python tools/probes/replace_probe.py [MiB] [repeats] [out file]     (default 1024 7 profiles/records_replace_probe.txt)"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import rejit_amd
from rejit_amd import records as R
from rejit_amd import workloads as W

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "records_replace_probe.txt")
WARM = 2
dev = torch.device("cuda:0")
n = mib << 20
text = W.log_like_torch(n, 5, dev)
rec_begin, rec_end = R.line_records(text)
lines = ["replace_probe: %d MiB of log-like text, %d line records; %d repeats after %d warm-up calls; ms, median (min .. max), GB/s of output at the median"
         % (mib, rec_begin.numel(), repeats, WARM)]


def show(ts, nbytes):
    med = float(np.median(ts))
    return "%9.3f (%8.3f .. %8.3f)  %8.1f GB/s" % (med, min(ts), max(ts), nbytes / med / 1e6 if med > 0 else 0.0)


def case(name, t, rb, re_, pattern, repl, whole=True):
    scan = rejit_amd.Scan(rejit_amd.Program(pattern))
    res = scan.run_records(t, rb, re_)
    total = int(scan.replace_records(t, rb, re_, res, repl, fill=10, lead=0, gap=1)[0].numel())
    buf = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    src = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream().cuda_stream
    ways = [("records", lambda: scan.replace_records(t, rb, re_, res, repl, fill=10, lead=0, gap=1, out=buf))]
    if whole:
        cap = int(t.numel()) + res.n_matches * len(repl) + 64
        wbuf = torch.empty(cap, dtype=torch.uint8, device=dev)
        ways.append(("whole", lambda: scan.replace(t.data_ptr(), int(t.numel()), repl, wbuf.data_ptr(), cap, stream=st)))
    ways.append(("copy", lambda: dst.copy_(src)))
    acc = {w: [] for w, _ in ways}
    for i in range(WARM + repeats):
        for w, fn in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARM:
                acc[w].append((time.perf_counter() - t0) * 1e3)
    out = ["", "%s: %d rows, %d matches, %d output bytes" % (name, rb.numel(), res.n_matches, total)]
    for w, _ in ways:
        out.append("  %-8s %s" % (w, show(acc[w], total)))
    print("\n".join(out), flush=True)
    return out


lines += case("a  sparse: `the` -> `THE`, every line", text, rec_begin, rec_end, b"the", b"THE")
lines += case("b  dense: `[0-9]+` -> `#`, every line", text, rec_begin, rec_end, b"[0-9]+", b"#")
big = 16 * 1000000
skew = torch.randint(ord("a"), ord("z") + 1, (big,), dtype=torch.uint8, device=dev)
blocks = skew.view(-1, 16)
blocks[:, 5], blocks[:, 6] = ord("@"), ord("#")
one_b = torch.zeros(1, dtype=torch.int64, device=dev)
one_e = torch.full((1,), big, dtype=torch.int64, device=dev)
lines += case("c  one record with 10^6 matches: `@#` -> `XYZ`", skew, one_b, one_e, b"@#", b"XYZ", whole=False)

text_out = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text_out)
