"""What rj_scan_records_pack costs next to the ceiling and next to what a caller would write today, in ONE run on one box:
log-like text (rejit_amd/workloads.py: log_like_torch) cut into its lines.  Per case, median and min..max of the repeats after
the warm-up calls, host clock around calls that end in a synchronise; the three ways alternate inside a repeat, so that all
see the same machine:
  pack     Scan.pack_records into a buffer of the caller's (ONE call: plan kernel, copy kernel, the summary's copy)
  copy     a device-to-device copy of the same number of bytes (Tensor.copy_ of a contiguous uint8 tensor: hipMemcpyAsync)
           -- the ceiling: every byte once in, once out, no table
  torch    the same pack from torch ops: cumsum over the lengths, repeat_interleave to a row per byte, an index gather and
           a scatter into a filled buffer
Cases:
  a  every line, fill 10, gap 1 (the text comes out as it was: its own check)
  b  every tenth line through indices
  c  the skew of tests/test_gpu_record_pack.py: one record of 64 MiB among 100 000 empty ones; a million empty records, gap 1
    python tools/probes/pack_probe.py [MiB] [repeats] [out file]     (default 1024 7 profiles/records_pack_probe.txt)"""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "records_pack_probe.txt")
WARM = 2
dev = torch.device("cuda:0")
n = mib << 20
text = W.log_like_torch(n, 5, dev)
rec_begin, rec_end = R.line_records(text)
k = rec_begin.numel()
scan = rejit_amd.Scan(rejit_amd.Program(b"the"))
lines = ["pack_probe: %d MiB of log-like text, %d line records; %d repeats after %d warm-up calls; ms, median (min .. max), GB/s of output at the median"
         % (mib, k, repeats, WARM)]


def show(ts, nbytes):
    med = float(np.median(ts))
    return "%9.3f (%8.3f .. %8.3f)  %8.1f GB/s" % (med, min(ts), max(ts), nbytes / med / 1e6 if med > 0 else 0.0)


def torch_pack(t, rb, re_, idx, fill, lead, gap):
    if idx is not None:
        rb, re_ = rb[idx], re_[idx]
    lens = re_ - rb
    step = lens + gap
    ob = lead + torch.cumsum(step, 0) - step
    total = lead + int(step.sum())
    out = torch.full((total,), fill, dtype=torch.uint8, device=t.device)
    row = torch.repeat_interleave(torch.arange(lens.numel(), device=t.device), lens)
    within = torch.arange(row.numel(), device=t.device) - (torch.cumsum(lens, 0) - lens)[row]
    out[ob[row] + within] = t[rb[row] + within]
    return out, ob, ob + lens


def case(name, t, rb, re_, idx, fill, lead, gap, with_torch=True):
    total = int(scan.pack_records(t, rb, re_, indices=idx, fill=fill, lead=lead, gap=gap)[0].numel())
    buf = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    src = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ways = [("pack", lambda: scan.pack_records(t, rb, re_, indices=idx, fill=fill, lead=lead, gap=gap, out=buf)),
            ("copy", lambda: dst.copy_(src))]
    if with_torch:
        ways.append(("torch", lambda: torch_pack(t, rb, re_, idx, fill, lead, gap)))
        got = scan.pack_records(t, rb, re_, indices=idx, fill=fill, lead=lead, gap=gap, out=buf)
        want = torch_pack(t, rb, re_, idx, fill, lead, gap)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), "the torch pack and the kernels disagree"
        del got, want
    acc = {w: [] for w, _ in ways}
    for i in range(WARM + repeats):
        for w, fn in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARM:
                acc[w].append((time.perf_counter() - t0) * 1e3)
    rows = k if idx is None and rb is rec_begin else (rb.numel() if idx is None else idx.numel())
    out = ["", "%s: %d rows, %d output bytes" % (name, rows, total)]
    for w, _ in ways:
        out.append("  %-6s %s" % (w, show(acc[w], total)))
    print("\n".join(out), flush=True)
    return out


lines += case("a  every line", text, rec_begin, rec_end, None, 10, 0, 1)
tenth = torch.arange(0, k, 10, device=dev)
lines += case("b  every tenth line (indices)", text, rec_begin, rec_end, tenth, 10, 0, 1)
big = 64 << 20
if n >= big + 100:
    sb = torch.cat([torch.full((50000,), 5, device=dev), torch.tensor([7], device=dev), torch.full((50000,), big + 50, device=dev)]).to(torch.int64)
    se = sb.clone()
    se[50000] = 7 + big
    lines += case("c1 one record of 64 MiB among 100 000 empty ones", text, sb, se, None, 10, 0, 1)
z = torch.full((1000000,), 3, dtype=torch.int64, device=dev)
lines += case("c2 a million empty records, gap 1", text, z, z, None, 10, 0, 1)

text_out = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text_out)
