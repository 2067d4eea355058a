"""What rj_scan_records_split costs next to the ceiling and next to what a caller would write today, in ONE run on one box:
log-like text (rejit_amd/workloads.py: log_like_torch) cut into its lines.  Per case, median and min..max of the repeats after
the warm-up calls, host clock around calls that end in a synchronise; the three ways alternate inside a repeat, so that all
see the same machine:
  split    rj_scan_records_split into tables of the caller's (ONE call: plan kernel, emit kernel, the summary's copy)
  copy     a device-to-device copy of the output's bytes (16 per piece, 8 per offset) -- the ceiling: every byte once in,
           once out, no table
  torch    the same three tables from torch ops: cumsum over the counts, repeat_interleave to a row per piece, gathers from
           the record table and the span list, where() at a row's ends; checked equal to the call's once before timing
Cases:
  a  sparse: `the`, every line, between and matches
  b  dense: `[0-9]+`, every tenth line through indices, between and matches
  c  the skew of tests/test_gpu_record_split.py: one record with 10^6 matches among 100 000 empty ones
    python tools/probes/split_probe.py [MiB] [repeats] [out file]     (default 1024 7 profiles/records_split_probe.txt)"""
import ctypes
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "records_split_probe.txt")
WARM = 2
dev = torch.device("cuda:0")
n = mib << 20
text = W.log_like_torch(n, 5, dev)
rec_begin, rec_end = R.line_records(text)
k_lines = rec_begin.numel()
lib = rejit_amd.load_library()
lines = ["split_probe: %d MiB of log-like text, %d line records; %d repeats after %d warm-up calls; ms, median (min .. max), GB/s of output at the median"
         % (mib, k_lines, repeats, WARM)]


def show(ts, nbytes):
    med = float(np.median(ts))
    return "%9.3f (%8.3f .. %8.3f)  %8.1f GB/s" % (med, min(ts), max(ts), nbytes / med / 1e6 if med > 0 else 0.0)


def torch_split(spans, rb, re_, counts, first, idx, what):
    if idx is not None:
        rb, re_, counts, first = rb[idx], re_[idx], counts[idx], first[idx]
    c = counts.to(torch.int64)
    per = c + 1 if what == "between" else c
    pf = torch.zeros(per.numel() + 1, dtype=torch.int64, device=per.device)
    pf[1:] = torch.cumsum(per, 0)
    row = torch.repeat_interleave(torch.arange(per.numel(), device=per.device), per)
    t = torch.arange(row.numel(), device=per.device) - pf[row]
    g = first[row] + t
    if what == "matches":
        return spans[g, 0], spans[g, 1], pf
    pb = torch.where(t == 0, rb[row], spans[(g - 1).clamp(min=0), 1])
    pe = torch.where(t == c[row], re_[row], spans[g.clamp(max=spans.shape[0] - 1), 0])
    return pb, pe, pf


def case(name, scan, n_text, rb, re_, res, idx, what):
    spans = scan.spans_tensor(dev)
    k = rb.numel() if idx is None else idx.numel()
    want = torch_split(spans, rb, re_, res.counts, res.first, idx, what)
    got = scan.split_records(rb, re_, res, n_text, indices=idx, what=what)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), "the torch split and the kernels disagree"
    P = int(got[0].numel())
    del got, want
    pb = torch.empty(P + 8, dtype=torch.int64, device=dev)
    pe = torch.empty(P + 8, dtype=torch.int64, device=dev)
    pf = torch.empty(k + 1, dtype=torch.int64, device=dev)
    nbytes = 16 * P + 8 * (k + 1)
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None else 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = 0 if what == "between" else 1

    def split():
        total = lib.rj_scan_records_split(scan._h, n_text, vp(rb), vp(re_), rb.numel(), vp(res.counts), vp(res.first), vp(idx), k, code, vp(pf), vp(pb),
                                          vp(pe), P, st)
        assert total == P, total
    ways = [("split", split), ("copy", lambda: dst.copy_(src)), ("torch", lambda: torch_split(spans, rb, re_, res.counts, res.first, idx, what))]
    acc = {w: [] for w, _ in ways}
    for i in range(WARM + repeats):
        for w, fn in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARM:
                acc[w].append((time.perf_counter() - t0) * 1e3)
    out = ["", "%s, %s: %d rows, %d matches in the list, %d pieces, %d output bytes" % (name, what, k, spans.shape[0], P, nbytes)]
    for w, _ in ways:
        out.append("  %-6s %s" % (w, show(acc[w], nbytes)))
    print("\n".join(out), flush=True)
    return out


scan = rejit_amd.Scan(rejit_amd.Program(b"the"))
res = scan.run_records(text, rec_begin, rec_end)
for what in ("between", "matches"):
    lines += case("a  sparse `the`, every line", scan, n, rec_begin, rec_end, res, None, what)
del scan, res
scan = rejit_amd.Scan(rejit_amd.Program(b"[0-9]+"))
res = scan.run_records(text, rec_begin, rec_end)
tenth = torch.arange(0, k_lines, 10, device=dev)
for what in ("between", "matches"):
    lines += case("b  dense `[0-9]+`, every tenth line (indices)", scan, n, rec_begin, rec_end, res, tenth, what)
del scan, res, text
blocks = 1000000
skew = torch.randint(ord("a"), ord("z") + 1, (4 * blocks + 16,), dtype=torch.uint8, device=dev)
body = skew[8:8 + 4 * blocks].view(blocks, 4)
body[:, 1], body[:, 2] = ord("@"), ord("#")
sb = torch.cat([torch.full((50000,), 2, device=dev), torch.tensor([8], device=dev), torch.full((50000,), 4 * blocks + 12, device=dev)]).to(torch.int64)
se = sb.clone()
se[50000] = 8 + 4 * blocks
scan = rejit_amd.Scan(rejit_amd.Program(b"@#"))
res = scan.run_records(skew, sb, se)
assert res.n_kept == blocks
for what in ("between", "matches"):
    lines += case("c  one record with 10^6 matches among 100 000 empty ones", scan, int(skew.numel()), sb, se, res, None, what)

text_out = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text_out)
