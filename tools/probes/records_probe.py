"""What the per-record join costs next to the run it follows and next to the ways a caller could get the same answer:
1 GiB of log-like text (rejit_amd/workloads.py: log_like_torch) cut into its lines, a sparse pattern (a literal) and a dense one
(`[a-z]+`).  Per pattern, median and min..max of the repeats after the warm-up calls, host clock around calls that end in a
synchronise:
  (a) the whole-text run alone                                   Scan.run_tensor
  (b) run_records end to end                                     Scan.run_records = (a) + the join kernel + the summary's copy
  (c) the join and the selection alone                           (b) - (a) per repeat pair; Scan.select_records (a call: two
                                                                 memsets, the kernel, the copy of the count); the kernels' own
                                                                 durations come from a rocprofv3 --kernel-trace --stats pass
  (d) the same join as two torch.searchsorted + a subtraction    on the same device tensors (with and without making the begins
                                                                 contiguous first: torch searches a contiguous sequence)
  (e) today's route                                              spans and line table downloaded, numpy.searchsorted on the host
    python tools/probes/records_probe.py [MiB] [repeats] [out file]     (default 1024 7 profiles/records_probe.txt)"""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "records_probe.txt")
WARM = 2
dev = torch.device("cuda:0")
n = mib << 20
text = W.log_like_torch(n, 5, dev)
rec_begin, rec_end = R.line_records(text)
k = rec_begin.numel()
lines = ["records_probe: %d MiB of log-like text, %d line records; %d repeats after %d warm-up calls; ms, median (min .. max)" % (mib, k, repeats, WARM)]


def timed(fn):
    ts = []
    for i in range(WARM + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def show(ts):
    return "%9.3f (%8.3f .. %8.3f)" % (float(np.median(ts)), min(ts), max(ts))


for name, rx in (("sparse", b"the"), ("dense", b"[a-z]+")):
    scan = rejit_amd.Scan(rejit_amd.Program(rx))
    counts = torch.empty(k, dtype=torch.int32, device=dev)
    first = torch.empty(k, dtype=torch.int64, device=dev)
    # (a) and (b) alternate, so that both see the same machine
    ta, tb = [], []
    for i in range(WARM + repeats):
        for which, acc in ((0, ta), (1, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if which == 0:
                m = scan.run_tensor(text)
            else:
                res = scan.run_records(text, rec_begin, rec_end, counts=counts, first=first)
            torch.cuda.synchronize()
            if i >= WARM:
                acc.append((time.perf_counter() - t0) * 1e3)
    tc_join = [b - a for a, b in zip(ta, tb)]
    tc_sel = timed(lambda: scan.select_records())
    tc_inv = timed(lambda: scan.select_records(invert=True))
    spans = scan.spans_tensor(dev)
    key = torch.minimum(rec_end + 1, torch.cat([rec_begin[1:], rec_end[-1:] + 1]))

    def torch_join(contiguous_begins=None):
        b = spans[:, 0].contiguous() if contiguous_begins is None else contiguous_begins
        f = torch.searchsorted(b, rec_begin)
        return f, torch.searchsorted(b, key) - f

    td_all = timed(torch_join)
    begins = spans[:, 0].contiguous()
    td_search = timed(lambda: torch_join(begins))
    f, c = torch_join(begins)
    assert torch.equal(f, res.first) and torch.equal(c.to(torch.int32), res.counts), "the torch join and the kernel disagree"
    del f, c, begins

    def host_route():
        sp = scan.spans_tensor(dev).cpu().numpy()                 # 16 bytes per match over the link
        rb, re_ = rec_begin.cpu().numpy(), rec_end.cpu().numpy()  # 16 bytes per line
        kk = np.minimum(re_ + 1, np.concatenate([rb[1:], re_[-1:] + 1]))
        ff = np.searchsorted(sp[:, 0], rb)
        return ff, np.searchsorted(sp[:, 0], kk) - ff

    te = timed(host_route)
    lines += ["",
              "%s: %r -- %d matches, %d kept, %d of %d lines match, %d cross; path %s" % (
                  name, rx.decode(), res.n_matches, res.n_kept, res.n_matching, k, res.n_crossing,
                  ",".join(x for x, v in scan.stats().items() if x.endswith("_path") and v) or "general"),
              "  (a) whole-text run alone                      %s" % show(ta),
              "  (b) run_records end to end                    %s" % show(tb),
              "  (c) join: (b) - (a), pair by pair             %s" % show(tc_join),
              "  (c) select_records call                       %s   inverted %s" % (show(tc_sel), show(tc_inv)),
              "  (d) torch: begins made contiguous + 2 searchsorted + sub  %s" % show(td_all),
              "  (d) torch: 2 searchsorted + sub alone         %s" % show(td_search),
              "  (e) download spans + table, numpy.searchsorted %s" % show(te)]
    del scan, spans, counts, first, key

text_out = "\n".join(lines) + "\n"
print(text_out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text_out)
