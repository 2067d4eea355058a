"""What rj_scan_records_parse_time costs, next to the number parse over rows of the same lengths and next to what a caller does
without it, in ONE run on one box.  Per case: the call into tables of the caller's, warm, timed by events around it, the median
(min .. max) of the repeats; and, in the same process and under the same shape,
  (1)  rj_scan_records_parse(RJ_PARSE_INT64, RJ_PARSE_TRIM) over as many rows of the same length at the same places (digits
       instead of a timestamp): a one-lane-per-row walk with the same loads and stores, timed the same way.  The expectation is
       parity; the margin is the min .. max spread of (1)'s own repeats.
  (2)  rj_scan_records_pack of a 10^5-row sample, the download and datetime.strptime of every row in Python (host clock, once),
       scaled to the case's rows, and checked to give the call's values.
Cases: 20-byte ISO rows `2026-10-20T17:15:00Z` under %Y-%m-%dT%H:%M:%S%z and 26-byte CLF rows `10/Oct/2000:13:55:36 -0700` under
%d/%b/%Y:%H:%M:%S %z, each as a packed column (one row per line) and as a field of longer lines (`10.0.0.1|<row>|GET /index.html
200`; the table is computed, not split), seconds, no flags.
    python tools/probes/time_probe.py [million rows] [repeats] [out file]     (default 10 20 profiles/time_probe.txt)"""
import ctypes
import datetime
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import rejit_amd

millions = float(sys.argv[1]) if len(sys.argv) > 1 else 10
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "time_probe.txt")
WARM = 3
SAMPLE = 100000
K = int(millions * 1e6)
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b","))
vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
lines = ["time_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max)" % (repeats, WARM),
         "(1) = rj_scan_records_parse(INT64, TRIM) over rows of the same length at the same places, same timing; inside (1)'s spread = the call's median is not above (1)'s max",
         "(2) = pack + download + datetime.strptime of a %d-row sample on the host, once, scaled to the rows" % SAMPLE,
         "", "| case | rows | ok | row bytes | call ms (min .. max) | rows/us | (1) int64 parse ms (min .. max) | call / (1) | inside (1)'s spread | (2) ms, scaled | (2) / call |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]


def timed(call):
    ts = []
    for i in range(WARM + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = call()
        e1.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append(e0.elapsed_time(e1))
    return rc, float(np.median(ts)), min(ts), max(ts)


gen = torch.Generator(device=dev).manual_seed(1970)
rand = lambda lo, hi: torch.randint(lo, hi, (K,), device=dev, generator=gen)
two = lambda x: [(x // 10) % 10 + 48, x % 10 + 48]
lit = lambda c: [torch.full((K,), ord(c), dtype=torch.int64, device=dev)]
year, month, day, hour, minute, second = rand(1970, 2038), rand(1, 13), rand(1, 29), rand(0, 24), rand(0, 60), rand(0, 60)
year4 = [(year // 1000) % 10 + 48, (year // 100) % 10 + 48] + two(year % 100)
names = torch.from_numpy(np.frombuffer(b"JanFebMarAprMayJunJulAugSepOctNovDec", dtype=np.uint8).copy()).to(dev).to(torch.int64).reshape(12, 3)
offset = rand(-12, 13)
iso_cols = year4 + lit("-") + two(month) + lit("-") + two(day) + lit("T") + two(hour) + lit(":") + two(minute) + lit(":") + two(second) + lit("Z")
clf_cols = (two(day) + lit("/") + [names[month - 1, i] for i in range(3)] + lit("/") + year4 + lit(":") + two(hour) + lit(":") + two(minute) + lit(":") + two(second)
            + lit(" ") + [torch.where(offset < 0, 45, 43)] + two(offset.abs()) + two(torch.zeros_like(offset)))


def laid(cols, lead, tail):
    """rows (a list of K-element byte columns) between `lead` and `tail` bytes on every line -> (text, begin, end)"""
    width = len(cols)
    mat = torch.empty((K, len(lead) + width + len(tail)), dtype=torch.uint8, device=dev)
    mat[:, :len(lead)] = torch.from_numpy(np.frombuffer(lead, dtype=np.uint8).copy()).to(dev) if lead else 0
    mat[:, len(lead):len(lead) + width] = torch.stack(cols, dim=1).to(torch.uint8)
    mat[:, len(lead) + width:] = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).to(dev)
    begin = (torch.arange(K, dtype=torch.int64, device=dev) * mat.shape[1] + len(lead)).contiguous()
    return mat.reshape(-1).contiguous(), begin, (begin + width).contiguous()


def case(name, cols, fmt, lead, tail):
    text, rb, re_ = laid(cols, lead, tail)
    k, n, width = K, int(text.numel()), len(cols)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    values, status = scan.parse_time_records(text, rb, re_, fmt, unit="s")
    d_value = torch.empty(k, dtype=torch.int64, device=dev)
    d_status = torch.empty(k, dtype=torch.uint8, device=dev)
    n_ok, med, lo, hi = timed(lambda: lib.rj_scan_records_parse_time(scan._h, vp(text), n, vp(rb), vp(re_), k, None, 0, fmt, len(fmt), 0, 0, vp(d_value), vp(d_status),
                                                                    None, st))
    assert n_ok == k == int((status == 0).sum()), lib.rj_last_error()
    assert torch.equal(d_value, values) and torch.equal(d_status, status)
    # (2) pack, download, strptime on the host: a sample, scaled
    sample = torch.arange(0, k, max(k // SAMPLE, 1), dtype=torch.int64, device=dev)[:SAMPLE].contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    packed, _, _ = scan.pack_records(text, rb, re_, indices=sample, fill=10, lead=0, gap=1)
    words = packed.cpu().numpy().tobytes().split(b"\n")
    words.pop()
    epoch = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
    py_fmt = fmt.decode()
    host = np.array([(datetime.datetime.strptime(w.decode(), py_fmt) - epoch) // datetime.timedelta(seconds=1) for w in words], dtype=np.int64)
    host_ms = (time.perf_counter() - t0) * 1e3 * (k / len(words))
    assert (host == values[sample].cpu().numpy()).all(), "the host route and the call disagree"
    del packed, words, host, values, status
    # (1) the number parse over digits at the same places
    digits = text.clone()
    place = torch.arange(width, device=dev).unsqueeze(0)
    rows_at = (rb.unsqueeze(1) + place).reshape(-1)
    digits[rows_at] = (torch.randint(0, 10, (k * width,), device=dev, generator=gen) * (place >= width - 9).expand(k, width).reshape(-1) + 48).to(torch.uint8)
    del rows_at
    p_ok, p_med, p_lo, p_hi = timed(lambda: lib.rj_scan_records_parse(scan._h, vp(digits), n, vp(rb), vp(re_), k, None, 0, 0, 1, vp(d_value), vp(d_status), None, st))
    assert p_ok == k, lib.rj_last_error()
    line = "| %s | %d | %d | %d | %.3f (%.3f .. %.3f) | %.0f | %.3f (%.3f .. %.3f) | %.2f | %s | %.0f | %.0fx |" % (
        name, k, n_ok, width, med, lo, hi, k / med / 1e3, p_med, p_lo, p_hi, med / p_med, "yes" if med <= p_hi else "NO", host_ms, host_ms / med)
    print(line, flush=True)
    lines.append(line)


ISO, CLF = b"%Y-%m-%dT%H:%M:%S%z", b"%d/%b/%Y:%H:%M:%S %z"
case("ISO 20 bytes, packed column", iso_cols, ISO, b"", b"\n")
case("ISO 20 bytes, field of a line", iso_cols, ISO, b"10.0.0.1|", b"|GET /index.html 200\n")
case("CLF 26 bytes, packed column", clf_cols, CLF, b"", b"\n")
case("CLF 26 bytes, field of a line", clf_cols, CLF, b"10.0.0.1|", b"|GET /index.html 200\n")

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
