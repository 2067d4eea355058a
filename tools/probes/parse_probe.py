"""What rj_scan_records_parse costs, next to the bytes it must move and next to what a caller does without it, in ONE run on one
box.  Per case: the call into tables of the caller's, warm, timed by events around it, the median (min .. max) of the repeats;
and, in the same process,
  (chk) the same call over a table whose LAST row is bad: the refused call, that is the row-check pass, the parse kernel's
        immediate return and the synchronise -- what the check-first refusal scheme costs;
  (i)   rj_scan_records_group over the same table (one call, group_cap 0: it writes d_group), timed the same way: it reads the
        same rows and then does strictly more (inserts, a unit scan, wider outputs), so the parse has to be below it;
  (ii)  rj_scan_records_pack of the table, the download, int() / float() of every row in Python (host clock, once), checked to
        give the call's values on the rows the call reads.
The model: per row the two table entries twice (check pass and parse pass: 32 bytes), the row's bytes once, 8
bytes of value and 1 of status.  The share of the 6.9 TB/s read-only rate (README) is a recorded figure, not a promise.
Cases:
  a  10^7 lines `kNNN,<1..12 digits>,x`: field 2 of the lines split at `,` (run_records + split_records + field_records), int64
  b  10^7 rows D+.DDD (1..8 digits before the point), one per line, float64
  c  the table of a with every fourth row spoilt (a letter for its last digit), int64
  d  10^5 rows of 4 KiB: zeros, then 16 digits, int64
    python tools/probes/parse_probe.py [million rows] [repeats] [out file]     (default 10 20 profiles/parse_probe.txt)"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import rejit_amd
from rejit_amd import records

millions = float(sys.argv[1]) if len(sys.argv) > 1 else 10
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "parse_probe.txt")
WARM = 3
READ_RATE = 6.9e12
K = int(millions * 1e6)
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b","))
KINDS = {"int64": 0, "float64": 2}
lines = ["parse_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max); model = 41 bytes per row + the rows' bytes"
         % (repeats, WARM),
         "(chk) = the refused call (row-check pass only); (i) = rj_scan_records_group over the same table, same timing; (ii) = pack + download + Python int() / float(), once",
         "", "| case | rows | ok | row bytes | call ms (min .. max) | model GB | GB/s | of 6.9 TB/s | (chk) ms | (i) group ms (min .. max) | call < (i) | (ii) ms | (ii) / call |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None


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


def case(name, text, rb, re_, kind):
    k, n = int(rb.numel()), int(text.numel())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    values, status = scan.parse_records(text, rb, re_, kind=kind)
    d_value = torch.empty(k, dtype=torch.int64, device=dev)
    d_status = torch.empty(k, dtype=torch.uint8, device=dev)
    n_ok, med, lo, hi = timed(lambda: lib.rj_scan_records_parse(scan._h, vp(text), n, vp(rb), vp(re_), k, None, 0, KINDS[kind], 0, vp(d_value), vp(d_status), None, st))
    assert n_ok == int((status == 0).sum()), lib.rj_last_error()
    assert torch.equal(d_value, values.view(torch.int64)) and torch.equal(d_status, status)
    # (chk) the last row ends behind the text: the call is refused behind the check pass
    bad_end = re_.clone()
    bad_end[-1] = n + 1
    rc, chk, _, _ = timed(lambda: lib.rj_scan_records_parse(scan._h, vp(text), n, vp(rb), vp(bad_end), k, None, 0, KINDS[kind], 0, vp(d_value), vp(d_status), None, st))
    assert rc == -4 and torch.equal(d_value, values.view(torch.int64)), "a refused call wrote a row"
    del bad_end
    # (i) the group call over the same table
    d_group = torch.empty(k, dtype=torch.int64, device=dev)
    g, g_med, g_lo, g_hi = timed(lambda: lib.rj_scan_records_group(scan._h, vp(text), n, vp(rb), vp(re_), k, None, 0, vp(d_group), None, None, 0, st))
    assert g > 0, lib.rj_last_error()
    del d_group
    # (ii) pack, download, parse on the host
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    packed, _, _ = scan.pack_records(text, rb, re_, fill=10, lead=0, gap=1)
    words = packed.cpu().numpy().tobytes().split(b"\n")
    words.pop()
    host = np.zeros(k, dtype=np.int64 if kind == "int64" else np.float64)
    conv = int if kind == "int64" else float
    for j, w in enumerate(words):
        try:
            host[j] = conv(w)
        except (ValueError, OverflowError):
            pass
    host_ms = (time.perf_counter() - t0) * 1e3
    ok = (status == 0).cpu().numpy()
    assert (host.view(np.int64)[ok] == values.view(torch.int64).cpu().numpy()[ok]).all(), "the host route and the call disagree"
    del packed, words, host
    row_bytes = int((re_ - rb).sum())
    model = 41 * k + row_bytes
    line = "| %s | %d | %d | %d | %.3f (%.3f .. %.3f) | %.3f | %.0f | %.1f %% | %.3f | %.3f (%.3f .. %.3f) | %s | %.0f | %.0fx |" % (
        name, k, n_ok, row_bytes, med, lo, hi, model / 1e9, model / med / 1e6, 100 * model / (med * 1e-3) / READ_RATE, chk, g_med, g_lo, g_hi,
        "yes" if med < g_med else "NO", host_ms, host_ms / med)
    print(line, flush=True)
    lines.append(line)


gen = torch.Generator(device=dev).manual_seed(5)


def digit_rows(lead, n_digits, values, tail):
    """row j = lead[j] (a fixed-width uint8 matrix) + the n_digits[j] decimal digits of values[j] + tail (bytes), packed -> (text, the begin of
    every row, the begin and the end of every row's digits)"""
    k, width = values.numel(), int(n_digits.max())
    place = torch.arange(width, device=dev).unsqueeze(0)
    power = (n_digits.unsqueeze(1) - 1 - place).clamp(min=0)
    digits = ((values.unsqueeze(1) // (10 ** power)) % 10 + ord("0")).to(torch.uint8)
    tail_t = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).to(dev).unsqueeze(0).expand(k, -1)
    mat = torch.cat([lead, digits, tail_t], dim=1)
    keep = torch.cat([torch.ones_like(lead, dtype=torch.bool), place < n_digits.unsqueeze(1), torch.ones_like(tail_t, dtype=torch.bool)], dim=1)
    lens = keep.sum(dim=1)
    begin = torch.cumsum(lens, 0) - lens
    return mat[keep].contiguous(), begin, (begin + lead.shape[1]).contiguous(), (begin + lead.shape[1] + n_digits).contiguous()


# a: field 2 of lines split at ','
n_digits = torch.randint(1, 13, (K,), device=dev, generator=gen)
vals = torch.randint(0, 10 ** 12, (K,), device=dev, generator=gen) % (10 ** n_digits)
key = torch.randint(0, 1000, (K,), device=dev, generator=gen)
lead = torch.stack([torch.full_like(key, ord("k"))] + [(key // 10 ** p) % 10 + ord("0") for p in (2, 1, 0)] + [torch.full_like(key, ord(","))], dim=1).to(torch.uint8)
text, line_b, fb, fe = digit_rows(lead, n_digits, vals, b",x\n")
line_e = torch.cat([line_b[1:] - 1, torch.tensor([int(text.numel()) - 1], device=dev)]).contiguous()
res = scan.run_records(text, line_b.contiguous(), line_e)
pb, pe, pf = scan.split_records(line_b.contiguous(), line_e, res, int(text.numel()), what="between")
rb, re_, present = records.field_records(pb, pe, pf, 1)
assert bool(present.all()) and torch.equal(rb, fb) and torch.equal(re_, fe)
del pb, pe, pf, present, res, fb, fe, lead, key
case("a field 2 of split lines, 1..12 digits", text, rb, re_, "int64")
# c: every fourth row's last digit becomes a letter
spoilt = text.clone()
spoilt[re_[::4] - 1] = ord("x")
case("c the same, every fourth row malformed", spoilt, rb, re_, "int64")
del text, spoilt, rb, re_, line_b, line_e, vals, n_digits
# b: D+.DDD
n_digits = torch.randint(1, 9, (K,), device=dev, generator=gen)
vals = torch.randint(0, 10 ** 8, (K,), device=dev, generator=gen) % (10 ** n_digits)
frac = torch.randint(0, 1000, (K,), device=dev, generator=gen)
whole = vals * 1000 + frac                                         # the digits of D+DDD; the point goes in below
text, line_b, fb, fe = digit_rows(torch.empty((K, 0), dtype=torch.uint8, device=dev), n_digits + 4, whole * 10, b"\n")
# (the row is n_digits + 4 digits wide: shift the last three one place right and put the point before them)
for p in (1, 2, 3):
    text[fe - p] = text[fe - p - 1]
text[fe - 4] = ord(".")
case("b D+.DDD floats", text, fb, fe, "float64")
del text, line_b, fb, fe, vals, frac, whole, n_digits
# d: 4 KiB rows
k_d = max(K // 100, 100)
rows_d = torch.full((k_d, 4096), ord("0"), dtype=torch.uint8, device=dev)
rows_d[:, 4079:4095] = torch.randint(ord("0"), ord("9") + 1, (k_d, 16), dtype=torch.uint8, device=dev, generator=gen)
rows_d[:, 4095] = 10
d_rb = (4096 * torch.arange(k_d, device=dev)).contiguous()
case("d 4 KiB rows", rows_d.reshape(-1).contiguous(), d_rb, (d_rb + 4095).contiguous(), "int64")

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
