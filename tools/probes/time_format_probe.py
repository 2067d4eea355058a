"""What rj_scan_records_format_time costs, next to the number format of the same values, next to merely moving its own output's
bytes, and next to what a caller does without it, in ONE run on one box.  Per case: the call into a text and tables of the
caller's, warm, timed by events around it, the median (min .. max) of the repeats; and, in the same process,
  (1)  rj_scan_records_format(RJ_FORMAT_INT64) of the same values: the sibling whose frame this call uses, timed the same way.
  (2)  rj_scan_records_pack of this call's own output text (every row, the same gap): the cost of merely moving those bytes
       through the family's copy, timed the same way.  The call costs more than (2) "by more than the run's spread" when its
       median is above (2)'s max.
  (3)  rj_scan_records_pack of a 10^5-row sample of the int64 column's bytes, the download and the formatting of every value in
       Python (host clock, once), scaled to the case's rows, and checked to give the call's bytes.
Cases: the 20-byte ISO format %Y-%m-%dT%H:%M:%SZ, the 26-byte CLF format %d/%b/%Y:%H:%M:%S %z and the longest format (64 format
bytes: 74 row bytes under "s", 77 under "ns"), each under "s" and under "ns"; gap 1, UTC.
    python tools/probes/time_format_probe.py [million rows] [repeats] [out file]     (default 10 20 profiles/time_format_probe.txt)"""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "time_format_probe.txt")
WARM = 3
SAMPLE = 100000
K = int(millions * 1e6)
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b","))
vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
lines = ["time_format_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max)" % (repeats, WARM),
         "(1) = rj_scan_records_format(INT64) of the same values; (2) = rj_scan_records_pack of the call's own output text; same timing",
         "above (2)'s spread = the call's median is above (2)'s max",
         "(3) = pack + download + formatting in Python of a %d-row sample of the values, once, scaled to the rows" % SAMPLE,
         "", "| case | rows | row bytes | out MB | call ms (min .. max) | rows/us | out GB/s | (1) int64 format ms (min .. max) | call / (1) | (2) pack of the output ms (min .. max) | call / (2) | above (2)'s spread | (3) ms, scaled | (3) / call |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]


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


MONTHS = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")


def host_text(value, fmt, unit):
    """the row in Python: datetime for the fields, the directives by hand (strftime has neither nine digits nor a padded %Y)"""
    per = 10 ** (3 * unit)
    secs, rest = divmod(value, per)
    dt = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=secs)
    parts = {"Y": "%04d" % dt.year, "m": "%02d" % dt.month, "d": "%02d" % dt.day, "H": "%02d" % dt.hour, "M": "%02d" % dt.minute, "S": "%02d" % dt.second,
             "b": MONTHS[dt.month - 1], "f": ("%09d" % (rest * 10 ** (9 - 3 * unit)))[:3 * unit] if unit else "000000", "z": "+0000", "%": "%"}
    out, i = "", 0
    while i < len(fmt):
        if fmt[i] == "%":
            out += parts[fmt[i + 1]]
            i += 2
        else:
            out += fmt[i]
            i += 1
    return out


gen = torch.Generator(device=dev).manual_seed(1970)
seconds = torch.randint(0, 1 << 31, (K,), device=dev, generator=gen)
nanos = seconds * 1000000000 + torch.randint(0, 1000000000, (K,), device=dev, generator=gen)


def case(name, fmt, unit_name, unit, values):
    k = K
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    text, ob, oe = scan.format_time_records(values, fmt, unit=unit_name)
    total, width = int(text.numel()), int(oe[0] - ob[0])
    d_out = torch.empty(total, dtype=torch.uint8, device=dev)
    d_ob, d_oe = torch.empty(k, dtype=torch.int64, device=dev), torch.empty(k, dtype=torch.int64, device=dev)
    rc, med, lo, hi = timed(lambda: lib.rj_scan_records_format_time(scan._h, vp(values), None, k, None, 0, fmt, len(fmt), unit, 0, 0, 10, 0, 1, vp(d_out), total,
                                                                    vp(d_ob), vp(d_oe), None, st))
    assert rc == total == k * (width + 1), lib.rj_last_error()
    assert torch.equal(d_out, text) and torch.equal(d_ob, ob) and torch.equal(d_oe, oe)
    # (3) the host route: the values' bytes packed and downloaded (a sample), formatted in Python, scaled
    sample = torch.arange(0, k, max(k // SAMPLE, 1), dtype=torch.int64, device=dev)[:SAMPLE].contiguous()
    raw = values.view(torch.uint8)
    vb = (torch.arange(k, dtype=torch.int64, device=dev) * 8).contiguous()
    ve = (vb + 8).contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    packed, _, _ = scan.pack_records(raw, vb, ve, indices=sample, fill=0, lead=0, gap=0)
    host_values = np.frombuffer(packed.cpu().numpy().tobytes(), dtype=np.int64)
    py_fmt = fmt.decode()
    host = "\n".join(host_text(int(v), py_fmt, unit) for v in host_values).encode() + b"\n"
    host_ms = (time.perf_counter() - t0) * 1e3 * (k / len(host_values))
    got, _, _ = scan.pack_records(text, ob, oe, indices=sample, fill=10, lead=0, gap=1)
    assert got.cpu().numpy().tobytes() == host, "the host route and the call disagree"
    del packed, got, raw, vb, ve
    # (2) the pack of the call's own output
    p_out = torch.empty(total, dtype=torch.uint8, device=dev)
    p_rc, p_med, p_lo, p_hi = timed(lambda: lib.rj_scan_records_pack(scan._h, vp(text), total, vp(ob), vp(oe), k, None, 0, 10, 0, 1, vp(p_out), total, vp(d_ob), vp(d_oe),
                                                                     st))
    assert p_rc == total and torch.equal(p_out, text), lib.rj_last_error()
    del p_out
    # (1) the number format of the same values
    n_total = int(lib.rj_scan_records_format(scan._h, vp(values), None, k, None, 0, 0, 0, 10, 0, 1, None, 0, None, None, st))
    n_out = torch.empty(n_total, dtype=torch.uint8, device=dev)
    f_rc, f_med, f_lo, f_hi = timed(lambda: lib.rj_scan_records_format(scan._h, vp(values), None, k, None, 0, 0, 0, 10, 0, 1, vp(n_out), n_total, vp(d_ob), vp(d_oe), st))
    assert f_rc == n_total, lib.rj_last_error()
    line = "| %s | %d | %d | %.1f | %.3f (%.3f .. %.3f) | %.0f | %.0f | %.3f (%.3f .. %.3f) | %.2f | %.3f (%.3f .. %.3f) | %.2f | %s | %.0f | %.0fx |" % (
        name, k, width, total / 1e6, med, lo, hi, k / med / 1e3, total / med / 1e6, f_med, f_lo, f_hi, med / f_med, p_med, p_lo, p_hi, med / p_med,
        "YES" if med > p_hi else "no", host_ms, host_ms / med)
    print(line, flush=True)
    lines.append(line)


ISO, CLF = b"%Y-%m-%dT%H:%M:%SZ", b"%d/%b/%Y:%H:%M:%S %z"
LONGEST = b"%Y-%b-%dT%H:%M:%S.%f%z|" + b"abcdefghijklmnopqrstuvwxyz0123456789ABCDE"
for unit_name, unit, values in (("s", 0, seconds), ("ns", 3, nanos)):
    case("ISO, %s" % unit_name, ISO, unit_name, unit, values)
    case("CLF, %s" % unit_name, CLF, unit_name, unit, values)
    case("longest format, %s" % unit_name, LONGEST, unit_name, unit, values)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
