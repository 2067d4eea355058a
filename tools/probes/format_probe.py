"""What rj_scan_records_format costs and what it replaces, in ONE run on one box (the protocol of parse_probe.py: the call into
buffers of the caller's, warm, timed by events around it, the median (min .. max) of the repeats).
Cases, 10^7 rows each, fill '\\n', gap 1:
  a  int64 of 1..12 digits
  b  doubles of the form D+.DDD (1..8 digits before the point, three behind it)
  e  random doubles whose repr() has 16 or 17 digits (random mantissas, exponents over the whole range)
Beside each:
  (i)   rj_scan_records_parse over the text the call just produced -- the inverse, over the same bytes, with the flags the round
        trip uses (RJ_PARSE_WIDE), checked to give the input's bits back
  (p)   rj_scan_records_pack over that same text and table -- the same output bytes and the same plan-and-copy frame, without
        the conversion
  (ii)  the route the call replaces: download the values, "\\n".join of str() / repr() on the host, upload; host clock, once;
        its bytes checked equal to the call's

    python tools/probes/format_probe.py [million rows] [repeats] [out file]      (default 10 20 profiles/format_probe.txt)"""
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import numpy as np
import torch

import rejit_amd

args = sys.argv[1:]
millions = float(args[0]) if len(args) > 0 else 10
repeats = int(args[1]) if len(args) > 1 else 20
out_path = args[2] if len(args) > 2 else os.path.join(HERE, "..", "..", "profiles", "format_probe.txt")
WARM = 3
K = int(millions * 1e6)
INT64, FLOAT64, WIDE = 0, 2, 4
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b","))
vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
gen = torch.Generator(device=dev).manual_seed(5)


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
    return rc, (float(np.median(ts)), min(ts), max(ts))


def fmt(t):
    return "%.3f (%.3f .. %.3f)" % t


def values_a():
    n_digits = torch.randint(1, 13, (K,), device=dev, generator=gen)
    vals = torch.randint(0, 10 ** 12, (K,), device=dev, generator=gen) % (10 ** n_digits)
    return torch.where(torch.randint(0, 4, (K,), device=dev, generator=gen) == 0, -vals, vals).contiguous()


def values_b():
    n_digits = torch.randint(1, 9, (K,), device=dev, generator=gen)
    whole = torch.randint(0, 10 ** 8, (K,), device=dev, generator=gen) % (10 ** n_digits)
    frac = torch.randint(0, 1000, (K,), device=dev, generator=gen)
    return ((whole * 1000 + frac).to(torch.float64) / 1000.0).contiguous()      # correctly rounded: the double nearest to D+.DDD


def values_e():
    bits = torch.randint(0, 1 << 52, (K,), device=dev, generator=gen) | (torch.randint(1, 2047, (K,), device=dev, generator=gen) << 52)
    bits = bits | (torch.randint(0, 2, (K,), device=dev, generator=gen) << 63)
    return bits.view(torch.float64).contiguous()


def case(name, title, values, kind, host_text):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    as_words = values.view(torch.int64)
    ob, oe = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
    total = lib.rj_scan_records_format(scan._h, vp(as_words), None, K, None, 0, kind, 0, 10, 0, 1, None, 0, vp(ob), vp(oe), st)
    assert total > 0, lib.rj_last_error()
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    call = lambda: lib.rj_scan_records_format(scan._h, vp(as_words), None, K, None, 0, kind, 0, 10, 0, 1, vp(out), total, vp(ob), vp(oe), st)
    rc, t_call = timed(call)
    assert rc == total, lib.rj_last_error()
    digits = (oe - ob).to(torch.float64)
    # (i) the inverse over the same bytes
    back, status = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.uint8, device=dev)
    n_ok, t_parse = timed(lambda: lib.rj_scan_records_parse(scan._h, vp(out), total, vp(ob), vp(oe), K, None, 0, kind, WIDE, vp(back), vp(status), None, st))
    assert n_ok == K and torch.equal(back, as_words), "the round trip does not give the input's bits back"
    # (p) the pack of the same rows: the same bytes out
    again = torch.empty(total, dtype=torch.uint8, device=dev)
    pb, pe = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
    rc, t_pack = timed(lambda: lib.rj_scan_records_pack(scan._h, vp(out), total, vp(ob), vp(oe), K, None, 0, 10, 0, 1, vp(again), total, vp(pb), vp(pe), st))
    assert rc == total and torch.equal(again, out)
    del again, pb, pe, back, status
    # (ii) the route the call replaces, once, on the host clock
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = host_text(values.cpu().tolist())
    up = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    assert torch.equal(up, out), "the host route and the call disagree"
    gb = total / 1e9
    return ["%s  %s" % (name, title),
            "   %d output bytes, %.2f bytes per row on average (longest %d)" % (total, float(digits.mean()), int(digits.max())),
            "   rj_scan_records_format            %s   %.1f GB/s of output" % (fmt(t_call), gb / (t_call[0] * 1e-3)),
            "   (i)  rj_scan_records_parse, WIDE   %s   format / parse %.2f (medians); every row OK with the input's bits" % (fmt(t_parse), t_call[0] / t_parse[0]),
            "   (p)  rj_scan_records_pack          %s   format / pack %.2f (medians); same bytes" % (fmt(t_pack), t_call[0] / t_pack[0]),
            "   (ii) download, join on the host, upload, once:  %.0f ms  (%.0fx the call); same bytes: yes" % (host_ms, host_ms / t_call[0]), ""], host_ms > t_call[0]


lines = ["format_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max); %d rows per case" % (repeats, WARM, K), ""]
passed = True
for name, title, make, kind, host_text in (
        ("a", "int64 of 1..12 digits, one in four negative", values_a, INT64, lambda xs: ("\n".join(map(str, xs)) + "\n").encode()),
        ("b", "doubles D+.DDD", values_b, FLOAT64, lambda xs: ("\n".join(map(repr, xs)) + "\n").encode()),
        ("e", "random doubles: random mantissa bits, every finite exponent", values_e, FLOAT64, lambda xs: ("\n".join(map(repr, xs)) + "\n").encode())):
    values = make()
    got, ok = case(name, title, values, kind, host_text)
    lines += got
    passed = passed and ok
    del values
    torch.cuda.empty_cache()
lines.append("the call beats (ii) on all three cases: %s" % ("yes" if passed else "NO"))
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
sys.exit(0 if passed else 1)
