"""What rj_scan_records_translate costs and what it replaces, in ONE run on one box (the protocol of parse_probe.py: the call into
buffers of the caller's, warm, timed by events around it, the median (min .. max) of the repeats).
Rows of 20 and of 100 bytes (10^7 each, a line break between two, fill '\\n', gap 1), three cases each:
  map   nothing dropped, A-Z -> a-z (str.lower)
  1/20  one byte in 20 is a ',' and dropped, the rest lowered
  1/2   every second byte (on average) is a ',' and dropped, the rest lowered
Beside each, what the parent commit offers for the same job:
  (q)   the call's own size query: the rows' plan and the count (or the layout) without the emit
  (p)   rj_scan_records_pack of the same table: the traffic of the map-only case, the yardstick for the LDS lookups
  (r)   the drop cases: run_records with `,` + replace_records with b"" (no map: the dropped bytes alone)
  (h)   download, bytes.translate per row, upload; host clock, once; its bytes checked equal to the call's

    python tools/probes/translate_probe.py [million rows] [repeats] [out file]      (default 10 20 profiles/translate_probe.txt)"""
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import numpy as np
import torch

import rejit_amd
from rejit_amd import records

args = sys.argv[1:]
millions = float(args[0]) if len(args) > 0 else 10
repeats = int(args[1]) if len(args) > 1 else 20
out_path = args[2] if len(args) > 2 else os.path.join(HERE, "..", "..", "profiles", "translate_probe.txt")
WARM = 3
K = int(millions * 1e6)
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b","))
vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
gen = torch.Generator(device=dev).manual_seed(7)
LOWER = records.ASCII_LOWER
COMMA = bytes(records.drop_set(b","))


def timed(call, n=None):
    ts = []
    for i in range(WARM + (repeats if n is None else n)):
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


def make_text(length, share):
    """K rows of `length` letters of both cases, a ',' with probability `share`, a line break behind each row"""
    n = K * (length + 1)
    text = torch.randint(0, 52, (n,), device=dev, generator=gen, dtype=torch.uint8)
    text = torch.where(text < 26, text + 65, text + 71)
    if share:
        text[torch.rand(n, device=dev, generator=gen) < share] = 44
    begins = (torch.arange(K, device=dev, dtype=torch.int64) * (length + 1)).contiguous()
    ends = (begins + length).contiguous()
    text[ends] = 10
    return text.contiguous(), begins, ends


def case(length, name, share):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    text, begins, ends = make_text(length, share)
    n = int(text.numel())
    drop = COMMA if share else None
    ob, oe = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
    call = lambda out, cap: lib.rj_scan_records_translate(scan._h, vp(text), n, vp(begins), vp(ends), K, None, 0, LOWER, drop, 10, 0, 1, out, cap, vp(ob), vp(oe), None, st)
    total = call(None, 0)
    assert total > 0, lib.rj_last_error()
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    rc, t_call = timed(lambda: call(vp(out), total))
    assert rc == total, lib.rj_last_error()
    _, t_query = timed(lambda: call(None, 0))
    call(vp(out), total)
    lines = ["%d-byte rows, %s" % (length, name),
             "   %d source bytes, %d output bytes" % (n, total),
             "   rj_scan_records_translate          %s   %.1f GB/s of source" % (fmt(t_call), n / 1e9 / (t_call[0] * 1e-3)),
             "   (q)  its size query alone           %s   the emit is the difference: %.3f" % (fmt(t_query), t_call[0] - t_query[0])]
    # (p) the pack of the same table
    packed = torch.empty(n, dtype=torch.uint8, device=dev)
    pb, pe = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
    rc, t_pack = timed(lambda: lib.rj_scan_records_pack(scan._h, vp(text), n, vp(begins), vp(ends), K, None, 0, 10, 0, 1, vp(packed), n, vp(pb), vp(pe), st))
    assert rc == n, lib.rj_last_error()
    lines.append("   (p)  rj_scan_records_pack           %s   translate / pack %.2f (medians)" % (fmt(t_pack), t_call[0] / t_pack[0]))
    del packed, pb, pe
    # (r) the dropped bytes alone, by the scan and the replace
    if share:
        try:
            def route():
                result = scan.run_records(text, begins, ends)
                return scan.replace_records(text, begins, ends, result, b"", fill=10, lead=0, gap=1)[0]
            new, t_repl = timed(route, n=3)
            same = torch.equal(new, scan.translate_records(text, begins, ends, delete=b",", fill=10)[0])
            lines.append("   (r)  run_records + replace_records  %s   %.1fx the call; same bytes (no map): %s" % (fmt(t_repl), t_repl[0] / t_call[0], "yes" if same else "NO"))
            del new
        except (rejit_amd.RejitError, RuntimeError) as err:
            lines.append("   (r)  run_records + replace_records  refused: %s" % str(err)[:120])
    # (h) the host route, once, on the host clock
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    data = text.cpu().numpy().tobytes()
    b, e = begins.cpu().tolist(), ends.cpu().tolist()
    delete = b"," if share else b""
    host = b"\n".join([data[x:y].translate(LOWER, delete) for x, y in zip(b, e)]) + b"\n"
    up = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    same = torch.equal(up, out)
    lines.append("   (h)  download, bytes.translate per row, upload, once:  %.0f ms  (%.0fx the call); same bytes: %s" % (host_ms, host_ms / t_call[0], "yes" if same else "NO"))
    lines.append("")
    del data, host, up, out, text
    return lines, same


lines = ["translate_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max); %d rows per case" % (repeats, WARM, K), ""]
passed = True
for length in (20, 100):
    for name, share in (("map only (lower)", 0.0), ("1 byte in 20 dropped, the rest lowered", 0.05), ("half the bytes dropped, the rest lowered", 0.5)):
        got, ok = case(length, name, share)
        lines += got
        passed = passed and ok
        print("\n".join(got), flush=True)
        torch.cuda.empty_cache()
lines.append("every case's bytes equal the host route's: %s" % ("yes" if passed else "NO"))
print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
sys.exit(0 if passed else 1)
