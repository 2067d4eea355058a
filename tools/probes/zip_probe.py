"""What rj_scan_records_zip costs and what it replaces, in ONE run on one box (the protocol of parse_probe.py: the call into
buffers of the caller's, warm, timed by events around it, the median (min .. max) of the repeats).
Cases, 10^7 rows each, fill '\\n', gap 1:
  a  the `uniq -c` line: a count (formatted, width 7), a word of about 8 bytes, an integer sum (formatted), sep ' '
  b  two fields of one text, swapped (awk '{print $2, $1}'), sep ' '
  c  the line number (formatted), ':' and the line, lines of about 80 bytes: the streaming tier
Beside each:
  (p)   rj_scan_records_pack over the zip's own output text and table -- the family's yardstick for a text of that size
  (ii)  the route the call replaces: pack or format each column, download, join row by row in Python, upload; host clock,
        once; its bytes checked equal to the call's

    python tools/probes/zip_probe.py [million rows] [repeats] [out file]      (default 10 20 profiles/zip_probe.txt)"""
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import numpy as np
import torch

import rejit_amd
from rejit_amd.api import ZipColumn

args = sys.argv[1:]
millions = float(args[0]) if len(args) > 0 else 10
repeats = int(args[1]) if len(args) > 1 else 20
out_path = args[2] if len(args) > 2 else os.path.join(HERE, "..", "..", "profiles", "zip_probe.txt")
WARM = 3
K = int(millions * 1e6)
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b","))
vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
gen = torch.Generator(device=dev).manual_seed(7)


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


def letters(n):
    return torch.randint(97, 123, (n,), device=dev, generator=gen, dtype=torch.uint8)


def strided(stride, lo, hi, offset=None):
    """K records of lo..hi bytes, record i at i * stride (+ offset[i]) -> (begins, ends)"""
    begins = torch.arange(K, device=dev, dtype=torch.int64) * stride
    if offset is not None:
        begins = begins + offset
    return begins.contiguous(), (begins + torch.randint(lo, hi + 1, (K,), device=dev, generator=gen)).contiguous()


def rows_of(text, begins, ends):
    """a column on the host, as the sample gets it: packed on the device, downloaded, split at the line breaks"""
    packed = scan.pack_records(text, begins, ends, fill=10, lead=0, gap=1)[0]
    return packed.cpu().numpy().tobytes().split(b"\n")[:-1]


def case(name, title, columns, widths, sep, host_route):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cols = (ZipColumn * len(columns))()
    for c, (t, b, e) in enumerate(columns):
        cols[c] = ZipColumn(t.data_ptr(), int(t.numel()), b.data_ptr(), e.data_ptr(), K, 0, 0, widths[c], 0)
    ob, oe = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
    total = lib.rj_scan_records_zip(scan._h, cols, len(columns), sep, len(sep), 32, 0, 10, 0, 1, None, 0, vp(ob), vp(oe), st)
    assert total > 0, lib.rj_last_error()
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    rc, t_call = timed(lambda: lib.rj_scan_records_zip(scan._h, cols, len(columns), sep, len(sep), 32, 0, 10, 0, 1, vp(out), total, vp(ob), vp(oe), st))
    assert rc == total, lib.rj_last_error()
    lens = (oe - ob).to(torch.float64)
    # (p) the pack of the zip's own output: the same bytes out
    again = torch.empty(total, dtype=torch.uint8, device=dev)
    pb, pe = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
    rc, t_pack = timed(lambda: lib.rj_scan_records_pack(scan._h, vp(out), total, vp(ob), vp(oe), K, None, 0, 10, 0, 1, vp(again), total, vp(pb), vp(pe), st))
    assert rc == total and torch.equal(again, out)
    del again, pb, pe
    # (ii) the route the call replaces, once, on the host clock
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = host_route()
    up = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    assert torch.equal(up, out), "the host route and the call disagree"
    gb = total / 1e9
    return ["%s  %s" % (name, title),
            "   %d output bytes, %.2f bytes per line on average (longest %d)" % (total, float(lens.mean()), int(lens.max())),
            "   rj_scan_records_zip               %s   %.1f GB/s of output" % (fmt(t_call), gb / (t_call[0] * 1e-3)),
            "   (p)  rj_scan_records_pack          %s   zip / pack %.2f (medians); same bytes" % (fmt(t_pack), t_call[0] / t_pack[0]),
            "   (ii) pack or format each column, download, join on the host, upload, once:  %.0f ms  (%.0fx the call); same bytes: yes" % (host_ms, host_ms / t_call[0]),
            ""], host_ms > t_call[0]


def case_a():
    counts = (torch.randint(0, 10 ** 6, (K,), device=dev, generator=gen) % (10 ** torch.randint(1, 7, (K,), device=dev, generator=gen))).contiguous()
    sums = torch.randint(-10 ** 9, 10 ** 9, (K,), device=dev, generator=gen).contiguous()
    text = letters(12 * K)
    wb, we = strided(12, 4, 12)
    count_col, sum_col = scan.format_records(counts), scan.format_records(sums)

    def host_route():      # the sample's: the counts as values, the words and the formatted sums as two texts
        words, sum_words = rows_of(text, wb, we), sum_col[0].cpu().numpy().tobytes().split(b"\n")
        return b"".join(b"%7d %s %s\n" % (c, w, a) for c, w, a in zip(counts.cpu().tolist(), words, sum_words))
    return case("a", "count (width 7), word of 4..12 bytes, int64 sum: b\"%7d %s %s\\n\"", [count_col, (text, wb, we), sum_col], [7, 0, 0], b" ", host_route)


def case_b():
    text = letters(24 * K)
    b1, e1 = strided(24, 3, 9)
    b2 = (e1 + 1).contiguous()
    e2 = (b2 + torch.randint(1, 9, (K,), device=dev, generator=gen)).contiguous()

    def host_route():
        first, second = rows_of(text, b1, e1), rows_of(text, b2, e2)
        return b"".join(b"%s %s\n" % (s, f) for f, s in zip(first, second))
    return case("b", "two fields of one text (3..9 and 1..8 bytes), swapped", [(text, b2, e2), (text, b1, e1)], [0, 0], b" ", host_route)


def case_c():
    text = letters(100 * K)
    lb, le = strided(100, 60, 100)
    numbers = scan.format_records(torch.arange(1, K + 1, device=dev, dtype=torch.int64))

    def host_route():
        lines = rows_of(text, lb, le)
        return b"".join(b"%d:%s\n" % (i + 1, line) for i, line in enumerate(lines))
    return case("c", "line number, ':', a line of 60..100 bytes: the streaming tier", [numbers, (text, lb, le)], [0, 0], b":", host_route)


lines = ["zip_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max); %d rows per case" % (repeats, WARM, K), ""]
passed = True
for make in (case_a, case_b, case_c):
    got, ok = make()
    lines += got
    passed = passed and ok
    torch.cuda.empty_cache()
lines.append("the call beats (ii) on all three cases: %s" % ("yes" if passed else "NO"))
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
sys.exit(0 if passed else 1)
