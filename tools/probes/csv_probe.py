"""What rj_scan_records_csv costs and what it replaces, in ONE run on one box (the protocol of parse_probe.py: the call into
tables of the caller's, warm, timed by events around it, the median (min .. max) of the repeats).  A generated CSV of 10^7
rows at two shapes:
  plain    8 short fields, about 60 bytes a row, no quotes
  quoted   8 fields, about 120 bytes a row, a third of them quoted, some with `""` and line breaks inside
Per shape:
  (i)    the call: size query plus fill (Scan.csv_records' two calls), and the fill alone with the caps given
  (ii)   the same run's read-only ceiling (stream_read_probe) over the same text, and the time that ceiling gives the bytes
         the call must move: two reads of the text plus the tables (20 bytes a field, 24 a row)
  (iii)  plain only, where both give the same tables: the route without the call -- records.line_records, a scan for the
         delimiter, run_records, split_records
  (iv)   download, Python's csv.reader, the offsets from the values' lengths (plain) or the rows alone (quoted), upload of the
         offsets: host clock, once, over the first 1/20 of the rows and scaled by 20

    python tools/probes/csv_probe.py [million rows] [repeats] [out file]      (default 10 20 profiles/csv_probe.txt)"""
import csv
import ctypes
import io
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import numpy as np
import torch

import rejit_amd
from rejit_amd import records
from rejit_amd.api import _CsvStats

args = sys.argv[1:]
millions = float(args[0]) if len(args) > 0 else 10
repeats = int(args[1]) if len(args) > 1 else 20
out_path = args[2] if len(args) > 2 else os.path.join(HERE, "..", "..", "profiles", "csv_probe.txt")
WARM = 3
BLOCK_ROWS = 10000
K = int(millions * 1e6) // BLOCK_ROWS * BLOCK_ROWS
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b","))
vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None


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


def block(shape, seed):
    rng = random.Random(seed)
    word = lambda lo, hi: "".join(rng.choice("abcdefghijklmnopqrstuvwxyz 0123456789") for _ in range(rng.randint(lo, hi)))
    rows = []
    for _ in range(BLOCK_ROWS):
        if shape == "plain":
            rows.append(",".join(word(3, 10) for _ in range(8)))
        else:
            fields = []
            for _ in range(8):
                kind = rng.random()
                v = word(6, 20)
                if kind < 1 / 3:
                    inner = v + (rng.choice([",", '""', "\n", ", "]) + word(1, 8) if rng.random() < 0.5 else "")
                    v = '"' + inner + '"'
                fields.append(v)
            rows.append(",".join(fields))
    return ("\n".join(rows) + "\n").encode()


def case(shape):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    one = block(shape, 5)
    host = one * (K // BLOCK_ROWS)
    text = torch.from_numpy(np.frombuffer(host, dtype=np.uint8)).to(dev)
    n = int(text.numel())
    cs = _CsvStats()
    call = lambda t, rcap, fcap: lib.rj_scan_records_csv(scan._h, vp(text), n, 44, 34, vp(t[0]), vp(t[1]), vp(t[2]), rcap, vp(t[3]), vp(t[4]), vp(t[5]), fcap,
                                                         ctypes.byref(cs), st)
    none = (None,) * 6
    fields = call(none, 0, 0)
    assert fields > 0, lib.rj_last_error()
    rows = int(cs.n_rows)
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)
    tables = (i64(rows + 1), i64(rows), i64(rows), i64(fields), i64(fields), torch.empty(fields, dtype=torch.int32, device=dev))
    _, t_fill = timed(lambda: call(tables, rows, fields))
    _, t_query = timed(lambda: call(none, 0, 0))
    _, t_both = timed(lambda: (call(none, 0, 0), call(tables, rows, fields)))
    moved = 2 * n + 20 * fields + 24 * rows
    read_ms = rejit_amd.stream_read_probe(text.data_ptr(), n, launches=10)
    floor_ms = read_ms * moved / n
    lines = ["%s: %d rows, %d fields, %d bytes (%.1f a row); %d quoted fields, %d escapes" % (shape, rows, fields, n, n / rows, cs.n_quoted, cs.n_escapes),
             "   (i)   size query + fill               %s" % fmt(t_both),
             "         fill alone, caps given          %s   %.1f GB/s of text" % (fmt(t_fill), n / 1e9 / (t_fill[0] * 1e-3)),
             "         size query alone                %s" % fmt(t_query),
             "   (ii)  read-only ceiling, one read     %.3f   %.1f GB/s" % (read_ms, n / 1e9 / (read_ms * 1e-3)),
             "         the call must move %d bytes (two reads of the text, 20 bytes a field, 24 a row): %.3f at the ceiling; fill / that = %.2f"
             % (moved, floor_ms, t_fill[0] / floor_ms)]
    ok = True
    if shape == "plain":
        def route():
            lb, le = records.line_records(text)
            lb, le = lb[:-1].contiguous(), le[:-1].contiguous()          # (`^` also matches behind the last line break)
            result = scan.run_records(text, lb, le)
            return scan.split_records(lb, le, result, n, what="between")
        try:
            (pb, pe, pf), t_route = timed(route, n=3)
            ok = torch.equal(pb, tables[3]) and torch.equal(pe, tables[4]) and torch.equal(pf, tables[0])
            lines.append("   (iii) line_records + scan + run_records + split_records  %s   %.1fx the fill; same tables: %s"
                         % (fmt(t_route), t_route[0] / t_fill[0], "yes" if ok else "NO"))
            del pb, pe, pf
        except (rejit_amd.RejitError, RuntimeError) as err:
            lines.append("   (iii) the route without the call: refused: %s" % str(err)[:120])
    # (iv) the host route over 1/20 of the rows, scaled
    part = one * max(K // BLOCK_ROWS // 20, 1)
    d_part = text[:len(part)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    data = d_part.cpu().numpy().tobytes()
    parsed = list(csv.reader(io.StringIO(data.decode("latin-1"), newline=""), strict=True))
    counts = np.fromiter((len(r) for r in parsed), dtype=np.int64, count=len(parsed))
    if shape == "plain":
        lengths = np.fromiter((len(v) for r in parsed for v in r), dtype=np.int64, count=int(counts.sum()))
        up = torch.from_numpy(np.cumsum(lengths + 1)).to(dev)
    else:
        up = torch.from_numpy(np.cumsum(counts)).to(dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3 * (len(host) / len(part))
    lines.append("   (iv)  download, csv.reader, offsets, upload (1/20 of the rows, scaled):  %.0f ms  (%.0fx size query + fill)" % (host_ms, host_ms / t_both[0]))
    ok = ok and len(parsed) * (len(host) // len(part)) == rows and int(counts.sum()) * (len(host) // len(part)) == fields
    lines.append("         its rows and fields are the call's: %s" % ("yes" if ok else "NO"))
    lines.append("")
    del text, tables, up
    return lines, ok


lines = ["csv_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max); %d rows per shape" % (repeats, WARM, K), ""]
passed = True
for shape in ("plain", "quoted"):
    got, ok = case(shape)
    lines += got
    passed = passed and ok
    print("\n".join(got), flush=True)
    torch.cuda.empty_cache()
lines.append("every shape's tables and counts agree with the other routes: %s" % ("yes" if passed else "NO"))
print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
sys.exit(0 if passed else 1)
