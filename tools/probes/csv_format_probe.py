"""What rj_scan_records_format_csv costs beside its two neighbours, in ONE run on one box (the protocol of zip_probe.py: the
call into buffers of the caller's, warm, timed by events around it, the median (min .. max) of the repeats).
Shapes, 10^7 rows each unless said otherwise, delimiter ',', quote '"', fill '\\n', gap 1:
  a  8 short columns (4..12 letters), no special byte: nothing is quoted -- the bytes are the zip's (checked)
  b  the same, a third of the fields hold a ',': quoted, no quote byte inside
  c  the same, a tenth of the fields hold a '"' as well: quoted and doubled (the bytes tier's inline doubling)
  d  8 raw columns from rj_scan_records_csv's tables over shape c's output (records.csv_cut's route); the bytes are shape c's (checked)
  e  one column of 100 letters: the stream tier
  f  the long expanding piece: 10^3 rows of 1 MiB, a '"' every 61 bytes -- the expand tier from its checkpoints
Beside each, in the same run:
  (z)  rj_scan_records_zip of the same columns with sep ',' (no quoting: other bytes, about the same number)
  (p)  rj_scan_records_pack over the call's own output text and table

    python tools/probes/csv_format_probe.py [million rows] [repeats] [out file]      (default 10 20 profiles/csv_format_probe.txt)"""
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
from rejit_amd.api import CSV_MALFORMED, ZipColumn

args = sys.argv[1:]
millions = float(args[0]) if len(args) > 0 else 10
repeats = int(args[1]) if len(args) > 1 else 20
out_path = args[2] if len(args) > 2 else os.path.join(HERE, "..", "..", "profiles", "csv_format_probe.txt")
WARM = 3
K = int(millions * 1e6)
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b","))
vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
gen = torch.Generator(device=dev).manual_seed(11)


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


def letters(n):
    return torch.randint(97, 123, (n,), device=dev, generator=gen, dtype=torch.uint8)


def case(name, title, columns, raw_mask=0, same_as_zip=False, same_as=None, n=None):
    """columns: (text, begins, ends) per column -> (lines, the call's median, the zip's median, the call's output)"""
    k = int(columns[0][1].numel())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cols = (ZipColumn * len(columns))()
    for c, (t, b, e) in enumerate(columns):
        cols[c] = ZipColumn(t.data_ptr(), int(t.numel()), b.data_ptr(), e.data_ptr(), k, 0, 0, 0, 0)
    ob, oe = torch.empty(k, dtype=torch.int64, device=dev), torch.empty(k, dtype=torch.int64, device=dev)
    form = lambda buf, cap: lib.rj_scan_records_format_csv(scan._h, cols, len(columns), 44, 34, 0, raw_mask, 0, 10, 0, 1, vp(buf), cap, vp(ob), vp(oe), None, st)
    total = form(None, 0)
    assert total > 0, lib.rj_last_error()
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    t0 = time.perf_counter()
    form(out, total)
    if n is None and time.perf_counter() - t0 > 2.0:      # a call of seconds: three repeats, and the line says so
        n = 3
        title += " (3 repeats)"
    rc, t_call = timed(lambda: form(out, total), n)
    assert rc == total, lib.rj_last_error()
    lens = (oe - ob).to(torch.float64)
    # (z) the zip of the same columns
    zb, ze = torch.empty(k, dtype=torch.int64, device=dev), torch.empty(k, dtype=torch.int64, device=dev)
    zipped = lambda buf, cap: lib.rj_scan_records_zip(scan._h, cols, len(columns), b",", 1, 32, 0, 10, 0, 1, vp(buf), cap, vp(zb), vp(ze), st)
    z_total = zipped(None, 0)
    z_out = torch.empty(z_total, dtype=torch.uint8, device=dev)
    rc, t_zip = timed(lambda: zipped(z_out, z_total), n)
    assert rc == z_total, lib.rj_last_error()
    checked = ""
    if same_as_zip:
        assert z_total == total and torch.equal(z_out, out) and torch.equal(zb, ob) and torch.equal(ze, oe)
        checked = "; same bytes and rows as the zip: yes"
    if same_as is not None:
        assert torch.equal(same_as, out)
        checked = "; same bytes as shape c: yes"
    del z_out, zb, ze
    # (p) the pack of the call's own output
    again = torch.empty(total, dtype=torch.uint8, device=dev)
    pb, pe = torch.empty(k, dtype=torch.int64, device=dev), torch.empty(k, dtype=torch.int64, device=dev)
    rc, t_pack = timed(lambda: lib.rj_scan_records_pack(scan._h, vp(out), total, vp(ob), vp(oe), k, None, 0, 10, 0, 1, vp(again), total, vp(pb), vp(pe), st), n)
    assert rc == total and torch.equal(again, out)
    del again, pb, pe
    gb = total / 1e9
    return ["%s  %s" % (name, title),
            "   %d rows, %d output bytes, %.2f bytes per line on average (longest %d)%s" % (k, total, float(lens.mean()), int(lens.max()), checked),
            "   rj_scan_records_format_csv         %s   %.1f GB/s of output" % (fmt(t_call), gb / (t_call[0] * 1e-3)),
            "   (z)  rj_scan_records_zip           %s   format_csv / zip  %.2f (medians)" % (fmt(t_zip), t_call[0] / t_zip[0]),
            "   (p)  rj_scan_records_pack          %s   format_csv / pack %.2f (medians)" % (fmt(t_pack), t_call[0] / t_pack[0]),
            ""], t_call[0], t_zip[0], out


def short_columns(text):
    base = torch.arange(K, device=dev, dtype=torch.int64) * 96
    cols = []
    for c in range(8):
        begins = (base + 12 * c).contiguous()
        cols.append((text, begins, (begins + torch.randint(4, 13, (K,), device=dev, generator=gen)).contiguous()))
    return cols


lines = ["csv_format_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max)" % (repeats, WARM), ""]
text = letters(96 * K)
cols = short_columns(text)
got, t_a, z_a, out = case("a", "8 columns of 4..12 letters, nothing to quote", cols, same_as_zip=True)
lines += got
ratio_a = t_a / z_a
del out
for c, (_, begins, _) in enumerate(cols):      # a third of the fields: a ',' as their first byte
    hit = torch.rand(K, device=dev, generator=gen) < 1 / 3
    text[begins[hit]] = 44
got, _, _, out = case("b", "the same, a third of the fields hold a ','", cols)
lines += got
del out
for c, (_, begins, _) in enumerate(cols):      # a tenth of the fields: a '"' as their second byte
    hit = torch.rand(K, device=dev, generator=gen) < 1 / 10
    text[begins[hit] + 1] = 34
got, _, _, out_c = case("c", "the same, a tenth of the fields hold a '\"' too", cols)
lines += got
table = scan.csv_records(out_c, rows=False)
assert table.n_rows == K and table.n_fields == 8 * K and not bool(((table.field_flags & CSV_MALFORMED) != 0).any())
raw_cols = []
for c in range(8):
    index, present = records.csv_column(table.row_first, c)
    assert bool(present.all())
    raw_cols.append((out_c, table.field_begin[index].contiguous(), table.field_end[index].contiguous()))
del text, cols
got, _, _, out = case("d", "8 raw columns from rj_scan_records_csv's tables over shape c's output", raw_cols, raw_mask=0xFF, same_as=out_c)
lines += got
del out, out_c, raw_cols, table
torch.cuda.empty_cache()
text = letters(100 * K)
begins = (torch.arange(K, device=dev, dtype=torch.int64) * 100).contiguous()
got, _, _, out = case("e", "one column of 100 letters", [(text, begins, (begins + 100).contiguous())], same_as_zip=True)
lines += got
del out, text, begins
torch.cuda.empty_cache()
rows, piece = 1000, 1 << 20
text = letters(rows * piece)
text[::61] = 34
begins = (torch.arange(rows, device=dev, dtype=torch.int64) * piece).contiguous()
got, t_f, _, out = case("f", "10^3 rows of 1 MiB, a '\"' every 61 bytes: every piece expands over 261 chunks", [(text, begins, (begins + piece).contiguous())])
lines += got
del out, text
lines.append("shape a against the zip of the same columns: %.2f (the yardstick: 1.5 by bytes moved, up to 2 allowed) -- %s" % (ratio_a, "within" if ratio_a <= 2 else "ABOVE"))
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
