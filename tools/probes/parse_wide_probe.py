"""What RJ_PARSE_WIDE costs and what it replaces, in ONE run on one box (the shape of parse_probe.py: the call into tables of
the caller's, warm, timed by events around it, the median (min .. max) of the repeats).
Cases:
  b  10^7 rows D+.DDD (1..8 digits before the point), float64, all inside the old window -- parse_probe.py's case b: the call
     without the flag and with it, in turns in the same process; next to them the PARENT commit's library on the same box (its
     own process: --yardstick, below), which is the yardstick -- not a recorded figure, and not the code under test
  e  10^7 rows of 17 significant digits, D.DDDDDDDDDDDDDDDDe[+-]DDD (what repr() and %.17g write for most doubles; generated
     on the device, the last digit never 0): the call with the flag, against the route it replaces -- the call without the
     flag, a download of the rows it left INEXACT, float() of each on the host (host clock, once) --, checked to give the
     same bits
  f  10^7 rows, every fourth with 25 significant digits (the rest as in e): the call with the flag, and its status counts

    python tools/probes/parse_wide_probe.py --yardstick OUT.json [million rows] [repeats]
        with REJIT_TREE=<a checkout of the parent commit, built>: times b and e WITHOUT the flag through that tree's library
    python tools/probes/parse_wide_probe.py [--parent OUT.json] [million rows] [repeats] [out file]
        (default 10 20 profiles/parse_wide_probe.txt)"""
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.environ.get("REJIT_TREE") or os.path.join(HERE, "..", "..")))
import numpy as np
import torch

import rejit_amd

args = sys.argv[1:]
yardstick = parent = None
if args and args[0] == "--yardstick":
    yardstick, args = args[1], args[2:]
if args and args[0] == "--parent":
    parent, args = args[1], args[2:]
millions = float(args[0]) if len(args) > 0 else 10
repeats = int(args[1]) if len(args) > 1 else 20
out_path = args[2] if len(args) > 2 else os.path.join(HERE, "..", "..", "profiles", "parse_wide_probe.txt")
WARM = 3
K = int(millions * 1e6)
FLOAT64, TRIM, WIDE = 2, 1, 4
OK, RANGE, INEXACT = 0, 3, 4
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


def parse(text, rb, re_, flags, d_value, d_status):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    k, n = int(rb.numel()), int(text.numel())
    return lambda: lib.rj_scan_records_parse(scan._h, vp(text), n, vp(rb), vp(re_), k, None, 0, FLOAT64, flags, vp(d_value), vp(d_status), None, st)


def fmt(t):
    return "%.3f (%.3f .. %.3f)" % t


def rows_b():
    """parse_probe.py's case b"""
    n_digits = torch.randint(1, 9, (K,), device=dev, generator=gen)
    vals = torch.randint(0, 10 ** 8, (K,), device=dev, generator=gen) % (10 ** n_digits)
    frac = torch.randint(0, 1000, (K,), device=dev, generator=gen)
    whole = (vals * 1000 + frac) * 10                              # the digits of D+DDD and a place for the point
    width = n_digits + 4
    place = torch.arange(12, device=dev).unsqueeze(0)
    power = (width.unsqueeze(1) - 1 - place).clamp(min=0)
    digits = ((whole.unsqueeze(1) // (10 ** power)) % 10 + ord("0")).to(torch.uint8)
    mat = torch.cat([digits, torch.full((K, 1), 10, dtype=torch.uint8, device=dev)], dim=1)
    keep = torch.cat([place < width.unsqueeze(1), torch.ones((K, 1), dtype=torch.bool, device=dev)], dim=1)
    lens = keep.sum(dim=1)
    begin = torch.cumsum(lens, 0) - lens
    text, fe = mat[keep].contiguous(), (begin + width).contiguous()
    for p in (1, 2, 3):                                            # shift the last three digits one place right, the point before them
        text[fe - p] = text[fe - p - 1]
    text[fe - 4] = ord(".")
    return text, begin.contiguous(), fe


def rows_sci(long_every=0):
    """D.DDDDDDDDDDDDDDDDe[+-]DDD, 17 significant digits, in a stride of 32 bytes; with long_every every such row has 25"""
    mat = torch.full((K, 32), 10, dtype=torch.uint8, device=dev)
    long_row = (torch.arange(K, device=dev) % long_every == 0) if long_every else torch.zeros(K, dtype=torch.bool, device=dev)
    n_frac = torch.where(long_row, 24, 16)
    body = torch.randint(ord("0"), ord("9") + 1, (K, 26), dtype=torch.uint8, device=dev, generator=gen)
    nonzero = torch.randint(ord("1"), ord("9") + 1, (K, 2), dtype=torch.uint8, device=dev, generator=gen)
    mat[:, 0] = nonzero[:, 0]
    mat[:, 1] = ord(".")
    mat[:, 2:26] = body[:, :24]
    rows = torch.arange(K, device=dev)
    mat[rows, 1 + n_frac] = nonzero[:, 1]                          # the last digit that counts is not 0
    exp = torch.randint(0, 300, (K,), device=dev, generator=gen)
    sign = torch.where(torch.randint(0, 2, (K,), device=dev, generator=gen) == 0, ord("+"), ord("-")).to(torch.uint8)
    at = 2 + n_frac
    mat[rows, at] = ord("e")
    mat[rows, at + 1] = sign
    for p, d in enumerate((100, 10, 1)):
        mat[rows, at + 2 + p] = ((exp // d) % 10 + ord("0")).to(torch.uint8)
    rb = (32 * rows).contiguous()
    return mat.reshape(-1).contiguous(), rb, (rb + at + 5).contiguous()


def host_route(text, rb, re_, d_value, d_status):
    """the call without the flag, the download of the rows it left INEXACT, float() of each -> (ms, values as uint64 bits)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parse(text, rb, re_, 0, d_value, d_status)()
    left = torch.nonzero(d_status == INEXACT).squeeze(1)
    host_text = text.cpu().numpy().tobytes()
    b, e, rows = rb[left].cpu().numpy(), re_[left].cpu().numpy(), left.cpu().numpy()
    bits = d_value.cpu().numpy().view(np.uint64).copy()
    parsed = np.array([float(host_text[x:y]) for x, y in zip(b.tolist(), e.tolist())], dtype=np.float64)
    bits[rows] = parsed.view(np.uint64)
    return (time.perf_counter() - t0) * 1e3, bits, int(left.numel())


d_value = torch.empty(K, dtype=torch.int64, device=dev)
d_status = torch.empty(K, dtype=torch.uint8, device=dev)

if yardstick:
    out = {}
    text, rb, re_ = rows_b()
    n_ok, out["b"] = timed(parse(text, rb, re_, 0, d_value, d_status))
    assert n_ok == K, lib.rj_last_error()
    del text, rb, re_
    text, rb, re_ = rows_sci()
    n_ok, out["e"] = timed(parse(text, rb, re_, 0, d_value, d_status))
    out["e_ok"] = int(n_ok)
    with open(yardstick, "w") as fh:
        json.dump(out, fh)
    print(out)
    sys.exit(0)

base = json.load(open(parent)) if parent else None
lines = ["parse_wide_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max); %d rows per case" % (repeats, WARM, K), ""]

# ---- b: inside the old window, without and with the flag, in turns
text, rb, re_ = rows_b()
plain, wide = parse(text, rb, re_, 0, d_value, d_status), parse(text, rb, re_, WIDE, d_value, d_status)
n_ok, t_plain = timed(plain)
keep = d_value.clone()
n_ok_w, t_wide = timed(wide)
assert n_ok == n_ok_w == K and torch.equal(keep, d_value), "WIDE changed a row inside the window"
_, t_plain2 = timed(plain)
_, t_wide2 = timed(wide)
lines += ["b  D+.DDD floats, all inside the exact window (one IEEE operation per row under either flag)",
          "   without the flag      %s   again %s" % (fmt(t_plain), fmt(t_plain2)),
          "   with RJ_PARSE_WIDE    %s   again %s" % (fmt(t_wide), fmt(t_wide2)),
          "   WIDE / without        %.3f (medians), %.3f (minima)" % (t_wide[0] / t_plain[0], t_wide[1] / t_plain[1])]
if base:
    tb = tuple(base["b"])
    lines += ["   the parent commit's library, same box, its own process, without the flag (the yardstick):  %s   max / min %.3f" % (fmt(tb), tb[2] / tb[1]),
              "   WIDE / parent         %.3f (medians)      without the flag / parent  %.3f (medians)" % (t_wide[0] / tb[0], t_plain[0] / tb[0])]
del text, rb, re_, keep

# ---- e: 17 significant digits
text, rb, re_ = rows_sci()
n_ok, t_e = timed(parse(text, rb, re_, WIDE, d_value, d_status))
wide_bits = d_value.cpu().numpy().view(np.uint64).copy()
counts = torch.bincount(d_status.to(torch.int64), minlength=5).tolist()
n_plain, t_e_plain = timed(parse(text, rb, re_, 0, d_value, d_status))
host_ms, host_bits, left = host_route(text, rb, re_, d_value, d_status)
assert n_ok == K and (host_bits == wide_bits).all(), "the host route and the call disagree"
lines += ["", "e  17 significant digits, D.DDDDDDDDDDDDDDDDe[+-]DDD",
          "   with RJ_PARSE_WIDE    %s   ok %d, range %d, inexact %d" % (fmt(t_e), counts[OK], counts[RANGE], counts[INEXACT]),
          "   without the flag      %s   ok %d: the other %d rows are INEXACT and have no value" % (fmt(t_e_plain), n_plain, K - n_plain),
          "   the route it replaces: the call without the flag + the download + float() of the %d INEXACT rows on the host, once:  %.0f ms  (%.0fx); same bits: yes"
          % (left, host_ms, host_ms / t_e[0])]
if base:
    lines += ["   the parent commit's library on these rows (ok %d: the rest INEXACT):  %s" % (base["e_ok"], fmt(tuple(base["e"])))]
del text, rb, re_, wide_bits, host_bits

# ---- f: every fourth row with 25 digits
text, rb, re_ = rows_sci(long_every=4)
n_ok, t_f = timed(parse(text, rb, re_, WIDE, d_value, d_status))
counts = torch.bincount(d_status.to(torch.int64), minlength=5).tolist()
assert sum(counts) == K and counts[OK] == n_ok
lines += ["", "f  as e, every fourth row with 25 significant digits (two products for its bracket)",
          "   with RJ_PARSE_WIDE    %s   ok %d, range %d, inexact %d (%.3f %% of the long rows)" % (fmt(t_f), counts[OK], counts[RANGE], counts[INEXACT],
                                                                                             100.0 * counts[INEXACT] / (K / 4))]
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
