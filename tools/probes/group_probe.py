"""What rj_scan_records_group costs, next to the bytes it must move and next to what a caller does without it, in ONE run on one
box.  Per case: the call into tables of the caller's, warm, timed by events around it, the median (min .. max) of the repeats;
and ONCE, in the same process, the route a caller takes without the call -- rj_scan_records_pack of the same rows, the download,
collections.Counter on the host (host clock; the two routes are checked to agree on G and on the counts).
The model: the rows' bytes twice (the hash, then the compare of every row that is not its string's first) plus the scratch
(record_group.h's layout: 12 bytes per slot, 20 per row); the share of the 6.9 TB/s read-only rate (README) is a recorded
figure, not a promise.
Cases:
  a  10^7 address-like rows of 7..15 bytes, 10^4 distinct values         (also with L = 32, 128)
  b  10^7 rows of 8 bytes, all distinct
  c  10^7 rows, all equal, with the wave peel and without (RJ_GROUP_PEEL=0)
  d  10^5 rows of 4 KiB, 100 distinct values                             (also with L = 32, 128: the wave tier either way)
  e  the skew of tests/test_gpu_record_group.py at 64 MiB: one long row, two equal to it, one that differs in its last byte,
     among 100 000 empty and one-byte rows
    python tools/probes/group_probe.py [million rows] [repeats] [out file]     (default 10 20 profiles/group_probe.txt)"""
import collections
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import rejit_amd

millions = float(sys.argv[1]) if len(sys.argv) > 1 else 10
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "group_probe.txt")
WARM = 3
READ_RATE = 6.9e12
K = int(millions * 1e6)
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b"x"))
lines = ["group_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max); model = 2 x row bytes + scratch"
         % (repeats, WARM),
         "", "| case | rows | distinct | row bytes | call ms (min .. max) | model GB | GB/s | of 6.9 TB/s | pack + download + Counter ms | speed-up |",
         "|---|---|---|---|---|---|---|---|---|---|"]


def slots(k):
    t = 64
    while t < 2 * k:
        t <<= 1
    return t


def pooled_text(pool, picks):
    """rows pool[picks[j]] laid out with one '\\n' behind each -> (text, rec_begin, rec_end) on the device, built by torch ops"""
    lens = torch.tensor([len(p) for p in pool], dtype=torch.int64, device=dev)
    begins = torch.cumsum(lens, 0) - lens
    flat = torch.from_numpy(np.frombuffer(b"".join(pool) + b"\n", dtype=np.uint8).copy()).to(dev)
    ln = lens[picks]
    rb = torch.cumsum(ln + 1, 0) - (ln + 1)
    total = int(rb[-1] + ln[-1] + 1)
    row = torch.repeat_interleave(torch.arange(picks.numel(), device=dev), ln + 1, output_size=total)
    off = torch.arange(total, device=dev) - rb[row]
    src = torch.where(off < ln[row], begins[picks[row]] + off, torch.full_like(off, flat.numel() - 1))
    return flat[src].contiguous(), rb.contiguous(), (rb + ln).contiguous()


def case(name, text, rb, re_, env=None, host=True):
    env = env or {}
    for key, v in env.items():
        os.environ[key] = v
    try:
        k = int(rb.numel())
        g, rep, cnt = scan.group_records(text, rb, re_)
        G = int(rep.numel())
        assert int(cnt.sum()) == k
        d_group = torch.empty(k, dtype=torch.int64, device=dev)
        d_rep = torch.empty(G, dtype=torch.int64, device=dev)
        d_cnt = torch.empty(G, dtype=torch.int64, device=dev)
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ts = []
        for i in range(WARM + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            total = lib.rj_scan_records_group(scan._h, vp(text), int(text.numel()), vp(rb), vp(re_), k, None, 0, vp(d_group), vp(d_rep), vp(d_cnt), G, st)
            e1.record()
            torch.cuda.synchronize()
            assert total == G, total
            if i >= WARM:
                ts.append(e0.elapsed_time(e1))
        assert torch.equal(d_rep, rep) and torch.equal(d_cnt, cnt) and torch.equal(d_group, g)
        row_bytes = int((re_ - rb).sum())
        model = 2 * row_bytes + 12 * slots(k) + 20 * k
        med = float(np.median(ts))
        host_ms = float("nan")
        if host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            packed, _, _ = scan.pack_records(text, rb, re_, fill=10, lead=0, gap=1)
            words = packed.cpu().numpy().tobytes().split(b"\n")
            words.pop()
            counter = collections.Counter(words)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert len(counter) == G and list(counter.values()) == cnt.cpu().tolist(), "the host route and the call disagree"
            del packed, words, counter
        label = name + ("" if not env else " (" + ", ".join("%s=%s" % (a.replace("RJ_GROUP_", ""), b) for a, b in env.items()) + ")")
        line = "| %s | %d | %d | %d | %.3f (%.3f .. %.3f) | %.3f | %.0f | %.1f %% | %s | %s |" % (
            label, k, G, row_bytes, med, min(ts), max(ts), model / 1e9, model / med / 1e6, 100 * model / (med * 1e-3) / READ_RATE,
            "%.0f" % host_ms if host else "-", "%.0fx" % (host_ms / med) if host else "-")
        print(line, flush=True)
        lines.append(line)
    finally:
        for key in env:
            del os.environ[key]


gen = torch.Generator(device=dev).manual_seed(5)
rng = np.random.RandomState(5)
# a
pool = sorted({b"%d.%d.%d.%d" % tuple(rng.randint(1, 255, 4)) for _ in range(10300)})[:10000]
picks = torch.randint(0, len(pool), (K,), device=dev, generator=gen)
text, rb, re_ = pooled_text(pool, picks)
case("a addresses", text, rb, re_)
for L in ("32", "128"):
    case("a addresses", text, rb, re_, env={"RJ_GROUP_LONG_BYTES": L}, host=False)
del text, rb, re_, picks
# b: row j = the eight base-26 digits of j
j = torch.arange(K, device=dev)
digits = torch.stack([(j // 26 ** p) % 26 + ord("a") for p in range(8)] + [torch.full_like(j, 10)], dim=1).to(torch.uint8)
text = digits.reshape(-1).contiguous()
rb = (9 * j).contiguous()
case("b all distinct", text, rb, (rb + 8).contiguous())
# c
text = torch.from_numpy(np.frombuffer(b"10.0.0.1\n" * K, dtype=np.uint8).copy()).to(dev)
case("c all equal", text, rb, (rb + 8).contiguous())
case("c all equal", text, rb, (rb + 8).contiguous(), env={"RJ_GROUP_PEEL": "0"}, host=False)
del text, rb, j, digits
# d
k_d = max(K // 100, 100)
pool_d = torch.randint(ord("a"), ord("z") + 1, (100, 4096), dtype=torch.uint8, device=dev, generator=gen)
text = pool_d[torch.randint(0, 100, (k_d,), device=dev, generator=gen)].reshape(-1).contiguous()
rb = (4096 * torch.arange(k_d, device=dev)).contiguous()
case("d 4 KiB rows", text, rb, (rb + 4096).contiguous())
for L in ("32", "128"):
    case("d 4 KiB rows", text, rb, (rb + 4096).contiguous(), env={"RJ_GROUP_LONG_BYTES": L}, host=False)
del text, rb, pool_d
# e
big = 64 << 20
body = torch.randint(ord("a"), ord("z") + 1, (big,), dtype=torch.uint8, device=dev, generator=gen)
other = body.clone()
other[-1] = ord("A")
small = torch.randint(ord("a"), ord("e") + 1, (50000,), dtype=torch.uint8, device=dev, generator=gen)
text = torch.cat([body, body, small, other]).contiguous()
at = 2 * big + torch.arange(50000, device=dev)
rb = torch.cat([torch.stack([at, at], dim=1).reshape(-1), torch.tensor([0, big, 2 * big + 50000, 0], device=dev)]).contiguous()
re_ = torch.cat([torch.stack([at + 1, at], dim=1).reshape(-1), torch.tensor([big, 2 * big, 3 * big + 50000, big], device=dev)]).contiguous()
case("e skew, 64 MiB rows", text, rb, re_)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
