"""What rj_scan_records_lookup costs, next to the bytes it must move and next to what a caller does without it, in ONE run on one
box.  Per case: the call into tables of the caller's, warm, timed by events around it, the median (min .. max) of the repeats;
and, in the same process and checked to give the same index, two routes a caller has without the call:
  (i)  on one shared text, Scan.group_records over the set's and the probe's rows in one table, then torch: a probe row's group,
       that group's representative, taken when it is a set row (events around the route, the median of a few runs);
  (ii) rj_scan_records_pack of both tables, the downloads, a Python dict on the host (host clock, once).
Both tables of a case lie in ONE device text, the set's rows in front, so that (i) can run; the lookup gets that text twice.
The model: the set side as the group call's (its rows' bytes twice, 12 bytes per slot, 20 per set row); the probe rows' bytes
once for the hash and, for a row that is found, once more for the compare together with the set row's; 16 bytes per probe row
(the staged answer written and read, the index written); with hit counts 4 bytes per slot and 8 per set row more.  The share of
the 6.9 TB/s read-only rate (README) is a recorded figure, not a promise.
Cases:
  a  10^7 address-like probe rows of 7..15 bytes against a dictionary of 10^4                (a dictionary encode)
  b  10^7 rows of 8 bytes against 10^7, all distinct on both sides, half of the probe rows present
  c  10^7 probe rows, all equal to one of 100 set rows: with hit counts, without (is_in), and with RJ_GROUP_PEEL=0
  d  10^5 rows of 4 KiB against 100
    python tools/probes/lookup_probe.py [million rows] [repeats] [out file]     (default 10 20 profiles/lookup_probe.txt)"""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "lookup_probe.txt")
WARM = 3
GROUP_RUNS = 5
READ_RATE = 6.9e12
K = int(millions * 1e6)
dev = torch.device("cuda:0")
lib = rejit_amd.load_library()
scan = rejit_amd.Scan(rejit_amd.Program(b"x"))
lines = ["lookup_probe: %d repeats after %d warm-up calls, events around the call; ms, median (min .. max); the model is the file's docstring's"
         % (repeats, WARM),
         "(i) = group_records over both tables in one + torch, median of %d; (ii) = pack + download + dict, once; both give the call's index" % GROUP_RUNS,
         "", "| case | set rows | probe rows | found | probe row bytes | call ms (min .. max) | model GB | GB/s | of 6.9 TB/s | (i) ms | (i) / call | (ii) ms | (ii) / call |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]


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


def shared(set_text, set_rb, set_re, text, rb, re_):
    """both tables over one text, the set's part in front"""
    off = int(set_text.numel())
    return torch.cat([set_text, text]).contiguous(), set_rb, set_re, (rb + off).contiguous(), (re_ + off).contiguous()


def case(name, text, set_rb, set_re, rb, re_, hits=True, env=None, others=True):
    env = env or {}
    for key, v in env.items():
        os.environ[key] = v
    try:
        ks, kp = int(set_rb.numel()), int(rb.numel())
        answer = scan.lookup_records(text, set_rb, set_re, text, rb, re_, hits=hits)
        index = answer[0] if hits else answer
        d_index = torch.empty(kp, dtype=torch.int64, device=dev)
        d_hits = torch.empty(ks, dtype=torch.int64, device=dev) if hits else None
        vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        n = int(text.numel())
        ts = []
        for i in range(WARM + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            found = lib.rj_scan_records_lookup(scan._h, vp(text), n, vp(set_rb), vp(set_re), ks, None, 0, vp(text), n, vp(rb), vp(re_), kp, None, 0,
                                               vp(d_index), vp(d_hits), None, st)
            e1.record()
            torch.cuda.synchronize()
            assert found >= 0, lib.rj_last_error()
            if i >= WARM:
                ts.append(e0.elapsed_time(e1))
        assert torch.equal(d_index, index) and found == int((index >= 0).sum())
        if hits:
            assert torch.equal(d_hits, answer[1]) and int(d_hits.sum()) == found
        set_bytes, probe_bytes = int((set_re - set_rb).sum()), int((re_ - rb).sum())
        found_bytes = int(((re_ - rb) * (index >= 0)).sum())
        model = 2 * set_bytes + 12 * slots(ks) + 20 * ks + probe_bytes + 2 * found_bytes + 16 * kp + ((4 * slots(ks) + 8 * ks) if hits else 0)
        med = float(np.median(ts))
        group_ms = host_ms = float("nan")
        if others:
            # (i) the group call over both tables in one, and the torch post-processing
            all_rb, all_re = torch.cat([set_rb, rb]).contiguous(), torch.cat([set_re, re_]).contiguous()
            gs = []
            for i in range(1 + GROUP_RUNS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                group, rep, _ = scan.group_records(text, all_rb, all_re)
                first = rep[group[ks:]]
                via_group = torch.where(first < ks, first, torch.full_like(first, -1))
                e1.record()
                torch.cuda.synchronize()
                if i >= 1:
                    gs.append(e0.elapsed_time(e1))
            assert torch.equal(via_group, index), "the group route and the call disagree"
            group_ms = float(np.median(gs))
            del all_rb, all_re, group, rep, first, via_group
            # (ii) pack both, download, a dict on the host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            packed, _, _ = scan.pack_records(text, set_rb, set_re, fill=10, lead=0, gap=1)
            set_words = packed.cpu().numpy().tobytes().split(b"\n")
            set_words.pop()
            packed, _, _ = scan.pack_records(text, rb, re_, fill=10, lead=0, gap=1)
            words = packed.cpu().numpy().tobytes().split(b"\n")
            words.pop()
            firsts = {}
            for i, w in enumerate(set_words):
                firsts.setdefault(w, i)
            via_host = np.fromiter((firsts.get(w, -1) for w in words), dtype=np.int64, count=len(words))
            host_ms = (time.perf_counter() - t0) * 1e3
            assert (via_host == index.cpu().numpy()).all(), "the host route and the call disagree"
            del packed, set_words, words, firsts, via_host
        label = name + ("" if hits else ", no hits") + ("" if not env else " (" + ", ".join("%s=%s" % (a.replace("RJ_GROUP_", ""), b) for a, b in env.items()) + ")")
        line = "| %s | %d | %d | %d | %d | %.3f (%.3f .. %.3f) | %.3f | %.0f | %.1f %% | %s | %s | %s | %s |" % (
            label, ks, kp, found, probe_bytes, med, min(ts), max(ts), model / 1e9, model / med / 1e6, 100 * model / (med * 1e-3) / READ_RATE,
            "%.3f" % group_ms if others else "-", "%.1fx" % (group_ms / med) if others else "-",
            "%.0f" % host_ms if others else "-", "%.0fx" % (host_ms / med) if others else "-")
        print(line, flush=True)
        lines.append(line)
    finally:
        for key in env:
            del os.environ[key]


gen = torch.Generator(device=dev).manual_seed(5)
rng = np.random.RandomState(5)
# a: the dictionary's rows are the pool itself, the probe rows are drawn from it (every one is present)
pool = sorted({b"%d.%d.%d.%d" % tuple(rng.randint(1, 255, 4)) for _ in range(10300)})[:10000]
s_text, s_rb, s_re = pooled_text(pool, torch.arange(len(pool), device=dev))
picks = torch.randint(0, len(pool), (K,), device=dev, generator=gen)
p_text, p_rb, p_re = pooled_text(pool, picks)
case("a dictionary encode", *shared(s_text, s_rb, s_re, p_text, p_rb, p_re))
case("a dictionary encode", *shared(s_text, s_rb, s_re, p_text, p_rb, p_re), hits=False, others=False)
del s_text, s_rb, s_re, p_text, p_rb, p_re, picks


def digits_text(values):
    """row j = the eight base-26 digits of values[j], a line break behind it"""
    d = torch.stack([(values // 26 ** p) % 26 + ord("a") for p in range(8)] + [torch.full_like(values, 10)], dim=1).to(torch.uint8)
    rb = 9 * torch.arange(values.numel(), device=dev)
    return d.reshape(-1).contiguous(), rb.contiguous(), (rb + 8).contiguous()


# b: set row i = 2 i, probe row j = j: the even probe rows are present
j = torch.arange(K, device=dev)
case("b all distinct, half present", *shared(*digits_text(2 * j), *digits_text(j)))
case("b all distinct, half present", *shared(*digits_text(2 * j), *digits_text(j)), hits=False, others=False)
# c
s_text, s_rb, s_re = digits_text(torch.arange(100, device=dev))
p_text, p_rb, p_re = digits_text(torch.full((K,), 57, device=dev))
case("c all equal to one set row", *shared(s_text, s_rb, s_re, p_text, p_rb, p_re))
case("c all equal to one set row", *shared(s_text, s_rb, s_re, p_text, p_rb, p_re), hits=False, others=False)
case("c all equal to one set row", *shared(s_text, s_rb, s_re, p_text, p_rb, p_re), env={"RJ_GROUP_PEEL": "0"}, others=False)
del s_text, s_rb, s_re, p_text, p_rb, p_re, j
# d
k_d = max(K // 100, 100)
pool_d = torch.randint(ord("a"), ord("z") + 1, (200, 4096), dtype=torch.uint8, device=dev, generator=gen)
pool_d[:, 4095] = 10
s_rb = (4096 * torch.arange(100, device=dev)).contiguous()
p_rb = (4096 * torch.arange(k_d, device=dev)).contiguous()
p_text = pool_d[torch.randint(0, 200, (k_d,), device=dev, generator=gen)].reshape(-1).contiguous()      # half of the probe rows are present
case("d 4 KiB rows", *shared(pool_d[:100].reshape(-1).contiguous(), s_rb, (s_rb + 4095).contiguous(), p_text, p_rb, (p_rb + 4095).contiguous()))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
