"""What rj_scan_records_sort costs, next to the bytes it must move and next to what a caller does without it, in ONE run on one
box.  Per case: the call into a table of the caller's, warm, timed by events around it, the median (min .. max) of the repeats;
and ONCE, in the same process, the route a caller takes without the call -- rj_scan_records_pack of the same rows, the download,
Python's sorted over the rows on the host (host clock; stable, so the two routes are checked to give the SAME order).
The model, from the call's own stats (rounds, keyed_rows, skip_rows): per round the k flags of the compaction; per keyed row
93 bytes of lists, tables and one 16-byte group of text plus 8 radix passes over 16 bytes read and written (the passes by the
segment number are not counted); per skipped row two groups of text.  The share of the 6.9 TB/s read-only rate (README) is a
recorded figure, not a promise.
Cases:
  a  10^7 address-like rows of 7..15 bytes, 10^4 distinct values         (also with L = 32, 128; also records.sorted_groups)
  b  10^7 rows of 8 bytes, all distinct
  c  10^7 rows, all equal                                                (also with RJ_SORT_SKIP=0)
  d  10^5 rows of 4 KiB, 100 distinct values                             (also with RJ_SORT_SKIP=0)
  f  10^7 URL-like rows of 40 bytes behind a shared 30-byte prefix       (also with RJ_SORT_SKIP=0)
Every environment configuration runs in a child process of its own, one at a time.
    python tools/probes/sort_probe.py [million rows] [repeats] [out file]     (default 10 20 profiles/sort_probe.txt)"""
import ctypes
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
WARM = 3
READ_RATE = 6.9e12
HEAD = ["| case | rows | row bytes | rounds | keyed rows | call ms (min .. max) | model GB | GB/s | of 6.9 TB/s | pack + download + sorted ms | speed-up |",
        "|---|---|---|---|---|---|---|---|---|---|---|"]
CONFIGS = [({}, "a,b,c,d,f,g"), ({"RJ_SORT_SKIP": "0"}, "c,d,f"), ({"RJ_SORT_LONG_BYTES": "32"}, "a"), ({"RJ_SORT_LONG_BYTES": "128"}, "a")]


def parent(argv):
    millions = argv[0] if len(argv) > 0 else "10"
    repeats = argv[1] if len(argv) > 1 else "20"
    out_path = argv[2] if len(argv) > 2 else os.path.join(HERE, "..", "..", "profiles", "sort_probe.txt")
    lines = ["sort_probe: %s repeats after %d warm-up calls, events around the call; ms, median (min .. max); one child process per environment"
             % (repeats, WARM), ""] + HEAD
    for env, cases in CONFIGS:
        child_env = dict(os.environ)
        child_env.update(env)
        label = ", ".join("%s=%s" % (a.replace("RJ_SORT_", ""), b) for a, b in env.items())
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cases, millions, repeats, label], env=child_env, stdout=subprocess.PIPE)
        if r.returncode != 0:
            sys.exit("sort_probe: the child for {%s} ended with %d" % (label, r.returncode))
        for ln in r.stdout.decode().splitlines():
            print(ln, flush=True)
            if ln.startswith("| "):
                lines.append(ln)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def child(cases, millions, repeats, label):
    import numpy as np
    import torch

    import rejit_amd
    from rejit_amd import records

    K = int(float(millions) * 1e6)
    dev = torch.device("cuda:0")
    lib = rejit_amd.load_library()
    scan = rejit_amd.Scan(rejit_amd.Program(b"x"))
    gen = torch.Generator(device=dev).manual_seed(5)
    rng = np.random.RandomState(5)

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

    def timed(call):
        ts = []
        for i in range(WARM + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= WARM:
                ts.append(e0.elapsed_time(e1))
        return ts

    def report(name, k, row_bytes, stats, ts, host_ms):
        model = stats["rounds"] * k + stats["keyed_rows"] * (93 + 8 * 32) + stats["skip_rows"] * 32
        med = float(np.median(ts))
        print("| %s | %d | %d | %d | %d | %.3f (%.3f .. %.3f) | %.3f | %.0f | %.1f %% | %s | %s |" % (
            name + (" (%s)" % label if label else ""), k, row_bytes, stats["rounds"], stats["keyed_rows"], med, min(ts), max(ts), model / 1e9,
            model / med / 1e6, 100 * model / (med * 1e-3) / READ_RATE, "-" if host_ms is None else "%.0f" % host_ms,
            "-" if host_ms is None else "%.1fx" % (host_ms / med)), flush=True)

    def case(name, text, rb, re_, host):
        k = int(rb.numel())
        order, stats = scan.sort_records(text, rb, re_, stats=True)
        d_order = torch.empty(k, dtype=torch.int64, device=dev)
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            assert lib.rj_scan_records_sort(scan._h, vp(text), int(text.numel()), vp(rb), vp(re_), k, None, 0, vp(d_order), None, st) == k
        ts = timed(call)
        assert torch.equal(d_order, order)
        host_ms = None
        if host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            packed, _, _ = scan.pack_records(text, rb, re_, fill=10, lead=0, gap=1)
            words = packed.cpu().numpy().tobytes().split(b"\n")
            words.pop()
            host_order = sorted(range(k), key=words.__getitem__)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(np.array(host_order, dtype=np.int64), order.cpu().numpy()), "the host route and the call disagree"
            del packed, words, host_order
        report(name, k, int((re_ - rb).sum()), stats, ts, host_ms)

    host = not label          # the host route does not depend on the knobs: once, in the default configuration
    if "a" in cases or "g" in cases:
        pool = sorted({b"%d.%d.%d.%d" % tuple(rng.randint(1, 255, 4)) for _ in range(10300)})[:10000]
        picks = torch.randint(0, len(pool), (K,), device=dev, generator=gen)
        text, rb, re_ = pooled_text(pool, picks)
        if "a" in cases:
            case("a addresses", text, rb, re_, host)
        if "g" in cases:
            # group, then sort the G distinct rows: `sort | uniq -c`; the stats are the sort's over the representatives
            rep, count, group = records.sorted_groups(scan, text, rb, re_)
            _, stats = scan.sort_records(text, rb, re_, indices=scan.group_records(text, rb, re_)[1], stats=True)
            ts = timed(lambda: records.sorted_groups(scan, text, rb, re_))
            packed, _, _ = scan.pack_records(text, rb, re_, indices=rep, fill=10, lead=0, gap=1)
            assert packed.cpu().numpy().tobytes().split(b"\n")[:-1] == pool and int(count.sum()) == K
            report("a addresses, records.sorted_groups (the model: the sort of the %d distinct rows alone)" % rep.numel(), K, int((re_ - rb).sum()), stats, ts, None)
        del text, rb, re_, picks
    j = torch.arange(K, device=dev)
    rb9 = (9 * j).contiguous()
    if "b" in cases:      # row j = the eight base-26 digits of j, least significant first: no order in the input
        digits = torch.stack([(j // 26 ** p) % 26 + ord("a") for p in range(8)] + [torch.full_like(j, 10)], dim=1).to(torch.uint8)
        case("b all distinct", digits.reshape(-1).contiguous(), rb9, (rb9 + 8).contiguous(), host)
        del digits
    if "c" in cases:
        text = torch.from_numpy(np.frombuffer(b"10.0.0.1\n" * K, dtype=np.uint8).copy()).to(dev)
        case("c all equal", text, rb9, (rb9 + 8).contiguous(), host)
        del text
    if "d" in cases:
        k_d = max(K // 100, 100)
        pool_d = torch.randint(ord("a"), ord("z") + 1, (100, 4096), dtype=torch.uint8, device=dev, generator=gen)
        text = pool_d[torch.randint(0, 100, (k_d,), device=dev, generator=gen)].reshape(-1).contiguous()
        rb = (4096 * torch.arange(k_d, device=dev)).contiguous()
        case("d 4 KiB rows", text, rb, (rb + 4096).contiguous(), host)
        del text, rb, pool_d
    if "f" in cases:      # 30 shared bytes, six letters, a slash, three digits
        prefix = torch.from_numpy(np.frombuffer(b"https://www.example.com/items/", dtype=np.uint8).copy()).to(dev)
        assert prefix.numel() == 30
        rows = torch.empty((K, 41), dtype=torch.uint8, device=dev)
        rows[:, :30] = prefix
        rows[:, 30:36] = torch.randint(ord("a"), ord("z") + 1, (K, 6), dtype=torch.uint8, device=dev, generator=gen)
        rows[:, 36] = ord("/")
        rows[:, 37:40] = torch.randint(ord("0"), ord("9") + 1, (K, 3), dtype=torch.uint8, device=dev, generator=gen)
        rows[:, 40] = 10
        rb = (41 * j).contiguous()
        case("f URLs, 30 shared bytes", rows.reshape(-1), rb, (rb + 40).contiguous(), host)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2].split(","), sys.argv[3], int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else "")
    else:
        parent(sys.argv[1:])
