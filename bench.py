#!/usr/bin/env python3
"""bench.py -- the headline measurement (BASELINE.json: "GB/s text scanned + matches/s,
regexdna 50M-line input, 1/2/4/8 MI355X").

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload regexdna|literal|complex|jrep] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

One STEP = one pass of the hot path over one batch of synthetic input.  Default workload (the one
BASELINE's metric is quoted on, configs[2]): the nine regex-dna patterns (reference
sample/regexdna.cc:51-67), one MatchAllCount each, over the stripped 50M-line FASTA text (500 MB per
GPU), resident in HBM when the timed region starts.  With N GPUs the text is N x 500 MB (weak
scaling), cut into contiguous byte ranges with a halo of max_match_len-1 bytes; the exchange step is
one RCCL all_gather of 8 integers per pattern written on the device (count + first / last match, which
carries the left-most-longest selection over the cuts; sharding.CarryExchange).  Rank 0 prints ONE JSON
line.  Without a launcher, --gpus N > 1 spawns the N ranks itself.

Other workloads (same contract; what an 8-GPU run of BASELINE configs[3] / [4] / [1] uses):
  --workload complex   ([complex]|(regexp)){2,7}abcdefgh(...) MatchAll, --literal-bytes per GPU
                       (6.25 GB at N=8), 57-byte halo, spans gathered to rank 0 as tensors
  --workload jrep      grep over a synthetic source tree (--tree-files files, ~20 KB each, per GPU),
                       file-sharded, host buffers: rj_match_all_batch + the `^` line table of the files
                       with matches, output gathered to rank 0
  --workload literal   literal `regexp` MatchAll over --literal-bytes per GPU

The headline step is ONE kernel over the text for all nine patterns: regexdna asks MatchAllCount (reference
sample/regexdna.cc:65), and for counts plane_count scans, classifies its candidates by table lookup and counts
(rj_multi_set_counts_only; plane_count.hip), a small kernel on the object's own stream adds the workgroups' rows up.
`--span-lists` / `step_variants_ms.span_lists`: round 4's loop, which lays out every pattern's (begin, end) list
(plane_scan + classify_shared_multi + offsets_gather_check_multi).

A plain run sets up, runs the step loop untimed (--settle-ms, then W warm-up steps), times the K steps and prints the
line; `--dump-outputs DIR` then writes what the last timed step computed (regexdna: matches_per_pass.npy, the nine
counts, and match_bounds.npy, per pattern the first / last match; literal / complex: spans.npy; jrep:
files_with_matches.npy, output_bytes.npy).  Everything else -- the entries below from cpu_baseline on, the same-run
read-only ceiling, the parity checks, the multi-rank latency -- runs only with `--full`.  Besides the contract fields
the line carries
  physical_GBps / step_frac -- n / t of the step: every text byte crosses the HBM interface once per step
  roofline      -- the dominant kernel (plane_count<ExactShape<2>>): the text's bytes (1 byte read per text byte and pass,
                   SURVEY.md section 8d) / the launch's average duration from HIP events on the run's stream,
                   traffic = FETCH_SIZE x 2 per launch from profiles/pmc_traffic.json; read_only_ceiling /
                   frac_of_ceiling (--full): against a kernel that only reads the same bytes, measured in this run (`hbm_ceiling`;
                   since round 6 with non-temporal loads, as the scans load: 6.9 TB/s; `default_policy_GB_per_s` beside it
                   is what rounds 1-5 quoted, 6.0-6.3)
  roofline_valu -- the same launch against the VALU peak (SQ_INSTS_VALU per byte from profiles/)
  cpu_baseline  -- the REAL reference (oracle/_ref, built from /root/reference) on the host: one core (>= 0.5 s of
                   work) and all cores over disjoint slices, on a bounded sample of the same text
  train / separate_launches / serial_calls / interleaved / overlapped -- the other ways to get the nine counts
  hbm_not_cache / one_pass_2p5gb -- per-pattern kernels and the one pass on a 2.5 GB text (10x the Infinity Cache)
  literal_scan / literal_50gb / complex_scan / behind_scan / dense_scan / line_table -- BASELINE configs[1] (5 GB and
                   the north star's 50 GB), configs[3]'s shape on one GPU and the other scan modes, each with
                   median / min of >= 10 calls, the first call, its roofline and CPU baseline
  jrep_10gb / end_to_end -- BASELINE configs[4] at full size on one GPU (host buffers, PCIe included) and the
                   reference's regexdna.cc unchanged on the library next to the published number
  parity_full_size -- the GPU's answers == the real reference's at BASELINE size (tests/golden/fullsize_vectors.json)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md
VALU_PEAK_TOPS = 78.6        # 256 CUs x 4 SIMD-32 x 32 lanes/clk x 2.4 GHz simple 32-bit VALU lane-ops per second (same guide:
                             # a wave64 instruction issues over 2 cycles; = the 157.3 TFLOP/s FP32 vector peak / 2 flops per FMA)
# ... and what this device issues when asked (round 5, tools/probes/valu_rate.hip, profiles/r05_valu_rate.txt: eight independent
# chains per lane, 8 waves per SIMD): v_and / v_xor / v_add 3.1-3.3 cycles per wave64 instruction, v_alignbit / v_dot4_u32_u8 /
# v_bitop3 / v_and_or / v_bfi / shifts / DPP moves 4.0-4.5 -- 35-39 T lane-ops/s for the mix these kernels are made of.
VALU_MEASURED_TOPS = 37.0


def pmc_traffic(key, **match):
    """HBM bytes per launch of the dominant kernel, measured with rocprofv3 --pmc FETCH_SIZE in a
    separate pass and corrected as the guide prescribes (x2 on gfx950); committed under
    profiles/.  Reported only when the profiled configuration is the one being run, else null."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))[key]
        if all(rec.get(k) == v for k, v in match.items()):
            return int(rec["hbm_read_bytes_per_launch"])
    except Exception:
        pass
    return None


def pmc_valu(key):
    """VALU lane-operations per text byte of a kernel (SQ_INSTS_VALU x 64 / text bytes, a separate rocprofv3 --pmc pass:
    tools/profile_round.sh + collect_profiles.py -> profiles/pmc_traffic.json); None when that kernel was not profiled."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))[key]
        return float(rec["valu_ops_per_text_byte"]), rec.get("valu_source", "profiles/pmc_traffic.json")
    except Exception:
        return None


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="regexdna", choices=["regexdna", "literal", "complex", "jrep"])
    ap.add_argument("--fasta-n", type=int, default=50_000_000, help="FASTA size parameter per GPU (50M = 500 MB stripped)")
    ap.add_argument("--literal-bytes", type=int, default=5_000_000_000, help="text bytes per GPU of the literal / complex workloads")
    ap.add_argument("--big-literal-bytes", type=int, default=50_000_000_000, help="the north star's 50 GB single-GPU scan (extra)")
    ap.add_argument("--tree-files", type=int, default=12_500, help="jrep workload: files per GPU (~20 KB each)")
    ap.add_argument("--in-flight", type=int, default=2, help="steps kept in flight by the headline loop (rj_multi objects used in turn)")
    ap.add_argument("--settle-ms", type=float, default=600.0, help="untimed run of the step loop before the W warm-up and K timed steps (device clocks)")
    ap.add_argument("--time-all-launches", action="store_true", help="headline loop: the start event on every scan launch (default: every second one)")
    ap.add_argument("--span-lists", action="store_true", help="headline loop as in round 4: the span pipeline (plane_scan + classify + gather: every "
                    "pattern's (begin, end) list) instead of MatchAllCount in one kernel (plane_count)")
    ap.add_argument("--one-stream", action="store_true", help="headline loop as in round 3: both rj_multi objects and their tails on one stream")
    ap.add_argument("--jrep-files", type=int, default=100_000, help="jrep_10gb extra: files (BASELINE configs[4]: 100 000)")
    ap.add_argument("--jrep-bytes", type=int, default=10_000_000_000, help="jrep_10gb extra: total bytes (BASELINE configs[4]: 10 GB)")
    ap.add_argument("--jrep-threads", type=int, default=1, help="jrep_10gb extra: caller threads, each with its own batches (the reference's jrep -j)")
    ap.add_argument("--no-extra", action="store_true", help="headline only")
    ap.add_argument("--tail-streams-probe", action="store_true", help="internal: the child process of the tails_on_own_streams extra")
    ap.add_argument("--no-big", action="store_true", help="skip the 50 GB and 2.5 GB extras")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--serial-calls", action="store_true", help="headline with nine synchronous rj_scan_run calls per step "
                    "instead of one rj_multi_run (separate scans, batched tails)")
    ap.add_argument("--cpu-sample-mib", type=int, default=64)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL); gloo only for "
                    "functional tests of the multi-rank path on a 1-GPU box together with --same-device")
    ap.add_argument("--same-device", action="store_true", help="testing only: every rank uses cuda:0")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: the extras, the CPU baseline, the same-run "
                    "read-only ceiling and the parity checks (--no-extra / --no-big / --no-cpu-baseline trim it); without it a run "
                    "sets up, warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps: what the last timed step computed, as DIR/<name>.npy "
                    "(float64; a seeded sample when larger than 64 MB in all)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------ CPU side
def _ref():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import checkers
    if not checkers.have_ref():
        return None, checkers
    # default flags except use_ff_reduce=0: the fast-forward configuration whose counts are correct
    # (SURVEY.md section 4.4, Q1); compile time excluded as in the reference harness
    return checkers.Ref(use_ff=1, ff_early=1, ff_reduce=0, parser_opt=1), checkers


def cpu_baseline(text_host: bytes, patterns, sample_desc: str, all_cores: bool = True, one_core_bytes: int = 64 << 20):
    """The reference's own x86 SIMD path on the GPU box's host (kind "reference"): ONE core over the first
    `one_core_bytes` of the sample, repeated until at least 0.5 s of work has been timed, and ALL cores the way
    sample/regexdna-multithread.cc:117-167 uses them -- independent Regej objects on independent threads -- here every
    hardware thread scans ITS OWN slice of the sample (disjoint slices: the whole sample is scanned once per
    pattern, from DRAM, not a cache-resident copy).  When the prebuilt oracle/_ref library is absent: our C
    restatement on one core (kind "port")."""
    ref, checkers = _ref()
    host_threads = os.cpu_count() or 1
    if ref is None:
        oracle = checkers.Oracle()
        n = min(len(text_host), 4 << 20)
        t0 = time.perf_counter()
        counts = [oracle.count(rx.encode(), text_host[:n]) for rx in patterns]
        dt = time.perf_counter() - t0
        return dict(value=len(patterns) * n / dt / 1e9, unit="GB/s", cores=1, kind="port", host_cores=host_threads,
                    sample=f"first {n} bytes of rank 0's text (oracle/_ref not present)", seconds=round(dt, 3)), None, n
    import ctypes
    total = len(text_host)
    buf = ctypes.create_string_buffer(text_host, total)
    addr = ctypes.addressof(buf)
    fn = ref.lib.ref_match_all_repeat
    fn.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    n1 = min(total, one_core_bytes)
    counts, passes, dt = [], 0, 0.0
    while dt < 0.5:                       # whole passes over the one-core sample until half a second is on the clock
        t0 = time.perf_counter()
        counts = [int(fn(rx.encode(), addr, n1, 1)) for rx in patterns]
        dt += time.perf_counter() - t0
        passes += 1
    out = dict(value=passes * len(patterns) * n1 / dt / 1e9, unit="GB/s", cores=1, kind="reference", host_cores=host_threads,
               sample=sample_desc + "; first %d bytes, %d pass(es); reference flags use_fast_forward=1 use_ff_reduce=0" % (n1, passes),
               seconds=round(dt, 3))
    # the same core over a sample that does NOT fit its caches (one pass over up to 1 GiB, from DRAM): the number the GPU's
    # HBM-streaming figure sits beside; the 64 MiB sample above is L3-resident on this host and flatters the CPU
    n_dram = min(total, 1 << 30)
    if n_dram > 2 * n1:
        t0 = time.perf_counter()
        for rx in patterns:
            fn(rx.encode(), addr, n_dram, 1)
        dtd = time.perf_counter() - t0
        out["one_core_dram_resident"] = dict(value=len(patterns) * n_dram / dtd / 1e9, unit="GB/s", cores=1,
                                             sample="ONE pass over the first %d bytes of the same text, every pattern" % n_dram, seconds=round(dtd, 3))
    if all_cores and host_threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        threads = host_threads
        step = -(-total // threads)
        overlap = 64                      # (a slice sees a few bytes of the next one: matches across the cut are counted once)
        slices = [(i * step, min(total, (i + 1) * step + overlap) - i * step) for i in range(threads) if i * step < total]

        def work(sl):
            return [int(fn(rx.encode(), addr + sl[0], sl[1], 1)) for rx in patterns]

        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(work, slices[:8]))      # warm the pool
            t0 = time.perf_counter()
            list(pool.map(work, slices))
            dta = time.perf_counter() - t0
        out["all_cores"] = dict(value=len(patterns) * total / dta / 1e9, unit="GB/s", cores=len(slices),
                                sample="%d disjoint slices of the %d-byte sample, one per hardware thread, every pattern over every slice "
                                       "(independent Regej per call)" % (len(slices), total), seconds=round(dta, 3))
    return out, counts, n1


# ------------------------------------------------------------------------------------------ helpers
def fullsize_fixture():
    try:
        return json.load(open(os.path.join(ROOT, "tests", "golden", "fullsize_vectors.json")))
    except Exception:
        return None


class Ctx:
    pass


def setup(args):
    import torch
    import torch.distributed as dist
    c = Ctx()
    c.torch, c.dist = torch, dist
    c.world = int(os.environ.get("WORLD_SIZE", "1"))
    c.rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert c.world == args.gpus, "WORLD_SIZE %d != --gpus %d" % (c.world, args.gpus)
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    if args.same_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    c.dev = torch.device("cuda", local_rank)
    c.cdev = c.dev if args.backend == "nccl" else torch.device("cpu")   # where collective buffers live
    if c.world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=c.dev)
        else:
            dist.init_process_group(args.backend)
    c.stream = torch.cuda.current_stream(c.dev).cuda_stream
    return c


def barrier(c):
    if c.world > 1:
        c.dist.barrier()
    c.torch.cuda.synchronize(c.dev)


def timed(c, args, step, finish=None):
    """W warm-up steps, then exactly K timed steps between barrier + synchronize; max over ranks."""
    for _ in range(args.warmup):
        step(False)
    if finish:
        finish()
    barrier(c)
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = step(True)
    if finish:
        last = finish() or last
    barrier(c)
    elapsed = time.perf_counter() - t0
    if c.world > 1:
        tmax = c.torch.tensor([elapsed], dtype=c.torch.float64, device=c.cdev)
        c.dist.all_reduce(tmax, op=c.dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    return elapsed, last


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: every array as path/<name>.npy in float64 (exact for the counts and byte offsets here); when the
    whole would pass 64 MB, each array keeps a fixed, seeded sample of its rows (sorted, so runs compare row for row)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > DUMP_LIMIT_BYTES and a.ndim > 0 and a.shape[0] > 1:
            keep = max(1, int(a.shape[0] * DUMP_LIMIT_BYTES / total))
            a = a[np.sort(np.random.default_rng(12345).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


def base_line(args, c, metric, value, elapsed, config):
    return {"metric": metric, "value": round(value, 3), "unit": "GB/s", "n_gpus": c.world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic", "config": config,
            "scaling_measured": "no SCALE record exists yet: multi-GPU numbers are unmeasured until the driver runs N=1,2,4,8"}


_CEILING = {}


def hbm_ceiling(ptr, n, stream):
    """The achievable ceiling of a read-only stream over THIS text on THIS device in THIS run: a kernel that
    only reads -- 16 bytes per lane and load, non-temporal policy (csrc/stream_load.h: what the scans use), XOR-reduced
    (tools/probes/read_probe.hip: librejit_bench.so, not the product library) --, GB/s, memoised per size."""
    import rejit_amd
    if n not in _CEILING:
        try:
            ms = rejit_amd.stream_read_probe(ptr, n, 10, stream)
            _CEILING[n] = n / (ms * 1e-3) / 1e9 if ms > 0 else None
        except Exception:
            _CEILING[n] = None
    return _CEILING[n]


def hbm_roofline(kernel, bytes_per_launch, avg_ms, traffic=None, launches=None, ceiling=None):
    ach = bytes_per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    r = {"bound": "hbm", "kernel": kernel, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic, "avg_launch_ms": round(avg_ms, 5),
         "bytes_per_launch": int(bytes_per_launch)}
    if launches is not None:
        r["launches_timed"] = launches
    if ceiling:
        # beside the spec peak: what a kernel that does nothing but read the same bytes reaches here, now
        r["read_only_ceiling"] = round(ceiling, 1)
        r["frac_of_ceiling"] = round(ach / ceiling, 4)
    return r


# ------------------------------------------------------------------------------------------ regexdna
def run_regexdna(args, c):
    import rejit_amd
    from rejit_amd import sharding, workloads as W
    torch, dist = c.torch, c.dist
    world, rank, dev = c.world, c.rank, c.dev
    patterns = W.REGEXDNA_PATTERNS
    progs = [rejit_amd.Program(rx) for rx in patterns]
    scans = [rejit_amd.Scan(p) for p in progs]
    max_len = max(p.info()["max_len"] for p in progs)

    # ---- input: N x (10 * fasta_n) bytes of stripped FASTA, rank r holds its range + halo
    n_fa = args.fasta_n * world
    n_total = W.fasta_stripped_size(n_fa)
    ranges = sharding.partition(n_total, world)
    own = ranges[rank]
    vis_lo, vis_hi = sharding.visible_range(n_total, own, max_len, whole_text=any(p.info()["ring_artefact_risk"] for p in progs))
    text = W.fasta_stripped_torch(n_fa, dev, lo=vis_lo, hi=vis_hi)
    n_local = int(text.numel())
    own_lo, own_hi = own[0] - vis_lo, min(own[1], n_total + 1) - vis_lo
    own_bytes = min(own[1], n_total) - own[0]
    stream = c.stream
    torch.cuda.synchronize(dev)
    text_ptr = text.data_ptr()
    scan_ms = []

    def run_one(i, st=None):
        return scans[i].run(text_ptr, n_local, own_begin=own_lo, own_end=own_hi, stream=stream if st is None else st)

    # Headline: the nine patterns of a step go through ONE rj_multi_run in its one-pass mode (mode 0): the
    # bit-plane scan (plane_scan.hip) reads the text ONCE for all nine patterns and leaves one shared candidate
    # list; classify_shared_multi + offsets_gather_check_multi are the tails of all nine patterns; ONE host
    # synchronise.  It is the fastest way to get the nine counts; its roofline is n / t of the scan kernel
    # (never 9 n / t) against the HBM peak, with the VALU roofline beside it.
    use_multi = not args.serial_calls
    multi_sep = sep_scans = None
    if use_multi:
        multi_sep = rejit_amd.MultiScan(progs)
        multi_sep.set_mode(0)
        sep_scans = [multi_sep.scan(i) for i in range(len(progs))]

    def local_counts():
        if use_multi:
            return multi_sep.run(text_ptr, n_local, stream=stream, own_begin=own_lo, own_end=own_hi)
        return [run_one(i) for i in range(len(scans))]

    def to_global(b):
        return None if b is None else tuple(x + vis_lo for x in b)

    def run_local():
        cnt = local_counts()
        if use_multi:
            bounds = [to_global(b) for b in multi_sep.bounds(stream)]
        else:
            bounds = []
            for sc in scans:
                sp = sc.spans()
                bounds.append(to_global((sp[0][0], sp[0][1], sp[-1][0], sp[-1][1])) if sp else None)
        return cnt, bounds

    def rerun_one(i, cur, prev_end, have=True):
        # (rare) the left neighbour's last match reaches into this shard's first one; a previous match that ends before
        # this shard's buffer is no carry for it
        sc = sep_scans[i] if use_multi else scans[i]
        have = bool(have) and prev_end >= vis_lo
        k = sc.run(text_ptr, n_local, own_begin=own_lo, own_end=own_hi, carry_cur=max(cur - vis_lo, 0) if have else 0,
                   carry_prev_end=prev_end - vis_lo if have else 0, have_prev=have, stream=stream)
        sp = sc.spans()
        return k, (to_global((sp[0][0], sp[0][1], sp[-1][0], sp[-1][1])) if sp else None)

    exchange = sharding.CarryExchange(len(patterns), rank, world, dist, dev, c.cdev) if (world > 1 and use_multi) else None

    # Two steps in flight (rj_multi_start / rj_multi_finish on two rj_multi objects used alternately): while the host
    # collects step k's counts -- and, with several ranks, runs its carry exchange on a side stream -- the kernels of
    # step k + 1 are already queued, so the device never waits for the host's turn-around (~25 us of a 170 us step).
    # Every step still is one complete pass of the path over the batch with its own result; the synchronous call is
    # reported as `call_latency`.
    def two_in_flight(own_streams, tail_streams=False, time_all=True, counts_only=False, time_first=True):
        """(step, drain, scan times) of a loop that keeps two steps in flight on two rj_multi objects.  own_streams:
        each object on its own stream, the scan kernels ordered one behind the other (rj_multi_order_after), so that the
        tails of step k run under the scan of step k + 1.  tail_streams: both objects on ONE stream, but each queues its
        tails on a stream of its own (rj_multi_set_tail_stream): the scan kernels then follow each other in order on the
        one stream, with no cross-stream wait between them."""
        depth = 2 if own_streams else max(2, args.in_flight)
        multis = [rejit_amd.MultiScan(progs) for _ in range(depth)]
        # time_all False: only the first object's scan launches carry the start event scan_ms() needs (every second launch of
        # the loop): that event costs ~6.5 us between two kernels of a stream, the end event nothing
        timed = [time_first] + [time_all] * (depth - 1)
        for mm, tt in zip(multis, timed):
            mm.set_mode(0)
            mm.set_timing(tt)
            if counts_only:
                # MatchAllCount semantics (what regexdna asks, sample/regexdna.cc:65): scan + classification + counting in
                # ONE kernel (plane_count.hip), its rows added up by a small kernel on the object's own stream
                assert mm.set_counts_only(True), "the regexdna set must take the one-kernel counts path"
            elif tail_streams:
                mm.set_tail_stream(True)
        second = torch.cuda.Stream(dev) if own_streams else None
        streams = [stream, second.cuda_stream] if own_streams else [stream] * depth
        if own_streams:
            multis[0].order_after(multis[1])
            multis[1].order_after(multis[0])
        side = torch.cuda.Stream(dev) if exchange is not None else None
        fly = {"k": 0, "busy": [False] * depth, "keep": (second, side)}
        times = []

        def collect(j, record):
            local = multis[j].finish()
            fly["busy"][j] = False
            fly["last"] = multis[j]                       # (the object of the newest result: --dump-outputs reads its bounds)
            if record and timed[j]:
                times.append(multis[j].scan_ms())         # ONE launch scans the nine patterns (plane_scan)
            if exchange is None:
                return local
            # exchange step of the path: per pattern 8 integers per rank (count, first / last match, carry used) written by
            # a kernel, one all_gather over RCCL/xGMI, the decision taken by a kernel: no host tensors, one synchronise of
            # the side stream; the other object's step runs on the main stream meanwhile
            def rerun_j(i, cur, prev_end, have):
                multis[j].scan(i).run(text_ptr, n_local, own_begin=own_lo, own_end=own_hi, carry_cur=cur, carry_prev_end=prev_end,
                                      have_prev=have, stream=side.cuda_stream)
            with torch.cuda.stream(side):
                return exchange.counts(multis[j], lambda: None, rerun_j, vis_lo, side.cuda_stream)

        def step(record):
            j = fly["k"] % depth
            fly["k"] += 1
            res = collect(j, record) if fly["busy"][j] else None
            multis[j].start(text_ptr, n_local, stream=streams[j], own_begin=own_lo, own_end=own_hi)
            fly["busy"][j] = True
            return res

        def drain():
            res = None
            for j in [(fly["k"] + d) % depth for d in range(depth)]:   # the oldest first
                if fly["busy"][j]:
                    res = collect(j, True)
            return res

        step.fly = fly
        return step, drain, times

    # Two steps in flight (rj_multi_start / rj_multi_finish on two rj_multi objects used alternately): while the host
    # collects step k's counts -- and, with several ranks, runs its carry exchange on a side stream -- the kernels of
    # step k + 1 are already queued, so the device never waits for the host's turn-around (~15 us of a 170 us step).
    # Every step still is one complete pass of the path over the batch with its own result; the synchronous call is
    # reported as `call_latency` / `synchronous_calls`, the variant with a stream per object as `overlapped_tails`.
    # Round 4: the headline loop keeps both objects on ONE stream and queues every run's tails (classify + gather,
    # latency-bound) on a stream of the object's own (rj_multi_set_tail_stream): the scan kernels follow each other in
    # order, the tails of step k run under the scan of step k + 1.  The scan kernel then shares the device with them,
    # so its duration inside this loop is longer than alone: `roofline` is measured in this loop (as the contract asks),
    # `roofline_kernel_alone` in the one-stream loop of round 3 (`one_stream`).
    # Round 5: regexdna asks for COUNTS (MatchAllCount, sample/regexdna.cc:65), and for counts the step is ONE kernel:
    # plane_count (scan + exact classification of the candidates + counting; rj_multi_set_counts_only) followed by a
    # small kernel that adds the workgroups' rows up, on the object's own stream.  Nothing shares the device with the
    # scan but that small kernel.  `--span-lists` keeps round 4's loop (every pattern's (begin, end) list is laid out:
    # plane_scan + classify + gather) as the headline; it is always reported as `step_variants_ms.span_lists`.
    counts_headline = use_multi and not args.span_lists
    if use_multi:
        step, drain, scan_ms = two_in_flight(False, tail_streams=not args.one_stream, time_all=args.time_all_launches, counts_only=counts_headline)
    else:
        drain = None

        def step(record):
            counts = [run_one(i) for i in range(len(scans))]
            if world > 1:
                counts = sharding.multi_pattern_counts(run_local, rerun_one, len(patterns), rank, world, dist, c.cdev)
            if record:
                scan_ms.extend(sc.stats()["scan_ms"] for sc in scans)
            return counts

    # The timed region is 3 ms long (K = 20 steps of 0.13 ms).  A device that has just been idle (the set-up above is host
    # work) runs its first half second of load below its steady clocks: measured, K = 20 after W = 5 warm-up steps gives
    # 0.141 ms per step, after 50 ms of load the same, after 500 ms 0.127.  A production caller streams texts for hours; so
    # the step loop first runs untimed for --settle-ms (more warm-up steps of the very same loop; `settle_steps` in the
    # line), and what K steps cost on the cold device is reported beside the headline (`cold_ms_per_step`).
    cold_elapsed = None
    settle_steps = 0
    if args.settle_ms > 0:
        cold_elapsed, _ = timed(c, args, step, drain)
        # (a step may hold a collective: every rank must run the SAME number of settle steps -- from the cold run's time per
        # step, which timed() has already made the maximum over the ranks)
        settle_steps = int(min(max(args.settle_ms / max(cold_elapsed / args.steps * 1e3, 1e-3), 1), 100000))
        for _ in range(settle_steps):
            step(False)
        if drain:
            drain()
        del scan_ms[:]                 # (kernel durations of the timed region only)
    elapsed, counts = timed(c, args, step, drain)
    if args.tail_streams_probe:
        # child process of the `tails_on_own_streams` extra (see below): this one variant, one JSON line, nothing else
        p_step, p_drain, p_times = two_in_flight(False, tail_streams=True)
        ep, cp = timed(c, args, p_step, p_drain)
        print(json.dumps({"tail_streams_probe": {"ms_per_step": round(ep / args.steps * 1e3, 4),
                                                 "value": round(len(patterns) * n_total * args.steps / ep / 1e9, 3), "unit": "GB/s",
                                                 "scan_kernel_ms": round(sum(p_times) / max(len(p_times), 1), 5),
                                                 "counts_equal_headline": cp == counts,
                                                 "headline_ms_per_step_in_this_process": round(elapsed / args.steps * 1e3, 4)}}))
        return None, False
    # --dump-outputs: what a caller of the timed path receives from its last step -- the nine counts and, per pattern, the
    # (first begin, first end, last begin, last end) that rj_multi leaves (-1 without a match; this rank's shard)
    dump = {"matches_per_pass": counts}
    last_multi = getattr(step, "fly", {}).get("last")
    if last_multi is not None:
        dump["match_bounds"] = [[-1] * 4 if b is None else list(to_global(b)) for b in last_multi.bounds(stream)]
    # Absolute match latency at N ranks (BASELINE's north star: "GB/s scan throughput and absolute match latency reported
    # at 1/2/4/8 GPUs"): ten synchronous steps -- one rj_multi_run over the rank's shard, then the exchange -- timed on every
    # rank, the shard's run and the exchange apart; rank 0 reports every rank's medians.  (A step of the timed loop above
    # overlaps these with the next step's kernels; this is what ONE call costs.)
    per_rank = None
    if use_multi and world > 1 and args.full:
        lat_multi = rejit_amd.MultiScan(progs)
        lat_multi.set_mode(0)
        if counts_headline:
            lat_multi.set_counts_only(True)

        def rerun_lat(i, cur, prev_end, have):
            lat_multi.scan(i).run(text_ptr, n_local, own_begin=own_lo, own_end=own_hi, carry_cur=cur, carry_prev_end=prev_end,
                                  have_prev=have, stream=stream)
        t_run, t_xch, lat_counts = [], [], None
        for it in range(12):
            barrier(c)
            t0 = time.perf_counter()
            lat_multi.run(text_ptr, n_local, stream=stream, own_begin=own_lo, own_end=own_hi)
            t1 = time.perf_counter()
            lat_counts = exchange.counts(lat_multi, lambda: None, rerun_lat, vis_lo, stream)
            t2 = time.perf_counter()
            if it >= 2:
                t_run.append(t1 - t0)
                t_xch.append(t2 - t1)
        assert lat_counts == counts, (lat_counts, counts)
        mine = torch.tensor([sorted(t_run)[len(t_run) // 2] * 1e3, sorted(t_xch)[len(t_xch) // 2] * 1e3], dtype=torch.float64, device=c.cdev)
        allr = [torch.zeros(2, dtype=torch.float64, device=c.cdev) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [{"rank": r, "shard_run_ms": round(float(v[0]), 4), "exchange_ms": round(float(v[1]), 4)} for r, v in enumerate(allr)]
        del lat_multi
    total_matches = int(sum(counts))
    scanned = len(patterns) * n_total * args.steps          # bytes of text scanned by the whole job
    avg_scan_ms = sum(scan_ms) / max(len(scan_ms), 1)
    out = base_line(args, c, "GB/s text scanned (regexdna 9 patterns, 50M-line input); matches/s alongside",
                    scanned / elapsed / 1e9, elapsed,
                    {"workload": "regexdna: 9 x MatchAllCount over the stripped 50M-line FASTA (BASELINE configs[2])",
                     "fasta_n_per_gpu": args.fasta_n, "text_bytes_per_gpu": int(own_bytes), "patterns": len(patterns),
                     "sharding": "contiguous byte ranges + %d-byte halo; all_gather of 8 integers per pattern (count, first / last match, carry used) per step, rows and decision on the device"
                                 % (max_len - 1),
                     "calls": (("rj_multi_set_counts_only + rj_multi_start / rj_multi_finish, %d steps in flight on %d rj_multi objects on one stream: per step ONE pass over the text for the nine "
                                "patterns that also classifies and counts (plane_count) + a small kernel adding up its rows on the object's own stream; MatchAllCount semantics, no span lists"
                                % (max(2, args.in_flight), max(2, args.in_flight))) if counts_headline else
                               ("rj_multi_start / rj_multi_finish, mode 0, %d steps in flight on rj_multi objects on one stream%s: one pass over the text for the nine patterns (plane_scan) + classify + gather per step"
                                % (max(2, args.in_flight), "" if args.one_stream else ", each run's tails on a stream of the object's own (rj_multi_set_tail_stream)"))) if use_multi else "9 x rj_scan_run per step",
                     "before_the_timed_region": "the same loop untimed for --settle-ms = %g ms (device clocks: `cold_ms_per_step` is K steps straight after the set-up), then W warm-up steps" % args.settle_ms})
    if per_rank is not None:
        out["latency"] = {"what": "one synchronous call per rank: rj_multi_run over the rank's shard (median of 10), then the carry exchange "
                                  "(rows written by a kernel, one all_gather of 8 integers per pattern, decision kernel, one synchronise)",
                          "latency_ms": round(max(r["shard_run_ms"] + r["exchange_ms"] for r in per_rank), 4),
                          "per_rank": per_rank}
    out["matches_per_s"] = round(total_matches * args.steps / elapsed, 1)
    out["matches_per_pass"] = counts
    # the physical rate of a step: every text byte crosses the HBM interface ONCE per step whatever the number of patterns
    # (`value` counts it once per pattern, the reference's convention for nine MatchAllCount calls)
    out["physical_GBps"] = round(n_total * args.steps / elapsed / 1e9, 1)
    # (what a reader should meet FIRST: the rate at which text bytes cross the HBM interface; `value` = this x the nine patterns)
    out = {"metric": out["metric"], "physical_GBps": out["physical_GBps"],
           "value_is": "physical_GBps x %d patterns: every pattern's MatchAllCount scans the whole text (the reference runs nine passes, sample/regexdna.cc:65); "
                       "the text crosses the HBM interface ONCE per step, and the roofline is quoted on that" % len(patterns),
           **{k: v for k, v in out.items() if k not in ("metric", "physical_GBps")}}
    out["step_frac"] = round(n_total * args.steps / elapsed / 1e9 / HBM_PEAK_GBS / world, 4)
    if cold_elapsed is not None:
        out["settle_ms"] = args.settle_ms
        out["settle_steps"] = settle_steps
        out["cold_ms_per_step"] = round(cold_elapsed / args.steps * 1e3, 4)
    out["step_variants_ms"] = {"headline": round(elapsed / args.steps * 1e3, 4)}   # (filled in by the extras below; kept near the top of the line)
    if use_multi:
        # the dominant kernel: plane_scan reads every text byte ONCE for all nine patterns: algorithmic bytes per
        # launch = text bytes (for a fused pass quote n / t_fused, never 9 n / t_fused, against HBM)
        # (--full: the synchronous call checked against the loop and the same-run read-only ceiling, runs of their own)
        one_pass, ceiling = last_multi is not None and last_multi.how == 1, None
        if args.full:
            assert multi_sep.run(text_ptr, n_local, stream=stream, own_begin=own_lo, own_end=own_hi) == (counts if world == 1 else multi_sep.run(text_ptr, n_local, stream=stream, own_begin=own_lo, own_end=own_hi))
            one_pass = multi_sep.how == 1
            ceiling = hbm_ceiling(text_ptr, n_local, stream) if rank == 0 else None
        kernel_name = ("plane_count<ExactShape<2>> (one pass, nine patterns: scan + classification + counts)" if counts_headline else
                       "plane_scan<2> (one pass, nine patterns)" if one_pass else "scan kernels of rj_multi_run")
        out["roofline"] = hbm_roofline(kernel_name, own_bytes, avg_scan_ms,
                                       pmc_traffic("plane_count" if counts_headline else "plane", fasta_n=args.fasta_n) if world == 1 else None, len(scan_ms),
                                       ceiling=ceiling)
        out["roofline"]["note"] = ("n / t of the one launch that scans the text for all nine patterns; `value` counts the text once per pattern "
                                   "(9 x n per step, the reference's convention: nine MatchAllCount calls); `physical_GBps` is n / t of the step")
        if ceiling:
            out["hbm_ceiling"] = {"what": "a kernel that only reads the same %d bytes (16 B per lane and load, NON-TEMPORAL loads as the scans use since round 6, XOR-reduced; tools/probes/read_probe.hip), this device, this run" % n_local,
                                  "GB_per_s": round(ceiling, 1), "frac_of_spec_peak": round(ceiling / HBM_PEAK_GBS, 4)}
            try:
                # what rounds 1-5 quoted as the ceiling: the same kernel with default-policy loads
                dms = rejit_amd.stream_read_probe(text_ptr, n_local, 10, stream, default_policy=True)
                out["hbm_ceiling"]["default_policy_GB_per_s"] = round(n_local / (dms * 1e-3) / 1e9, 1)
            except Exception:
                pass
        if not args.time_all_launches:
            out["roofline"]["timing"] = ("HIP events of one scan launch in %d of the timed region (the first of the rj_multi objects used in turn): the start event "
                                         "costs ~6.5 us between two kernels of a stream; `step_variants_ms.every_launch_timed` is the loop with it on all"
                                         % max(2, args.in_flight))
        pv = pmc_valu("plane_count" if counts_headline else "plane")
        if pv is not None:
            ops_per_byte, ops_source = pv
            valu = own_bytes * ops_per_byte / (avg_scan_ms * 1e-3) / 1e12 if avg_scan_ms > 0 else 0.0
            out["roofline_valu"] = {"bound": "valu", "kernel": "plane_count<ExactShape<2>>" if counts_headline else "plane_scan<2>", "ops_per_text_byte": ops_per_byte,
                                    "achieved": round(valu, 2), "peak": VALU_PEAK_TOPS, "unit": "T lane-ops/s",
                                    "frac": round(valu / VALU_PEAK_TOPS, 4),
                                    "measured_issue_rate": VALU_MEASURED_TOPS, "frac_of_measured": round(valu / VALU_MEASURED_TOPS, 4),
                                    "note": "ops_per_text_byte from " + ops_source + " (a separate PMC pass over the same kernel; not typed in by hand)"}
    else:
        out["roofline"] = hbm_roofline("scan_windows<2,NIB>", own_bytes, avg_scan_ms, None, len(scan_ms))
    extras = rank == 0 and world == 1 and args.full and not args.no_extra

    call_times = {}

    def time_steps(fn, warm=2, steps=None, key=None):
        steps = steps or max(args.steps, 10)
        for _ in range(warm):
            r = fn()
        torch.cuda.synchronize(dev)
        per = []
        t1 = time.perf_counter()
        for _ in range(steps):
            t2 = time.perf_counter()
            r = fn()
            per.append(time.perf_counter() - t2)
        torch.cuda.synchronize(dev)
        if key:
            call_times[key] = {"calls_timed": steps, "median_ms": round(sorted(per)[len(per) // 2] * 1e3, 4), "min_ms": round(min(per) * 1e3, 4)}
        return (time.perf_counter() - t1) * args.steps / steps, r

    if extras and use_multi:
        ek0, ck0 = time_steps(lambda: multi_sep.run(text_ptr, n_local, stream=stream, own_begin=own_lo, own_end=own_hi), key="headline")
        out["call_latency"] = call_times["headline"]
        assert ck0 == counts, (ck0, counts)
        if world == 1 and counts_headline:
            # MatchAllCount in one kernel, one synchronous call after the other: the kernel with nothing else on the device
            multi_c = rejit_amd.MultiScan(progs)
            assert multi_c.set_counts_only(True)
            c_ms = []

            def counts_call():
                r = multi_c.run(text_ptr, n_local, stream=stream, own_begin=own_lo, own_end=own_hi)
                c_ms.append(multi_c.scan_ms())
                return r

            ec, cc = time_steps(counts_call, key="counts_only")
            assert cc == counts and multi_c.how == 3, (cc, counts, multi_c.how)
            c_ms = c_ms[2:]
            out["counts_call_latency"] = call_times["counts_only"]
            out["step_variants_ms"]["counts_synchronous_calls"] = round(ec / args.steps * 1e3, 4)
            out["roofline_kernel_alone"] = hbm_roofline("plane_count<ExactShape<2>> with nothing else on the device (synchronous calls)", own_bytes,
                                                        sum(c_ms) / len(c_ms), pmc_traffic("plane_count", fasta_n=args.fasta_n), len(c_ms),
                                                        ceiling=hbm_ceiling(text_ptr, n_local, stream))
            # the first / last match per pattern the counts kernel leaves for the carry exchange == the span pipeline's
            multi_sep.run(text_ptr, n_local, stream=stream, own_begin=own_lo, own_end=own_hi)
            assert multi_c.bounds() == multi_sep.bounds(), "counts-mode bounds differ from the span pipeline's"
            out["counts_bounds_equal_span_lists"] = True
            del multi_c
            # round 4's headline loop: the span pipeline, tails on a stream per object
            l_step, l_drain, l_times = two_in_flight(False, tail_streams=True, time_all=args.time_all_launches)
            el, cl = timed(c, args, l_step, l_drain)
            assert cl == counts, (cl, counts)
            out["span_lists"] = {"calls": "round 4's headline loop: every pattern's (begin, end) list laid out -- plane_count<ListShape<2>> (rounds 3-5: plane_scan<2>) + classify_shared_multi + offsets_gather_check_multi per step, "
                                          "steps in flight on one stream, tails on a stream per object",
                                 "ms_per_step": round(el / args.steps * 1e3, 4),
                                 "value": round(len(patterns) * n_total * args.steps / el / 1e9, 3), "unit": "GB/s",
                                 "roofline": hbm_roofline("plane_count<ListShape<2>> inside that loop", own_bytes, sum(l_times) / max(len(l_times), 1),
                                                          pmc_traffic("plane", fasta_n=args.fasta_n), len(l_times))}
            out["step_variants_ms"]["span_lists"] = out["span_lists"]["ms_per_step"]
            # Throughput with the scan kernels of consecutive steps OVERLAPPING: four rj_multi objects, a stream each, no order
            # between them -- a caller with several texts in flight.  The next kernels' workgroups fill the wave slots that a
            # kernel's last workgroups and the launch ramp leave idle (the 500 MB kernel loses ~13 us to them when it runs
            # alone).  Not the headline: a kernel's own duration is then no roofline input (several share the device).
            ov_depth = 4
            ov = [rejit_amd.MultiScan(progs) for _ in range(ov_depth)]
            ov_streams = [torch.cuda.Stream(dev) for _ in range(ov_depth)]
            for mm in ov:
                assert mm.set_counts_only(True)
                mm.set_timing(False)
            ov_state = {"k": 0, "busy": [False] * ov_depth}

            def ov_step(record):
                j = ov_state["k"] % ov_depth
                ov_state["k"] += 1
                res = ov[j].finish() if ov_state["busy"][j] else None
                ov[j].start(text_ptr, n_local, stream=ov_streams[j].cuda_stream, own_begin=own_lo, own_end=own_hi)
                ov_state["busy"][j] = True
                return res

            def ov_drain():
                res = None
                for j in [(ov_state["k"] + d) % ov_depth for d in range(ov_depth)]:
                    if ov_state["busy"][j]:
                        res = ov[j].finish()
                        ov_state["busy"][j] = False
                return res

            for _ in range(40):
                ov_step(False)
            ov_drain()
            eov, cov = timed(c, args, ov_step, ov_drain)
            assert cov == counts, (cov, counts)
            out["overlapped_scans"] = {"calls": "%d rj_multi objects (counts only), a stream each, no order between their kernels: the scan kernels of consecutive steps overlap" % ov_depth,
                                       "ms_per_step": round(eov / args.steps * 1e3, 4),
                                       "physical_GBps": round(n_total * args.steps / eov / 1e9, 1),
                                       "step_frac": round(n_total * args.steps / eov / 1e9 / HBM_PEAK_GBS, 4),
                                       "value": round(len(patterns) * n_total * args.steps / eov / 1e9, 3), "unit": "GB/s"}
            out["step_variants_ms"]["overlapped_scans"] = out["overlapped_scans"]["ms_per_step"]
            del ov, ov_streams
            if not args.time_all_launches:
                a_step, a_drain, a_times = two_in_flight(False, time_all=True, counts_only=True)
                ea, ca = timed(c, args, a_step, a_drain)
                assert ca == counts, (ca, counts)
                out["step_variants_ms"]["every_launch_timed"] = round(ea / args.steps * 1e3, 4)
                # ... and with it on NO launch: the step of a caller who does not time kernels (nothing to quote a roofline from)
                u_step, u_drain, _ = two_in_flight(False, time_all=False, counts_only=True, time_first=False)
                eu, cu = timed(c, args, u_step, u_drain)
                assert cu == counts, (cu, counts)
                out["step_variants_ms"]["no_launch_timed"] = round(eu / args.steps * 1e3, 4)
        if world == 1 and not counts_headline:
            # the same loop with a stream per object: the tails of step k (classify + gather, latency-bound) run under the
            # scan of step k + 1 -- more steps per second, but the scan kernel shares the device with them and takes
            # longer, which is why the headline (and its roofline) keeps both objects on one stream
            o_step, o_drain, o_times = two_in_flight(True)
            eo, co = timed(c, args, o_step, o_drain)
            assert co == counts, (co, counts)
            out["overlapped_tails"] = {"calls": "two steps in flight, a stream per rj_multi object, scans ordered (rj_multi_order_after)",
                                       "ms_per_step": round(eo / args.steps * 1e3, 4),
                                       "value": round(len(patterns) * n_total * args.steps / eo / 1e9, 3), "unit": "GB/s",
                                       "scan_kernel_ms": round(sum(o_times) / max(len(o_times), 1), 5)}
            # the loop of round 3's headline: both objects AND their tails on one stream -- the scan kernel alone on the device
            s_step, s_drain, s_times = two_in_flight(False, tail_streams=args.one_stream)
            es1, cs1 = timed(c, args, s_step, s_drain)
            assert cs1 == counts, (cs1, counts)
            key = "tails_on_own_streams" if args.one_stream else "one_stream"
            out[key] = {"calls": "two steps in flight on one stream, tails %s" % ("on a stream per object" if args.one_stream else "on the same stream (round 3's headline loop)"),
                        "ms_per_step": round(es1 / args.steps * 1e3, 4),
                        "value": round(len(patterns) * n_total * args.steps / es1 / 1e9, 3), "unit": "GB/s",
                        "scan_kernel_ms": round(sum(s_times) / max(len(s_times), 1), 5)}
            out["step_variants_ms"][key] = out[key]["ms_per_step"]
            out["step_variants_ms"]["overlapped_tails"] = out["overlapped_tails"]["ms_per_step"]
            if not args.one_stream and not args.time_all_launches:
                # the headline loop with the start event on EVERY scan launch (what `--time-all-launches` makes the headline)
                a_step, a_drain, a_times = two_in_flight(False, tail_streams=True, time_all=True)
                ea, ca = timed(c, args, a_step, a_drain)
                assert ca == counts, (ca, counts)
                out["step_variants_ms"]["every_launch_timed"] = round(ea / args.steps * 1e3, 4)
            if not args.one_stream and s_times:
                out["roofline_kernel_alone"] = hbm_roofline("plane_count<ListShape<2>> with nothing else on the device (the one-stream loop)", own_bytes,
                                                            sum(s_times) / len(s_times), pmc_traffic("plane", fasta_n=args.fasta_n), len(s_times))
        out["step_variants_ms"]["synchronous_calls"] = round(ek0 / args.steps * 1e3, 4)
        out["synchronous_calls"] = {"calls": "rj_multi_run mode 0, one call after the other (one step in flight): what rounds 1-2 timed",
                                    "ms_per_step": round(ek0 / args.steps * 1e3, 4),
                                    "value": round(len(patterns) * n_total * args.steps / ek0 / 1e9, 3), "unit": "GB/s"}
        # The nine per-pattern scans as ONE launch (rj_multi mode 1, round 2's headline): a wave runs its own 32 KB
        # span through pattern after pattern, so passes 2..9 are served by the 256 MiB Infinity Cache -- 9 n / t of
        # that launch is a rate of algorithmic bytes, not an HBM rate, and is reported as such.
        multi_t = rejit_amd.MultiScan(progs)
        multi_t.set_mode(1)
        tms = []

        def train_step():
            r = multi_t.run(text_ptr, n_local, stream=stream)
            tms.append(multi_t.scan_ms())
            return r

        et, ct = time_steps(train_step, key="train")
        assert ct == counts, "the train of scans disagrees with the one-pass run"
        tms = tms[2:]
        out["train"] = {"calls": "rj_multi_run mode 1: the nine per-pattern scans as one launch (scan_windows_train) + batched tails",
                        "value": round(scanned / et / 1e9, 3), "unit": "GB/s", "ms_per_step": round(et / args.steps * 1e3, 4),
                        "call": call_times["train"],
                        "algorithmic_rate": {"kernel": "scan_windows_train<NIB>", "bytes_per_launch": int(len(patterns) * own_bytes),
                                             "avg_launch_ms": round(sum(tms) / len(tms), 5),
                                             "GB_per_s": round(len(patterns) * own_bytes / (sum(tms) / len(tms) * 1e-3) / 1e9, 1),
                                             "note": "NOT an HBM roofline: passes 2..9 of a wave's span hit the Infinity Cache (one HBM pass + eight cached ones)"}}
        del multi_t
        # One launch PER PATTERN (rj_multi mode 3, the headline of round 1): every kernel streams the whole text
        # from HBM with nothing of it left in a cache from the pattern before, so this is the per-kernel HBM
        # roofline of the streaming scan; the train above is faster because a wave's passes 2..9 over its own
        # 32 KB span hit the Infinity Cache.
        multi_k = rejit_amd.MultiScan(progs)
        multi_k.set_mode(3)
        kms = []

        def per_kernel_step():
            r = multi_k.run(text_ptr, n_local, stream=stream)
            kms.extend(multi_k.scan(i).stats()["scan_ms"] for i in range(len(progs)))
            return r

        ek, ck = time_steps(per_kernel_step)
        assert ck == counts, "per-kernel launches disagree with the train"
        kms = kms[2 * len(progs):]
        out["separate_launches"] = {"calls": "rj_multi_run mode 3: one scan kernel per pattern, back to back, batched tails",
                                    "value": round(scanned / ek / 1e9, 3), "unit": "GB/s", "ms_per_step": round(ek / args.steps * 1e3, 4),
                                    "roofline": hbm_roofline("scan_windows<2,NIB>", own_bytes, sum(kms) / len(kms),
                                                             pmc_traffic("regexdna_single", fasta_n=args.fasta_n), len(kms))}
        del multi_k
        es, cs = time_steps(lambda: [run_one(i) for i in range(len(scans))])
        assert cs == counts, "synchronous calls disagree with rj_multi_run"
        out["serial_calls"] = {"calls": "9 x rj_scan_run per step", "value": round(scanned / es / 1e9, 3), "unit": "GB/s",
                               "ms_per_step": round(es / args.steps * 1e3, 4)}
        # the scan kernels alternating between two streams (rj_multi mode 2): consecutive kernels overlap at
        # their boundaries.  Faster, but a per-kernel duration is no roofline input any more.
        multi_il = rejit_amd.MultiScan(progs)
        multi_il.set_mode(2)
        ei, ci = time_steps(lambda: multi_il.run(text_ptr, n_local, stream=stream))
        assert ci == counts, "interleaved run disagrees"
        out["interleaved"] = {"calls": "rj_multi_run mode 2 (scan kernels on two alternating streams)",
                              "value": round(scanned / ei / 1e9, 3), "unit": "GB/s", "ms_per_step": round(ei / args.steps * 1e3, 4)}
        del multi_il

    if extras:
        # the 9 calls from 3 host threads, one stream each (sample/regexdna-multithread.cc:65-78)
        from concurrent.futures import ThreadPoolExecutor
        streams = [torch.cuda.Stream(device=dev) for _ in scans]

        def threaded(i):
            torch.cuda.set_device(dev)
            return run_one(i, streams[i].cuda_stream)

        with ThreadPoolExecutor(max_workers=3) as pool3:
            e3, c3 = time_steps(lambda: list(pool3.map(threaded, range(len(scans)))))
        assert c3 == counts, "threaded run disagrees with the serial run"
        out["overlapped"] = {"pattern_threads": 3, "value": round(scanned / e3 / 1e9, 3), "unit": "GB/s",
                             "ms_per_step": round(e3 / args.steps * 1e3, 4)}

    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        # bounded sample taken from the lower-case (matching) part of the text: the first 20 %
        # is the upper-case ALU repeat, which no pattern can match
        # the all-core leg scans the WHOLE text (9 x 500 MB = 4.5 GB, disjoint slices); the one-core leg a 64 MiB
        # sample taken from the lower-case part (the first 20 % is the upper-case ALU repeat, which no pattern matches)
        sample = min(n_local, args.cpu_sample_mib << 20)
        s0 = min(max(0, n_local - sample), (int(n_local * 0.6) // 4096) * 4096)
        host_all = text.cpu().numpy().tobytes()
        host = host_all[s0:] + host_all[:s0]          # (rotated: the one-core sample is the head of the buffer)
        del host_all
        base, ref_counts, n1 = cpu_baseline(host, patterns, f"bytes [{s0}, {s0 + sample}) of the same text, 9 patterns", one_core_bytes=sample)
        del host
        out["cpu_baseline"] = base
        if ref_counts is not None:
            # in-run parity check against the real reference on the sample
            gpu_counts = []
            for sc in scans:
                sc.run(text.data_ptr() + s0, n1, own_begin=0, own_end=n1 + 1, stream=stream)
                gpu_counts.append(sc.stats()["n_matches"])
            assert gpu_counts == ref_counts, ("GPU and reference disagree on the sample", gpu_counts, ref_counts)
            out["cpu_baseline"]["parity_on_sample"] = "GPU counts == reference counts: %s" % ref_counts

    del text
    torch.cuda.empty_cache()
    if rank == 0 and world == 1 and args.full:
        fx = fullsize_fixture()
        if fx and "c3" in fx and fx["c3"]["fasta_n"] == args.fasta_n:
            want = [p["digest"]["count"] for p in fx["c3"]["patterns"]]
            assert counts == want, ("the nine counts differ from the reference's at full size", counts, want)
            out["parity_full_size"] = "nine counts == the real reference's over the same 500 MB text (tests/golden/fullsize_vectors.json)"
    if extras and not args.no_big:
        # Is the streaming scan's rate an HBM rate?  One kernel per pattern (mode 3) over a 2.5 GB text: every launch
        # streams 10x the 256 MiB Infinity Cache, so nothing of the text survives from one pattern to the next.
        nf = 250_000_000
        big = W.fasta_stripped_torch(nf, dev)
        nb = int(big.numel())
        m2 = rejit_amd.MultiScan(progs)
        m2.set_mode(3)
        ms2 = []

        def big_step():
            r = m2.run(big.data_ptr(), nb, stream=stream)
            ms2.extend(m2.scan(i).stats()["scan_ms"] for i in range(len(progs)))
            return r

        settle_device(big_step, args.settle_ms)
        del ms2[:]
        eb, cb = time_steps(big_step, warm=1, steps=5)
        ms2 = ms2[len(progs):]
        out["hbm_not_cache"] = {"workload": "the same nine patterns, one kernel per pattern (mode 3), over a 2.5 GB stripped FASTA (fasta_n 250M)",
                                "value": round(9 * nb / (eb / args.steps) / 1e9, 3), "unit": "GB/s", "ms_per_step": round(eb / args.steps * 1e3, 4),
                                "matches_per_pass": cb,
                                "roofline": hbm_roofline("scan_windows<2,NIB>", nb, sum(ms2) / len(ms2), pmc_traffic("regexdna_single_2p5gb", bytes=nb), len(ms2),
                                                         ceiling=hbm_ceiling(big.data_ptr(), nb, stream))}
        m0 = rejit_amd.MultiScan(progs)
        ms0 = []

        def big_plane_step():
            r = m0.run(big.data_ptr(), nb, stream=stream)
            ms0.append(m0.scan_ms())
            return r

        e0, c0 = time_steps(big_plane_step, warm=1, steps=5)
        assert c0 == cb, "one-pass and per-pattern runs disagree on the 2.5 GB text"
        ms0 = ms0[1:]
        out["one_pass_2p5gb"] = {"workload": "the span-list pipeline's one-pass run (round 4's headline) over the same 2.5 GB text",
                                 "value": round(9 * nb / (e0 / args.steps) / 1e9, 3), "unit": "GB/s",
                                 "ms_per_step": round(e0 / args.steps * 1e3, 4),
                                 "roofline": hbm_roofline("plane_count<ListShape<2>>", nb, sum(ms0) / len(ms0), pmc_traffic("plane_2p5gb", bytes=nb), len(ms0),
                                                          ceiling=hbm_ceiling(big.data_ptr(), nb, stream))}
        mc = rejit_amd.MultiScan(progs)
        assert mc.set_counts_only(True)
        msc = []

        def big_count_step():
            r = mc.run(big.data_ptr(), nb, stream=stream)
            msc.append(mc.scan_ms())
            return r

        ecb, ccb = time_steps(big_count_step, warm=1, steps=5)
        assert ccb == cb and mc.how == 3, "the counts kernel and the per-pattern runs disagree on the 2.5 GB text"
        msc = msc[1:]
        out["counts_2p5gb"] = {"workload": "the headline's one-kernel MatchAllCount over the same 2.5 GB text",
                               "value": round(9 * nb / (ecb / args.steps) / 1e9, 3), "unit": "GB/s",
                               "ms_per_step": round(ecb / args.steps * 1e3, 4),
                               "roofline": hbm_roofline("plane_count<ExactShape<2>>", nb, sum(msc) / len(msc), pmc_traffic("plane_count_2p5gb", bytes=nb), len(msc),
                                                        ceiling=hbm_ceiling(big.data_ptr(), nb, stream))}
        del big, m2, m0, mc
        torch.cuda.empty_cache()
    out["_dump"] = dump
    return out, extras


# ------------------------------------------------------------------------------------------ literal / complex
def plant_literal(W, t, n, seed):
    offs = W.plant_offsets(n, 6, 1000, seed=seed, boundaries=[16, 1024, 1 << 20, 1 << 30, n // 2])
    W.plant(t, offs, b"regexp")
    return offs


def settle_device(fn, ms):
    """Run fn() for `ms` milliseconds, untimed: an extra's ten timed calls last a few ms, and a device that idled while the
    host prepared the text or timed the reference runs its first half second of load below its steady clocks."""
    t = time.perf_counter()
    while ms > 0 and (time.perf_counter() - t) * 1e3 < ms:
        fn()


def single_pattern_extra(c, rejit_amd, t, n, rx, label, kernel, steps, check, traffic_key=None, cpu=True, args=None):
    torch, dev, stream = c.torch, c.dev, c.stream
    sc = rejit_amd.Scan(rejit_amd.Program(rx))
    t_cold = time.perf_counter()
    sc.run(t.data_ptr(), n, stream=stream)      # the first call of a fresh scan: buffers, region sizing, path discovery
    cold = time.perf_counter() - t_cold
    sc.run(t.data_ptr(), n, stream=stream)
    settle_device(lambda: sc.run(t.data_ptr(), n, stream=stream), getattr(args, "settle_ms", 0.0))
    steps = max(steps, 10)
    ms, wall = [], []
    torch.cuda.synchronize(dev)
    for _ in range(steps):
        t0 = time.perf_counter()
        cnt = sc.run(t.data_ptr(), n, stream=stream)   # (synchronous: returns with the count)
        wall.append(time.perf_counter() - t0)
        ms.append(sc.stats()["scan_ms"])
    torch.cuda.synchronize(dev)
    check(sc)
    a_ms = sum(ms) / len(ms)
    # (extras report the MEDIAN call: a one-off hiccup of the box in five calls -- seen once as a 10 ms call
    # among 1 ms ones -- would otherwise be the number; the slowest call is listed beside it)
    dt = sorted(wall)[len(wall) // 2]
    rec = {"workload": label, "value": round(n / dt / 1e9, 1), "unit": "GB/s", "matches": int(cnt),
           "latency_ms": round(dt * 1e3, 4), "latency_ms_min": round(min(wall) * 1e3, 4), "latency_ms_max": round(max(wall) * 1e3, 4),
           "cold_call_ms": round(cold * 1e3, 3), "calls_timed": steps,
           "roofline": hbm_roofline(kernel, n, a_ms, pmc_traffic(traffic_key, bytes=n) if traffic_key else None,
                                    ceiling=hbm_ceiling(t.data_ptr(), n, stream))}
    if cpu and args is not None and not args.no_cpu_baseline:
        big = min(n, 4 << 30)                       # all cores: 4 GiB of the text in disjoint slices
        host = t[:big].cpu().numpy().tobytes()
        sample = min(n, args.cpu_sample_mib << 20)
        base, ref_counts, sample = cpu_baseline(host, [rx], f"first {big} bytes of the same text", one_core_bytes=sample)
        del host
        if ref_counts is not None:
            sc.run(t.data_ptr(), sample, stream=stream)
            base["parity_on_sample"] = "GPU count %d, reference count %d" % (sc.stats()["n_matches"], ref_counts[0])
            # (the reference's default-flag path mis-places matches of the complex regex, SURVEY 4.4 Q2: counts
            # are reported, not asserted, for that pattern)
        rec["cpu_baseline"] = base
    return rec


def literal_and_complex_extras(args, c, out):
    import random as _random
    import rejit_amd
    from rejit_amd import workloads as W
    torch, dev = c.torch, c.dev
    n = args.literal_bytes
    t = W.random_ascii_torch(n, 0xC0FFEE, dev)
    offs = plant_literal(W, t, n, 0xC0FFEE)

    def check_literal(sc):
        found = {b for b, _ in sc.spans()}
        assert set(offs) <= found, "a planted occurrence was missed"
        fx = fullsize_fixture()
        if fx and "c2" in fx and fx["c2"]["bytes"] == n:
            assert W.span_digest_torch(sc.spans_tensor(dev)) == fx["c2"]["digest"], "literal scan differs from the reference's answer at 5 GB"
            out["parity_full_size_literal"] = "count and span digest == the real reference's over the same 5 GB text"

    out["literal_scan"] = single_pattern_extra(
        c, rejit_amd, t, n, "regexp",
        "literal 'regexp' MatchAll over %d bytes random ASCII ['0','z'), %d planted (BASELINE configs[1])" % (n, len(offs)),
        "scan_windows<1>", max(5, min(args.steps, 20)), check_literal, "literal", True, args)

    # The same literal scan with two calls in flight (rj_scan_start / rj_scan_finish on two rj_scan objects: the scan
    # kernel on the caller's stream, the latency-bound tail on the scan's own): the whole-call rate when the caller has
    # the next text ready -- what a reader thread feeding a scanner does.  Guarded: an extra must never cost the line.
    try:
        prog_p = rejit_amd.Program("regexp")
        pair = [rejit_amd.Scan(prog_p), rejit_amd.Scan(prog_p)]
        want_p = [sc.run(t.data_ptr(), n, stream=c.stream) for sc in pair][0]
        calls_p = 20
        torch.cuda.synchronize(dev)
        t0p = time.perf_counter()
        pair[0].start(t.data_ptr(), n, stream=c.stream)
        got_p = []
        for k in range(1, calls_p):
            pair[k & 1].start(t.data_ptr(), n, stream=c.stream)
            got_p.append(pair[(k - 1) & 1].finish())
        got_p.append(pair[(calls_p - 1) & 1].finish())
        torch.cuda.synchronize(dev)
        dtp = (time.perf_counter() - t0p) / calls_p
        out["literal_scan"]["two_in_flight"] = {"calls": "rj_scan_start / rj_scan_finish, two rj_scan objects, %d calls" % calls_p,
                                                "ms_per_call": round(dtp * 1e3, 4), "value": round(n / dtp / 1e9, 1), "unit": "GB/s",
                                                "frac_of_hbm_peak": round(n / dtp / 1e9 / HBM_PEAK_GBS, 4),
                                                "counts_equal": all(g == want_p for g in got_p)}
        del pair, prog_p
    except Exception as e:  # noqa: BLE001
        out["literal_scan"]["two_in_flight"] = {"error": repr(e)[:300]}

    # BASELINE configs[3] shape on one GPU: the complex benchmark regex (floating fast-forward window
    # `abcdefgh`) over the same text with strings of its language planted
    rx = W.BENCH_REGEXES[3][0]
    rng = _random.Random(7)
    offs2 = W.plant_offsets(n, 80, 1000, seed=7)
    samples = [W.complex_regex_sample(rng) for _ in offs2]
    for o, smp in zip(offs2, samples):
        W.plant(t, [o + 8], smp)

    def check_complex(sc):
        ends = {e for _, e in sc.spans()}
        assert all(o + 8 + len(smp) in ends for o, smp in zip(offs2, samples)), "a planted complex match was missed"

    out["complex_scan"] = single_pattern_extra(
        c, rejit_amd, t, n, rx, "%s MatchAll over %d bytes random ASCII, %d planted (BASELINE configs[3] shape, 1 GPU)" % (rx, n, len(offs2)),
        "scan_windows<1> (floating window)", 5, check_complex, "complex", True, args)
    # a required literal BEHIND an unbounded prefix (the reference's backward pass from the fast-forward hit,
    # src/x64/codegen-x64.cc:643-650): the window scan finds `abcdefgh`, verify_behind_lds (verify_lds.hip) walks the
    # reverse automaton to the start.  Round 1 ran these patterns in dense mode (0.6 TB/s).
    rxb = "[a-z]+abcdefgh"

    def check_behind(sc):
        sp = sc.spans()
        assert len(sp) >= 300 and all(e - b >= 9 for b, e in sp), "behind-mode matches missing"

    out["behind_scan"] = single_pattern_extra(
        c, rejit_amd, t, n, rxb, "%s MatchAll over the same %d bytes (window behind an unbounded prefix)" % (rxb, n),
        "scan_windows<1> + verify_behind_lds", 5, check_behind, "behind", True, args)
    # A one-pass run of a pattern set that is NOT the regexdna shape (round 4: plane_scan_general): two literal alternations of
    # the reference's benchmark regexes (tools/benchmarks/run.py:352,356), windows of 7 / 8 bytes at offsets 0 / 1, four
    # base windows compared exactly as 2-bit codes over an alphabet of 74 symbols (codes alias: a filter).
    try:
        gset = ["alternation|strings", "prefix abcd|prefix 1234"]
        for k, o in enumerate(W.plant_offsets(n, 32, 400, seed=11)):
            W.plant(t, [o], [b"alternation", b"strings", b"prefix abcd", b"prefix 1234"][k % 4])
        gprogs = [rejit_amd.Program(rx) for rx in gset]
        gmulti = rejit_amd.MultiScan(gprogs)
        gcounts = gmulti.run(t.data_ptr(), n, stream=c.stream)
        ghow = gmulti.how
        gsingle = [rejit_amd.Scan(p).run(t.data_ptr(), n, stream=c.stream) for p in gprogs]
        settle_device(lambda: gmulti.run(t.data_ptr(), n, stream=c.stream), args.settle_ms)
        gms, gwall = [], []
        for _ in range(10):
            t0g = time.perf_counter()
            gmulti.run(t.data_ptr(), n, stream=c.stream)
            gwall.append(time.perf_counter() - t0g)
            gms.append(gmulti.scan_ms())
        gmed = sorted(gwall)[len(gwall) // 2]
        out["general_one_pass"] = {"workload": "%s over the same %d bytes in ONE pass (plane_count<GeneralListShape>: 4 exact base windows of 7 bytes, offsets 0 and 1; round 4-5: plane_scan_general)" % (" + ".join(gset), n),
                                   "how": ghow, "counts": gcounts, "counts_equal_single_runs": gcounts == gsingle,
                                   "latency_ms": round(gmed * 1e3, 4), "value": round(n / gmed / 1e9, 1), "unit": "GB/s of text (once for both patterns)",
                                   "roofline": hbm_roofline("plane_count<GeneralListShape<false>> (the span pipeline's scan kernel)", n, sum(gms) / len(gms), pmc_traffic("general", bytes=n), len(gms), ceiling=hbm_ceiling(t.data_ptr(), n, c.stream))}
        # the same set as MatchAllCount in ONE kernel (round 6: plane_count<GeneralShape>, rj_multi_set_counts_only): the filter
        # through code planes, every candidate classified by the patterns' automata out of LDS, nothing written but the counts;
        # and nine random 12-mers (nine bases: the filter's cost grows with the bases)
        import random as _r
        r12 = _r.Random(3)
        w12 = ["".join(r12.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(12)) for _ in range(9)]
        for key, cset, plants in (("counts_general", gset, None), ("counts_nine_12mers", w12, [w.encode() for w in w12])):
            if plants:
                for k, o in enumerate(W.plant_offsets(n, 32, 450, seed=13)):
                    W.plant(t, [o], plants[k % len(plants)])
            cprogs = [rejit_amd.Program(rx) for rx in cset]
            cm = rejit_amd.MultiScan(cprogs)
            took = cm.set_counts_only(True)
            ccounts = cm.run(t.data_ptr(), n, stream=c.stream)
            chow = cm.how
            lm = rejit_amd.MultiScan(cprogs)
            lcounts = lm.run(t.data_ptr(), n, stream=c.stream)
            same_bounds = cm.bounds() == lm.bounds()
            del lm
            settle_device(lambda: cm.run(t.data_ptr(), n, stream=c.stream), args.settle_ms)
            cms, cwall = [], []
            for _ in range(10):
                t0g = time.perf_counter()
                cm.run(t.data_ptr(), n, stream=c.stream)
                cwall.append(time.perf_counter() - t0g)
                cms.append(cm.scan_ms())
            cmed = sorted(cwall)[len(cwall) // 2]
            out[key] = {"workload": "MatchAllCount of %s over the same %d bytes in ONE kernel (%d base windows)" % (" + ".join(cset) if len(cset) < 4 else "nine random 12-mers", n, 4 if not plants else 9),
                        "took_counts_path": bool(took), "how": chow, "counts": ccounts, "counts_equal_span_pipeline": ccounts == lcounts,
                        "bounds_equal_span_pipeline": same_bounds,
                        "latency_ms": round(cmed * 1e3, 4), "value": round(n / cmed / 1e9, 1), "unit": "GB/s of text (once for all patterns)",
                        "roofline": hbm_roofline("plane_count<GeneralShape>", n, sum(cms) / len(cms), pmc_traffic("counts_general", bytes=n) if not plants else None, len(cms), ceiling=hbm_ceiling(t.data_ptr(), n, c.stream))}
            assert ccounts == lcounts and same_bounds, (key, ccounts, lcounts)
            del cm, cprogs
        del gmulti, gprogs
    except Exception as e:  # noqa: BLE001 (an extra must never cost the line)
        out["general_one_pass"] = {"error": repr(e)[:300]}
    # Patterns WITHOUT a fast-forward window (the NFA half of the north star): scan_dense_walk finds, walks and
    # compacts the candidates in one kernel.  `[a-f]+[0-9]`: a start at 8 % of the bytes of this text (only the
    # first byte of every run of [a-f] is taken, DevProgram::loop_first); the first four automaton steps of all
    # starts run lane-packed, four starts per register (dense_swar.h).
    def check_dense(sc):
        st_d = sc.stats()
        assert st_d["n_matches"] > 1000
        out["dense_path"] = {"stream_path": st_d["stream_path"], "slow_starts": st_d["slow_starts"]}

    out["dense_scan"] = single_pattern_extra(
        c, rejit_amd, t, n, "[a-f]+[0-9]", "[a-f]+[0-9] MatchAll over the same %d bytes (no fast-forward window: dense mode)" % n,
        "dense_streams<2,2> (bit streams, position-major steps, pairs written once)", 5, check_dense, "dense", True, args)
    # (the dense kernel is issue-bound, not HBM-bound: its VALU roofline says how close to the other ceiling it runs)
    _dl = out["dense_scan"]["roofline"]["avg_launch_ms"]
    if _dl:
        # (`frac` counts the text bytes only; the kernel also writes 16 B per match, once: both together)
        _k = int(out["dense_scan"].get("matches", 0))
        out["dense_scan"]["roofline"]["with_pairs_written"] = {"bytes_per_launch": n + 16 * _k, "achieved": round((n + 16 * _k) / (_dl * 1e-3) / 1e9, 1),
                                                               "frac": round((n + 16 * _k) / (_dl * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        _pv = pmc_valu("dense")
        if _pv is not None:
            _valu = n * _pv[0] / (_dl * 1e-3) / 1e12
            out["dense_scan"]["roofline_valu"] = {"bound": "valu", "kernel": "dense_streams<2,2>",
                                                  "ops_per_text_byte": _pv[0], "achieved": round(_valu, 2),
                                                  "peak": VALU_PEAK_TOPS, "unit": "T lane-ops/s", "frac": round(_valu / VALU_PEAK_TOPS, 4),
                                                  "measured_issue_rate": VALU_MEASURED_TOPS, "frac_of_measured": round(_valu / VALU_MEASURED_TOPS, 4),
                                                  "note": "ops_per_text_byte from " + _pv[1] + "; the issue rate measured for this kernel's instruction mix: profiles/r05_valu_rate.txt -- the kernel is VALU-bound"}
    # Candidates that CAN overlap (`[0-9][0-9][0-9]`: VERDICT r04 item 4): the same kernel with the reference's left-most-longest
    # selection made inside it (StreamPlan::select, round 5); until then this pattern took scan_dense_walk.  Parity at this size:
    # the digest of all (begin, end) pairs against scan_dense_walk's over the same text (tests: both against the oracle).
    try:
        def spans_digest(sc):
            x = sc.spans_tensor(dev)
            return [int(x.shape[0]), int((x[:, 0] * 1000003 + x[:, 1]).sum().item()) & ((1 << 62) - 1)] if x.numel() else [0, 0]

        sel_digest = []

        def check_select(sc):
            st_d = sc.stats()
            assert st_d["n_matches"] > 1000
            sel_digest.append(spans_digest(sc))
            sel_digest.append(st_d["stream_path"])

        out["dense_select"] = single_pattern_extra(
            c, rejit_amd, t, n, "[0-9][0-9][0-9]", "[0-9][0-9][0-9] MatchAll over the same %d bytes (dense mode, candidates overlap: selection in the kernel)" % n,
            "dense_streams<3,1,select> (bit streams, left-most-longest selection by lane speculation, pairs written once)", 5, check_select, "dense_select", False, args)
        out["dense_select"]["stream_path"] = sel_digest[1]
        os.environ["RJ_NO_STREAMS"] = "1"          # (read when a pattern is lowered)
        try:
            sc_w = rejit_amd.Scan(rejit_amd.Program("[0-9][0-9][0-9]"))
        finally:
            del os.environ["RJ_NO_STREAMS"]
        sc_w.run(t.data_ptr(), n, stream=c.stream)
        sc_w.run(t.data_ptr(), n, stream=c.stream)
        t0w = time.perf_counter()
        sc_w.run(t.data_ptr(), n, stream=c.stream)
        walk_ms = (time.perf_counter() - t0w) * 1e3
        out["dense_select"]["scan_dense_walk"] = {"latency_ms": round(walk_ms, 3), "kernel_ms": round(sc_w.stats()["scan_ms"], 3),
                                                  "same_pairs": spans_digest(sc_w) == sel_digest[0], "pairs_digest": sel_digest[0]}
        del sc_w
    except Exception as e:  # noqa: BLE001 (an extra must never cost the line)
        out["dense_select"] = {"error": repr(e)[:300]}
    # The line table of a grep-like caller (sample/jrep.cc:294: MatchAll of "^"): a class scan whose OUTPUT is
    # the traffic -- 16 bytes per line start next to 1 byte read per text byte.
    nl = torch.arange(60, n, 61, device=dev)
    t[nl] = 10
    del nl
    sc_l = rejit_amd.Scan(rejit_amd.Program("^"))
    t_cold = time.perf_counter()
    sc_l.run(t.data_ptr(), n, stream=c.stream)
    cold_l = time.perf_counter() - t_cold
    sc_l.run(t.data_ptr(), n, stream=c.stream)
    settle_device(lambda: sc_l.run(t.data_ptr(), n, stream=c.stream), args.settle_ms)
    lms, ltot = [], []
    for _ in range(10):
        k = sc_l.run(t.data_ptr(), n, stream=c.stream)
        st = sc_l.stats()
        lms.append(st["scan_ms"])
        ltot.append(st["total_ms"])
    assert k == n // 61 + 1 + (1 if n % 61 > 60 else 0) or k >= n // 61, "line table count"
    a_l = sum(lms) / len(lms)
    bytes_l = n + 16 * k
    out["line_table"] = {"workload": "`^` MatchAll over %d bytes with a line break every 61 bytes (jrep's line table)" % n, "matches": int(k),
                         "value": round(n / (sorted(ltot)[len(ltot) // 2] * 1e-3) / 1e9, 1), "unit": "GB/s of text",
                         "latency_ms": round(sorted(ltot)[len(ltot) // 2], 4), "latency_ms_min": round(min(ltot), 4), "cold_call_ms": round(cold_l * 1e3, 3),
                         "calls_timed": len(ltot), "write_bytes_per_launch": 16 * int(k),
                         "roofline": hbm_roofline("emit_assertions (one pass, prefix scan resolved a round late: n text bytes read + 16 B written per match)", bytes_l, a_l,
                                                  pmc_traffic("line_table", bytes=n), ceiling=hbm_ceiling(t.data_ptr(), n, c.stream))}
    out["line_table"]["roofline"]["ceiling_note"] = "the ceiling is a READ-only kernel over the text; this kernel also writes 16 B per match"
    del t
    torch.cuda.empty_cache()

    # The reference's ring artefact on a stretch WITHOUT a synchronisation point: `.{0,2}.` over 63 MiB
    # without a line break -- every byte keeps a thread alive, so the whole text is ONE segment of the exact replay.  Until
    # round 4 one lane replayed a segment (6 us per byte: minutes) and nothing beyond 16 MiB; now it is taken in parts.
    try:
        nx = 63 << 20
        tx = W.random_ascii_torch(nx, 7, dev, ord("a"), ord("e"))
        sx = rejit_amd.Scan(rejit_amd.Program(".{0,2}."))
        sx.run(tx.data_ptr(), nx, stream=c.stream)
        xs = []
        for _ in range(3):
            t0x = time.perf_counter()
            kx = sx.run(tx.data_ptr(), nx, stream=c.stream)
            xs.append(time.perf_counter() - t0x)
        spans_x = sx.spans_tensor(dev)
        # (without line breaks the reference's matches of this pattern tile the text: each begins where the one before ended)
        tiles = bool((spans_x[1:, 0] == spans_x[:-1, 1]).all().item()) and int(spans_x[0, 0]) == 0 and int(spans_x[-1, 1]) == nx
        out["exact_replay_long"] = {"workload": "`.{0,2}.` (at risk of the reference's ring artefact) MatchAll over %d bytes without a line break: one segment of the exact replay, in parts" % nx,
                                    "seconds": round(sorted(xs)[1], 4), "matches": int(kx), "exact_path": sx.stats()["exact_path"],
                                    "matches_tile_the_text": tiles}
        # ... and a thread that lives for megabytes: `[xy]+z[xy]` inside 63 MiB of x (one match from 0 to the z in the middle)
        ty = torch.full((nx + 16,), ord("x"), dtype=torch.uint8, device=dev)
        ty[nx // 2] = ord("z")
        ty[nx - 6:nx] = torch.tensor(list(b"zx xzy"), dtype=torch.uint8, device=dev)
        sy = rejit_amd.Scan(rejit_amd.Program("[xy]+z[xy]"))
        sy.run(ty.data_ptr(), nx, stream=c.stream)
        t0y = time.perf_counter()
        ky = sy.run(ty.data_ptr(), nx, stream=c.stream)
        dty = time.perf_counter() - t0y
        first_y = sy.spans()[0] if ky else None
        out["exact_replay_long"]["long_lived_thread"] = {"workload": "`[xy]+z[xy]` inside %d bytes of x, a z in the middle" % nx, "seconds": round(dty, 4),
                                                         "matches": int(ky), "exact_path": sy.stats()["exact_path"],
                                                         "first_match_is_the_whole_first_half": first_y == (0, nx // 2 + 2)}
        del tx, sx, spans_x, ty, sy
        torch.cuda.empty_cache()
    except Exception as e:  # noqa: BLE001  (an extra must not take the line down)
        out.setdefault("exact_replay_long", {})["error"] = repr(e)[:300]

    # Quoted strings: `"[^"]*"` over 1 GiB of JSON-like text (a quote every ~32 bytes) and over 1 GiB holding a few long strings --
    # the PAIR kernels of run_scan.hip (the matches are the pairs of the quotes since the last reset: a parity per segment carried
    # from tile to tile).  Before them every quote was a window hit and a walk (41 ms per GiB) and long strings took
    # the carry scan (130 ms per GiB): profiles/r06_pair_probe.txt.  Checked here by properties (every match begins and ends on a
    # quote and holds no other; matches == quotes / 2), against the oracle in tests/test_gpu_pairs.py.
    try:
        nq = 1 << 30
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        letters = torch.tensor(list((b"\"\"\n" + b"abcdefghijklmnopqrstuvwxyz0123456789 ,:{}[]_-.ABCDEFGHIJKLMNOPQRS")[:64]), device=dev, dtype=torch.uint8)
        tq = letters[torch.randint(0, 64, (nq,), device=dev, generator=g).long()].contiguous()
        sq_ = rejit_amd.Scan(rejit_amd.Program("\"[^\"]*\""))
        sq_.run(tq.data_ptr(), nq, stream=c.stream)
        qs, qk = [], []
        for _ in range(5):
            t0q = time.perf_counter()
            kq = sq_.run(tq.data_ptr(), nq, stream=c.stream)
            qs.append(time.perf_counter() - t0q)
            qk.append(sq_.stats()["scan_ms"])
        spans_q = sq_.spans_tensor(dev)
        is_q = tq == ord("\"")
        csum = torch.cumsum(is_q.to(torch.int32), 0)
        ok_q = bool(is_q[spans_q[:, 0]].all().item()) and bool(is_q[spans_q[:, 1] - 1].all().item()) and \
            bool(((csum[spans_q[:, 1] - 1] - csum[spans_q[:, 0]]) == 1).all().item()) and int(kq) == int(is_q.sum().item()) // 2
        t0q = time.perf_counter()
        kc = sq_.count(tq.data_ptr(), nq, stream=c.stream)
        dtc = time.perf_counter() - t0q
        out["quoted_strings"] = {"workload": "`\"[^\"]*\"` MatchAll over %d bytes of JSON-like text (64 letters, 2 of them quotes, 1 a line break)" % nq,
                                 "matches": int(kq), "latency_ms": round(sorted(qs)[len(qs) // 2] * 1e3, 4), "latency_ms_min": round(min(qs) * 1e3, 4),
                                 "value": round(nq / sorted(qs)[len(qs) // 2] / 1e9, 1), "unit": "GB/s of text",
                                 "kernels_ms": round(sorted(qk)[len(qk) // 2], 4), "run_path": sq_.stats()["run_path"],
                                 "pairs_are_the_quotes_in_twos": ok_q,
                                 "count_only": {"call": "rj_scan_count (MatchAllCount): one pass, no list", "matches": int(kc), "latency_ms": round(dtc * 1e3, 4),
                                                "value": round(nq / dtc / 1e9, 1), "unit": "GB/s of text"},
                                 "algorithmic_bytes": "2 x the text read (summary + emit) + 16 B written per match = %d" % (2 * nq + 16 * int(kq)),
                                 "before": "profiles/r06_pair_probe.txt: 41 ms for this text (every quote a window hit and a walk), 130 ms for 1 GiB of long strings (carry scan)"}
        del spans_q, is_q, csum
        tl = torch.full((nq,), ord("x"), dtype=torch.uint8, device=dev)
        tl[torch.randint(0, nq, (nq // 30000,), device=dev, generator=g)] = ord("\"")
        sq_.run(tl.data_ptr(), nq, stream=c.stream)
        ls = []
        for _ in range(5):
            t0q = time.perf_counter()
            kl = sq_.run(tl.data_ptr(), nq, stream=c.stream)
            ls.append(time.perf_counter() - t0q)
        out["quoted_strings"]["long_strings"] = {"workload": "the same pattern over %d bytes with a quote every ~30 000 bytes" % nq, "matches": int(kl),
                                                 "latency_ms": round(sorted(ls)[len(ls) // 2] * 1e3, 4), "value": round(nq / sorted(ls)[len(ls) // 2] / 1e9, 1),
                                                 "unit": "GB/s of text", "run_path": sq_.stats()["run_path"], "linear_path": sq_.stats()["linear_path"]}
        del tq, tl, sq_
        torch.cuda.empty_cache()
    except Exception as e:  # noqa: BLE001
        out.setdefault("quoted_strings", {})["error"] = repr(e)[:300]

    # Everyday patterns on everyday text: `#.*` (a comment to the end of its line) and `a.*b` over 1 GiB of synthetic log-like text
    # (letters, digits, punctuation, a line break every ~70 bytes: tools/probes/zoo.py's text).  Their fast-forward window is ONE byte that
    # such a text holds everywhere; until the last session of round 6 every hit was a walk (`#.*` 6.9 ms, `a.*b` 33.7 ms:
    # profiles/r06_zoo.txt), now windows-mode run shapes take the run kernels first (DESIGN.md 4.11 "When").  `#.*` is checked in
    # full against torch (the first `#` of every line that holds one, to the line's end), `a.*b` by properties.
    try:
        nz = 1 << 30
        gz = torch.Generator(device=dev)
        gz.manual_seed(5)
        weights = {ch: 30 for ch in b"etaoinshrdlucmfwypvbgkqjxz"}
        weights.update({ch: 6 for ch in b"0123456789"})
        weights[ord(" ")] = 60
        weights.update({ch: 4 for ch in b".,:;=-_/@()<>\"'#"})
        weights.update({ch: 8 for ch in b"ETAOINSHR"})
        weights[10] = 16
        syms = torch.tensor(list(weights.keys()), dtype=torch.uint8, device=dev)
        wz = torch.tensor([float(v) for v in weights.values()], device=dev)
        tz = syms[torch.multinomial(wz, nz, replacement=True, generator=gz)].contiguous()
        rec = {"workload": "MatchAll over %d bytes of synthetic log-like text (tools/probes/zoo.py)" % nz, "patterns": {}}
        nl_pos = torch.nonzero(tz == 10).flatten()
        for rx in ("#.*", "a.*b"):
            sz = rejit_amd.Scan(rejit_amd.Program(rx))
            sz.run(tz.data_ptr(), nz, stream=c.stream)
            zs = []
            for _ in range(5):
                t0z = time.perf_counter()
                kz = sz.run(tz.data_ptr(), nz, stream=c.stream)
                zs.append(time.perf_counter() - t0z)
            spz = sz.spans_tensor(dev)
            first_byte = ord(rx[0])
            # per line: the first position of the pattern's first byte; the match ends at the line's end (`#.*`) / behind the line's last b
            hp = torch.nonzero(tz == first_byte).flatten()
            line_of = torch.searchsorted(nl_pos, hp)                      # the number of line breaks before the position
            firsts = hp[torch.cat([torch.ones(1, dtype=torch.bool, device=dev), line_of[1:] != line_of[:-1]])]
            ends_of_line = torch.cat([nl_pos, torch.tensor([nz], device=dev)])[torch.searchsorted(nl_pos, firsts)]
            if rx == "#.*":
                ok = int(kz) == int(firsts.numel()) and bool((spz[:, 0] == firsts).all().item()) and bool((spz[:, 1] == ends_of_line).all().item())
            else:
                # every match begins at its line's first a, ends behind a b inside the line, and no b lies between its end and the line's end
                sel = torch.searchsorted(firsts, spz[:, 0].contiguous())
                on_first = bool((firsts[sel.clamp(max=firsts.numel() - 1)] == spz[:, 0]).all().item())
                eol = ends_of_line[sel.clamp(max=firsts.numel() - 1)]
                bcs = torch.cumsum((tz == ord("b")).to(torch.int32), 0)
                no_b_behind = bool((bcs[(eol - 1).clamp(min=0)] == bcs[spz[:, 1] - 1]).all().item())
                ok = on_first and bool((tz[spz[:, 1] - 1] == ord("b")).all().item()) and bool((spz[:, 1] <= eol).all().item()) and no_b_behind
                del bcs
            st_z = sz.stats()
            rec["patterns"][rx] = {"matches": int(kz), "latency_ms": round(sorted(zs)[len(zs) // 2] * 1e3, 4), "value": round(nz / sorted(zs)[len(zs) // 2] / 1e9, 1),
                                   "unit": "GB/s of text", "kernels_ms": round(st_z["scan_ms"], 4), "run_path": st_z["run_path"], "checked_against_torch": ok}
            del spz, hp, line_of, firsts, ends_of_line, sz
        rec["before"] = "profiles/r06_zoo.txt (RJ_NO_RUNS=1): `#.*` 6.9 ms, `a.*b` 33.8 ms -- the window scan + a walk per hit"
        out["everyday_patterns"] = rec
        del tz, nl_pos
        torch.cuda.empty_cache()
    except Exception as e:  # noqa: BLE001
        out.setdefault("everyday_patterns", {})["error"] = repr(e)[:300]

    if not args.no_big:
        # the north star's target run: the fast-forward scan over a 50 GB synthetic text on ONE GPU
        nb = args.big_literal_bytes
        free, _ = torch.cuda.mem_get_info(dev)
        if free > nb + (8 << 30):
            tb = W.random_ascii_torch(nb, 0xC0FFEE, dev)
            offs_b = W.plant_offsets(nb, 6, 1000, seed=11, boundaries=[1 << 32, 1 << 35, nb // 2])
            W.plant(tb, offs_b, b"regexp")

            def check_big(sc):
                found = {b for b, _ in sc.spans()}
                assert set(offs_b) <= found, "a planted occurrence was missed (50 GB)"

            out["literal_50gb"] = single_pattern_extra(
                c, rejit_amd, tb, nb, "regexp",
                "literal 'regexp' MatchAll over %d bytes random ASCII, %d planted (north star: 50 GB fast-forward scan, 1 GPU)" % (nb, len(offs_b)),
                "scan_windows<1>", 5, check_big, "literal_50gb", False, args)
            del tb
            torch.cuda.empty_cache()
        else:
            out["literal_50gb"] = {"skipped": "not enough free HBM (%d bytes)" % free}


def run_single_pattern(args, c, which):
    """--workload literal / complex: one pattern, --literal-bytes per GPU, contiguous shards with the
    pattern's halo, the left-most-longest selection carried over the cuts (sharding.sharded_match_all),
    spans gathered to rank 0 as tensors."""
    import random as _random
    import rejit_amd
    from rejit_amd import sharding, workloads as W
    torch, dist, world, rank, dev = c.torch, c.dist, c.world, c.rank, c.dev
    rx = "regexp" if which == "literal" else W.BENCH_REGEXES[3][0]
    prog = rejit_amd.Program(rx)
    sc = rejit_amd.Scan(prog)
    max_len = prog.info()["max_len"]
    n_total = args.literal_bytes * world
    ranges = sharding.partition(n_total, world)
    own = ranges[rank]
    vis_lo, vis_hi = sharding.visible_range(n_total, own, max_len, whole_text=bool(prog.info()["ring_artefact_risk"]))
    t = W.random_ascii_torch(vis_hi - vis_lo, 0xC0FFEE, dev, start=vis_lo)
    n_local = vis_hi - vis_lo
    # planted occurrences, also across the cuts (global offsets; every rank writes the part it sees)
    cuts = [r[0] for r in ranges[1:]]
    if which == "literal":
        needles = [(o, b"regexp") for o in W.plant_offsets(n_total, 6, 200 * world, seed=3, boundaries=cuts)]
    else:
        rng = _random.Random(7)
        needles = [(o, W.complex_regex_sample(rng)) for o in W.plant_offsets(n_total, 64, 200 * world, seed=7, boundaries=cuts)]
    for o, s in needles:
        lo, hi = max(o, vis_lo), min(o + len(s), vis_hi)
        if lo < hi:
            W.plant(t, [lo - vis_lo], s[lo - o:hi - o])
    own_lo, own_hi = own[0] - vis_lo, min(own[1], n_total + 1) - vis_lo
    stream = c.stream
    torch.cuda.synchronize(dev)
    ms = []

    def local_scan(lo, hi, cur, prev_end, have):
        sc.run(t.data_ptr(), n_local, own_begin=lo - vis_lo, own_end=min(hi, n_total + 1) - vis_lo, carry_cur=max(cur - vis_lo, 0),
               carry_prev_end=max(prev_end - vis_lo, 0), have_prev=have, stream=stream)
        return sc.spans_tensor(dev) + vis_lo      # (k, 2) int64 on the device, global offsets

    def step(record):
        total, gathered, _ = sharding.sharded_match_all_tensor(local_scan, ranges, rank, world, dist if world > 1 else None, c.cdev)
        if record:
            ms.append(sc.stats()["scan_ms"])
        return total, gathered

    elapsed, (total, gathered) = timed(c, args, step)
    if rank == 0:
        got = {int(b): int(e) for b, e in gathered.cpu().tolist()}
        for o, s in needles:
            if which == "literal":
                assert got.get(o) == o + 6, ("planted occurrence missed", o)
            else:
                assert o + len(s) in set(got.values()), ("planted complex match missed", o)
        assert len(got) == total
    own_bytes = min(own[1], n_total) - own[0]
    out = base_line(args, c, "GB/s text scanned (%s MatchAll); matches alongside" % which, n_total * args.steps / elapsed / 1e9, elapsed,
                    {"workload": "%s MatchAll over %d bytes random ASCII per GPU (BASELINE configs[%d] shape)" % (rx, args.literal_bytes,
                                                                                                                     1 if which == "literal" else 3),
                     "text_bytes_per_gpu": int(own_bytes),
                     "sharding": "contiguous byte ranges + %d-byte halo; carry all_gather + tensor gather of the spans to rank 0" % (max_len - 1)})
    out["matches"] = int(total)
    a_ms = sum(ms) / max(len(ms), 1)
    out["roofline"] = hbm_roofline("scan_windows<1>", own_bytes, a_ms, None, len(ms))
    # --dump-outputs: the job's (begin, end) spans as gathered on rank 0, global offsets
    if rank == 0:
        out["_dump"] = {"spans": gathered.cpu().numpy().reshape(-1, 2)}
    return out


# ------------------------------------------------------------------------------------------ jrep
def synthetic_tree(n_files, seed):
    """Source-like files: lines of ~40 bytes of words, sizes log-normal around 20 KB; 1 % hold the needle."""
    import numpy as np
    rng = np.random.default_rng(seed)
    words = [w.encode() for w in ("int return for while static const char void if else struct size_t uint64_t include define "
                                  "buffer length offset index count result value pointer match text begin end state table").split()]
    sizes = np.clip(rng.lognormal(np.log(20000), 0.6, n_files), 200, 400000).astype(np.int64)
    files = []
    for i in range(n_files):
        k = int(sizes[i]) // 7 + 1
        ws = rng.integers(0, len(words), k)
        brk = rng.random(k) < 0.15
        parts = []
        for j in range(k):
            parts.append(words[ws[j]])
            parts.append(b"\n" if brk[j] else b" ")
        data = b"".join(parts)[:int(sizes[i])] + b"\n"
        if rng.random() < 0.01:
            at = int(rng.integers(0, max(1, len(data) - 10)))
            data = data[:at] + b" regexp " + data[at:]
        files.append(data)
    return files


def run_jrep(args, c):
    """--workload jrep (BASELINE configs[4] shape): every rank owns --tree-files files (file-sharded: no
    text crosses ranks), matches them in batches through rj_match_all_batch (host buffers, PCIe included),
    builds the `^` line table of the files with matches (sample/jrep.cc:294-313) and formats
    file:line:text; the exchange step gathers the output bytes to rank 0."""
    import io
    import rejit_amd
    from rejit_amd import sharding
    sys.path.insert(0, os.path.join(ROOT, "samples"))
    import jrep_gpu
    world, rank = c.world, c.rank
    files = synthetic_tree(args.tree_files, 1000 + rank)
    names = ["r%d/f%06d.c" % (rank, i) for i in range(len(files))]
    prog = rejit_amd.Program(b"regexp")
    sol = rejit_amd.Program(b"^")
    fmt = argparse.Namespace(with_filename=True, line_number=True, before=0, after=0, color=False)
    total_bytes = sum(len(f) for f in files)

    def step(record):
        out = io.BytesIO()
        results = prog.match_all_batch(files)
        hit = [i for i, r in enumerate(results) if r]
        lines = sol.match_all_batch([files[i] for i in hit]) if hit else []
        for i, ls in zip(hit, lines):
            jrep_gpu.print_file(out, names[i], files[i], results[i], [b for b, _ in ls], fmt)
        whole = sharding.gather_bytes(out.getvalue(), rank, world, c.dist, device=c.cdev if args.backend == "nccl" else None)
        return (len(hit), whole)

    elapsed, (hits, whole) = timed(c, args, step)
    tb = c.torch.tensor([total_bytes, hits], dtype=c.torch.int64, device=c.cdev)
    if world > 1:
        c.dist.all_reduce(tb)
    job_bytes, job_hits = int(tb[0]), int(tb[1])
    out = base_line(args, c, "GB/s text searched end to end (jrep over a synthetic source tree, host buffers, PCIe included)",
                    job_bytes * args.steps / elapsed / 1e9, elapsed,
                    {"workload": "jrep -R -H -n regexp over %d files per GPU (BASELINE configs[4] shape)" % args.tree_files,
                     "text_bytes_per_gpu": int(total_bytes), "sharding": "by file; gather of the output bytes to rank 0"})
    out["files_with_matches"] = job_hits
    if rank == 0:
        out["output_lines"] = whole.count(b"\n")
        assert out["output_lines"] >= job_hits
    out["roofline"] = {"bound": "hbm", "note": "PCIe- and host-bound end to end; the device pass is the regexdna / literal kernel",
                       "achieved": round(job_bytes * args.steps / elapsed / 1e9 / max(world, 1), 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": round(job_bytes * args.steps / elapsed / 1e9 / max(world, 1) / HBM_PEAK_GBS, 5), "traffic": None}
    # --dump-outputs: the files with matches and the formatted output (file:line:text) as its bytes
    if rank == 0:
        import numpy as np
        out["_dump"] = {"files_with_matches": [job_hits], "output_bytes": np.frombuffer(whole, dtype=np.uint8)}
    return out


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves, one process per GPU under
    torch.distributed.run on this node (the way sample/regexdna-multithread.cc:65-78 fans out threads), and pass
    rank 0's JSON line through."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(cmd, env=env))


# ------------------------------------------------------------------------------------------ whole programs
def end_to_end_extra(args, c, out):
    """The reference's headline is a WHOLE-PROGRAM time (README.md:66: regexdna, 50M-line input, 14.624 s on an
    i5-2400): read the FASTA file, strip it, nine counts, eleven replaces (sample/regexdna.cc:41-91).  Timed here as
    processes, H2D copies, start-up and all: the reference's regexdna.cc UNCHANGED on librejit_hip.so, the same
    program on the reference's own library on this host (one core), and samples/regexdna_gpu.py (text resident in
    HBM for the whole program)."""
    import subprocess
    import tempfile
    from rejit_amd import workloads as W
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    exe_hip, exe_ref = os.path.join(ref_dir, "regexdna_hip"), os.path.join(ref_dir, "regexdna_ref")
    if not os.path.exists(exe_hip):
        return
    raw = W.fasta_raw_torch(args.fasta_n, c.dev).cpu().numpy()
    d = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    path = os.path.join(d, "rejit_bench_fasta_%d.txt" % os.getpid())
    raw.tofile(path)
    n_raw = int(raw.size)
    del raw
    c.torch.cuda.empty_cache()
    rec = {"input": "Benchmarks-Game FASTA, n = %d: %d bytes (%s)" % (args.fasta_n, n_raw, path),
           "published_reference_s": {"value": 14.624, "hardware": "i5-2400 @ 3.1 GHz, 1 thread", "source": "reference README.md:66"}}

    def run(cmd, key, note):
        best, text_out = None, b""
        for _ in range(2):
            with open(path, "rb") as fh:
                t0 = time.perf_counter()
                r = subprocess.run(cmd, stdin=fh, capture_output=True)
                dt = time.perf_counter() - t0
            if r.returncode != 0:
                rec[key] = {"failed": r.stderr.decode()[-300:]}
                return None
            if best is None or dt < best:
                best, where = dt, r.stderr.decode().strip().splitlines()[-1:] if "--timing" in cmd else None
            text_out = r.stdout
        rec[key] = {"seconds": round(best, 3), "what": note}
        if where:
            rec[key]["where"] = where[0][:300]     # (the sample's own account of its wall time: imports / input / context + upload / device)
        return text_out.decode().split()

    try:
        got = run([exe_hip], "reference_regexdna_on_librejit_hip", "sample/regexdna.cc unchanged, linked against librejit_hip.so; process wall time, 2 runs, best")
        native_exe = os.path.join(ROOT, "samples", "regexdna_gpu")
        native = None
        if os.path.exists(native_exe):
            native = run([native_exe], "regexdna_gpu_native", "samples/regexdna_gpu (C++ over the C ABI): one upload, strip + nine counts in one pass + eleven "
                         "replacements on the device, the counts and the replacements in flight together; process wall time, 2 runs, best")
        gpu = run([sys.executable, os.path.join(ROOT, "samples", "regexdna_gpu.py"), "--timing"], "regexdna_gpu_py",
                  "samples/regexdna_gpu.py: one upload, text stays in HBM; process wall time incl. the Python / torch start-up (`where`: the "
                  "sample's own account -- BENCH_r04's 12.4 s on a fresh lease against 1.4-1.6 s elsewhere is import time, not device time)")
        if os.path.exists(exe_ref):
            run([exe_ref], "reference_regexdna_on_its_own_library", "the same program on the reference's library, this host, 1 core (default flags: its counts are "
                "wrong for six patterns, SURVEY 4.4 Q1 -- timing only)")
        fx = fullsize_fixture()
        if got and fx and "c3" in fx and fx["c3"]["fasta_n"] == args.fasta_n:
            want = [p["digest"]["count"] for p in fx["c3"]["patterns"]]
            counts = [int(got[2 * i + 1]) for i in range(9)]
            assert counts == want, ("regexdna_hip counts differ from the reference's (ff=0) counts", counts, want)
            rec["parity"] = "the nine counts printed by regexdna_hip == the real reference's (correct configuration)"
            if gpu:
                assert gpu == got, "regexdna_gpu.py and regexdna_hip print different results"
                rec["parity"] += "; regexdna_gpu.py prints the same 12 lines"
            if native:
                assert native == got, "samples/regexdna_gpu and regexdna_hip print different results"
                rec["parity"] += "; so does the native samples/regexdna_gpu"
    finally:
        os.unlink(path)
    out["end_to_end"] = rec


def jrep_tree(n_files, total_bytes):
    """The synthetic tree of the jrep_10gb extra (BASELINE configs[4]: 100 000 files, 10 GB): log-normal sizes with a heavy
    tail, bodies cut from a ~12 MB corpus of source-like lines, ` regexp ` planted in every hundredth file.  Deterministic
    (tests/golden/make_fullsize.py runs the real reference over the same files)."""
    import numpy as np
    rng = np.random.default_rng(5)
    corpus = b"".join(synthetic_tree(600, 77))                       # ~12 MB of source-like lines without the needle
    corpus = corpus.replace(b"regexp", b"regexq")
    cn = len(corpus)
    sizes = np.clip(rng.lognormal(np.log(20000), 1.8, n_files), 200, 64 << 20).astype(np.int64)
    sizes = (sizes * (total_bytes / sizes.sum())).astype(np.int64) + 1
    starts = rng.integers(0, cn, n_files)
    files = []
    for i in range(n_files):
        a, k = int(starts[i]), int(sizes[i])
        reps = (a + k + cn - 1) // cn
        body = (corpus * reps)[a:a + k] if reps > 1 else corpus[a:a + k]
        if i % 100 == 7:
            at = (i * 7919) % max(1, k - 8)
            body = body[:at] + b" regexp " + body[at + 8:]
        files.append(body)
    return files


def jrep_digest(rows):
    """rows: (file index, matches in the file, line starts of the file) of every file with a match, in file order."""
    import hashlib
    h = hashlib.sha256()
    for i, k, l in rows:
        h.update(b"%d:%d:%d\n" % (i, k, l))
    return h.hexdigest()


def jrep_extra(args, c, out):
    """BASELINE configs[4] at its size on ONE GPU: 100 000 source-like files, 10 GB, log-normal sizes with a heavy tail,
    1 % hold the needle -- host buffers through rj_match_all_batch (packing, PCIe and result copies included) + the `^`
    line tables of the files with matches, in batches of 256 MiB like samples/jrep_gpu.  The reference on the host: its own
    jrep loop (one MatchAll per file + `^` for the files with a match) over a bounded sample of the same files, one core."""
    import rejit_amd
    n_files = args.jrep_files
    files = jrep_tree(n_files, args.jrep_bytes)
    total = sum(len(f) for f in files)
    prog, sol = rejit_amd.Program(b"regexp"), rejit_amd.Program(b"^")

    # the batches of one pass: files [b, e) of at most 256 MiB
    batches, at = [], 0
    while at < n_files:
        b, size = at, 0
        while at < n_files and (at == b or size + len(files[at]) <= (256 << 20)):
            size += len(files[at])
            at += 1
        batches.append((b, at))
    n_threads = max(1, int(getattr(args, "jrep_threads", 1)))

    # the caller's file table per batch (pointers + sizes, as samples/jrep_gpu.cc holds them from reading the tree): built once,
    # outside the timed region -- ctypes marshalling of 100 000 Python objects is the binding's cost (36 ms per pass), not the library's
    import numpy as np
    tables = {be: prog.batch_table(files[be[0]:be[1]]) for be in batches}

    def one_batch(be):
        b, e = be
        res = prog.match_all_batch_table(tables[be])
        idx = [b + int(i) for i in np.flatnonzero(res)]
        lc = sol.match_all_batch_counts([files[i] for i in idx]) if idx else []
        return [(i, int(res[i - b]), l) for i, l in zip(idx, lc)]

    def one_pass():
        # (--jrep-threads N: caller threads as the reference's jrep has them, sample/jrep.cc:408-493, each with its own batches and
        # its own scratch below the boundary.  Measured, round 6: 1 thread 41 GB/s, 2: 37, 3: 33, 4: 29 -- the batches' packing and
        # uploads contend for the same host memory and the same link; one caller is the default)
        if n_threads == 1:
            parts = [one_batch(be) for be in batches]
        else:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=n_threads) as pool:
                parts = list(pool.map(one_batch, batches))
        rows = [r for part in parts for r in part]
        return len(rows), sum(r[2] for r in rows), rows

    one_pass()
    t0 = time.perf_counter()
    hits, lines, rows = one_pass()
    dt = time.perf_counter() - t0
    rec = {"workload": "jrep shape at BASELINE size: %d files, %d bytes (log-normal sizes, sigma 1.8), needle in 1 %% of them; rj_match_all_batch in "
                       "256 MiB batches (the file table -- pointers, sizes -- built once, as a native caller holds it) + `^` line tables of the files with matches, %d caller thread(s) (the reference's jrep: a worker pool, sample/jrep.cc:408-493); host buffers, PCIe included" % (n_files, total, n_threads),
           "value": round(total / dt / 1e9, 2), "unit": "GB/s end to end", "seconds": round(dt, 3), "files_with_matches": hits, "line_starts": lines}
    fx = fullsize_fixture()
    if fx and "c5" in fx and fx["c5"]["files"] == n_files and fx["c5"]["bytes_asked"] == args.jrep_bytes:
        c5 = fx["c5"]
        assert (hits, lines, sum(k for _, k, _ in rows)) == (c5["files_with_matches"], c5["line_starts"], c5["matches"]), \
            ("jrep_10gb differs from the real reference's answer", hits, lines, c5)
        assert jrep_digest(rows) == c5["sha256"], "jrep_10gb: per-file counts differ from the real reference's"
        rec["parity_full_size"] = "files with matches, matches and line starts per file == the real reference's over the same 100 000 files (sha256 of the rows)"
    ref, _ = _ref()
    if ref is not None and not args.no_cpu_baseline:
        ref.set_flags(1, 1, 0, 1)
        sample, budget, done_bytes, ref_hits = files[: max(1, n_files // 50)], 0, 0, 0
        t0 = time.perf_counter()
        for f in sample:
            k = int(ref.lib.ref_match_all_repeat(b"regexp", f, len(f), 1))
            if k:
                ref_hits += 1
                ref.lib.ref_match_all_repeat(b"^", f, len(f), 1)
            done_bytes += len(f)
        dtr = time.perf_counter() - t0
        rec["cpu_baseline"] = {"value": round(done_bytes / dtr / 1e9, 2), "unit": "GB/s", "cores": 1, "kind": "reference",
                               "sample": "the first %d files (%d bytes): one MatchAll per file + `^` for the %d files with a match, buffers in memory"
                                         % (len(sample), done_bytes, ref_hits), "seconds": round(dtr, 3)}
    out["jrep_10gb"] = rec


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        spawn_ranks(args)
    c = setup(args)
    import rejit_amd
    rejit_amd.build()
    if args.workload == "regexdna":
        out, extras = run_regexdna(args, c)
        if out is None:
            return
        if extras:
            literal_and_complex_extras(args, c, out)
            if not args.no_big:
                jrep_extra(args, c, out)
                end_to_end_extra(args, c, out)
    elif args.workload in ("literal", "complex"):
        out = run_single_pattern(args, c, args.workload)
    else:
        out = run_jrep(args, c)
    dump = out.pop("_dump", None)
    if c.rank == 0 and args.dump_outputs and dump is not None:
        dump_outputs(args.dump_outputs, dump)
    if c.rank == 0:
        print(json.dumps(out))
    if c.world > 1:
        c.dist.destroy_process_group()


if __name__ == "__main__":
    main()
