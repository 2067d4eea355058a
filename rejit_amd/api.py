"""ctypes binding of include/rejit_hip.h + the in-tree build of librejit_hip.so."""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import List, Optional, Tuple

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
SOURCES = ["kernels.hip", "scan_windows.hip", "dense_walk.hip", "select_kernels.hip", "plane_scan.hip", "plane_count.hip", "run_scan.hip", "emit_scan.hip", "dense_streams.hip", "dense_streams_select.hip", "verify_lds.hip", "carry_kernels.hip", "engine.hip", "multi_pattern.hip", "host_api.hip", "record_join.hip", "record_pack.hip", "record_replace.hip", "record_split.hip", "record_group.hip", "record_sort.hip", "record_lookup.hip", "record_parse.hip", "record_time.hip", "record_format.hip", "record_zip.hip", "record_time_format.hip", "record_translate.hip", "record_csv.hip", "record_csv_format.hip", "linear.hip", "exact_replay.hip", "multi_device.hip", "parser.cc", "lowering.cc", "rejit_api.cc"]
HEADERS = ["kernels.h", "device_program.h", "lowering.h", "carry_scan.h", "behind_walk.h", "exact_replay.h", "engine_internal.h", "table_layout.h", "lds_walk.h", "trace_stamp.h", "dense_swar.h", "dense_streams.h", "tile_lookback.h", "exact_count.h", "plane_args.h", "short_walk.h", "run_scan.h", "kernel_util.h", "wave_ops.h", "plane_codes.h", "plane_network.h", "stream_load.h", "record_join.h", "record_pack.h", "record_rows.h", "record_replace.h", "record_split.h", "record_group.h", "record_group_build.h", "record_sort.h", "record_lookup.h", "record_parse.h", "record_time.h", "pow5_table.h", "record_format.h", "pow10_table.h", "record_zip.h", "record_time_format.h", "record_translate.h", "record_csv.h", "record_csv_format.h", "record_frame.h", "dense_streams.hip"]  # (dense_streams_select.hip includes dense_streams.hip)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread"]  # of every compile (tools/device_code_diff.py uses them too)
LIB = os.path.join(PKG, "librejit_hip.so")

_u64p = ctypes.POINTER(ctypes.c_uint64)


def _raise(e):
    raise e


class RejitError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"rejit_hip status {status}: {message}")
        self.status = status
        self.message = message


def library_path() -> str:
    return LIB


HASH = os.path.join(PKG, "librejit_hip.srchash")


def _source_hash() -> str:
    import hashlib
    h = hashlib.sha256()
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS]
    deps += [os.path.join(PKG, "..", "include", f) for f in ("rejit.h", "rejit_hip.h")]
    deps += [os.path.join(PKG, "..", "tools", "probes", "read_probe.hip")]
    for d in deps:
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _stale() -> bool:
    """The library is rebuilt when the CONTENT of a source differs from what it was built
    from (mtimes do not survive the copy to the GPU box)."""
    if not os.path.exists(LIB) or not os.path.exists(HASH) or not os.path.exists(os.path.join(PKG, "librejit_bench.so")):
        return True
    try:
        with open(HASH) as fh:
            return fh.read().strip() != _source_hash()
    except OSError:
        return True


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP/C++ source for gfx950 into rejit_amd/librejit_hip.so (in-tree, so
    the built library travels with the repo snapshot).  hipcc cross-compiles without a GPU."""
    if not force and not _stale():
        return LIB
    # several ranks of one job may arrive here together: serialise, and re-check under the lock
    import fcntl
    lock = open(os.path.join(PKG, ".build.lock"), "w")
    fcntl.flock(lock, fcntl.LOCK_EX)
    try:
        if not force and not _stale():
            return LIB
        return _build_locked(verbose)
    finally:
        fcntl.flock(lock, fcntl.LOCK_UN)
        lock.close()


def _build_locked(verbose: bool) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    # one object per source, compiled side by side (kernels.hip alone takes about a minute), then linked
    objdir = os.path.join(PKG, "build")
    os.makedirs(objdir, exist_ok=True)
    flags = FLAGS

    # an object is kept when it was compiled from this very source and the very headers IT includes (content hash beside
    # it): kernels.hip alone takes about a minute, a change to one file -- or to a header three sources use -- should cost
    # those files only
    import hashlib
    import re
    inc_re = re.compile(rb'^\s*#\s*include\s+"([^"]+)"', re.M)

    def closure(path, seen):
        path = os.path.normpath(path)
        if path in seen or not os.path.exists(path):
            return
        seen.add(path)
        with open(path, "rb") as fh:
            body = fh.read()
        for m in inc_re.finditer(body):
            closure(os.path.join(os.path.dirname(path), m.group(1).decode()), seen)

    def compile_one(src):
        obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
        deps = set()
        closure(os.path.join(CSRC, src), deps)
        hh = hashlib.sha256(" ".join(flags).encode())
        for d in sorted(deps):
            hh.update(os.path.basename(d).encode())
            with open(d, "rb") as fh:
                hh.update(fh.read())
        want = hh.hexdigest()
        stamp = obj + ".srchash"
        try:
            if os.path.exists(obj) and open(stamp).read().strip() == want:
                return obj
        except OSError:
            pass
        cmd = [hipcc] + flags + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        with open(stamp, "w") as fh:
            fh.write(want + "\n")
        return obj

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(8, len(SOURCES))) as pool:
        objs = list(pool.map(compile_one, SOURCES))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", LIB + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(LIB + ".tmp", LIB)
    # the measurement library (bench.py's read-only ceiling): its own shared object, not part of the product's ABI
    probe_src = os.path.join(PKG, "..", "tools", "probes", "read_probe.hip")
    cmd = [hipcc] + flags + ["-shared", probe_src, "-o", BENCH_LIB + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(BENCH_LIB + ".tmp", BENCH_LIB)
    with open(HASH, "w") as f:
        f.write(_source_hash() + "\n")
    return LIB


class _Info(ctypes.Structure):
    _fields_ = [("n_positions", ctypes.c_int32), ("n_words", ctypes.c_int32), ("has_assertions", ctypes.c_int32),
                ("scan_mode", ctypes.c_int32), ("n_windows", ctypes.c_int32), ("window_offset", ctypes.c_uint32),
                ("window_len", ctypes.c_uint32), ("min_len", ctypes.c_uint64), ("max_len", ctypes.c_uint64),
                ("ring_artefact_risk", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class _Stats(ctypes.Structure):
    _fields_ = [("n_hits", ctypes.c_uint64), ("n_candidates", ctypes.c_uint64), ("n_matches", ctypes.c_uint64),
                ("scan_ms", ctypes.c_float), ("total_ms", ctypes.c_float), ("retries", ctypes.c_int32),
                ("large_path", ctypes.c_int32), ("exact_path", ctypes.c_int32), ("linear_path", ctypes.c_int32),
                ("stream_path", ctypes.c_int32), ("slow_starts", ctypes.c_int32), ("count_path", ctypes.c_int32), ("run_path", ctypes.c_int32)]


class _RecordStats(ctypes.Structure):
    _fields_ = [("n_kept", ctypes.c_uint64), ("n_matching", ctypes.c_uint64), ("n_crossing", ctypes.c_uint64), ("n_matches", ctypes.c_uint64)]


class _SortStats(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_uint64), ("keyed_rows", ctypes.c_uint64), ("skip_rows", ctypes.c_uint64), ("long_rows", ctypes.c_uint64)]


class _LookupStats(ctypes.Structure):
    _fields_ = [("n_found", ctypes.c_uint64), ("n_set_distinct", ctypes.c_uint64), ("n_set_hit", ctypes.c_uint64), ("long_rows", ctypes.c_uint64)]


class _ParseStats(ctypes.Structure):
    _fields_ = [("n_ok", ctypes.c_uint64), ("n_empty", ctypes.c_uint64), ("n_malformed", ctypes.c_uint64), ("n_range", ctypes.c_uint64),
                ("n_inexact", ctypes.c_uint64)]


class _FormatTimeStats(ctypes.Structure):
    _fields_ = [("n_ok", ctypes.c_uint64), ("n_null", ctypes.c_uint64), ("n_range", ctypes.c_uint64)]


class _TranslateStats(ctypes.Structure):
    _fields_ = [("bytes_in", ctypes.c_uint64), ("bytes_dropped", ctypes.c_uint64), ("bytes_changed", ctypes.c_uint64)]


class _CsvStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("n_rows", "n_fields", "n_quoted", "n_escapes", "n_bad_quote", "n_bad_close", "n_bare_cr", "open_at_end",
                                               "first_bad")]


class _CsvFormatStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("n_rows", "n_fields", "n_quoted", "n_doubled", "total")]


class CsvResult:
    """What Scan.csv_records returns: the tables of rj_scan_records_csv as tensors on the text's device -- row_first (int64,
    n_rows + 1), row_begin / row_end (int64, n_rows; None with rows=False), field_begin / field_end (int64, n_fields),
    field_flags (int32, n_fields: the CSV_* bits) -- and stats, rj_csv_stats as a dict (first_bad: None when nothing is
    malformed)."""

    def __init__(self, row_first, row_begin, row_end, field_begin, field_end, field_flags, stats):
        self.row_first, self.row_begin, self.row_end = row_first, row_begin, row_end
        self.field_begin, self.field_end, self.field_flags = field_begin, field_end, field_flags
        self.stats = stats
        self.n_rows, self.n_fields = stats["n_rows"], stats["n_fields"]


CSV_ESCAPED, CSV_BAD_QUOTE, CSV_BAD_CLOSE, CSV_BARE_CR, CSV_OPEN = 1, 2, 4, 8, 16
CSV_MALFORMED = CSV_BAD_QUOTE | CSV_BAD_CLOSE | CSV_BARE_CR | CSV_OPEN


class ZipColumn(ctypes.Structure):
    """rj_zip_column: one column of rj_scan_records_zip (64 bytes)"""
    _fields_ = [("d_text", ctypes.c_void_p), ("n", ctypes.c_uint64), ("d_rec_begin", ctypes.c_void_p), ("d_rec_end", ctypes.c_void_p),
                ("n_records", ctypes.c_uint64), ("d_indices", ctypes.c_void_p), ("n_indices", ctypes.c_uint64), ("width", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


PARSE_KINDS = {"int64": 0, "uint64": 1, "float64": 2}                      # RJ_PARSE_INT64, _UINT64, _FLOAT64
PARSE_TRIM, PARSE_WIDE = 1, 4                                              # flags (RJ_PARSE_TRIM, RJ_PARSE_WIDE; 2 is reserved)
TIME_UNITS = {"s": 0, "ms": 1, "us": 2, "ns": 3}                             # RJ_TIME_SECOND, _MILLI, _MICRO, _NANO
PARSE_OK, PARSE_EMPTY, PARSE_MALFORMED, PARSE_RANGE, PARSE_INEXACT = range(5)   # a row's status (RJ_PARSE_OK, ...)


class RecordsResult:
    """What Scan.run_records returns: rj_record_stats (n_kept, n_matching, n_crossing, n_matches) and the per-record tensors --
    counts (int32: the library's uint32, saturating, so 2^32 - 1 reads -1) and first (int64), both on the text's device.
    Record i's matches are spans[first[i] : first[i] + counts[i]] of the scan's own list (Scan.spans_tensor)."""

    def __init__(self, stats: _RecordStats, counts, first, n_records: int):
        self.n_kept, self.n_matching = int(stats.n_kept), int(stats.n_matching)
        self.n_crossing, self.n_matches = int(stats.n_crossing), int(stats.n_matches)
        self.counts, self.first, self.n_records = counts, first, n_records

    def __repr__(self):
        return "RecordsResult(n_records=%d, n_kept=%d, n_matching=%d, n_crossing=%d, n_matches=%d)" % (
            self.n_records, self.n_kept, self.n_matching, self.n_crossing, self.n_matches)


_lib = None

# every symbol include/rejit_hip.h declares
# rj_allgather_fn (include/rejit_hip.h): ctx, d_send, d_recv, bytes per rank, hip stream -> 0 on success
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p)
# rj_gatherv_fn: ctx, d_send, send_bytes, d_recv (root only), recv_offsets[world], recv_bytes[world], root, hip stream -> 0 on success
GATHERV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                              ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_void_p)

C_ABI_SYMBOLS = ["rj_compile", "rj_program_free", "rj_program_info", "rj_last_error", "rj_match_full",
                 "rj_match_anywhere", "rj_match_first", "rj_match_all", "rj_free_spans", "rj_scan_create",
                 "rj_scan_destroy", "rj_scan_run", "rj_scan_device_spans", "rj_scan_copy_spans", "rj_scan_stats",
                 "rj_scan_match_full", "rj_device_count", "rj_replace_all", "rj_free_text", "rj_scan_replace",
                 "rj_match_all_batch", "rj_multi_create", "rj_multi_destroy", "rj_multi_run", "rj_multi_scan",
                 "rj_multi_scan_ms", "rj_scan_start", "rj_scan_finish", "rj_multi_set_mode", "rj_multi_run_range",
                 "rj_multi_bounds", "rj_batch_separator", "rj_match_all_packed", "rj_host_alloc", "rj_host_free",
                 "rj_multi_bounds_device", "rj_carry_decide", "rj_multi_start", "rj_multi_finish", "rj_multi_order_after",
                 "rj_multi_device_counts", "rj_multi_device_counts_via", "rj_multi_set_tail_stream", "rj_multi_set_timing", "rj_scan_set_timing", "rj_set_default_timing",
                 "rj_scan_gather_spans", "rj_scan_gather_spans_via", "rj_scan_gathered_spans", "rj_multi_set_counts_only", "rj_scan_stats_sized", "rj_scan_copy_gathered_spans", "rj_scan_count", "rj_host_stats", "rj_replace_all_begin", "rj_replace_all_fetch",
                 "rj_scan_records", "rj_scan_records_select", "rj_scan_records_pack", "rj_scan_records_replace", "rj_scan_records_split", "rj_scan_records_group", "rj_scan_records_sort", "rj_scan_records_lookup", "rj_scan_records_parse", "rj_scan_records_parse_time", "rj_scan_records_format", "rj_scan_records_zip", "rj_scan_records_format_time", "rj_scan_records_translate", "rj_scan_records_csv", "rj_scan_records_format_csv"]


def load_library():
    """Load the product library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise FileNotFoundError(f"{LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        # PyTorch ships its own copy of the HIP runtime.  If librejit_hip.so (linked against
        # /opt/rocm's) is loaded first, the process ends up with two runtimes and the later one sees
        # no device; loading torch first makes both use the one runtime.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB)
    vp, cp, sz, i64, u64 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_uint64
    L.rj_compile.restype = ctypes.c_int
    L.rj_compile.argtypes = [cp, ctypes.POINTER(vp)]
    L.rj_program_free.argtypes = [vp]
    L.rj_program_info.argtypes = [vp, ctypes.POINTER(_Info)]
    L.rj_last_error.restype = cp
    L.rj_match_full.argtypes = [vp, cp, sz]
    L.rj_match_anywhere.argtypes = [vp, cp, sz]
    L.rj_match_first.argtypes = [vp, cp, sz, _u64p, _u64p]
    L.rj_match_all.restype = i64
    L.rj_match_all.argtypes = [vp, cp, sz, ctypes.POINTER(_u64p)]
    L.rj_free_spans.argtypes = [_u64p]
    L.rj_match_all_batch.restype = i64
    L.rj_match_all_batch.argtypes = [vp, ctypes.POINTER(cp), ctypes.POINTER(sz), sz, _u64p, ctypes.POINTER(_u64p)]
    L.rj_scan_create.argtypes = [vp, ctypes.POINTER(vp)]
    L.rj_multi_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(vp)]
    L.rj_multi_destroy.argtypes = [vp]
    L.rj_multi_run.argtypes = [vp, vp, u64, _u64p, vp]
    L.rj_multi_run_range.argtypes = [vp, vp, u64, u64, u64, _u64p, vp]
    L.rj_multi_start.argtypes = [vp, vp, u64, u64, u64, vp]
    L.rj_multi_finish.argtypes = [vp, _u64p]
    L.rj_multi_order_after.argtypes = [vp, vp]
    L.rj_multi_scan.restype = vp
    L.rj_multi_scan.argtypes = [vp, ctypes.c_int]
    L.rj_multi_scan_ms.restype = ctypes.c_float
    L.rj_multi_scan_ms.argtypes = [vp]
    L.rj_multi_set_mode.argtypes = [vp, ctypes.c_int]
    L.rj_multi_set_tail_stream.argtypes = [vp, ctypes.c_int]
    L.rj_multi_set_timing.argtypes = [vp, ctypes.c_int]
    L.rj_multi_set_counts_only.argtypes = [vp, ctypes.c_int]
    L.rj_scan_stats_sized.argtypes = [vp, vp, sz]
    L.rj_scan_copy_gathered_spans.restype = i64
    L.rj_scan_copy_gathered_spans.argtypes = [vp, _u64p, u64]
    L.rj_scan_set_timing.argtypes = [vp, ctypes.c_int]
    L.rj_set_default_timing.argtypes = [ctypes.c_int]
    L.rj_set_default_timing(1)   # bench.py, the tests and the tools read scan_ms: the scan kernel's start event is on for them
    L.rj_multi_bounds.argtypes = [vp, _u64p, vp]
    L.rj_multi_bounds_device.argtypes = [vp, ctypes.c_int64, ctypes.c_int, vp, vp]
    L.rj_carry_decide.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    L.rj_multi_device_counts.argtypes = [vp, vp, u64, u64, u64, ctypes.c_int64, vp, ctypes.c_int, ctypes.c_int, _u64p, vp]
    L.rj_multi_device_counts_via.argtypes = [vp, vp, u64, u64, u64, ctypes.c_int64, ALLGATHER_FN, vp, ctypes.c_int, ctypes.c_int, _u64p, vp]
    L.rj_scan_destroy.argtypes = [vp]
    L.rj_scan_gather_spans.restype = i64
    L.rj_scan_gather_spans.argtypes = [vp, vp, u64, u64, u64, ctypes.c_int64, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    L.rj_scan_gather_spans_via.restype = i64
    L.rj_scan_gather_spans_via.argtypes = [vp, vp, u64, u64, u64, ctypes.c_int64, ALLGATHER_FN, GATHERV_FN, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    L.rj_scan_gathered_spans.restype = vp
    L.rj_scan_gathered_spans.argtypes = [vp, _u64p]
    L.rj_scan_run.restype = i64
    L.rj_host_stats.restype = ctypes.c_int
    L.rj_host_stats.argtypes = [vp, vp, sz]
    L.rj_scan_count.restype = i64
    L.rj_scan_count.argtypes = [vp, vp, u64, vp]
    L.rj_scan_run.argtypes = [vp, vp, u64, u64, u64, u64, u64, ctypes.c_int, vp]
    L.rj_scan_start.argtypes = [vp, vp, u64, vp]
    L.rj_scan_finish.restype = i64
    L.rj_scan_finish.argtypes = [vp]
    L.rj_scan_device_spans.restype = vp
    L.rj_scan_device_spans.argtypes = [vp]
    L.rj_scan_copy_spans.restype = i64
    L.rj_scan_copy_spans.argtypes = [vp, _u64p, u64]
    L.rj_scan_stats.argtypes = [vp, ctypes.POINTER(_Stats)]
    L.rj_scan_match_full.argtypes = [vp, vp, u64, vp]
    L.rj_replace_all_begin.restype = i64
    L.rj_replace_all_begin.argtypes = [vp, cp, sz, cp, sz, ctypes.POINTER(sz)]
    L.rj_replace_all_fetch.restype = ctypes.c_int
    L.rj_replace_all_fetch.argtypes = [vp, vp, sz]
    L.rj_replace_all.restype = i64
    L.rj_replace_all.argtypes = [vp, cp, sz, cp, sz, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz)]
    L.rj_free_text.argtypes = [ctypes.c_void_p]
    L.rj_scan_replace.restype = i64
    L.rj_scan_replace.argtypes = [vp, vp, u64, cp, u64, vp, u64, vp]
    L.rj_device_count.restype = ctypes.c_int
    L.rj_batch_separator.restype = ctypes.c_int
    L.rj_batch_separator.argtypes = [vp]
    L.rj_match_all_packed.restype = i64
    L.rj_match_all_packed.argtypes = [vp, vp, _u64p, ctypes.POINTER(sz), sz, u64, _u64p, ctypes.POINTER(_u64p)]
    L.rj_host_alloc.restype = vp
    L.rj_host_alloc.argtypes = [sz]
    L.rj_host_free.argtypes = [vp]
    L.rj_scan_records.restype = i64
    L.rj_scan_records.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, ctypes.POINTER(_RecordStats), vp]
    L.rj_scan_records_select.restype = i64
    L.rj_scan_records_select.argtypes = [vp, ctypes.c_int, vp, u64, vp]
    L.rj_scan_records_pack.restype = i64
    L.rj_scan_records_pack.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, ctypes.c_int, u64, u64, vp, u64, vp, vp, vp]
    L.rj_scan_records_replace.restype = i64
    L.rj_scan_records_replace.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, cp, u64, ctypes.c_int, u64, u64, vp, u64, vp, vp, vp]
    L.rj_scan_records_split.restype = i64
    L.rj_scan_records_split.argtypes = [vp, u64, vp, vp, u64, vp, vp, vp, u64, ctypes.c_int, vp, vp, vp, u64, vp]
    L.rj_scan_records_group.restype = i64
    L.rj_scan_records_group.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, vp, vp, u64, vp]
    L.rj_scan_records_sort.restype = i64
    L.rj_scan_records_sort.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, ctypes.POINTER(_SortStats), vp]
    L.rj_scan_records_lookup.restype = i64
    L.rj_scan_records_lookup.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, u64, vp, vp, u64, vp, u64, vp, vp, ctypes.POINTER(_LookupStats), vp]
    L.rj_scan_records_parse.restype = i64
    L.rj_scan_records_parse.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, ctypes.c_int, ctypes.c_uint, vp, vp, ctypes.POINTER(_ParseStats), vp]
    L.rj_scan_records_parse_time.restype = i64
    L.rj_scan_records_parse_time.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, cp, u64, ctypes.c_int, ctypes.c_uint, vp, vp, ctypes.POINTER(_ParseStats), vp]
    L.rj_scan_records_format.restype = i64
    L.rj_scan_records_format.argtypes = [vp, vp, vp, u64, vp, u64, ctypes.c_int, ctypes.c_uint, ctypes.c_int, u64, u64, vp, u64, vp, vp, vp]
    L.rj_scan_records_zip.restype = i64
    L.rj_scan_records_zip.argtypes = [vp, ctypes.POINTER(ZipColumn), ctypes.c_int, ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_uint, ctypes.c_int, u64, u64, vp, u64, vp, vp, vp]
    L.rj_scan_records_format_time.restype = i64
    L.rj_scan_records_format_time.argtypes = [vp, vp, vp, u64, vp, u64, cp, u64, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int, u64, u64, vp, u64, vp, vp,
                                              ctypes.POINTER(_FormatTimeStats), vp]
    L.rj_scan_records_translate.restype = i64
    L.rj_scan_records_translate.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, cp, cp, ctypes.c_int, u64, u64, vp, u64, vp, vp, ctypes.POINTER(_TranslateStats), vp]
    L.rj_scan_records_csv.restype = i64
    L.rj_scan_records_csv.argtypes = [vp, vp, u64, ctypes.c_int, ctypes.c_int, vp, vp, vp, u64, vp, vp, vp, u64, ctypes.POINTER(_CsvStats), vp]
    L.rj_scan_records_format_csv.restype = i64
    L.rj_scan_records_format_csv.argtypes = [vp, ctypes.POINTER(ZipColumn), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint,
                                             ctypes.c_int, u64, u64, vp, u64, vp, vp, ctypes.POINTER(_CsvFormatStats), vp]
    _lib = L
    return L


def carry_decide(all_rows, world: int, rank: int, n_patterns: int, out, stream: int = 0) -> None:
    """rj_carry_decide on tensors: all_rows (world, P, 8) int64 on the device, out (4 P + 1) int64 (device or pinned)."""
    lib = load_library()
    _check(lib.rj_carry_decide(ctypes.c_void_p(all_rows.data_ptr()), world, rank, n_patterns, ctypes.c_void_p(out.data_ptr()),
                               ctypes.c_void_p(stream)))


BENCH_LIB = os.path.join(PKG, "librejit_bench.so")
_bench_lib = None


def stream_read_probe(d_text_ptr: int, n: int, launches: int = 10, stream: int = 0, default_policy: bool = False) -> float:
    """Average ms of a read-only kernel over device memory (the achievable ceiling of a scan): MEASUREMENT, from
    rejit_amd/librejit_bench.so (tools/probes/read_probe.hip) -- not part of the product library or its C ABI.
    The probe loads with the scans' own non-temporal policy (csrc/stream_load.h); default_policy=True: plain loads,
    what rounds 1-5 quoted as the ceiling."""
    global _bench_lib
    if _bench_lib is None:
        load_library()   # (torch's copy of the HIP runtime first)
        if not os.path.exists(BENCH_LIB):
            raise FileNotFoundError(f"{BENCH_LIB} is missing: run rejit_amd.build()")
        _bench_lib = ctypes.CDLL(BENCH_LIB)
        _bench_lib.rjb_stream_read_probe_policy.restype = ctypes.c_float
        _bench_lib.rjb_stream_read_probe_policy.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    ms = float(_bench_lib.rjb_stream_read_probe_policy(ctypes.c_void_p(d_text_ptr), n, launches, ctypes.c_void_p(stream), 1 if default_policy else 0))
    if ms < 0:
        raise RejitError(-3, "rjb_stream_read_probe failed")
    return ms


def device_count() -> int:
    return int(load_library().rj_device_count())


def _check(rc: int):
    if rc < 0:
        raise RejitError(int(rc), load_library().rj_last_error().decode("latin1"))
    return rc


class Program:
    """A compiled pattern (rj_program)."""

    def __init__(self, regexp):
        self._lib = load_library()
        if isinstance(regexp, str):
            regexp = regexp.encode("latin1")
        self.regexp = regexp
        h = ctypes.c_void_p()
        _check(self._lib.rj_compile(regexp, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.rj_program_free(h)
            self._h = None

    def info(self) -> dict:
        i = _Info()
        _check(self._lib.rj_program_info(self._h, ctypes.byref(i)))
        return _stats_dict(i)

    # host-text entry points (the four JIT function pointers of the reference)
    def match_all(self, text: bytes) -> List[Tuple[int, int]]:
        spans = _u64p()
        n = _check(self._lib.rj_match_all(self._h, text, len(text), ctypes.byref(spans)))
        out = [(int(spans[2 * i]), int(spans[2 * i + 1])) for i in range(n)]
        if n:
            self._lib.rj_free_spans(spans)
        return out

    def match_all_batch(self, texts: List[bytes]) -> List[List[Tuple[int, int]]]:
        """MatchAll over many independent texts (files) in one device pass; offsets are relative to
        each text."""
        k = len(texts)
        arr = (ctypes.c_char_p * k)(*texts)
        sizes = (ctypes.c_size_t * k)(*[len(t) for t in texts])
        counts = (ctypes.c_uint64 * k)()
        spans = _u64p()
        total = _check(self._lib.rj_match_all_batch(self._h, arr, sizes, k, counts, ctypes.byref(spans)))
        return self._take_spans(counts, k, spans, total)

    def _take_spans(self, counts, k, spans, total) -> List[List[Tuple[int, int]]]:
        """a counted span list of the library's as one list of pairs per text; the library's list is freed"""
        out, at = [], 0
        for i in range(k):
            c = int(counts[i])
            out.append([(int(spans[2 * (at + j)]), int(spans[2 * (at + j) + 1])) for j in range(c)])
            at += c
        assert at == total, (at, total)
        if total:
            self._lib.rj_free_spans(spans)
        return out

    def match_all_batch_counts(self, texts: List[bytes]) -> List[int]:
        """rj_match_all_batch as a native caller pays for it -- the spans DO cross PCIe and are handed out -- but
        without turning them into Python tuples: the per-text counts only (bench.py's jrep extra: 10^8 line starts)."""
        return [int(c) for c in self.match_all_batch_table(self.batch_table(texts))]

    def batch_table(self, texts: List[bytes]):
        """The caller's file table for rj_match_all_batch -- the arrays of pointers and sizes a native caller holds anyway
        (samples/jrep_gpu.cc builds them while it reads the tree) -- built once, so that a timed loop measures the library
        and not ctypes marshalling (2 500 texts: ~1 ms per call).  Keeps the texts alive."""
        k = len(texts)
        return {"k": k, "texts": texts, "arr": (ctypes.c_char_p * k)(*texts), "sizes": (ctypes.c_size_t * k)(*[len(t) for t in texts]),
                "counts": (ctypes.c_uint64 * k)()}

    def match_all_batch_table(self, table):
        """rj_match_all_batch over a batch_table(): the spans cross PCIe and are handed out (and freed here); returns the
        per-text counts as a numpy array (a view of the table's own count array: copy it to keep it)."""
        import numpy as np

        spans = _u64p()
        total = _check(self._lib.rj_match_all_batch(self._h, table["arr"], table["sizes"], table["k"], table["counts"], ctypes.byref(spans)))
        if total:
            self._lib.rj_free_spans(spans)
        return np.ctypeslib.as_array(table["counts"])

    def batch_separator(self) -> int:
        """The byte that ends a text inside a packed batch, or -1 (the pattern is matched text by text)."""
        return int(self._lib.rj_batch_separator(self._h))

    def match_all_packed(self, buf_ptr: int, offsets: List[int], sizes: List[int], total_bytes: int) -> List[List[Tuple[int, int]]]:
        """rj_match_all_packed over a buffer the caller laid out (a raw pointer: rj_host_alloc'ed or ordinary memory):
        per text the spans relative to the text."""
        k = len(offsets)
        off = (ctypes.c_uint64 * max(k, 1))(*offsets)
        sz_ = (ctypes.c_size_t * max(k, 1))(*sizes)
        counts = (ctypes.c_uint64 * max(k, 1))()
        spans = _u64p()
        total = _check(self._lib.rj_match_all_packed(self._h, ctypes.c_void_p(buf_ptr), off, sz_, k, total_bytes, counts, ctypes.byref(spans)))
        return self._take_spans(counts, k, spans, total)

    def count(self, text: bytes) -> int:
        """Regej::MatchAllCount: rj_match_all with a NULL span list."""
        return int(_check(self._lib.rj_match_all(self._h, text, len(text), None)))

    def host_stats(self) -> dict:
        """rj_host_stats: which kernels answered this thread's last host-text call of the pattern."""
        s = _Stats()
        _check(self._lib.rj_host_stats(self._h, ctypes.byref(s), ctypes.sizeof(s)))
        return {k: (float(getattr(s, k)) if k.endswith("_ms") else int(getattr(s, k))) for k, _ in _Stats._fields_}

    def replace_all(self, text: bytes, repl: bytes) -> Tuple[int, bytes]:
        """(number of matches, new text): MatchAll + Replace, spliced on the GPU."""
        out = ctypes.c_void_p()
        out_len = ctypes.c_size_t()
        m = _check(self._lib.rj_replace_all(self._h, text, len(text), repl, len(repl), ctypes.byref(out), ctypes.byref(out_len)))
        data = ctypes.string_at(out, out_len.value)
        self._lib.rj_free_text(out)
        return int(m), data

    def replace_all_into(self, text: bytes, repl: bytes, dst: bytearray) -> Tuple[int, int]:
        """rj_replace_all_begin + rj_replace_all_fetch: the new text into a buffer of the caller's (number of matches, new length)."""
        out_len = ctypes.c_size_t()
        m = _check(self._lib.rj_replace_all_begin(self._h, text, len(text), repl, len(repl), ctypes.byref(out_len)))
        if out_len.value > len(dst):
            raise RejitError(-4, "replace_all_into: the new text has %d bytes, the buffer %d" % (out_len.value, len(dst)))
        buf = (ctypes.c_char * len(dst)).from_buffer(dst)
        _check(self._lib.rj_replace_all_fetch(self._h, ctypes.addressof(buf), len(dst)))
        return int(m), int(out_len.value)

    def match_first(self, text: bytes) -> Optional[Tuple[int, int]]:
        b, e = ctypes.c_uint64(), ctypes.c_uint64()
        r = _check(self._lib.rj_match_first(self._h, text, len(text), ctypes.byref(b), ctypes.byref(e)))
        return (int(b.value), int(e.value)) if r else None

    def match_anywhere(self, text: bytes) -> bool:
        return bool(_check(self._lib.rj_match_anywhere(self._h, text, len(text))))

    def match_full(self, text: bytes) -> bool:
        return bool(_check(self._lib.rj_match_full(self._h, text, len(text))))


# The argument layer of Scan's record calls: the host protocol they share, each piece once.  A record method is
# its own argument checks, one `call` closure that lists the C arguments in include/rejit_hip.h's order, and its result.

def _ptr(x):
    """the pointer of a tensor as a C argument: NULL for None and for an empty tensor"""
    return ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)


def _stream(device, stream):
    """stream=None: the device's current stream"""
    import torch

    return torch.cuda.current_stream(device).cuda_stream if stream is None else stream


def _check_text(t, device=None):
    import torch

    assert t.dtype == torch.uint8 and t.is_contiguous() and t.is_cuda and (device is None or t.device == device)


def _check_column(x, dtype, device, n):
    assert x.dtype == dtype and x.is_contiguous() and x.device == device and x.numel() == n


def _check_table(rec_begin, rec_end, device) -> int:
    """-> n_records"""
    import torch

    n_records = int(rec_begin.numel())
    _check_column(rec_begin, torch.int64, device, n_records)
    _check_column(rec_end, torch.int64, device, n_records)
    return n_records


def _rows(indices, every, device):
    """A row list -> (the tensor to pass, k).  None: every row.  The caller keeps the tensor until the library has returned."""
    import torch

    if indices is None:
        return None, every
    assert indices.dtype == torch.int64 and indices.is_contiguous() and indices.device == device
    if indices.numel() == 0:
        return torch.zeros(1, dtype=torch.int64, device=device), 0   # (a non-null pointer: NULL means every record)
    return indices, int(indices.numel())


def _stats_dict(s) -> dict:
    return {f: int(getattr(s, f)) for f, _ in s._fields_}


def _sized_text(call, out, device, name, noun):
    """A new device text through call(buf, cap) -> total.  Without `out` ONE size query, exactly `total` bytes allocated and
    filled (no second call for an empty text); with `out` one call into it, RejitError when it is too small, else out[:total]."""
    import torch

    if out is None:
        total = call(None, 0)
        out = torch.empty(total, dtype=torch.uint8, device=device)
        if total:
            call(out, total)
        return out
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.device == device
    cap = int(out.numel())
    total = call(out if cap else None, cap)
    if total > cap:
        raise RejitError(-4, "%s: %s has %d bytes, `out` %d" % (name, noun, total, cap))
    return out[:total]


def _fill_byte(fill, program, name) -> int:
    """fill=None: the pattern's batch separator"""
    if fill is not None:
        return int(fill)
    fill = program.batch_separator()
    if fill < 0:
        raise RejitError(-4, "%s: the pattern has no batch separator (it is matched text by text): pass fill" % name)
    return fill


def _one_byte(x, name, what) -> int:
    """an int, or bytes of length one"""
    if isinstance(x, int):
        return int(x)
    if len(bytes(x)) != 1:
        raise ValueError("%s: %s is not one byte" % (name, what))
    return bytes(x)[0]


def _zip_columns(columns, widths, name):
    """The rj_zip_column array of (text, rec_begin, rec_end[, indices]) columns -> (array, k, the tensors it points into).  An
    absent row list is pointer 0 and n_indices 0, an empty one _rows' dummy and 0."""
    if not columns:
        raise RejitError(-4, "%s: no columns (a call takes 1 to 16)" % name)
    device = columns[0][0].device
    cols = (ZipColumn * len(columns))()
    keep = []
    for c, column in enumerate(columns):
        if len(column) not in (3, 4):
            raise ValueError("%s: a column is (text, rec_begin, rec_end) or (text, rec_begin, rec_end, indices)" % name)
        t, rec_begin, rec_end = column[:3]
        _check_text(t, device)
        n_records = _check_table(rec_begin, rec_end, device)
        indices, rows = _rows(column[3] if len(column) == 4 else None, n_records, device)
        keep.append((t, rec_begin, rec_end, indices))
        cols[c] = ZipColumn(_ptr(t).value, int(t.numel()), _ptr(rec_begin).value, _ptr(rec_end).value, n_records, _ptr(indices).value,
                            0 if indices is None else rows, widths[c], 0)
        if c == 0:
            k = rows
    return cols, k, keep


def _parse_rows(call, t, rec_begin, rec_end, indices, dtype, stats, stream):
    """parse_records and parse_time_records behind their own checks: call(n_records, indices, k, values, status, stats, stream) is
    the library call"""
    import torch

    n_records = _check_table(rec_begin, rec_end, t.device)
    indices, k = _rows(indices, n_records, t.device)
    values = torch.empty(k, dtype=dtype, device=t.device)
    status = torch.empty(k, dtype=torch.uint8, device=t.device)
    out = _ParseStats()
    _check(call(n_records, indices, k, values, status, ctypes.byref(out) if stats else None, ctypes.c_void_p(_stream(t.device, stream))))
    return (values, status, _stats_dict(out)) if stats else (values, status)


class Scan:
    """Device-resident scanning (rj_scan): text stays in HBM, results stay in HBM."""

    def set_timing(self, on: bool = True) -> None:
        """rj_scan_set_timing: without the scan kernel's start event stats()["scan_ms"] reads 0 and a call is 6-9 us shorter."""
        _check(self._lib.rj_scan_set_timing(self._h, int(on)))

    def __init__(self, program: Program):
        self._lib = load_library()
        self.program = program
        h = ctypes.c_void_p()
        _check(self._lib.rj_scan_create(program._h, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.rj_scan_destroy(h)
            self._h = None

    def run(self, d_text_ptr: int, n: int, own_begin: int = 0, own_end: Optional[int] = None, carry_cur: int = 0,
            carry_prev_end: int = 0, have_prev: bool = False, stream: int = 0) -> int:
        if own_end is None:
            own_end = n + 1
        return int(_check(self._lib.rj_scan_run(self._h, ctypes.c_void_p(d_text_ptr), n, own_begin, own_end, carry_cur,
                                                carry_prev_end, int(have_prev), ctypes.c_void_p(stream))))

    def count(self, d_text_ptr: int, n: int, stream: int = 0) -> int:
        """rj_scan_count: MatchAllCount over device text (the one-kernel count when the pattern has the shape:
        stats()["count_path"] == 1, no span list)."""
        return int(_check(self._lib.rj_scan_count(self._h, ctypes.c_void_p(d_text_ptr), n, ctypes.c_void_p(stream))))

    def count_tensor(self, t, n: Optional[int] = None, stream=None) -> int:
        _check_text(t)
        return self.count(t.data_ptr(), int(t.numel() if n is None else n), stream=_stream(t.device, stream))

    def gather_spans(self, d_text_ptr: int, n: int, offset: int, rank: int, world: int, root: int = 0, comm: Optional[int] = None,
                     allgather=None, gatherv=None, own_begin: int = 0, own_end: Optional[int] = None, stream: int = 0):
        """rj_scan_gather_spans: this rank's shard, the carry over the cuts, every rank's pairs (global offsets) gathered on
        `root` in text order.  Returns (job-wide count, the list on root / None elsewhere)."""
        args = (self._h, ctypes.c_void_p(d_text_ptr), n, own_begin, n + 1 if own_end is None else own_end, ctypes.c_int64(offset))
        if allgather is not None:
            total = _check(self._lib.rj_scan_gather_spans_via(*args, allgather, gatherv, None, rank, world, root, ctypes.c_void_p(stream)))
        else:
            total = _check(self._lib.rj_scan_gather_spans(*args, ctypes.c_void_p(comm), rank, world, root, ctypes.c_void_p(stream)))
        cnt = ctypes.c_uint64()
        ptr = self._lib.rj_scan_gathered_spans(self._h, ctypes.byref(cnt))
        if not ptr:
            return int(total), None
        k = int(cnt.value)
        buf = (ctypes.c_uint64 * max(2 * k, 1))()
        got = _check(self._lib.rj_scan_copy_gathered_spans(self._h, buf, k))   # (through the library: no HIP binding of our own)
        if got != k:
            raise RejitError(-3, "rj_scan_copy_gathered_spans returned %d pairs, %d were gathered" % (got, k))
        v = list(buf)
        return int(total), [(v[2 * i], v[2 * i + 1]) for i in range(int(cnt.value))]

    def start(self, d_text_ptr: int, n: int, stream: int = 0) -> None:
        """Enqueue a whole-text run; finish() returns its count (several scans can be in flight)."""
        _check(self._lib.rj_scan_start(self._h, ctypes.c_void_p(d_text_ptr), n, ctypes.c_void_p(stream)))

    def finish(self) -> int:
        return int(_check(self._lib.rj_scan_finish(self._h)))

    def run_tensor(self, t, n: Optional[int] = None, stream=None, **kw) -> int:
        """t: a contiguous uint8 torch tensor on the GPU."""
        _check_text(t)
        return self.run(t.data_ptr(), int(t.numel() if n is None else n), stream=_stream(t.device, stream), **kw)

    def run_records(self, text_tensor, rec_begin, rec_end, counts=None, first=None, stream=None) -> RecordsResult:
        """rj_scan_records: one whole-text run over `text_tensor` (contiguous uint8 on the GPU), its matches handed to the
        records text[rec_begin[i], rec_end[i]) -- int64 tensors on the same device, ascending, not overlapping (gaps allowed).
        counts (int32) / first (int64): tensors of the caller's to write into, else new ones.  spans() / spans_tensor() /
        stats() afterwards are those of the whole-text run."""
        import torch

        t = text_tensor
        _check_text(t)
        k = _check_table(rec_begin, rec_end, t.device)
        if counts is None:
            counts = torch.empty(k, dtype=torch.int32, device=t.device)
        if first is None:
            first = torch.empty(k, dtype=torch.int64, device=t.device)
        _check_column(counts, torch.int32, t.device, k)
        _check_column(first, torch.int64, t.device, k)
        st = _stream(t.device, stream)
        rs = _RecordStats()
        _check(self._lib.rj_scan_records(self._h, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), k, _ptr(counts), _ptr(first), ctypes.byref(rs),
                                         ctypes.c_void_p(st)))
        self._records = (t.device, k, counts, st)   # (the selection reads these counts: kept alive)
        return RecordsResult(rs, counts, first, k)

    def select_records(self, invert: bool = False, cap: Optional[int] = None, stream=None):
        """rj_scan_records_select: the ascending indices (int64 tensor on the text's device) of the records of the last
        run_records with a match -- invert: without one.  cap: write at most that many (the tensor is then cap long at most);
        self.n_selected holds the full number."""
        import torch

        rec = getattr(self, "_records", None)
        if rec is None:
            # (no run_records yet: the library refuses, with its own message)
            _check(self._lib.rj_scan_records_select(self._h, int(invert), None, 0, None))
            raise RejitError(-4, "select_records without run_records")
        device, k, _counts, st0 = rec
        room = k if cap is None else min(int(cap), k)
        out = torch.empty(max(room, 1), dtype=torch.int64, device=device)
        st = st0 if stream is None else stream
        total = int(_check(self._lib.rj_scan_records_select(self._h, int(invert), _ptr(out), room, ctypes.c_void_p(st))))
        self.n_selected = total
        return out[:min(total, room)]

    def pack_records(self, text_tensor, rec_begin, rec_end, indices=None, fill=None, lead: int = 0, gap: int = 1, out=None, stream=None):
        """rj_scan_records_pack: the records text[rec_begin[i], rec_end[i]) -- all of them, or those `indices` (an int64 device
        tensor: any order, repeats allowed; select_records' result is the common case) names -- gathered into a new contiguous
        device text, `gap` bytes of `fill` behind each and `lead` in front.  Returns (out_text, out_begin, out_end): a uint8
        tensor of exactly `total` bytes and the new int64 record table.  fill=None: program.batch_separator(), the byte that
        makes the packed records independent (RejitError when the pattern has none).  Without `out` the call makes ONE size
        query (the plan alone) and allocates exactly `total` bytes; with `out` (contiguous uint8, 16-byte aligned) it packs
        into it in one call and raises RejitError when it is too small.  The scan's spans, stats and select_records stay as
        they were."""
        import torch

        t = text_tensor
        _check_text(t)
        n_records = _check_table(rec_begin, rec_end, t.device)
        fill = _fill_byte(fill, self.program, "pack_records")
        indices, k = _rows(indices, n_records, t.device)
        st = _stream(t.device, stream)
        out_begin = torch.empty(k, dtype=torch.int64, device=t.device)
        out_end = torch.empty(k, dtype=torch.int64, device=t.device)

        def call(buf, cap):
            return int(_check(self._lib.rj_scan_records_pack(self._h, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), n_records, _ptr(indices), k,
                                                             fill, int(lead), int(gap), _ptr(buf), cap, _ptr(out_begin), _ptr(out_end), ctypes.c_void_p(st))))
        return _sized_text(call, out, t.device, "pack_records", "the packed text"), out_begin, out_end

    def translate_records(self, text_tensor, rec_begin, rec_end, table=None, delete: bytes = b"", indices=None, fill=None, lead: int = 0, gap: int = 1,
                          out=None, stream=None, stats=False):
        """rj_scan_records_translate: pack_records in which every packed record goes through Python's
        bytes.translate(table, delete) on the device -- `tr A-Z a-z`, `tr -d '\\r'`, str.lower / str.upper / str.translate
        over a column.  `table`: 256 bytes (records.ASCII_LOWER, records.ASCII_UPPER, records.byte_map), None is the identity;
        `delete`: the bytes to remove, as bytes or as records.drop_set's 32-byte set -- judged on the source byte, before the
        table.  indices, fill (None: the batch separator), lead, gap, out and the returned (out_text, out_begin, out_end) are
        pack_records': without `out` ONE size query and an exact allocation, with `out` (contiguous uint8, 16-byte aligned)
        one call and RejitError when it is too small.  stats=True adds {"bytes_in", "bytes_dropped", "bytes_changed"}.  In
        front of group_records / sort_records / lookup_records it makes them `uniq -ci`, `sort -f` and a case-insensitive
        join.  The scan's spans, stats and select_records stay as they were."""
        import torch
        from . import records as _records

        t = text_tensor
        _check_text(t)
        n_records = _check_table(rec_begin, rec_end, t.device)
        if table is not None:
            table = bytes(table)
            if len(table) != 256:
                raise ValueError("translate_records: table has %d bytes, not 256" % len(table))
        drop = None
        if isinstance(delete, _records.DropSet):
            drop = bytes(delete)
        elif delete:
            drop = bytes(_records.drop_set(delete))
        fill = _fill_byte(fill, self.program, "translate_records")
        indices, k = _rows(indices, n_records, t.device)
        st = _stream(t.device, stream)
        out_begin = torch.empty(k, dtype=torch.int64, device=t.device)
        out_end = torch.empty(k, dtype=torch.int64, device=t.device)
        counts = _TranslateStats()

        def call(buf, cap):
            return int(_check(self._lib.rj_scan_records_translate(self._h, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), n_records, _ptr(indices), k,
                                                                  table, drop, fill, int(lead), int(gap), _ptr(buf), cap, _ptr(out_begin), _ptr(out_end),
                                                                  ctypes.byref(counts) if stats else None, ctypes.c_void_p(st))))
        text = _sized_text(call, out, t.device, "translate_records", "the translated text")
        return (text, out_begin, out_end, _stats_dict(counts)) if stats else (text, out_begin, out_end)

    def csv_records(self, text_tensor, delimiter: bytes = b",", quote=b'"', rows: bool = True, stream=None, row_cap: Optional[int] = None,
                    field_cap: Optional[int] = None) -> CsvResult:
        """rj_scan_records_csv: the rows and fields of the CSV text `text_tensor` (contiguous uint8 on the GPU) with quoted fields
        -- delimiters and line breaks inside quotes are data, `""` inside a quoted field is flagged CSV_ESCAPED (records.csv_values
        unescapes), malformed quoting is flagged per field, never guessed.  delimiter / quote: one byte each (or an int); quote=None:
        no quoting.  One size query, then the fill into exact allocations; with row_cap and field_cap both given the fill alone,
        and RejitError when either was too small.  rows=False leaves row_begin / row_end out.  Returns a CsvResult; every
        (begin, end) pair of it is a record table for the other record calls.  The scan's spans, stats and select_records stay
        as they were."""
        import torch

        t = text_tensor
        _check_text(t)
        d = _one_byte(delimiter, "csv_records", "delimiter")
        q = -1 if quote is None else _one_byte(quote, "csv_records", "quote")
        st = _stream(t.device, stream)
        cs = _CsvStats()

        def call(tables, rcap, fcap):
            rf, rb, re, fb, fe, ff = tables
            return int(_check(self._lib.rj_scan_records_csv(self._h, _ptr(t), int(t.numel()), d, q, _ptr(rf), _ptr(rb), _ptr(re), rcap, _ptr(fb), _ptr(fe),
                                                            _ptr(ff), fcap, ctypes.byref(cs), ctypes.c_void_p(st))))
        if row_cap is None or field_cap is None:
            call((None,) * 6, 0, 0)
            row_cap, field_cap = int(cs.n_rows), int(cs.n_fields)
        row_cap, field_cap = int(row_cap), int(field_cap)
        i64 = lambda k: torch.empty(k, dtype=torch.int64, device=t.device)
        tables = (i64(row_cap + 1), i64(row_cap) if rows else None, i64(row_cap) if rows else None, i64(field_cap), i64(field_cap),
                  torch.empty(field_cap, dtype=torch.int32, device=t.device))
        call(tables, row_cap, field_cap)
        n_rows, n_fields = int(cs.n_rows), int(cs.n_fields)
        if n_rows > row_cap or n_fields > field_cap:
            raise RejitError(-4, "csv_records: the text has %d rows and %d fields, the caps were %d and %d" % (n_rows, n_fields, row_cap, field_cap))
        stats = _stats_dict(cs)
        if stats["first_bad"] == (1 << 64) - 1:
            stats["first_bad"] = None
        rf, rb, re, fb, fe, ff = tables
        return CsvResult(rf[:n_rows + 1], rb[:n_rows] if rows else None, re[:n_rows] if rows else None, fb[:n_fields], fe[:n_fields], ff[:n_fields], stats)

    def replace_records(self, text_tensor, rec_begin, rec_end, result: RecordsResult, repl: bytes, indices=None, fill=None, lead: int = 0,
                        gap: int = 1, out=None, stream=None):
        """rj_scan_records_replace: pack_records in which every packed record has its own matches replaced by `repl` (bytes) --
        `sed 's/RE/repl/g'` over lines, str.replace over a column.  `result` is the RecordsResult of the run_records that
        produced the scan's current list (its counts and first are passed down); indices, fill, lead, gap, out and the
        returned (out_text, out_begin, out_end) are pack_records'.  Without `out` the call makes ONE size query (table and plan
        only) and allocates exactly `total` bytes.  RejitError (RJ_BAD_ARGUMENT, naming the first bad row) when a packed record
        has a match that ends beyond it (the records are not independent: pack_records with the separator first), when
        `result` is not of the scan's last run, or when that run was counts-only."""
        import torch

        t = text_tensor
        _check_text(t)
        n_records = _check_table(rec_begin, rec_end, t.device)
        _check_column(result.first, torch.int64, t.device, n_records)
        _check_column(result.counts, torch.int32, t.device, n_records)
        repl = bytes(repl)
        fill = _fill_byte(fill, self.program, "replace_records")
        indices, k = _rows(indices, n_records, t.device)
        st = _stream(t.device, stream)
        out_begin = torch.empty(k, dtype=torch.int64, device=t.device)
        out_end = torch.empty(k, dtype=torch.int64, device=t.device)

        def call(buf, cap):
            return int(_check(self._lib.rj_scan_records_replace(self._h, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), n_records,
                                                                _ptr(result.counts), _ptr(result.first), _ptr(indices), k, repl, len(repl), fill, int(lead),
                                                                int(gap), _ptr(buf), cap, _ptr(out_begin), _ptr(out_end), ctypes.c_void_p(st))))
        return _sized_text(call, out, t.device, "replace_records", "the new text"), out_begin, out_end

    def split_records(self, rec_begin, rec_end, result: RecordsResult, n: int, indices=None, what: str = "between", stream=None):
        """rj_scan_records_split: the fields (what="between": the pieces between a record's own matches -- `awk -F RE`,
        str.split) or the matches themselves (what="matches": `grep -o`, str.findall) of the records [rec_begin[i],
        rec_end[i]) of a text of n bytes -- all of them, or those `indices` names, as pack_records' -- as a piece table over
        the same text.  `result` is the RecordsResult of the run_records that produced the scan's current list.  Returns
        (piece_begin, piece_end, piece_first): int64 device tensors; row j's pieces are rows piece_first[j] ..
        piece_first[j + 1] of the first two (offsets into the text), piece_first has k + 1 entries.  ONE size query (the plan
        alone), exactly P rows allocated, one call.  Without indices (piece_begin, piece_end) is a valid record table for
        run_records and pack_records.  RejitError (RJ_BAD_ARGUMENT, naming the first bad row) as replace_records."""
        import torch

        device = rec_begin.device
        n_records = _check_table(rec_begin, rec_end, device)
        _check_column(result.first, torch.int64, device, n_records)
        _check_column(result.counts, torch.int32, device, n_records)
        if what not in ("between", "matches"):
            raise ValueError("split_records: what is 'between' or 'matches', not %r" % (what,))
        code = 0 if what == "between" else 1
        indices, k = _rows(indices, n_records, device)
        st = _stream(device, stream)
        piece_first = torch.empty(k + 1, dtype=torch.int64, device=device)

        def call(pb, pe, cap):
            return int(_check(self._lib.rj_scan_records_split(self._h, int(n), _ptr(rec_begin), _ptr(rec_end), n_records, _ptr(result.counts),
                                                              _ptr(result.first), _ptr(indices), k, code, _ptr(piece_first), _ptr(pb), _ptr(pe), cap,
                                                              ctypes.c_void_p(st))))
        total = call(None, None, 0)
        piece_begin = torch.empty(total, dtype=torch.int64, device=device)
        piece_end = torch.empty(total, dtype=torch.int64, device=device)
        if total:
            call(piece_begin, piece_end, total)
        return piece_begin, piece_end, piece_first

    def group_records(self, text_tensor, rec_begin, rec_end, indices=None, stream=None):
        """rj_scan_records_group: the rows text[rec_begin[i], rec_end[i]) -- all of them, or those `indices` names, as
        pack_records' -- grouped by their bytes, exactly: Arrow's dictionary_encode / value_counts, `sort | uniq -c` in order of
        first appearance.  Returns (group, rep, count), int64 device tensors: group[j] is the group of row j (k entries), rep[g]
        the smallest row with group g's string (strictly ascending) and count[g] the number of its rows (G entries each).  The
        dictionary is pack_records over the rows rep (indices[rep] when there are indices); records.top_groups picks the most
        frequent.  ONE size query (which writes `group` already), exactly G rows allocated.  RejitError (RJ_BAD_ARGUMENT,
        naming the first bad row) for a bad index or row.  The scan's spans, stats and select_records stay as they were."""
        import torch

        t = text_tensor
        _check_text(t)
        n_records = _check_table(rec_begin, rec_end, t.device)
        indices, k = _rows(indices, n_records, t.device)
        st = _stream(t.device, stream)
        group = torch.empty(k, dtype=torch.int64, device=t.device)

        def call(g, rep, count, cap):
            return int(_check(self._lib.rj_scan_records_group(self._h, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), n_records, _ptr(indices), k,
                                                              _ptr(g), _ptr(rep), _ptr(count), cap, ctypes.c_void_p(st))))
        total = call(group, None, None, 0)
        rep = torch.empty(total, dtype=torch.int64, device=t.device)
        count = torch.empty(total, dtype=torch.int64, device=t.device)
        if total:
            call(None, rep, count, total)
        return group, rep, count

    def sort_records(self, text_tensor, rec_begin, rec_end, indices=None, stream=None, stats=False):
        """rj_scan_records_sort: the rows text[rec_begin[i], rec_end[i]) -- all of them, or those `indices` names, as
        pack_records' -- in the order of their bytes: unsigned bytes as memcmp and `LC_ALL=C sort` compare them, a proper
        prefix first, equal rows in ascending row number (stable).  Returns `order`, an int64 device tensor of k entries: THE
        permutation with row(order[i]) <= row(order[i + 1]); pack_records(..., indices=order) (indices[order] when there are
        indices) prints the sorted table, torch.flip(order, [0]) is the descending order.  With stats=True returns (order,
        {"rounds", "keyed_rows", "skip_rows", "long_rows"}).  records.sorted_groups sorts the distinct rows and their counts.
        RejitError (RJ_BAD_ARGUMENT, naming the first bad row) for a bad index or row.  The scan's spans, stats and
        select_records stay as they were."""
        import torch

        t = text_tensor
        _check_text(t)
        n_records = _check_table(rec_begin, rec_end, t.device)
        indices, k = _rows(indices, n_records, t.device)
        order = torch.empty(k, dtype=torch.int64, device=t.device)
        out = _SortStats()
        _check(self._lib.rj_scan_records_sort(self._h, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), n_records, _ptr(indices), k, _ptr(order),
                                              ctypes.byref(out), ctypes.c_void_p(_stream(t.device, stream))))
        return (order, _stats_dict(out)) if stats else order

    def lookup_records(self, set_text, set_begin, set_end, text, rec_begin, rec_end, set_indices=None, indices=None, hits=False, stats=False, stream=None):
        """rj_scan_records_lookup: the probe rows text[rec_begin[i], rec_end[i]) looked up in the set rows set_text[set_begin[i],
        set_end[i]) -- on either side all rows, or those the side's index list names, as pack_records' -- by their bytes,
        exactly: Arrow's index_in / is_in, `grep -F -x -f`, a semi-join.  The two texts may be one tensor, overlap or be
        unrelated; they are on the same device.  Returns `index`, an int64 device tensor of kp entries: the smallest set row
        equal to probe row j, or -1 (RJ_LOOKUP_NONE); index >= 0 is is_in.  With hits=True also `hits` (int64, ks entries):
        at the smallest set row of a string the number of probe rows that found it, 0 at a later duplicate -- 0 at a first
        occurrence is the anti-join's right side.  With stats=True also {"n_found", "n_set_distinct", "n_set_hit",
        "long_rows"}.  With set_indices = the `rep` of group_records over the set table, index holds the probe rows' group
        numbers (records.join_rows makes the inner join of them).  RejitError (RJ_BAD_ARGUMENT, naming the table and the first
        bad row: "set row <i> " / "row <j> ") for a bad index or row.  The scan's spans, stats and select_records stay as
        they were."""
        import torch

        t = text
        _check_text(t)
        _check_text(set_text, t.device)
        n_set_records = _check_table(set_begin, set_end, t.device)
        n_records = _check_table(rec_begin, rec_end, t.device)
        set_indices, ks = _rows(set_indices, n_set_records, t.device)
        indices, kp = _rows(indices, n_records, t.device)
        index = torch.empty(kp, dtype=torch.int64, device=t.device)
        set_hits = torch.empty(ks, dtype=torch.int64, device=t.device) if hits else None
        out = _LookupStats()
        _check(self._lib.rj_scan_records_lookup(self._h, _ptr(set_text), int(set_text.numel()), _ptr(set_begin), _ptr(set_end), n_set_records, _ptr(set_indices),
                                                ks, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), n_records, _ptr(indices), kp, _ptr(index),
                                                _ptr(set_hits), ctypes.byref(out) if stats else None, ctypes.c_void_p(_stream(t.device, stream))))
        answer = (index,)
        if hits:
            answer += (set_hits,)
        if stats:
            answer += (_stats_dict(out),)
        return answer if len(answer) > 1 else index

    def parse_records(self, text_tensor, rec_begin, rec_end, indices=None, kind="int64", trim=False, stats=False, stream=None, wide=False):
        """rj_scan_records_parse: the rows text[rec_begin[i], rec_end[i]) -- all of them, or those `indices` names, as
        pack_records' -- read as numbers, exactly or not at all: Arrow's cast(utf8 -> int64 / uint64 / float64), the value
        behind `awk '{s[$1] += $3}'` and `sort -n`.  kind is "int64", "uint64" or "float64"; trim=True drops the spaces and tabs
        before and behind the number first.  Returns (values, status), device tensors of k entries: status (uint8) is
        PARSE_OK, PARSE_EMPTY, PARSE_MALFORMED, PARSE_RANGE (the integer kinds) or PARSE_INEXACT ("float64": the value is
        outside the window m <= 2^53, |q| <= 22 in which one IEEE operation gives float()'s bits); values holds what Python's
        int() / float() make of an OK row, bit for bit, and 0 for every other row.  values is an int64 tensor for "int64", a
        float64 tensor for "float64", and for "uint64" an int64 tensor that holds the value's 64 BITS (torch has no arithmetic
        on uint64): a value >= 2^63 reads as value - 2^64.  With stats=True also {"n_ok", "n_empty", "n_malformed", "n_range",
        "n_inexact"}.  (status == PARSE_OK) is the `ok` of records.group_sums.  RejitError (RJ_BAD_ARGUMENT, naming the first
        bad row) for a bad index or row.  The scan's spans, stats and select_records stay as they were.
        wide=True (RJ_PARSE_WIDE; without effect for the integer kinds) widens "float64" beyond that window: every row whose
        significant digits fit 64 bits -- repr() of a double, %.17g, 1e23, 0.30000000000000004 -- is OK with float()'s bits, or
        PARSE_RANGE when float() would give inf (so PARSE_RANGE can occur for "float64" under wide); a longer mantissa is OK when
        the two 64-bit decimals that bracket it round to one double, and PARSE_INEXACT only when they do not."""
        import torch

        t = text_tensor
        _check_text(t)
        if kind not in PARSE_KINDS:
            raise ValueError("parse_records: kind is 'int64', 'uint64' or 'float64', not %r" % (kind,))
        flags = (PARSE_TRIM if trim else 0) | (PARSE_WIDE if wide else 0)

        def call(n_records, rows, k, values, status, out, st):
            return self._lib.rj_scan_records_parse(self._h, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), n_records, _ptr(rows), k, PARSE_KINDS[kind],
                                                   flags, _ptr(values), _ptr(status), out, st)
        return _parse_rows(call, t, rec_begin, rec_end, indices, torch.float64 if kind == "float64" else torch.int64, stats, stream)

    def parse_time_records(self, text_tensor, rec_begin, rec_end, fmt, indices=None, unit="s", trim=False, stats=False, stream=None):
        """rj_scan_records_parse_time: the rows text[rec_begin[i], rec_end[i]) -- all of them, or those `indices` names, as
        parse_records' -- read as timestamps under the strptime-style format `fmt` (bytes or str, 1..64 bytes): Arrow's
        strptime / cast(utf8 -> timestamp[unit]).  The directives are %Y %m %b %d %H %M %S %f %z %%, every field of exactly
        its digits (%f: 1 to 9, greedy; %b: jan..dec in any case; %z: Z or [+-]hh[:]mm), every other byte of the format a
        literal; without %z the fields are UTC.  unit is "s", "ms", "us" or "ns"; trim=True drops the spaces and tabs before
        and behind the row first.  Returns (values, status), device tensors of k entries: values (int64) holds the count of
        units since 1970-01-01T00:00:00Z of an OK row -- what datetime.strptime makes of it, as (dt - epoch) // unit -- and 0
        for every other row; status (uint8) is PARSE_OK, PARSE_EMPTY, PARSE_MALFORMED, PARSE_RANGE (a field outside its range,
        the day against its month and year; under "ns" an instant outside int64) or PARSE_INEXACT (a non-zero fraction digit
        below the unit: never truncated or rounded).  With stats=True also {"n_ok", "n_empty", "n_malformed", "n_range",
        "n_inexact"}.  records.time_buckets floors the values to buckets.  RejitError (RJ_BAD_ARGUMENT) for a bad index or row
        (naming the first bad row) and for a refused format (naming the byte offset).  The scan's spans, stats and
        select_records stay as they were.  format_time_records is the inverse; %y %j %e %a %p, named zones, locales and leap
        seconds stay out."""
        import torch

        t = text_tensor
        _check_text(t)
        if unit not in TIME_UNITS:
            raise ValueError("parse_time_records: unit is 's', 'ms', 'us' or 'ns', not %r" % (unit,))
        fmt = fmt.encode("utf-8") if isinstance(fmt, str) else bytes(fmt)

        def call(n_records, rows, k, values, status, out, st):
            return self._lib.rj_scan_records_parse_time(self._h, _ptr(t), int(t.numel()), _ptr(rec_begin), _ptr(rec_end), n_records, _ptr(rows), k, fmt, len(fmt),
                                                        TIME_UNITS[unit], PARSE_TRIM if trim else 0, _ptr(values), _ptr(status), out, st)
        return _parse_rows(call, t, rec_begin, rec_end, indices, torch.int64, stats, stream)

    def format_records(self, values, kind=None, status=None, indices=None, fill: int = 10, lead: int = 0, gap: int = 1, out=None, stream=None, flags: int = 0):
        """rj_scan_records_format: the inverse of parse_records -- a column of numbers written as decimal text on the device,
        laid out as pack_records lays records out.  `values` is an int64 or float64 device tensor; kind is "int64", "uint64" or
        "float64" and defaults from the dtype ("uint64" takes the int64 tensor of bits parse_records returns).  Row j is
        Python's str(int) / repr(float) of values[indices[j]] (or values[j]), byte for byte -- the shortest digits that read
        back as the same double, `inf`, `-inf`, `nan` for the non-finite ones --, or the EMPTY row where `status` (uint8,
        parse_records' status column) is given and not PARSE_OK.  Returns (out_text, out_begin, out_end) as pack_records does:
        `gap` bytes of `fill` (default: a newline) behind every row, `lead` in front; without `out` one size query and an
        exact allocation, with `out` (contiguous uint8, 16-byte aligned) one call and RejitError when it is too small.
        parse_records(out_text, out_begin, out_end, kind=kind, wide=True) gives every finite value's bits back.  `flags` must
        be 0 (no style is defined yet).  The scan's spans, stats and select_records stay as they were."""
        import torch

        v = values
        assert v.is_contiguous() and v.is_cuda and v.dim() == 1
        if kind is None:
            kind = {torch.int64: "int64", torch.float64: "float64"}.get(v.dtype)
        if kind not in PARSE_KINDS:
            raise ValueError("format_records: kind is 'int64', 'uint64' or 'float64', not %r" % (kind,))
        assert v.dtype == (torch.float64 if kind == "float64" else torch.int64)
        n_values = int(v.numel())
        if status is not None:
            _check_column(status, torch.uint8, v.device, n_values)
        indices, k = _rows(indices, n_values, v.device)
        st = _stream(v.device, stream)
        out_begin = torch.empty(k, dtype=torch.int64, device=v.device)
        out_end = torch.empty(k, dtype=torch.int64, device=v.device)

        def call(buf, cap):
            return int(_check(self._lib.rj_scan_records_format(self._h, _ptr(v), _ptr(status), n_values, _ptr(indices), k, PARSE_KINDS[kind], int(flags),
                                                               int(fill), int(lead), int(gap), _ptr(buf), cap, _ptr(out_begin), _ptr(out_end),
                                                               ctypes.c_void_p(st))))
        return _sized_text(call, out, v.device, "format_records", "the text"), out_begin, out_end

    def format_time_records(self, values, fmt, unit="s", status=None, indices=None, zone_minutes: int = 0, fill: int = 10, lead: int = 0, gap: int = 1, out=None,
                            stream=None, stats=False):
        """rj_scan_records_format_time: the inverse of parse_time_records -- a column of int64 instants (counts of `unit`, "s",
        "ms", "us" or "ns", since 1970-01-01T00:00:00Z) written as text on the device under the strftime-style format `fmt`
        (bytes or str, 1..64 bytes), laid out as format_records lays its rows out.  The directives are parse_time_records'
        own, every one of a fixed width: %Y (4 digits), %m %d %H %M %S (2 each), %b (Jan..Dec), %f (the unit's fraction
        digits: 3, 6 or 9; six zeros under "s"), %z (+hhmm of zone_minutes), %%; every other byte is a literal.  The instant
        is floored toward minus infinity and shifted by `zone_minutes` (-1439..1439, one offset for the whole column).  Row j
        is what Python's strftime writes for values[indices[j]] (or values[j]) -- %Y as isoformat's four digits --, or the
        EMPTY row where `status` (uint8) is given and not PARSE_OK, or where the shifted year is outside 0001..9999.  Returns
        (out_text, out_begin, out_end) as format_records does -- `gap` bytes of `fill` behind every row, `lead` in front;
        without `out` one size query and an exact allocation, with `out` (contiguous uint8, 16-byte aligned) one call and
        RejitError when it is too small --, with stats=True also {"n_ok", "n_null", "n_range"}.  RejitError (RJ_BAD_ARGUMENT)
        for a bad index (naming the first bad row) and for a refused format (naming the byte offset).  The scan's spans,
        stats and select_records stay as they were."""
        import torch

        v = values
        assert v.is_contiguous() and v.is_cuda and v.dim() == 1 and v.dtype == torch.int64
        if unit not in TIME_UNITS:
            raise ValueError("format_time_records: unit is 's', 'ms', 'us' or 'ns', not %r" % (unit,))
        fmt = fmt.encode("utf-8") if isinstance(fmt, str) else bytes(fmt)
        n_values = int(v.numel())
        if status is not None:
            _check_column(status, torch.uint8, v.device, n_values)
        indices, k = _rows(indices, n_values, v.device)
        st = _stream(v.device, stream)
        out_begin = torch.empty(k, dtype=torch.int64, device=v.device)
        out_end = torch.empty(k, dtype=torch.int64, device=v.device)
        counts = _FormatTimeStats()

        def call(buf, cap):
            return int(_check(self._lib.rj_scan_records_format_time(self._h, _ptr(v), _ptr(status), n_values, _ptr(indices), k, fmt, len(fmt), TIME_UNITS[unit],
                                                                    int(zone_minutes), 0, int(fill), int(lead), int(gap), _ptr(buf), cap, _ptr(out_begin),
                                                                    _ptr(out_end), ctypes.byref(counts), ctypes.c_void_p(st))))
        text = _sized_text(call, out, v.device, "format_time_records", "the text")
        return (text, out_begin, out_end, _stats_dict(counts)) if stats else (text, out_begin, out_end)

    def zip_records(self, columns, sep: bytes = b"", widths=None, pad: int = 32, fill: int = 10, lead: int = 0, gap: int = 1, out=None, stream=None,
                    flags: int = 0):
        """rj_scan_records_zip: the inverse of split_records -- the rows of several columns put side by side into lines on the
        device.  `columns` is a list (1 to 16) of (text, rec_begin, rec_end) or (text, rec_begin, rec_end, indices): each a
        record table over a uint8 device text of its own (several may share one), rows as pack_records takes them; every
        column has the same number of rows.  Line j is the columns' rows j joined with `sep` (bytes, at most 64), column c
        padded with the byte `pad` to |widths[c]| bytes first: on the left for a positive width ("%7d"), on the right for a
        negative one ("%-7s"); 0, the default, adds nothing, and nothing is truncated.  Returns (out_text, out_begin, out_end)
        as pack_records does: `gap` bytes of `fill` (default: a newline) behind every line, `lead` in front; without `out` one
        size query and an exact allocation, with `out` (contiguous uint8, 16-byte aligned) one call and RejitError when it is
        too small.  The scan's spans, stats and select_records stay as they were."""
        import torch

        columns = [tuple(c) for c in columns]
        widths = [0] * len(columns) if widths is None else [int(w) for w in widths]
        if len(widths) != len(columns):
            raise ValueError("zip_records: %d widths for %d columns" % (len(widths), len(columns)))
        cols, k, keep = _zip_columns(columns, widths, "zip_records")   # (`keep` lives until the calls below have returned)
        sep = bytes(sep)
        device = columns[0][0].device
        st = _stream(device, stream)
        out_begin = torch.empty(k, dtype=torch.int64, device=device)
        out_end = torch.empty(k, dtype=torch.int64, device=device)

        def call(buf, cap):
            return int(_check(self._lib.rj_scan_records_zip(self._h, cols, len(columns), sep, len(sep), int(pad), int(flags), int(fill), int(lead), int(gap),
                                                            _ptr(buf), cap, _ptr(out_begin), _ptr(out_end), ctypes.c_void_p(st))))
        return _sized_text(call, out, device, "zip_records", "the text"), out_begin, out_end

    def format_csv_records(self, columns, delimiter: bytes = b",", quote: bytes = b'"', always=(), raw=(), fill: int = 10, lead: int = 0, gap: int = 1,
                           out=None, stream=None, stats: bool = False, flags: int = 0):
        """rj_scan_records_format_csv: the inverse of csv_records -- the rows of several columns written as quoted CSV lines on
        the device.  `columns` is zip_records' list (1 to 16) of (text, rec_begin, rec_end) or (text, rec_begin, rec_end,
        indices).  Line j is the columns' rows j joined with the byte `delimiter`; a field that holds the delimiter, the
        quote, \\r or \\n -- or whose column is listed in `always`, or the lone empty field of a one-column line -- stands
        between two `quote` bytes with every quote byte inside doubled, exactly as Python's csv.writer quotes it.  A column
        listed in `raw` holds the interiors of fields as csv_records delimits them (their "" still in place): it is quoted
        by the same rule, but nothing is doubled.  Returns (out_text, out_begin, out_end) as zip_records does -- `gap` bytes of
        `fill` (default: a newline) behind every line, `lead` in front; without `out` one size query and an exact allocation,
        with `out` (contiguous uint8, 16-byte aligned) one call and RejitError when it is too small -- and with stats=True a
        fourth value, rj_csv_format_stats as a dict.  The scan's spans, stats and select_records stay as they were."""
        import torch

        columns = [tuple(c) for c in columns]
        cols, k, keep = _zip_columns(columns, [0] * len(columns), "format_csv_records")   # (`keep` lives until the calls below have returned)
        delimiter, quote = _one_byte(delimiter, "format_csv_records", "delimiter"), _one_byte(quote, "format_csv_records", "quote")
        mask = lambda listed, name: sum({1 << (int(c) if 0 <= int(c) < 32 else _raise(ValueError("format_csv_records: %s names column %d" % (name, c)))) for c in listed})
        always_mask, raw_mask = mask(always, "always"), mask(raw, "raw")
        device = columns[0][0].device
        st = _stream(device, stream)
        out_begin = torch.empty(k, dtype=torch.int64, device=device)
        out_end = torch.empty(k, dtype=torch.int64, device=device)
        cs = _CsvFormatStats()

        def call(buf, cap):
            return int(_check(self._lib.rj_scan_records_format_csv(self._h, cols, len(columns), delimiter, quote, always_mask, raw_mask, int(flags), int(fill),
                                                                   int(lead), int(gap), _ptr(buf), cap, _ptr(out_begin), _ptr(out_end),
                                                                   ctypes.byref(cs) if stats else None, ctypes.c_void_p(st))))
        text = _sized_text(call, out, device, "format_csv_records", "the text")
        return (text, out_begin, out_end, _stats_dict(cs)) if stats else (text, out_begin, out_end)

    def replace(self, d_text_ptr: int, n: int, repl: bytes, d_out_ptr: int, out_cap: int, stream: int = 0) -> int:
        """Replace the matches of the last run(); returns the new length (text stays in HBM)."""
        return int(_check(self._lib.rj_scan_replace(self._h, ctypes.c_void_p(d_text_ptr), n, repl, len(repl),
                                                    ctypes.c_void_p(d_out_ptr), out_cap, ctypes.c_void_p(stream))))

    def spans(self) -> List[Tuple[int, int]]:
        n = int(_check(self._lib.rj_scan_copy_spans(self._h, None, 0)))
        buf = (ctypes.c_uint64 * (2 * max(n, 1)))()
        _check(self._lib.rj_scan_copy_spans(self._h, buf, n))
        return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n)]

    def spans_tensor(self, device):
        """The matches of the last run as an (k, 2) int64 torch tensor on `device` (no trip through Python
        lists: what the multi-GPU gather of many matches works on)."""
        import torch

        n = int(_check(self._lib.rj_scan_copy_spans(self._h, None, 0)))
        out = torch.empty((max(n, 1), 2), dtype=torch.int64, device=device)
        if n:
            _check(self._lib.rj_scan_copy_spans(self._h, ctypes.cast(ctypes.c_void_p(out.data_ptr()), _u64p), n))
        return out[:n]

    def device_spans_ptr(self) -> int:
        return int(self._lib.rj_scan_device_spans(self._h) or 0)

    def stats(self) -> dict:
        s = _Stats()
        _check(self._lib.rj_scan_stats(self._h, ctypes.byref(s)))
        return {k: (float(getattr(s, k)) if k.endswith("_ms") else int(getattr(s, k))) for k, _ in _Stats._fields_}

    def match_full(self, d_text_ptr: int, n: int, stream: int = 0) -> bool:
        return bool(_check(self._lib.rj_scan_match_full(self._h, ctypes.c_void_p(d_text_ptr), n, ctypes.c_void_p(stream))))


class _BorrowedScan(Scan):
    """A rj_scan owned by a rj_multi (not destroyed from Python)."""

    def __init__(self, handle, program, owner):
        self._lib = load_library()
        self.program = program
        self._h = handle
        self._owner = owner

    def __del__(self):
        self._h = None


class MultiScan:
    """Several patterns over the same device-resident text (rj_multi): one pass over the text when
    every pattern has a nibble-form window set, else one pattern after the other."""

    def __init__(self, programs: List[Program]):
        self._lib = load_library()
        self.programs = list(programs)
        arr = (ctypes.c_void_p * len(programs))(*[p._h for p in programs])
        h = ctypes.c_void_p()
        _check(self._lib.rj_multi_create(arr, len(programs), ctypes.byref(h)))
        self._h = h
        self.fused = False
        self.how = 0

    def set_mode(self, mode: int) -> None:
        """0: fuse the scans when possible (default); 1: every pattern scans the text on its own, as one launch
        when possible; 2: one kernel per pattern on two alternating streams; 3: one kernel per pattern."""
        _check(self._lib.rj_multi_set_mode(self._h, mode))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.rj_multi_destroy(h)
            self._h = None

    def run(self, d_text_ptr: int, n: int, stream: int = 0, own_begin: int = 0, own_end: Optional[int] = None) -> List[int]:
        counts = (ctypes.c_uint64 * len(self.programs))()
        r = _check(self._lib.rj_multi_run_range(self._h, ctypes.c_void_p(d_text_ptr), n, own_begin,
                                                n + 1 if own_end is None else own_end, counts, ctypes.c_void_p(stream)))
        self.how = int(r)          # 1 fused scan, 2 separate scans + batched tails, 0 one by one
        self.fused = r == 1
        return [int(c) for c in counts]

    def start(self, d_text_ptr: int, n: int, stream: int = 0, own_begin: int = 0, own_end: Optional[int] = None) -> None:
        """Enqueue a run; finish() collects its counts.  Two MultiScan objects of the same patterns used alternately
        keep the device busy while the host turns a result around."""
        _check(self._lib.rj_multi_start(self._h, ctypes.c_void_p(d_text_ptr), n, own_begin, n + 1 if own_end is None else own_end,
                                        ctypes.c_void_p(stream)))

    def set_tail_stream(self, on: bool = True) -> None:
        """start() queues only the scan kernel on the caller's stream, the tails on a stream of the object's own."""
        _check(self._lib.rj_multi_set_tail_stream(self._h, int(on)))

    def set_counts_only(self, on: bool = True) -> bool:
        """rj_multi_set_counts_only: MatchAllCount semantics -- counts (and bounds) only, no span lists; True when the
        pattern set takes the one-kernel path (plane_count.hip)."""
        return bool(_check(self._lib.rj_multi_set_counts_only(self._h, int(on))))

    def set_timing(self, on: bool = True) -> None:
        """rj_multi_set_timing: without the scan kernel's start event scan_ms() reads 0 and consecutive kernels follow closer.
        (The one-kernel counts path takes its duration from the device's wall clock: no event, nothing to gain by switching it off.)"""
        _check(self._lib.rj_multi_set_timing(self._h, int(on)))

    def order_after(self, other: Optional["MultiScan"]) -> None:
        """This object's scan kernels wait for the scan kernel of `other`'s run in flight (two objects, two streams)."""
        self._after = other   # (keeps it alive)
        _check(self._lib.rj_multi_order_after(self._h, other._h if other is not None else None))

    def finish(self) -> List[int]:
        counts = (ctypes.c_uint64 * len(self.programs))()
        r = _check(self._lib.rj_multi_finish(self._h, counts))
        self.how = int(r)
        self.fused = r == 1
        return [int(c) for c in counts]

    def device_counts(self, d_text_ptr: int, n: int, offset: int, rank: int, world: int, comm: Optional[int] = None, allgather=None,
                      own_begin: int = 0, own_end: Optional[int] = None, stream: int = 0) -> List[int]:
        """rj_multi_device_counts: run over this rank's shard, then the carry exchange between the shards, behind one call.
        `comm` = an ncclComm_t (integer handle) of RCCL, or `allgather` = an ALLGATHER_FN(ctx, d_send, d_recv, bytes, stream)
        callable.  Returns the job-wide counts (the same on every rank)."""
        counts = (ctypes.c_uint64 * len(self.programs))()
        args = (self._h, ctypes.c_void_p(d_text_ptr), n, own_begin, n + 1 if own_end is None else own_end, ctypes.c_int64(offset))
        if allgather is not None:
            fn = allgather if isinstance(allgather, ALLGATHER_FN) else ALLGATHER_FN(allgather)
            r = _check(self._lib.rj_multi_device_counts_via(*args, fn, None, rank, world, counts, ctypes.c_void_p(stream)))
        else:
            r = _check(self._lib.rj_multi_device_counts(*args, ctypes.c_void_p(comm), rank, world, counts, ctypes.c_void_p(stream)))
        self.how = int(r)
        self.fused = r == 1
        return [int(c) for c in counts]

    def scan(self, i: int) -> Scan:
        return _BorrowedScan(ctypes.c_void_p(self._lib.rj_multi_scan(self._h, i)), self.programs[i], self)

    def scan_ms(self) -> float:
        return float(self._lib.rj_multi_scan_ms(self._h))

    def bounds_rows(self, rows_tensor, offset: int = 0, first_round: bool = True, stream: int = 0) -> None:
        """rj_multi_bounds_device: this rank's rows of the carry exchange (8 integers per pattern, include/rejit_hip.h)
        into the (P, 8) int64 device tensor `rows_tensor`; queued on `stream`, nothing waits."""
        assert rows_tensor.dtype.itemsize == 8 and rows_tensor.numel() >= 8 * len(self.programs) and rows_tensor.is_contiguous()
        _check(self._lib.rj_multi_bounds_device(self._h, ctypes.c_int64(offset), int(first_round), ctypes.c_void_p(rows_tensor.data_ptr()),
                                                ctypes.c_void_p(stream)))

    def bounds(self, stream: int = 0) -> List[Optional[Tuple[int, int, int, int]]]:
        """Per pattern (first begin, first end, last begin, last end) of the last run, None without a
        match: what neighbouring shards exchange to carry the selection over a cut (rj_multi_bounds)."""
        k = len(self.programs)
        buf = (ctypes.c_uint64 * (4 * k))()
        _check(self._lib.rj_multi_bounds(self._h, buf, ctypes.c_void_p(stream)))
        none = (1 << 64) - 1
        return [None if buf[4 * i] == none else tuple(int(buf[4 * i + j]) for j in range(4)) for i in range(k)]
