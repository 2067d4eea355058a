"""GPU tests (-m gpu) of REUSED objects: an rj_scan carries routing state from one call to the next (engine_internal.h:
linear_hint, runs_sparse / window_dense, streams_off, behind_conflicts, no_local_select, region_cap_hint / hits_hint,
counter_state / counter, want_exact), and the host-text entry points share ONE cached scan per (thread, program)
(host_api.hip: host_scan_for, 16 entries, purged by epoch when a program is freed on another thread).

A sequence runner drives one object through a list of steps (entry, text, arguments) and compares every step with the
oracle on that step alone: own ranges with a carried-in match, counts, start / finish, match_full, replace, the host
entries.  On a mismatch the same step runs on a FRESH object as well, and the message says whether that one agrees, with
the seed and the whole step history -- a state bug and a plain path bug look different there.

Every scenario proves through stats() / host_stats() that its trigger really switched the route, then runs a fixed
battery of other texts and entries on the same object, then the trigger again; where the code promises a way back
(linear_hint cleared by the carry scan, the one-kernel count after a void run) that is asserted too."""
import random
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from checkers import Oracle

pytestmark = pytest.mark.gpu

SMALL_MAX = 32768          # engine: kSmallMaxText
WINDOW_RUNS = 256 << 10    # engine.hip: window_runs needs a range of this many bytes that reaches the text's end


@pytest.fixture(scope="module")
def rj():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rejit_amd
    rejit_amd.build()
    rejit_amd.load_library()
    return rejit_amd


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def device_text(data: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(data + b"\0" * (16 if not data else 0), dtype=np.uint8).copy()).cuda()


def splice(text: bytes, spans, repl: bytes) -> bytes:
    out, p = bytearray(), 0
    for b, e in spans:
        out += text[p:b] + repl
        p = e
    return bytes(out + text[p:])


class Want:
    """The oracle's answers, cached per (pattern, text)."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.cache = {}

    def all(self, rx, text):
        key = (rx, len(text), hash(text))
        if key not in self.cache:
            got = self.oracle.match_all(rx, text)
            assert not isinstance(got, int), (rx, got)
            self.cache[key] = got
        return self.cache[key]

    def full(self, rx, text):
        return self.oracle.match_full(rx, text) > 0


def fits_range(got, want_whole, rx, text, ob, oe, want):
    """An independent range (no carry): the selection starts afresh at own_begin -- or, for kernels that look at the byte
    before the range, as in the whole text (tests/test_gpu_runs.py: check); either is exact."""
    fresh = [(b + ob, e + ob) for b, e in want.all(rx, text[ob:]) if b + ob < oe]
    return got == fresh or got == [m for m in want_whole if ob <= m[0] < oe]


class Seq:
    """One reused Scan (and the Program's host entries) driven through steps; every step checked alone."""

    ENTRIES = ("run", "halves", "tail", "empty", "count", "start", "full", "replace",
               "h_all", "h_count", "h_first", "h_anywhere", "h_full", "h_replace", "h_batch")

    def __init__(self, rj, want, rx, seed=None, q8=None):
        self.rj, self.want, self.rx, self.seed = rj, want, rx, seed
        self.prog = rj.Program(rx)
        self.scan = rj.Scan(self.prog)
        self.q8 = self.prog.info()["ring_artefact_risk"] != 0 if q8 is None else q8
        self.history = []

    # -- one step on a given (scan, program); returns the stats of the call that answered, raises AssertionError on a mismatch
    def _do(self, scan, prog, entry, text, arg):
        rj, rx, W = self.rj, self.rx, self.want
        whole = W.all(rx, text)
        n = len(text)
        if entry.startswith("h_"):
            if entry == "h_all":
                got = prog.match_all(text)
                assert got == whole, ("match_all", len(got), len(whole), got[:3], whole[:3])
            elif entry == "h_count":
                got = prog.count(text)
                assert got == len(whole), ("count", got, len(whole))
            elif entry == "h_first":
                got = prog.match_first(text)
                assert got == (whole[0] if whole else None), ("match_first", got, whole[:1])
            elif entry == "h_anywhere":
                assert prog.match_anywhere(text) == bool(whole), ("match_anywhere", bool(whole))
            elif entry == "h_full":
                assert prog.match_full(text) == W.full(rx, text), ("match_full", W.full(rx, text))
            elif entry == "h_replace":
                m, out = prog.replace_all(text, b"<#>")
                assert m == len(whole) and out == splice(text, whole, b"<#>"), ("replace_all", m, len(whole))
            elif entry == "h_batch":
                others = arg or []
                texts = [text] + others + [text[: n // 2]]
                got = prog.match_all_batch(texts)
                exp = [W.all(rx, t) for t in texts]
                assert got == exp, ("match_all_batch", [len(g) for g in got], [len(e) for e in exp])
            return prog.host_stats()
        d = device_text(text)
        p = d.data_ptr()
        if entry == "run":
            k = scan.run(p, n)
            got = scan.spans()
            assert k == len(whole) and got == whole, ("run", k, len(whole), got[:3], whole[:3])
        elif entry == "halves":
            # [0, cut) -- a range that ends before the text does -- then [cut, n] with the selection carried over the cut; their
            # concatenation is the whole text's answer (at-risk patterns own whole segments between sync points: exact_replay.hip)
            cut = arg
            k1 = scan.run(p, n, own_begin=0, own_end=cut)
            first = scan.spans()
            assert k1 == len(first)
            if not self.q8:
                assert first == [m for m in whole if m[0] < cut], ("range [0, cut)", cut, len(first))
            carry = dict(carry_cur=0, carry_prev_end=0, have_prev=False)
            if first:
                b, e = first[-1]
                carry = dict(carry_cur=e if e > b else b + 1, carry_prev_end=e, have_prev=True)
            k2 = scan.run(p, n, own_begin=cut, own_end=n + 1, **carry)
            second = scan.spans()
            assert k2 == len(second) and first + second == whole, ("halves", cut, carry, len(first), len(second), len(whole))
        elif entry == "tail":
            ob = arg
            k = scan.run(p, n, own_begin=ob, own_end=n + 1)
            got = scan.spans()
            assert k == len(got)
            if self.q8:
                assert got == [m for m in whole if m[0] >= got[0][0]] if got else True, ("tail", ob)
            else:
                assert fits_range(got, whole, rx, text, ob, n + 1, W), ("tail [ob, n]", ob, got[:3])
        elif entry == "empty":
            ob = arg
            k = scan.run(p, n, own_begin=ob, own_end=ob)
            got = scan.spans()
            assert k == 0 and got == [], ("empty range", ob, k, got[:3])
        elif entry == "count":
            k = scan.count(p, n)
            assert k == len(whole), ("count", k, len(whole))
            # afterwards there is either no list (RJ_BAD_ARGUMENT) or the list of THIS text -- never an earlier call's; after the
            # one-kernel count the device list pointer is NULL (include/rejit_hip.h), looked at before anything is copied
            if scan.stats()["count_path"] == 1:
                assert scan.device_spans_ptr() == 0, ("a list pointer after the one-kernel count", scan.device_spans_ptr())
            try:
                got = scan.spans()
            except rj.RejitError:
                got = None
            assert got is None or got == whole, ("spans after count", len(got), len(whole), got[:3], whole[:3])
            if whole:
                out = device_text(b"\0" * (len(splice(text, whole, b"<#>")) + 64))
                try:
                    m = scan.replace(p, n, b"<#>", out.data_ptr(), out.numel())
                except rj.RejitError:
                    m = None
                if m is not None:
                    assert bytes(out[:m].cpu().numpy()) == splice(text, whole, b"<#>"), ("replace after count", m)
        elif entry == "start":
            scan.start(p, n)
            k = scan.finish()
            got = scan.spans()
            assert k == len(whole) and got == whole, ("start/finish", k, len(whole), got[:3], whole[:3])
        elif entry == "full":
            assert scan.match_full(p, n) == W.full(rx, text), ("match_full", W.full(rx, text))
        elif entry == "replace":
            k = scan.run(p, n)
            assert k == len(whole)
            exp = splice(text, whole, b"<#>")
            out = device_text(b"\0" * (len(exp) + 64))
            m = scan.replace(p, n, b"<#>", out.data_ptr(), out.numel())
            assert m == len(exp) and bytes(out[:m].cpu().numpy()) == exp, ("replace", m, len(exp))
        else:
            raise ValueError(entry)
        return scan.stats()

    def step(self, entry, text, arg=None, name="?"):
        """Run one step on the reused objects; on a mismatch, the same step on fresh ones, and a message with the history."""
        self.history.append((entry, name, len(text), arg if not isinstance(arg, list) else "%d texts" % len(arg)))
        try:
            return self._do(self.scan, self.prog, entry, text, arg)
        except (AssertionError, self.rj.RejitError) as err:
            fresh_prog = self.rj.Program(self.rx)
            try:
                self._do(self.rj.Scan(fresh_prog), fresh_prog, entry, text, arg)
                fresh = "a FRESH object agrees with the oracle: state left by earlier steps"
            except (AssertionError, self.rj.RejitError) as err2:
                fresh = "a FRESH object fails too (%s): a path bug, not a state bug" % (err2,)
            hist = "\n".join("  %3d %-10s %-14s n=%-8d %s" % (i, e, nm, ln, a) for i, (e, nm, ln, a) in enumerate(self.history))
            raise AssertionError("pattern %r seed %s: step %d %s on %r (%d bytes, arg %s) differs: %s\n%s\nsteps:\n%s"
                                 % (self.rx, self.seed, len(self.history) - 1, entry, name, len(text), arg, err, fresh, hist)) from None

    def battery(self, maker, contrast, trigger, host=True):
        """The fixed battery after a trigger: `contrast` = (name, text) of the other character, `maker(n)` = texts of the
        scenario's alphabet at the sizes where paths switch."""
        for name, t in contrast:
            self.step("run", t, name=name)
        t = maker(70001)
        self.step("halves", t, 70001 // 3 + 17, name="mix70001")
        big = maker(WINDOW_RUNS + 1)
        self.step("tail", big, len(big) // 2 + 5, name="mix256K+1")     # begins inside the text, reaches its end
        self.step("halves", big, len(big) - 1000, name="mix256K+1")
        self.step("empty", big, 1234, name="mix256K+1")
        self.step("empty", big, len(big), name="mix256K+1")
        for n in (0, 1, 15, 16, SMALL_MAX, SMALL_MAX + 1, WINDOW_RUNS - 1, WINDOW_RUNS + 1):
            self.step("run", maker(n), name="mix%d" % n)
        self.step("count", big, name="mix256K+1")
        self.step("count", maker(16), name="mix16")
        self.step("count", maker(15), name="mix15")
        self.step("start", maker(WINDOW_RUNS - 1), name="mix256K-1")
        self.step("full", maker(SMALL_MAX + 1), name="mix32769")
        self.step("replace", big, name="mix256K+1")
        if host:
            for e in ("h_all", "h_count", "h_first", "h_anywhere", "h_full", "h_replace"):
                self.step(e, big, name="mix256K+1")
            self.step("h_batch", maker(SMALL_MAX), [maker(100)], name="mix32768")
        return self.step("run", trigger, name="trigger")


def alphabet_maker(alphabet: bytes, seed: int, plant: bytes = b"", every: int = 0):
    cache = {}

    def make(n):
        if n not in cache:
            rng = np.random.default_rng(seed * 1000003 + n)
            t = bytearray(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes())
            if plant and every:
                for p in range(int(rng.integers(every)), max(n - len(plant), 0), every):
                    t[p:p + len(plant)] = plant
            cache[n] = bytes(t)
        return cache[n]
    return make


# ---------------------------------------------------------------- one scenario per routing flag


def test_linear_hint_carry_scan_and_the_way_back(rj, oracle):
    """linear_hint (engine.hip: set where a walk outlived max_walk; linear.hip clears it when no walk reached max_walk): a
    wide cyclic automaton over a hundred kilobytes of its own words takes the carry scan; the next texts go there directly;
    a text of short candidates clears the hint -- the call after it is back on the parallel verifier."""
    rng = random.Random(9)
    words = ["".join(rng.choice("abcd") for _ in range(rng.randint(6, 10))) for _ in range(40)]
    rx = ("(" + "|".join(words) + ")+").encode()
    want = Want(oracle)
    seq = Seq(rj, want, rx, seed=9)
    trigger = ("".join(rng.choice(words) for _ in range(20_000)) + "x" + "".join(rng.choice(words) for _ in range(1000)) + "ab").encode()
    st = seq.step("run", trigger, name="one-candidate")
    assert st["linear_path"] == 1, st                       # the trigger: linear_hint set

    def short(n):    # candidates of one or two words, a break byte between them
        r = random.Random(n)
        out = bytearray()
        while len(out) < n:
            out += (rng.choice(words) * r.randint(1, 2) + r.choice(["x", " ", "\n"])).encode()
        return bytes(out[:n])
    st = seq.step("run", short(200_000), name="short")
    assert st["linear_path"] == 1, st                       # the hint sends the next text straight to the carry scan ...
    st = seq.step("run", short(200_001), name="short")
    assert st["linear_path"] == 0, st                       # ... which found no long walk and cleared it (linear.hip)
    st = seq.step("run", trigger, name="one-candidate")
    assert st["linear_path"] == 1, st
    st = seq.battery(short, [("short", short(100_000))], trigger)
    assert st["linear_path"] == 1, st


def test_window_run_shapes_runs_sparse_and_window_dense(rj, oracle):
    """runs_sparse / window_dense (engine.hip: window_runs): `a.*b`, `#.*`, `<[^>]*>` over log-like text take the run kernels,
    a sparse text sends the next run to the window scan, a window scan that meets dense hits sends the object back to the
    run kernels for good (there is no way back from window_dense: asserted).  Each route is then given the whole battery."""
    rng = random.Random(48)
    n = 400000
    dense = bytes(rng.choice(b"abcdefgh <>#()\n ") for _ in range(n))
    sparse = bytearray(rng.choice(b"cdefgh\n") for _ in range(n))
    for rx, plant in ((b"a.*b", b"a cd b"), (b"#.*", b"# x"), (b"<[^>]*>", b"<cd>")):
        sp = bytearray(sparse)
        sp[n // 2:n // 2 + len(plant)] = plant
        sp = bytes(sp)
        want = Want(oracle)
        seq = Seq(rj, want, rx, seed=48)
        mix = alphabet_maker(b"abcdefgh <>#()\n ", 48)
        assert seq.step("run", dense, name="dense")["run_path"] == 1, rx
        assert seq.step("run", sp, name="sparse")["run_path"] == 1, rx         # one match in 400 KB: runs_sparse
        assert seq.step("run", sp, name="sparse")["run_path"] == 0, rx         # the trigger: the window scan
        # the battery on the window route (runs_sparse set, window_dense not): texts without the window byte keep it (a hit
        # per 32 KiB or denser -- any plant in the battery's small texts -- would set window_dense)
        sparse_mix = alphabet_maker(b"cdefgh\n", 49)
        st = seq.battery(sparse_mix, [("sparse-short", sp[: SMALL_MAX + 1])], sp)
        assert st["run_path"] == 0, (rx, st)
        assert seq.step("run", dense, name="dense")["run_path"] == 0, rx       # the window scan meets dense hits: window_dense
        st = seq.battery(mix, [("sparse", sp), ("sparse", sp)], sp)
        assert st["run_path"] == 1, (rx, st)                                   # the run kernels for good
        assert seq.step("run", sp, name="sparse")["run_path"] == 1, rx


def test_streams_off_hands_over_to_the_run_kernels(rj, oracle):
    """streams_off (engine.hip: dense_streams gave a text up -- a run longer than it decides in registers): `[acgt]+` over
    short runs takes dense_streams (stream_path 1); a text with one run of 300 KB sets the flag and the run kernels answer
    (stream_path 1 -> 0, run_path 0 -> 1); from then on the object stays there, on short runs too."""
    rng = random.Random(47)
    rx = b"[acgt]+"
    short = alphabet_maker(b"acgtacgtacgtacgtN\xf0", 47)
    t = bytearray(short(600000))
    t[200000:500000] = bytes(rng.choice(b"acgt") for _ in range(300000))
    long_run = bytes(t)
    seq = Seq(rj, Want(oracle), rx, seed=47)
    st = seq.step("run", short(300000), name="short-runs")
    assert st["stream_path"] == 1 and st["run_path"] == 0, st
    st = seq.step("run", long_run, name="300K-run")
    assert st["stream_path"] == 0 and st["run_path"] == 1, st    # the trigger
    st = seq.step("run", short(300001), name="short-runs")
    assert st["stream_path"] == 0 and st["run_path"] == 1, st    # no way back: streams_off is for good
    st = seq.battery(short, [("short-runs", short(500000)), ("none", b"N" * 300000)], long_run)
    assert st["run_path"] == 1, st


def test_behind_conflicts_stay_dense(rj, oracle):
    """behind_conflicts (engine.hip: behind mode met a hidden candidate reaching past the match that hides it -> dense path,
    retries >= 1): `[a-z]+@[a-z]+` over text holding `ab@cd@ef`.  The object stays dense: the trigger text again needs no
    retry, where a fresh object retries."""
    rx = b"[a-z]+@[a-z]+"
    mix = alphabet_maker(b"abcdx \nAB@.", 31)
    t = bytearray(mix(300000))
    for at in range(1000, 300000, 9000):
        t[at:at + 8] = b"ab@cd@ef"
    trigger = bytes(t)
    seq = Seq(rj, Want(oracle), rx, seed=31)
    no_conflict = alphabet_maker(b"abcdefgh xyz\n", 32, b" qq@rr ", 3000)
    seq.step("run", no_conflict(300000), name="no-conflict")
    st = seq.step("run", trigger, name="ab@cd@ef")
    assert st["retries"] >= 1, st                                # the trigger
    st = seq.battery(mix, [("no-conflict", no_conflict(300001)), ("no-conflict", no_conflict(40000))], trigger)
    assert st["retries"] == 0, st                                # dense for good: no second retry
    fresh = rj.Scan(rj.Program(rx))
    d = device_text(trigger)
    fresh.run(d.data_ptr(), len(trigger))
    assert fresh.stats()["retries"] >= 1 and fresh.spans() == seq.want.all(rx, trigger)


def test_no_local_select_floating_windows(rj, oracle, monkeypatch):
    """no_local_select (engine.hip: floating windows whose in-region selection left overlapping candidates across two regions
    -> the general selection, retries >= 1, for good).  Floating-window patterns of tools/fuzz_floating.py over texts dense in
    groups whose matches overlap the next group's candidates; the trigger is the first (pattern, text) whose retry goes away
    under RJ_NO_LOCAL_SELECT (read at every run): that retry was the in-region selection's."""
    def group_text(seed, lit):
        rng = random.Random(seed)
        parts, n = [], 0
        while n < 400000:
            p = rng.choice([b"a" + lit + b"abab" + lit + b"b", b"bb" + lit + b"a" + lit + b"ab", lit, b"ab", b"c", b" ", b"abab"])
            p += bytes(rng.choice(b"abc " + lit) for _ in range(rng.randrange(0, 40)))
            parts.append(p)
            n += len(p)
        return b"".join(parts)
    found = None
    for rx in (b"[ab]{1,4}xyz[ab]+", b"(ab|b){2,5}xyz[ab]+", b"[ab]{2,7}c?xyz(a|bc)", b"(a|bb){1,3}xyzb{0,2}", b"([ab]|cc){1,6}xyz[ab]"):
        info = rj.Program(rx).info()
        if not (info["scan_mode"] == 1 and info["window_offset"] == 0 and info["min_len"] != info["window_len"]):
            continue     # (not floating on this lowering)
        for seed in range(4):
            trigger = group_text(seed, b"xyz")
            sc = rj.Scan(rj.Program(rx))
            d = device_text(trigger)
            sc.run(d.data_ptr(), len(trigger))
            if sc.stats()["retries"] == 0:
                continue
            monkeypatch.setenv("RJ_NO_LOCAL_SELECT", "1")
            sc2 = rj.Scan(rj.Program(rx))
            sc2.run(d.data_ptr(), len(trigger))
            monkeypatch.delenv("RJ_NO_LOCAL_SELECT")
            assert sc.spans() == sc2.spans() == oracle.match_all(rx, trigger), (rx, seed)
            if sc2.stats()["retries"] == 0:
                found = (rx, seed, trigger)
                break
        if found:
            break
    assert found, "no floating pattern met overlapping candidates across regions"
    rx, seed, trigger = found
    seq = Seq(rj, Want(oracle), rx, seed=seed)
    st = seq.step("run", trigger, name="overlaps")
    assert st["retries"] >= 1, st                                # the trigger
    mix = alphabet_maker(b"abcxyz \n", 78, b"bxyzab", 700)
    st = seq.battery(mix, [("few", alphabet_maker(b"abc \n", 79, b"xyzb", 20000)(300000))], trigger)
    assert st["retries"] == 0, st                                # the in-region selection is not tried again


def test_region_cap_and_hits_hints(rj, oracle):
    """region_cap_hint / hits_hint (engine.hip: a hit region overflowed -> the run is repeated with regions sized for the
    fullest one, retries >= 1; the next run starts with that size): `regexp` back to back, then sparse texts (the hints far
    too big), then the dense text again (no retry: the hint held)."""
    rx = b"regexp"
    trigger = b"regexp" * 60000
    seq = Seq(rj, Want(oracle), rx, seed=5)
    st = seq.step("run", trigger, name="back-to-back")
    assert st["retries"] >= 1, st                                # the trigger
    sparse = alphabet_maker(b"regxp ab\n\x80", 5, b"regexp", 40000)
    st = seq.battery(sparse, [("sparse", sparse(1 << 20)), ("none", b"z" * 300000)], trigger)
    assert st["retries"] == 0, st


def test_counter_state_void_run_and_the_way_back(rj, oracle):
    """counter_state / counter (multi_pattern.hip: scan_count): a regexdna pattern's count takes the one-kernel count
    (count_path 1); a block full of candidates voids its run, the span pipeline answers THAT call (count_path 0), the next
    call tries the kernel again (include/rejit_hip.h) -- count_path 1 -> 0 -> 1.  After each count the list is refused or is
    this text's, never the run's before it."""
    from rejit_amd import workloads as W
    rx = W.REGEXDNA_PATTERNS[0].encode()
    seq = Seq(rj, Want(oracle), rx, seed=23)
    clean = W.fasta_stripped_numpy(40000).tobytes()[:400000]
    void = b"agggtaaa" * 400000 + b"acgt" * 1000
    seq.step("run", clean, name="fasta")                          # a list first: the count after it must not hand it out
    assert seq.step("count", clean, name="fasta")["count_path"] == 1
    assert seq.step("count", void, name="void")["count_path"] == 0      # the trigger
    assert seq.step("count", clean, name="fasta")["count_path"] == 1    # the way back
    maker = lambda n: (clean * (n // len(clean) + 1))[:n]
    seq.battery(maker, [("void", void)], clean)
    assert seq.step("count", void, name="void")["count_path"] == 0
    st = seq.step("count", clean[:SMALL_MAX + 5], name="fasta")
    assert st["count_path"] == 1, st
    # the host entries share a cached scan: the same route changes behind rj_match_all(..., NULL)
    for e in ("h_all", "h_count", "h_replace", "h_count"):
        seq.step(e, clean, name="fasta")
    assert seq.prog.host_stats()["count_path"] == 1
    seq.step("h_count", void, name="void")
    assert seq.prog.host_stats()["count_path"] == 0
    seq.step("h_count", clean, name="fasta")
    assert seq.prog.host_stats()["count_path"] == 1


def test_want_exact_is_per_call(rj, oracle):
    """want_exact (engine.hip: the run met an adjacency the reference's ring artefact can apply to -> the exact replay,
    exact_path >= 1; reset at the next call): `.{0,2}.` over text where the artefact applies, then texts where it cannot."""
    rx = b".{0,2}."
    mix = alphabet_maker(b"abcdefghijklmnopqrstuvwxyz0123456789  \n", 5)
    trigger = mix(300000)
    assert oracle.match_all(rx, trigger) != oracle.match_all_spec(rx, trigger)   # the artefact applies on this text
    seq = Seq(rj, Want(oracle), rx, seed=5)
    assert seq.q8
    st = seq.step("run", trigger, name="artefact")
    assert st["exact_path"] >= 1, st                            # the trigger
    seq.step("run", b"\n" * 300000, name="lines")
    st = seq.battery(mix, [("lines", b"ab\n" * 100000)], trigger)
    assert st["exact_path"] >= 1, st


# ---------------------------------------------------------------- the list tail (automata of more than 128 positions)


def test_list_tail_small_finalize_and_large_path(rj, oracle):
    """engine.hip, list_tail: an automaton of more than 128 positions (n_words > 4) never takes the one-workgroup kernel nor the
    in-region tail -- region_offsets, verify_wave, finalize_small; more than kFinalizeCap (2048) candidate slots send the run on
    to finalize_large (large_path 1), a dozen matches do not (large_path 0).  One object: the hints of each run meet the other."""
    rx = b"qzvw[a-z]{1,140}"
    seq = Seq(rj, Want(oracle), rx, seed=11)
    info = seq.prog.info()
    assert info["scan_mode"] == 1 and info["n_words"] > 4, info
    rng = random.Random(11)
    parts = []
    while sum(map(len, parts)) < 60000:
        parts.append(b"qzvw" + bytes(rng.choice(b"abqz") for _ in range(rng.randrange(0, 6))) + rng.choice([b" ", b"\n", b"Q", b"qzv "]))
    many = b"".join(parts)[:60000]
    assert many.count(b"qzvw") > 2048 and len(many) <= 64 << 10
    few = alphabet_maker(b"abcqzvw \n", 12, b"qzvwabc ", 5000)(60000)
    assert 10 <= len(seq.want.all(rx, few)) <= 40
    for text, name, large in ((many, "many", 1), (few, "few", 0), (many, "many", 1), (few, "few", 0)):
        st = seq.step("run", text, name=name)
        assert st["large_path"] == large and st["n_matches"] == len(seq.want.all(rx, text)), (name, st)
    seq.step("halves", many, 20011, name="many")
    seq.step("tail", few, 30001, name="few")


def _floating_wide(rj):
    rx = b"(ab|b){2,5}xyz[ab]{1,140}"
    info = rj.Program(rx).info()
    # windows mode, more than 128 positions, and floating: the window `xyz` sits behind 2..10 bytes of prefix (offset 0 with a
    # match longer than the window is how info() shows it, as in test_no_local_select_floating_windows)
    assert info["scan_mode"] == 1 and info["n_words"] > 4 and info["window_offset"] == 0 and info["min_len"] != info["window_len"], info
    return rx


def test_floating_windows_on_the_list_tail_read_their_hit_count(rj, oracle):
    """engine.hip, list_tail: floating windows of an automaton too wide for the regions (expand > 1, no floating_regions) -- the
    run reads the hit count between the scan and the verify kernel, which sizes the candidate slots.  A few hundred hits, twice
    on one object: cold hints and warm ones; hits x 9 possible starts are more than finalize_small takes (large_path 1: the
    sort of the interleaved starts)."""
    rx = _floating_wide(rj)
    text = alphabet_maker(b"ab c\n", 13, b"babxyzab", 600)(200000)
    t = bytearray(text)
    for at in range(150, len(t) - 8, 4100):
        t[at:at + 8] = b" xyzabab"          # a hit without its prefix, and `bbabxyz` chains
    text = bytes(t)
    assert 300 <= text.count(b"xyz") <= 999 and len(text) <= 256 << 10
    seq = Seq(rj, Want(oracle), rx, seed=13)
    for name in ("cold", "warm"):
        st = seq.step("run", text, name=name)
        assert st["large_path"] == 1 and st["n_hits"] == text.count(b"xyz"), (name, st)
    seq.step("halves", text, 70001, name="warm")


def test_floating_windows_on_the_list_tail_grow_their_candidate_slots(rj, oracle):
    """The same route with more candidate slots than the lists start with (65536): they grow between the scan and the verify
    kernel, on the cold run; the warm run finds them grown."""
    rx = _floating_wide(rj)
    text = alphabet_maker(b"ab c\n", 14, b"abxyzb ", 24)(240000)
    assert text.count(b"xyz") * 9 > 65536 and len(text) <= 256 << 10
    seq = Seq(rj, Want(oracle), rx, seed=14)
    for name in ("cold", "warm"):
        st = seq.step("run", text, name=name)
        assert st["large_path"] == 1 and st["n_hits"] == text.count(b"xyz"), (name, st)


# ---------------------------------------------------------------- host entries and their cached scans


def test_host_entries_interleaved_on_one_program(rj, oracle):
    """All host entries of one Program on the section texts (the flag-setting texts and the small pinned-text path), in an
    order that mixes entries and sizes; the routes claimed are checked through host_stats()."""
    rng = random.Random(61)
    n = 400000
    dense = bytes(rng.choice(b"abcdefgh <>#()\n ") for _ in range(n))
    sparse = bytearray(rng.choice(b"cdefgh\n") for _ in range(n))
    sparse[n // 2:n // 2 + 6] = b"a cd b"
    sparse = bytes(sparse)
    seq = Seq(rj, Want(oracle), b"a.*b", seed=61)
    mix = alphabet_maker(b"abcdefgh <>#()\n ", 61)
    texts = [("dense", dense), ("sparse", sparse), ("small", dense[:100]), ("pinned", dense[:SMALL_MAX]), ("empty", b""),
             ("one", b"a"), ("16", dense[:16]), ("32769", dense[:SMALL_MAX + 1])]
    seq.step("h_all", dense, name="dense")
    assert seq.prog.host_stats()["run_path"] == 1
    seq.step("h_all", sparse, name="sparse")
    assert seq.prog.host_stats()["run_path"] == 1
    seq.step("h_all", sparse, name="sparse")
    assert seq.prog.host_stats()["run_path"] == 0            # runs_sparse on the cached scan: the window scan
    entries = ["h_all", "h_count", "h_first", "h_anywhere", "h_full", "h_replace", "h_batch"]
    for i in range(3):
        for e in entries:
            name, t = texts[(i * 3 + entries.index(e)) % len(texts)]
            seq.step(e, t, [mix(3000), b""] if e == "h_batch" else None, name=name)
    seq.step("h_all", dense, name="dense")
    seq.step("h_all", dense, name="dense")
    assert seq.prog.host_stats()["run_path"] == 1            # window_dense (small texts with hits set it): the run kernels
    for e in entries:
        seq.step(e, dense, [sparse[:5000]] if e == "h_batch" else None, name="dense")
    # the regexdna pattern: the one-kernel count behind rj_match_all(..., NULL), a void text, the way back
    from rejit_amd import workloads as W
    rx = W.REGEXDNA_PATTERNS[1].encode()
    seq2 = Seq(rj, seq.want, rx, seed=62)
    clean = W.fasta_stripped_numpy(30000).tobytes()[:300000]
    void = b"tttaccct" * 400000
    for name, t in (("fasta", clean), ("void", void), ("fasta", clean)):
        for e in entries:
            seq2.step(e, t, [clean[:20000]] if e == "h_batch" else None, name=name)
        seq2.step("h_count", t, name=name)
        assert seq2.prog.host_stats()["count_path"] == (0 if name == "void" else 1), (name, seq2.prog.host_stats())


def test_host_cache_eviction_round_robin(rj, oracle):
    """18 programs round robin on one thread: the cache holds 16 scans per thread, so every call meets an eviction (and
    a scan made afresh); every answer stays exact."""
    want = Want(oracle)
    pats = [b"regexp", b"a.*b", b"[acgt]+", b"\"[^\"]*\"", b"agggtaaa|tttaccct", b"x*", b"[a-z]+@[a-z]+", b"#.*$", b".{0,2}.",
            b"[a-f]+[0-9]", b"<[^>]*>", b" +", b"(a|b)*abb", b"^[a-z]+", b"ab|ba", b"[0-9]+x", b"q[a-z]*[0-9]", b"reg+exp$"]
    progs = [rj.Program(rx) for rx in pats]
    mix = alphabet_maker(b"abcgtx\"<>#@ 0129q\nregexp", 71)
    sizes = [100, SMALL_MAX + 1, 70001, 3000]
    for rnd in range(3):
        for i, (rx, p) in enumerate(zip(pats, progs)):
            t = mix(sizes[(i + rnd) % len(sizes)])
            got = p.match_all(t) if (i + rnd) % 3 else p.count(t)
            exp = want.all(rx, t)
            assert got == (exp if (i + rnd) % 3 else len(exp)), (rnd, rx, len(t))


def test_freed_program_then_new_pattern(rj, oracle):
    """A program freed and a different pattern compiled (often at the same address): its first host call gives its own
    answer, for every entry."""
    want = Want(oracle)
    mix = alphabet_maker(b"abcdefgh <>#()\n agggtaaa", 81)
    t = mix(70001)
    pairs = [(b"a.*b", b"regexp"), (b"agggtaaa|tttaccct", b"[acgt]+"), (b"x*", b"<[^>]*>"), (b"#.*", b".{0,2}.")]
    for a, b in pairs:
        for entry in ("match_all", "count", "match_first", "match_full"):
            p = rj.Program(a)
            p.match_all(t)
            p.count(t)
            del p
            q = rj.Program(b)
            exp = want.all(b, t)
            got = getattr(q, entry)(t)
            exp_entry = {"match_all": exp, "count": len(exp), "match_first": exp[0] if exp else None, "match_full": want.full(b, t)}[entry]
            assert got == exp_entry, (a, b, entry)
            del q


def test_freed_on_another_thread_epoch_purge(rj, oracle):
    """A program run on a worker thread and freed on the main thread: the worker's cached scan of it is purged by epoch
    (host_api.hip: purge_freed_scans) before a new program -- possibly at the same address -- runs there."""
    want = Want(oracle)
    mix = alphabet_maker(b"abcdefgh <>#()\n regexp", 91)
    t1, t2 = mix(70001), mix(SMALL_MAX + 3)
    with ThreadPoolExecutor(max_workers=1) as pool:
        worker = pool.submit(threading.get_ident).result()
        for a, b in ((b"a.*b", b"regexp"), (b"regexp", b"a.*b"), (b"<[^>]*>", b"#.*"), (b"[a-h]+", b" +")):
            p = rj.Program(a)
            assert pool.submit(p.match_all, t1).result() == want.all(a, t1)
            assert pool.submit(p.count, t2).result() == len(want.all(a, t2))
            del p                                                 # freed on the main thread
            q = rj.Program(b)
            assert pool.submit(threading.get_ident).result() == worker
            assert pool.submit(q.match_all, t1).result() == want.all(b, t1), (a, b)
            assert pool.submit(q.count, t2).result() == len(want.all(b, t2)), (a, b)
            assert q.match_all(t2) == want.all(b, t2)
            del q


# ---------------------------------------------------------------- MultiScan reuse


def test_multiscan_reuse(rj, oracle):
    """One MultiScan of a run shape and a literal, and one of two regexdna patterns (the one-kernel count), driven through
    run / run_range, set_counts_only(True / False) and text sizes: every inner scan's list equals the oracle wherever a list
    exists, and is refused -- never stale -- where it does not."""
    import torch
    want = Want(oracle)
    from rejit_amd import workloads as W
    fasta = W.fasta_stripped_numpy(40000).tobytes()
    mixed = [b"[acgt]+", b"agggtaaa"]
    dna = [W.REGEXDNA_PATTERNS[0].encode(), W.REGEXDNA_PATTERNS[1].encode()]
    ms_mixed = rj.MultiScan([rj.Program(rx) for rx in mixed])
    ms_dna = rj.MultiScan([rj.Program(rx) for rx in dna])
    t = bytearray(fasta[:300000])
    t[100000:100000 + 8 * 2000] = b"agggtaaa" * 2000
    texts = [("fasta", fasta[:300000]), ("small", fasta[:5000]), ("runs", bytes(t)), ("fasta17", fasta[:17]),
             ("void", b"agggtaaa" * 400000), ("N", fasta[:70001].replace(b"c", b"N"))]
    history = []
    rng = random.Random(33)
    for i in range(24):
        ms, pats = (ms_mixed, mixed) if i % 2 == 0 else (ms_dna, dna)
        name, text = texts[rng.randrange(len(texts))]
        counts_only = rng.random() < 0.5
        ranged = rng.random() < 0.4
        history.append((i, "mixed" if ms is ms_mixed else "dna", name, counts_only, ranged))
        ms.set_counts_only(counts_only)
        d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        n = len(text)
        ob = n // 3 if ranged else 0
        counts = ms.run(d.data_ptr(), n, own_begin=ob, own_end=n + 1) if ranged else ms.run(d.data_ptr(), n)
        torch.cuda.synchronize()
        for j, rx in enumerate(pats):
            whole = want.all(rx, text)
            if ms.how == 3:     # the one-kernel count: no list, the pointer NULL (looked at before anything is copied)
                assert ms.scan(j).device_spans_ptr() == 0, ("a list pointer after the one-kernel count", j, history)
            try:
                got = ms.scan(j).spans()
            except rj.RejitError:
                got = None
                assert counts_only, ("no list without counts-only", history)
            if ranged:
                assert got is None or fits_range(got, whole, rx, text, ob, n + 1, want), ("range", j, history)
                if got is not None:
                    assert counts[j] == len(got), history
            else:
                assert counts[j] == len(whole), (j, counts, len(whole), history)
                assert got is None or got == whole, ("stale list", j, len(got), len(whole), history)


# ---------------------------------------------------------------- a seeded random sequence


RANDOM_PATTERNS = [b"regexp", b"agggtaaa|tttaccct", b"(a|ab)(c|bcd)*", b"[a-f]+[0-9]", b"[acgt]+", b"\"[^\"]*\"", b"[a-z]+@[a-z]+",
                   b"[ab]{0,3}xyz[ab]+", b"(a|b)*abb", b".{0,2}.", b"#.*$", b"x*"]


def random_text(rng, n):
    kind = rng.randrange(6)
    if kind == 0:
        alphabet = bytes(range(256))
    elif kind == 1:
        alphabet = b"acgt"
    elif kind == 2:
        alphabet = b"abcdefgh xyz\n\"#@0123456789"
    elif kind == 3:
        alphabet = b"ab@cd@ef xyz"
    elif kind == 4:
        alphabet = b"\x80\xff\xc3ab\n"
    else:
        alphabet = b"x"
    t = bytearray(rng.choice(alphabet) for _ in range(n)) if n < 400 else bytearray(
        np.frombuffer(alphabet, dtype=np.uint8)[np.random.default_rng(rng.randrange(1 << 30)).integers(0, len(alphabet), n)].tobytes())
    every = rng.choice([0, 7, 300, 20000])
    if every and n:
        plant = rng.choice([b"regexp", b"agggtaaa", b"ab@cd@ef", b"axyzababxyz", b"\"q\"", b"# x\n", b"abb", b"acgtacgt"])
        for p in range(rng.randrange(every), max(n - len(plant), 0), every):
            t[p:p + len(plant)] = plant
    return bytes(t), "k%d/e%d" % (kind, every)


@pytest.mark.parametrize("seed", [20260, 20261])
def test_random_sequences(rj, oracle, seed):
    """Every route's pattern on one reused object, through random entries over random texts (sizes where paths switch,
    densities from every few bytes to none, bytes >= 0x80); the seed and the steps print on a failure."""
    rng = random.Random(seed)
    want = Want(oracle)
    sizes = [0, 1, 15, 16, 100, SMALL_MAX, SMALL_MAX + 1, 70001, WINDOW_RUNS - 1, WINDOW_RUNS + 1]
    for rx in RANDOM_PATTERNS:
        seq = Seq(rj, want, rx, seed=seed)
        for _ in range(12):
            n = rng.choice(sizes)
            text, name = random_text(rng, n)
            entry = rng.choice(Seq.ENTRIES)
            arg = None
            if entry == "halves":
                arg = rng.randrange(n + 1)
            elif entry in ("tail", "empty"):
                arg = rng.randrange(n + 1)
            elif entry == "h_batch":
                arg = [random_text(rng, rng.choice([0, 50, 3000]))[0]]
            seq.step(entry, text, arg, name=name)
