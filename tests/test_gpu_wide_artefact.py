"""GPU tests (-m gpu) of at-risk patterns past the limits of the exact replay (tests/wide_artefact_cases.py: class A, the control,
within them; class B, rings of more than 448 slots; class C, automata of more than 1024 positions).  The promise tested: every
call answers with the reference's list, or fails with RJ_TOO_LARGE naming the ring artefact -- never the documented semantics
with RJ_OK where the reference differs -- and no call runs for longer than the one-lane budget (about 2 s) allows.
Expectations: tests/golden/wide_artefact_vectors.json (the real reference's answers) and Oracle.match_all live."""
import hashlib
import json
import os
import random
import time

import numpy as np
import pytest

import wide_artefact_cases as WA
from test_gpu_linear import gpu_spans_np, oracle_spans_np, rj, oracle  # noqa: F401  (fixtures)
from test_lowering import pe  # noqa: F401  (fixture: the CPU harness, for the lowering's edge counts)
from test_wide_artefact_fixture import ring_info

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CALL_LIMIT = 6.0       # s: one library call (the budgets are ~2-2.5 s of one-lane work; loose for a shared machine)
# engine_internal.h: one lane walks at most these units of work (bytes x one_lane_work) in a call
SEQUENTIAL_BUDGET = 7 << 26      # kSequentialBudget: exact_sequential over a whole text (more than 1024 positions)
REPLAY_LANE_BUDGET = 1 << 28     # kReplayLaneBudget: xr_replay, one lane per stretch (rings of more than 448 slots)
TOO_LARGE = -2
CASES = {c["name"]: c for c in WA.patterns()}


def fixture():
    with open(os.path.join(HERE, "golden", "wide_artefact_vectors.json")) as f:
        return json.load(f)


def digest(ms):
    h = hashlib.sha256()
    for b, e in ms:
        h.update(int(b).to_bytes(8, "little"))
        h.update(int(e).to_bytes(8, "little"))
    return h.hexdigest()


def call(rj, fn, *a, **kw):
    """(result, None) or (None, RejitError of status RJ_TOO_LARGE); any other error propagates; the call's wall clock is bounded."""
    t0 = time.perf_counter()
    try:
        out, err = fn(*a, **kw), None
    except rj.RejitError as e:
        assert e.status == TOO_LARGE and "ring artefact" in e.message, e
        out, err = None, e
    dt = time.perf_counter() - t0
    assert dt < CALL_LIMIT, (getattr(fn, "__name__", fn), dt)
    return out, err


def device(text):
    import torch
    return torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()


def as_pairs(x):
    return [tuple(int(v) for v in p) for p in x]


def one_lane_work(pe, rx):  # noqa: F811
    """engine_internal.h: one_lane_work -- slots + 64 x byte edges + 2 x control edges^2 per text byte"""
    info = ring_info(pe, rx)
    return info["slots"] + 64 * info["byte_edges"] + 2 * info["control_edges"] ** 2


def over_budget(pe, c, n_bytes):  # noqa: F811
    """may a call over n_bytes of text be refused by the rule?  Only when one lane over all of them is more work than the
    budget of the path the pattern's class takes"""
    budget = SEQUENTIAL_BUDGET if c["cls"] == "C" else REPLAY_LANE_BUDGET
    return c["cls"] != "A" and n_bytes * one_lane_work(pe, c["regex"].encode()) > budget


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_cases_through_every_entry(rj, pe, name):  # noqa: F811
    """Scan.run_tensor on device text, host match_all / match_first / match_full, and a two-pattern rj_multi_run set: the
    reference's answer, or RJ_TOO_LARGE -- which class A, texts of up to 16 KiB and texts whose one-lane work is within the
    budget never get."""
    import torch
    t_test = time.perf_counter()
    c = CASES[name]
    rx = c["regex"].encode()
    cls = c["cls"]
    prog = rj.Program(rx)
    assert prog.info()["ring_artefact_risk"] == 1
    lit = rj.Program(b"ba\n")
    refused = 0
    for k in [k for k in fixture()["cases"] if k["name"] == name]:
        text = WA.make_text(c, k["size"], k["kind"])
        assert hashlib.sha256(text).hexdigest() == k["text_sha256"]
        may_refuse = k["size"] > (16 << 10) and over_budget(pe, c, k["size"])
        where = (name, k["size"], k["kind"])

        def check(got, err, what):
            nonlocal refused
            if err is not None:
                assert may_refuse, (where, what, err)
                assert "budget" in err.message, (where, what, err)
                refused += 1
                return
            if what == "first":
                assert (list(got) if got else None) == k["all_first"], (where, what, got)
            else:
                assert len(got) == k["count"] and digest(got) == k["spans_sha256"], (where, what, len(got), k["count"])

        d = device(text)
        scan = rj.Scan(prog)
        cnt, err = call(rj, scan.run_tensor, d)
        check(None if err else as_pairs(gpu_spans_np(rj, scan)), err, "run_tensor")
        got, err = call(rj, prog.match_all, text)
        check(got, err, "match_all")
        got, err = call(rj, prog.match_first, text)
        check(got, err, "first")
        got, err = call(rj, prog.match_full, text)
        assert err is None and int(got) == k["full"], (where, "match_full")
        multi = rj.MultiScan([prog, lit])
        counts, err = call(rj, multi.run, d.data_ptr(), len(text), stream=torch.cuda.current_stream().cuda_stream)
        check(None if err else as_pairs(multi.scan(0).spans()), err, "rj_multi_run")
        if err is None:
            assert counts[0] == k["count"] and counts[1] == text.count(b"ba\n"), (where, counts)
    assert time.perf_counter() - t_test < 60


def planted(c, n, seed, spread):
    """Texts of megabytes like test_gpu_exact.py::test_wide_at_risk_automaton_beyond_1mib: words planted over `abcd\\n`, some
    back to back ('spread': on lines of their own, so that no candidate begins where another ends)."""
    if spread:
        return WA.make_text(c, n, "spread", seed=seed)
    rng = np.random.default_rng(seed)
    buf = bytearray(np.frombuffer(b"abcd\n", dtype=np.uint8)[rng.integers(0, 5, size=n)].tobytes())
    r2 = random.Random(seed)
    for _ in range(n // 1000):
        w = r2.choice(c["pieces"]).encode()
        at = r2.randrange(0, n - 40)
        buf[at:at + len(w)] = w
        if r2.random() < 0.5:
            w2 = r2.choice(c["pieces"]).encode()
            buf[at + len(w):at + len(w) + len(w2)] = w2
    return bytes(buf)


@pytest.mark.parametrize("size", [2 << 20, 6 << 20])
def test_class_c_beyond_1mib(rj, oracle, size):
    """A class C pattern over 2 and 6 MiB: where the artefact arises the reference's answer or RJ_TOO_LARGE, never another list
    with RJ_OK (until this test the documented semantics came back silently); with the words spread apart RJ_OK and exact."""
    t_test = time.perf_counter()
    c = CASES["C_words140"]
    rx = c["regex"].encode()
    for spread in (False, True):
        text = planted(c, size, 5, spread)
        t = np.frombuffer(text, dtype=np.uint8)
        want = oracle_spans_np(oracle, rx, t)
        spec = oracle_spans_np(oracle, rx, t, spec=True)
        assert len(want) > 1000
        assert (len(want) != len(spec) or not np.array_equal(want, spec)) != spread, "the text should (not) hit the artefact"
        scan = rj.Scan(rj.Program(rx))
        cnt, err = call(rj, scan.run_tensor, device(text))
        if spread:
            assert err is None, err
        if err is None:
            got = gpu_spans_np(rj, scan)
            assert cnt == len(want) and np.array_equal(got, want), (size, spread, cnt, len(want), len(spec))
        got, err = call(rj, rj.Program(rx).match_all, text)
        if spread:
            assert err is None, err
        if err is None:
            assert np.array_equal(np.array(got, dtype=np.uint64).reshape(-1, 2), want), (size, spread, "match_all")
    assert time.perf_counter() - t_test < 60


def run_ranges_or_refuse(rj, scan, d, cuts):
    parts, refused = [], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cnt, err = call(rj, scan.run_tensor, d, own_begin=lo, own_end=hi)
        if err is not None:
            refused += 1
            parts.append(None)
        else:
            parts.append(gpu_spans_np(rj, scan).copy())
    return parts, refused


@pytest.mark.parametrize("name,size,kind", [("C_words140", 16 << 10, "adjacent"), ("C_words140", 2 << 20, "spread"),
                                            ("C_words140", 64 << 10, "adjacent"), ("B_dot8_lit4", 64 << 10, "adjacent"),
                                            ("B_nested_anchors", 64 << 10, "adjacent")])
def test_own_ranges(rj, oracle, name, size, kind):
    """Ranges of a sharded run (sharding.visible_range(..., whole_text=True): every rank holds the whole text), 2 and 3 of them:
    each range exact or RJ_TOO_LARGE; when all answer their concatenation is the whole text's answer.  Class C ranges own the
    matches that begin in them (checked one by one); class B ranges own whole segments between synchronisation points."""
    from rejit_amd import sharding
    t_test = time.perf_counter()
    c = CASES[name]
    rx = c["regex"].encode()
    text = WA.make_text(c, size, kind) if size <= (64 << 10) else planted(c, size, 7, kind == "spread")
    n = len(text)
    assert sharding.visible_range(n, (n // 3, n // 2), None, whole_text=True) == (0, n)
    want = oracle_spans_np(oracle, rx, np.frombuffer(text, dtype=np.uint8))
    d = device(text)
    scan = rj.Scan(rj.Program(rx))
    answered = 0
    for cuts in ([0, n // 2 + 7, n + 1], [0, n // 3, 2 * n // 3 + 5, n + 1]):
        parts, refused = run_ranges_or_refuse(rj, scan, d, cuts)
        for (lo, hi), got in zip(zip(cuts[:-1], cuts[1:]), parts):
            if got is not None and c["cls"] == "C":
                own = want[(want[:, 0] >= lo) & (want[:, 0] < hi)] if len(want) else want
                assert np.array_equal(got, own), (name, size, kind, lo, hi, len(got), len(own))
        if refused == 0:
            assert np.array_equal(np.concatenate(parts), want), (name, size, kind, cuts)
            answered += 1
    if not (c["cls"] == "C" and size > (16 << 10) and kind == "adjacent"):
        assert answered == 2, (name, size, kind)     # (ranges that can answer do: refusing every range is no answer)
    assert time.perf_counter() - t_test < 60


def test_class_b_stretch_beyond_16mib(rj, oracle):
    """A ring of 650 slots over 20 MiB without a synchronisation point (`.` keeps a thread alive at every byte of a text without
    line breaks): more than the 16 MiB that were the one-lane replay's former limit, where the documented semantics came back silently.
    The reference's answer or RJ_TOO_LARGE, and a refusal within seconds."""
    t_test = time.perf_counter()
    c = CASES["B_dot8_lit4"]
    rx = c["regex"].encode()
    n = 20 << 20
    rng = np.random.default_rng(11)
    buf = bytearray(np.frombuffer(b"ab", dtype=np.uint8)[rng.integers(0, 2, size=n)].tobytes())
    r2 = random.Random(11)
    for at in range(0, n - 300, 4093):
        w = (r2.choice(c["pieces"]) + r2.choice(c["pieces"])).encode()
        buf[at:at + len(w)] = w
    text = bytes(buf)
    scan = rj.Scan(rj.Program(rx))
    t0 = time.perf_counter()
    cnt, err = call(rj, scan.run_tensor, device(text))
    if err is not None:
        assert time.perf_counter() - t0 < 10.0
        assert "448" in err.message or "budget" in err.message, err.message
    else:
        want = oracle_spans_np(oracle, rx, np.frombuffer(text, dtype=np.uint8))
        assert cnt == len(want) and np.array_equal(gpu_spans_np(rj, scan), want)
    assert time.perf_counter() - t_test < 60


@pytest.mark.parametrize("adjacent", [False, True])
def test_class_b_range_past_the_replay(rj, oracle, adjacent):
    """Ranges of a class B pattern over 1 MiB without a synchronisation point (`.` keeps a thread alive at every byte of a text
    without line breaks): the range replay would be more one-lane work than a call's budget, so the range is served from the
    text's beginning (engine.hip: the replay's own segments, then keep_begins) -- exact where no candidate begins where another
    ends, RJ_TOO_LARGE where one does and no replay can take the whole text."""
    t_test = time.perf_counter()
    c = CASES["B_dot8_lit4"]
    rx = c["regex"].encode()
    n = 1 << 20
    rng = np.random.default_rng(13)
    buf = bytearray(np.frombuffer(b"ab", dtype=np.uint8)[rng.integers(0, 2, size=n)].tobytes())
    r2 = random.Random(13)
    for at in range(100, n - 300, 997):
        w = (r2.choice(c["pieces"]) + (r2.choice(c["pieces"]) if adjacent else "")).encode()
        buf[at:at + len(w)] = w
    text = bytes(buf)
    t = np.frombuffer(text, dtype=np.uint8)
    want = oracle_spans_np(oracle, rx, t)
    spec = oracle_spans_np(oracle, rx, t, spec=True)
    assert len(want) > 500 and (len(want) != len(spec) or not np.array_equal(want, spec)) == adjacent
    d = device(text)
    scan = rj.Scan(rj.Program(rx))
    cnt, err = call(rj, scan.run_tensor, d)
    assert (err is not None) == adjacent, err          # (whole text: 1 MiB on one lane is over the budget)
    if err is None:
        assert cnt == len(want) and np.array_equal(gpu_spans_np(rj, scan), want)
    for cuts in ([0, n // 2 + 7, n + 1], [0, n // 3, 2 * n // 3 + 5, n + 1]):
        parts, refused = run_ranges_or_refuse(rj, scan, d, cuts)
        if adjacent:
            assert refused > 0, cuts
        else:
            assert refused == 0 and np.array_equal(np.concatenate(parts), want), cuts
    assert time.perf_counter() - t_test < 60
