"""CPU tests of tests/golden/wide_artefact_vectors.json: at-risk patterns past the limits of the exact replay (classes A, B, C of
tests/wide_artefact_cases.py), the real reference's answers over seeded texts.  Each case's class is CHECKED from the lowering
(tests/support/program_exec.cc: pe_ring_info), the texts regenerate from their seed, the oracle reproduces every answer, and a
third of the B and C texts at least hit the ring artefact (the reference differs from the documented semantics there)."""
import ctypes
import hashlib
import json
import os

import pytest

import wide_artefact_cases as WA
from checkers import Oracle
from test_lowering import pe  # noqa: F401  (fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "wide_artefact_vectors.json")


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def digest(ms):
    h = hashlib.sha256()
    for b, e in ms:
        h.update(int(b).to_bytes(8, "little"))
        h.update(int(e).to_bytes(8, "little"))
    return h.hexdigest()


def ring_info(lib, rx: bytes):
    lib.pe_ring_info.restype = ctypes.c_int
    lib.pe_ring_info.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    a = (ctypes.c_uint64 * 8)()
    assert lib.pe_ring_info(rx, a) == 0, rx
    return dict(n_pos=int(a[0]), n_words=int(a[1]), slots=int(a[2]), risk=int(a[5]), byte_edges=int(a[6]), control_edges=int(a[7]))


def test_every_case_sits_in_its_class(pe):  # noqa: F811
    fx = load()
    assert fx["seed"] == WA.SEED
    assert [p["regex"] for p in fx["patterns"]] == [c["regex"] for c in WA.patterns()]
    per_class = {}
    for p in fx["patterns"]:
        info = ring_info(pe, p["regex"].encode())
        assert info["risk"] == 1, (p["name"], info)
        assert WA.classify(info["n_pos"], info["n_words"], info["slots"]) == p["cls"], (p["name"], info)
        if p["cls"] == "B":
            assert info["n_pos"] <= 1024 and info["slots"] > WA.WALK_SLOTS
        if p["cls"] == "C":
            assert info["n_pos"] > 1024
        per_class[p["cls"]] = per_class.get(p["cls"], 0) + 1
    assert all(per_class.get(c, 0) >= 4 for c in "ABC"), per_class


def test_oracle_reproduces_every_reference_answer():
    fx = load()
    oracle = Oracle()
    cases = {c["name"]: c for c in WA.patterns()}
    assert len(fx["cases"]) == len(cases) * len(WA.SIZES) * len(WA.KINDS)
    quirks = []
    for k in fx["cases"]:
        c = cases[k["name"]]
        rx = c["regex"].encode()
        text = WA.make_text(c, k["size"], k["kind"])
        assert hashlib.sha256(text).hexdigest() == k["text_sha256"], (k["name"], k["size"], k["kind"])
        want = oracle.match_all(rx, text)
        assert len(want) == k["count"] and digest(want) == k["spans_sha256"], (k["name"], k["size"], k["kind"], len(want), k["count"])
        first = oracle.match_first(rx, text)
        assert (list(first) if first else None) == k["all_first"], (k["name"], k["size"], k["kind"])
        if k["first"] != k["all_first"]:
            # (the reference's own MatchFirst disagrees with its MatchAll on one input here; this project's MatchFirst is
            # documented as the first match of the exact MatchAll)
            quirks.append((k["name"], k["size"], k["kind"]))
        assert oracle.match_full(rx, text) == k["full"], (k["name"], k["size"], k["kind"])
        assert ([tuple(x) for x in oracle.match_all_spec(rx, text)] != [tuple(x) for x in want]) == k["spec_differs"]
    assert quirks == [("B_class6_lit6", 16384, "spread")], quirks


def test_the_artefact_is_exercised():
    fx = load()
    cls = {p["name"]: p["cls"] for p in fx["patterns"]}
    wide = [k for k in fx["cases"] if cls[k["name"]] in "BC"]
    hit = [k for k in wide if k["spec_differs"]]
    assert 3 * len(hit) >= len(wide), (len(hit), len(wide))
    for c in "BC":
        assert any(k["spec_differs"] for k in wide if cls[k["name"]] == c), c
    # texts where the two agree too, and the 'spread' texts are such texts
    assert all(not k["spec_differs"] for k in fx["cases"] if k["kind"] == "spread")
    assert os.path.getsize(FIXTURE) < 256 << 10
