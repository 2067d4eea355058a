"""CPU test of the window sweep's case planner (tests/window_sweep.py): the schedule it restates from scan_windows_body, the
coverage that keeps tests/test_gpu_window_seams.py from quietly skipping the hard cases -- every (seam class x planted length x
offset) per family, every unguarded count as a wave before the last and as the last wave with one and two guarded chunks
behind it, every tail --, and the kernel variant (TWO, MASKED, TWOLEVEL, NIB) and K class each family claims, derived from the
lowering (tests/support/program_exec.cc: pe_plan) with the rules of engine.hip restated here."""
import ctypes
import os
import subprocess

import pytest

import window_sweep as W
from checkers import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "support", "libprogram_exec.so")
SRCS = [os.path.join(HERE, "support", "program_exec.cc"), os.path.join(ROOT, "rejit_amd", "csrc", "parser.cc"), os.path.join(ROOT, "rejit_amd", "csrc", "lowering.cc")]
_u64p = ctypes.POINTER(ctypes.c_uint64)
PLACES = ("before", "last1", "last2")


@pytest.fixture(scope="module")
def pe():
    deps = SRCS + [os.path.join(ROOT, "rejit_amd", "csrc", "lowering.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", SO] + SRCS)
    lib = ctypes.CDLL(SO)
    lib.pe_plan.restype = ctypes.c_int
    lib.pe_plan.argtypes = [ctypes.c_char_p, _u64p, ctypes.POINTER(ctypes.c_uint32)]
    return lib


def lowered(lib, rx):
    info = (ctypes.c_uint64 * 16)()
    vals = (ctypes.c_uint32 * 64)()
    assert lib.pe_plan(rx, info, vals) == 0, rx
    return dict(windows=bool(info[0]), n_windows=int(info[1]), offset=int(info[2]), behind=bool(info[11]), wlen=int(info[12]),
                values=[tuple(int(v) for v in vals[4 * i:4 * i + 4]) for i in range(int(info[1]))])


def variant_of(p):
    """engine.hip, rj_compile (window_alphabet, window_nibbles) and make_window_set, launch_scan_windows: the instantiation"""
    def byte(w, k, what):       # what: 0 value, 1 mask
        return ((w[what] >> (8 * k)) if k < 4 else (w[2 + what] >> (8 * (k - 4)))) & 0xFF
    wlen = p["wlen"]
    alphabet = {byte(w, k, 0) for w in p["values"] for k in range(wlen) if byte(w, k, 1)}
    nibbles_ok = len({b & 15 for b in alphabet}) == len(alphabet) and all(byte(w, k, 1) in (0, 0xFF) for w in p["values"] for k in range(8))
    masked = any(w[1] != 0xFFFFFFFF or (wlen > 4 and w[3] != 0xFFFFFFFF) for w in p["values"])
    two = wlen > 4
    two_level = len(alphabet) > 4
    nibble = two and not two_level and nibbles_ok
    if nibble:      # the nibble form's own mask: 4 bits per compared byte of the 8
        masked = any(not byte(w, k, 1) for w in p["values"] for k in range(8))
    return (two, masked, two and two_level, nibble)


@pytest.fixture(scope="module")
def planned():
    return {(name, grid): W.family_cases(name, grid) for name in W.FAMILIES for grid in W.GRIDS}


def every_plan(planned):
    plans = [c.plan for v in planned.values() for c in v[0]]
    for grid in W.GRIDS:
        for sweep in ["own", "busy", "multi"] + list(W.TAILS):
            plans += [c.plan for c in W.cases_of(sweep, grid)]
    return plans + list(W.anchor_plants()[0].values())


def test_schedule_invariants(planned):
    """Every chunk of [first_chunk, end_chunk) has one role in one wave; roles come in the kernel's order; the pipeline is entered
    exactly when F >= 8 and left through an epilogue with 1..4 plain chunks behind it; guarded chunks are exactly those at or
    above (n - 8) / 1024."""
    order = {r: i for i, r in enumerate(("S", "E", "P", "G"))}
    checked = 0
    for plan in every_plan(planned):
        seen = []
        for w in plan.waves:
            assert [c for c, _ in w.roles] == list(range(w.c0, w.c1))
            seen += [c for c, _ in w.roles]
            roles = [r for _, r in w.roles]
            stages = [order[r[0].upper()] for r in roles]
            assert stages == sorted(stages), roles
            piped = [r for r in roles if r in W.PIPE]
            assert bool(piped) == (w.fast >= 8), (w.fast, roles)
            if piped:
                assert len(piped) % 4 == 0 and piped == list(W.PIPE) * (len(piped) // 4)
                k = len(piped)
                assert roles[k:k + 3] == list(W.EPI)
                plain = [r for r in roles if r in ("P", "p")]
                assert 1 <= len(plain) <= 4 and set(plain) == {"P"}, roles
                assert len(piped) + 3 + len(plain) == w.fast
            else:
                assert not set(roles) & set(W.EPI + ("P",)) and roles.count("p") == w.fast
            guard = plan.n // W.CHUNK if plan.n < W.CHUNK + 8 else (plan.n - 8) // W.CHUNK
            for c, r in w.roles:
                assert (r == "G") == (c >= (0 if plan.n < W.CHUNK + 8 else guard)), (plan.n, c, r)
                if r != "G":        # an unguarded chunk and the 8 bytes behind it lie inside the text
                    assert (c + 1) * W.CHUNK + 8 <= plan.n
        assert seen == list(range(plan.first_chunk, plan.end_chunk)), (plan.n, plan.sb, plan.se)
        checked += 1
    assert checked > 1500


def test_two_guarded_chunks_need_a_short_window():
    """GG, SW:G, SG:G and the place `last2`: over every tail the launch has two guarded chunks exactly when window_len <= tail <= 7,
    so an 8-byte window never has them."""
    for wlen, offset in sorted({(f["wlen"], f["offset"]) for f in W.FAMILIES.values()}):
        two = [t for t in range(1024) if W.guarded_chunks(wlen, offset, t) == 2]
        assert two == list(range(wlen, 8)), (wlen, two)
        assert all(W.guarded_chunks(wlen, offset, t) == 1 for t in range(1024) if t not in two)


@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_every_seam_class_at_every_offset(planned, family):
    fam = W.FAMILIES[family]
    lengths = sorted({len(s) for s in fam["plants"]})
    seen, near_seen = W.Coverage(), W.Coverage()
    places, tails, empty, short_last = set(), set(), False, False
    bg = W.background(fam)
    for grid in W.GRIDS:
        cases, cover, near_cover = planned[(family, grid)]
        assert cases and W.text_count(family, grid) == len(cases)
        for into, c in ((seen, cover), (near_seen, near_cover)):
            for k, v in c.seen.items():
                into.seen[k] = into.seen.get(k, 0) + v
        for c in cases:
            assert 4 * W.CHUNK <= c.n <= W.MAX_TEXT + W.CHUNK and c.plan.grid == grid
            places |= c.plan.f_positions()
            tails.add(c.n % W.CHUNK)
            empty = empty or any(w.length == 0 for w in c.plan.waves)
            short_last = short_last or 0 < c.plan.busy()[-1].length < c.plan.span_chunks
            spans = sorted((p[0], p[0] + len(p[1])) for p in c.plants + c.near)
            assert all(b[0] - a[1] >= W.MIN_GAP for a, b in zip(spans, spans[1:])), c.label
            seams = dict(c.plan.seams())
            for start, s, tags, seam in c.plants + c.near:
                assert c.text[start:start + len(s)] == s and -len(s) <= start - seam <= 1 and seams[seam] == tags
            assert set(c.text) <= set(b"".join(fam["plants"] + fam["near"])) | {bg}
    short = fam["wlen"] <= 7
    classes = W.BASE_CLASSES + W.TAGGED + (("GG",) if short else ())
    if family == "chains":      # (three lengths of overlapping candidates: every class with every length, every offset of every length)
        for length in lengths:
            assert all(any(seen.count(t, length, k) for k in range(length + 2)) for t in classes), (length, [t for t in classes if not any(seen.count(t, length, k) for k in range(length + 2))])
            assert all(any(seen.count(t, length, k) for t in classes) for k in range(length + 2))
    else:
        assert seen.missing(lengths, tags=classes) == [], (family, seen.missing(lengths, tags=classes)[:12])
    assert all(k[2] == 0 for k in seen.seen if k[0] == "GE")                   # the end of the text: a string can only end there
    if short:
        assert any(seen.count(t, length, k) for t in ("SW:G",) for length in lengths for k in range(length + 2))
        assert any(seen.count(t, length, k) for t in ("SG:G",) for length in lengths for k in range(length + 2))
    else:
        assert not any(k[0] in ("GG", "SW:G", "SG:G") for k in seen.seen)
    want = {(f, p) for f in W.F_LIST for p in (PLACES if short else PLACES[:2])}
    assert want <= places, (family, sorted(want - places))
    assert tails >= set(W.tails_of(fam["wlen"])), (family, tails)
    assert empty and short_last
    for s in fam["near"]:       # every near miss is planted, at lane and chunk seams
        assert sum(near_seen.count(t, len(s), k) for t in W.BASE_CLASSES for k in range(len(s) + 2)) >= 20
    assert all(any(s in c.text for g in W.GRIDS for c in planned[(family, g)][0]) for s in fam["near"])


def test_variants_and_near_misses(pe):
    """Every family dispatches the instantiation its row claims; the eight (TWO, MASKED, TWOLEVEL, NIB) the launcher has and every K
    class are covered, the nibble form with an odd and an even K; no near miss matches, and a nibble alias is one."""
    oracle = Oracle()
    variants, classes, nib_k = set(), set(), set()
    for name, fam in W.FAMILIES.items():
        p = lowered(pe, fam["rx"])
        assert p["windows"] and not p["behind"], name
        assert (p["n_windows"], p["offset"], p["wlen"]) == (fam["K"], fam["offset"], fam["wlen"]), (name, p)
        assert variant_of(p) == fam["variant"], (name, variant_of(p))
        variants.add(fam["variant"])
        classes.add(W.K_CLASS[fam["K"]])
        if fam["variant"][3]:
            nib_k.add(W.K_CLASS[fam["K"]] & 1)
        bg = bytes([W.background(fam)]) * 40
        for s in fam["plants"]:
            assert oracle.match_all(fam["rx"], bg + s + bg), (name, s)
        for s in fam["near"]:
            assert oracle.match_all(fam["rx"], bg + s + bg) == [], (name, s)
            assert any(len(s) == len(q) and sum(a != b for a, b in zip(s, q)) == 1 for q in fam["plants"]) or name == "chains", (name, s)
        window_bytes = {b for w in p["values"] for k, b in enumerate(w[0].to_bytes(4, "little") + w[2].to_bytes(4, "little")) if k < p["wlen"]}
        for s in fam["alias"]:      # one byte of a matching string replaced by another with the same low nibble
            assert s in fam["near"] and any(len(q) == len(s) and [(a ^ b) for a, b in zip(s, q) if a != b] in ([0x10], [0x20], [0x30]) for q in fam["plants"]), (name, s)
        assert bool(fam["alias"]) == fam["variant"][3]
        if fam["variant"][3]:
            assert (bg[0] & 15) not in {b & 15 for b in window_bytes}
        assert bg[0] not in b"".join(fam["plants"] + fam["near"])
    assert variants == {(False, m, False, False) for m in (False, True)} | {(True, m, tl, nib) for m in (False, True) for tl, nib in ((True, False), (False, True), (False, False))}
    assert len(variants) == 8 and classes == {1, 2, 3, 4, 6, 8} and nib_k == {0, 1}
    for name, t in W.TAILS.items():
        p = lowered(pe, t["rx"])
        assert p["windows"] and (p["offset"], p["wlen"]) == t["window"] and p["behind"] == t["behind"], (name, p)


def test_own_busy_tails_multi_and_anchor():
    oracle = Oracle()
    own_seen = {}
    for grid in W.GRIDS:
        cases, covers = W.own_cases(grid)
        assert len(cases) >= 60 and W.text_count("own", grid) == len(cases)
        shapes = set()
        for c in cases:
            shapes.add((c.own[0] == 0, c.own[1] > c.n))
            assert c.plan.wlo == c.own[0] + W.FAMILIES[c.family]["offset"]
        assert shapes == {(False, True), (True, False), (False, False)}
        assert any(c.plan.first_chunk > 0 and c.plan.wlo % W.CHUNK for c in cases) and any(c.plan.whi % W.CHUNK and c.plan.end_chunk * W.CHUNK < c.n for c in cases)
        for name, (cover, _) in covers.items():
            into = own_seen.setdefault(name, W.Coverage())
            for k, v in cover.seen.items():
                into.seen[k] = into.seen.get(k, 0) + v
    for name in W.OWN_FAMILIES:     # sb / se under a planted string at every offset
        lengths = sorted({len(s) for s in W.FAMILIES[name]["plants"]})
        assert own_seen[name].missing(lengths, tags=("OWN",)) == [], (name, own_seen[name].missing(lengths, tags=("OWN",)))
    for grid in W.GRIDS:
        cases = W.cases_of("busy", grid)
        assert len(cases) == 2 * len(W.BUSY_FAMILIES) == W.text_count("busy", grid)
        for c in cases:
            needle = W.FAMILIES[c.family]["plants"][0]
            per_span = max(sum(c.text.count(needle, ch * W.CHUNK, (ch + 1) * W.CHUNK) for ch, _ in w.roles) for w in c.plan.waves)
            assert per_span > 64 and c.text.count(needle) > 16 * c.plan.n_regions       # a region overflows; the warm hint takes the two-launch gather
            assert set(c.lanes) >= {"S0", "S3", "E0", "E2", "P"}
            for role, ch in c.lanes.items():
                if (ch + 1) * W.CHUNK + 32 <= c.n and ch * W.CHUNK >= 32:
                    hit = {(m - ch * W.CHUNK) // 16 for m in range(ch * W.CHUNK, (ch + 1) * W.CHUNK) if c.text.startswith(needle, m)}
                    assert len(hit) >= 6 and {0, 62, 63} <= hit, (role, hit)
    for name, t in W.TAILS.items():
        classes = set()
        lengths = set()
        for grid in W.GRIDS:
            cases = W.cases_of(name, grid)
            assert cases and W.text_count(name, grid) == len(cases)
            for c in cases:
                classes |= {tag for p in c.plants for tag in p[2]}
                lengths |= {len(p[1]) for p in c.plants}
        assert set(W.BASE_CLASSES) <= classes, (name, set(W.BASE_CLASSES) - classes)
        assert lengths == {len(s) for s in t["plants"]}
        for s in t["plants"]:
            assert len(oracle.match_all(t["rx"], b"--" + s + b"--")) == 1
    for grid in W.GRIDS:
        cases = W.cases_of("multi", grid)
        assert cases and W.text_count("multi", grid) == len(cases)
        assert {tag for c in cases for p in c.plants for tag in p[2]} >= ({"S3E", "E2P", "PG", "SW"} | ({"SG"} if grid > 1 else set()))
        assert all(c.plan.span_chunks == max(-(-(-(-c.n // W.CHUNK)) // c.plan.n_regions), 1) for c in cases)
    plans, plants, cover = W.anchor_plants()
    for plan in plans.values():
        assert plan.grid == 272 and plan.span_chunks == 32 and {w.fast for w in plan.busy()[:-1]} == {32}
    for s in W.ANCHOR_STRINGS:
        got = {p[2][0] for p in plants if p[1] == s}
        assert got >= {"S01", "S12", "S23", "S30", "S3E", "E01", "E12", "E2P", "SW", "SG"}, (s, got)
    starts = sorted(p[0] for p in plants)
    assert len(plants) >= 300 and all(b - a > 64 for a, b in zip(starts, starts[1:]))
