"""CPU test of the run sweep's case planner (tests/run_sweep.py): the coverage that keeps tests/test_gpu_run_seams.py from quietly
skipping the hard cases.

* The geometry the planner restates: its constants are those of run_scan.hip / kernels.h, the two overrides it sets are read there by
  name, every byte of a text lies in exactly one iteration of one tile.
* Every seam class a configuration can have is planted at every (motif length x offset); every ordered pair of tile kinds meets
  across a seam of every resolve class, and with a quiet stretch between the two that covers a whole thread chunk / block; the own
  sweep holds every (seam, d, mode).  Nothing is left out: uncovered count = 0, asserted.
* Every family's plan is what the planner claims (tests/support/program_exec.cc: pe_run_plan -> make_run_plan): the families cover
  the NR classes 1 / 2 / 4 / 8 x HAS_B of run_summary / run_emit, every plan flag, and the pair kernels at NR 1 / 2 / 4 / 8.
* A byte-level classifier of a tile's kind, written from the classes and not from the generator, agrees with the generator.
* The expected answers are pinned twice before a GPU is involved: the CPU walk of the segment rule / the pair rule
  (pe_run_match_all, pe_pair_match_all) equals the oracle on the intra-tile texts of one configuration per family."""
import ctypes
import hashlib
import os
import re
import subprocess

import pytest

import run_sweep as R
from checkers import Oracle
from test_lowering import ROOT, SO, SRCS

_u64p = ctypes.POINTER(ctypes.c_uint64)
PLAN_FLAGS = ("lag", "bol", "eol", "a_neg", "l_neg", "b_neg", "high")
RESOLVE_CLASSES = {"RC", "RI", "R4", "BK", "BKR", "TC", "TI"}


@pytest.fixture(scope="module")
def pe():
    deps = SRCS + [os.path.join(ROOT, "rejit_amd", "csrc", h) for h in ("lowering.h", "exact_count.h", "table_layout.h", "run_scan.h", "dense_streams.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", SO] + SRCS)
    lib = ctypes.CDLL(SO)
    lib.pe_run_plan.restype = ctypes.c_int
    lib.pe_run_plan.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.pe_run_match_all.restype = ctypes.c_long
    lib.pe_run_match_all.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, _u64p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
    lib.pe_pair_match_all.restype = ctypes.c_long
    lib.pe_pair_match_all.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, _u64p, ctypes.c_uint64]
    return lib


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def intra():
    return {(config, name): R.intra_cases(config, name) for config in R.INTRA_CONFIGS for name in R.FAMILIES}


def plan_of(pe, rx):
    info = (ctypes.c_uint32 * 11)()
    assert pe.pe_run_plan(rx, info) == 0, rx
    return dict(zip(("ok", "pair", "has_b", "n_ranges") + PLAN_FLAGS, (int(x) for x in info)))


def source(*path):
    with open(os.path.join(ROOT, *path)) as fh:
        return fh.read()


def test_constants_and_overrides_are_the_code_s():
    hip = source("rejit_amd", "csrc", "run_scan.hip")
    for name in (R.ENV_TILE, R.ENV_LEVELS):
        assert 'getenv("%s")' % name in hip, name
    engine = source("rejit_amd", "csrc", "engine.hip")
    for name in ("RJ_NO_SMALL", "RJ_RUNS_FIRST"):
        assert 'getenv("%s")' % name in engine, name
    assert re.search(r"kIterBytes = (\d+);", hip).group(1) == str(R.ITER)
    assert re.search(r"kBlockTiles = (\d+);", hip).group(1) == str(R.BLOCK_TILES)
    assert re.search(r"kOneLevelTiles = (\d+);", hip).group(1) == str(R.ONE_LEVEL_TILES)
    assert re.search(r"span <= \(256ull << 20\) \? kRunTile : 4 \* kRunTile", hip)
    assert re.search(r"kRunTile = (\d+);", source("rejit_amd", "csrc", "kernels.h")).group(1) == "8192"
    assert "blocks <= 1024) hipLaunchKernelGGL(pair_resolve_blocks<256>" in hip
    # the accessor: exported by the library, test support, in no public header
    assert 'extern "C" void rj_test_run_geometry(' in hip
    for header in ("rejit.h", "rejit_hip.h"):
        assert "rj_test_run_geometry" not in source("include", header)
    assert R.Geo(1 << 20).tile_bytes == 8192 and R.Geo((256 << 20) + 1).tile_bytes == 32768 and R.Geo(1 << 20, 0, 5).tile_bytes == 4096
    assert R.Geo(8192 * 4096 - 1).levels == 1 and R.Geo(8192 * 4096).levels == 2 and R.Geo(5000, 0, 2, 3).levels == 2
    g = R.Geo(100000, 30000, 2)
    assert g.accessor() == (2048, 14, 35, 1024, 1) and g.base(0) == 28672


def test_every_byte_has_one_iteration(intra):
    for (config, name), (cases, _) in intra.items():
        if name not in ("a.*b", "p2"):
            continue
        for c in cases:
            g = c.geo
            assert g.n == c.n and g.first_tile == 0 and g.n_tiles == c.n // g.tile_bytes + 1 and g.levels == 1 and g.C == 1
            assert g.tile_bytes == {"t2": 2048, "default": 8192, "t32": 32768}[config] and c.n <= R.MAX_TEXT
            live = [(t, it) for t in range(g.n_tiles) for it in range(g.iters) if g.iteration(t, it) != "skipped"]
            assert [g.base(t) + it * R.ITER for t, it in live] == list(range(0, c.n + 1, R.ITER))      # position n included
            guarded = [x for x in live if g.iteration(*x) == "guarded"]
            assert guarded == live[-1:]           # the iteration that holds the text's end, and no other
            for pos, tags in g.seams():
                assert 0 < pos <= c.n and tags


@pytest.mark.parametrize("config", R.INTRA_CONFIGS)
def test_every_seam_class_at_every_offset(intra, config):
    classes = R.INTRA_CLASSES[config] + R.GE_CLASSES
    for name, fam in R.FAMILIES.items():
        cases, cover = intra[(config, name)]
        assert R.missing(cover, classes) == [], (config, name, R.missing(cover, classes)[:12])
        lengths = sorted({len(p[1]) for c in cases for p in c.plants})
        assert tuple(lengths) == R.MOTIF_LENGTHS == tuple(sorted({len(m) for m in R.MOTIFS}))
        produced = {t for c in cases for _, tags in c.geo.seams() for t in tags}
        assert produced == set(classes), (config, produced ^ set(classes))      # the table names what the geometry has, no more, no less
        for c in cases:
            seams = dict(c.geo.seams())
            for start, s, tags, seam in c.plants:
                assert c.text[start:start + len(s)] == s and -len(s) <= start - seam <= 1 and set(tags) <= set(seams[seam])
        used = {p[1] for c in cases for p in c.plants}
        assert used == {fam.bytes_of(m, k) for k, m in enumerate(R.MOTIFS)}, name       # every motif is planted
        dense = cases[0]
        assert "dense" in dense.label and not dense.plants
        if not fam.pair:        # a break every two to three bytes
            breaks = [i for i, b in enumerate(dense.text) if b in fam.sets[2][1]]
            assert breaks[0] <= 3 and max(b - a for a, b in zip(breaks, breaks[1:])) <= 3, name
    # t4 is the own sweep's: its classes are named too
    g = R.Geo(5 * 4096 + 2048 + 77, 0, 4)
    assert {t for _, tags in g.seams() for t in tags} - set(R.GE_CLASSES) == set(R.INTRA_CLASSES["t4"])


def test_text_counts_are_deterministic(intra):
    for sweep, config in (("intra:1", "t2"), ("intra:7", "t32")):
        if sweep.startswith("intra"):
            assert R.text_count(sweep, config) == sum(len(intra[(config, n)][0]) for n in R.families_of(sweep, config)) > 0
    assert R.text_count("own:0", "t4") == R.text_count("own:0", "t4") == len(R.OWN_FAMILIES) // 2 * len(R.own_cases("t4", "a.*b")) == 4 * (176 + 8)
    assert R.text_count("level:pairs", "l5") == R.text_count("level:pairs", "l5") > 0
    digest = [hashlib.sha256(b"".join(c.text for c in R.cases_of(s, c_, n))).hexdigest() for _ in range(2)
              for s, c_, n in (("intra:0", "t2", "a.*b"), ("level:runsA", "l3", "a[bc]*"), ("own:0", "t2", "#.+"))]
    assert digest[:3] == digest[3:]
    assert len(R.sweeps()) + 1 <= 50 and len(set(R.sweeps())) == len(R.sweeps())
    for config in R.INTRA_CONFIGS:
        assert sorted(n for s, c in R.sweeps() if s.startswith("intra") and c == config for n in R.families_of(s, c)) == sorted(R.FAMILIES)
    assert sorted(n for s, c in R.sweeps() if s.startswith("own") and c == "t4" for n in R.families_of(s, c)) == sorted(R.OWN_FAMILIES)


def test_family_plans_and_kernel_instantiations(pe, oracle):
    """run_summary / run_emit <NR, HAS_B> and pair_summary / pair_emit <NR>: every instantiation has a family, every flag too."""
    runs, pairs, flags_seen = set(), set(), {}
    for name, fam in R.FAMILIES.items():
        p = plan_of(pe, fam.rx)
        assert (p["ok"], p["pair"]) == ((0, 1) if fam.pair else (1, 0)), (name, p)
        assert p["has_b"] == int(fam.has_b) and R.nr_class(p["n_ranges"]) == fam.nr, (name, p)
        got = {f for f in PLAN_FLAGS if p[f]}
        assert got == set(fam.flags) - {"a_break", "b_break"}, (name, got, fam.flags)
        if fam.pair:
            pairs.add((fam.nr, fam.reset))
        else:
            runs.add((fam.nr, fam.has_b))
            for f in got:
                flags_seen.setdefault(f, set()).add(fam.has_b)
            if got >= {"bol", "eol"}:
                flags_seen.setdefault("bol+eol", set()).add(fam.has_b)
        A, B, l = bytes([fam.byte("A")]), bytes([fam.byte("B")]), bytes([fam.byte("l")])
        if "a_break" in fam.flags and not set(fam.flags) & {"lag", "bol", "eol"}:      # the A byte is itself a break: a match begins ON the break
            assert 2 in [m[0] for m in oracle.match_all(fam.rx, l + A + A + l + B + bytes([fam.byte("n")]))], name
        if "b_break" in fam.flags and not fam.pair:      # B may be the break: the match ends behind the FIRST B
            assert oracle.match_all(fam.rx, A + l + B + l + B)[0] == (0, 3), name
        if fam.pair:                    # a reset drops the open Q
            r = bytes([fam.byte("r")])
            assert oracle.match_all(fam.rx, A + l + r + A + l + A) == ([(3, 6)] if fam.reset else [(0, 4)]), name
    assert runs == {(nr, b) for nr in (1, 2, 4, 8) for b in (False, True)}, runs
    assert {nr for nr, _ in pairs} == {1, 2, 4, 8} and {r for _, r in pairs} == {True, False}, pairs
    assert flags_seen["lag"] == {False, True} and flags_seen["bol"] == {False, True}
    assert set(flags_seen) == set(PLAN_FLAGS) | {"bol+eol"}, flags_seen
    for group in R.LEVEL_GROUPS.values():
        for name in group:      # the level sweep's symbols are four different bytes: a tile's kind can be read from its bytes
            fam = R.FAMILIES[name]
            assert len({fam.byte("l")} | {b for _, s in fam.sets for b in s}) == 1 + sum(len(s) for _, s in fam.sets if not fam.pair or _ != "B"), name
    level = {f for g in R.LEVEL_GROUPS.values() for n in g for f in R.FAMILIES[n].flags}
    assert level >= {"lag", "bol", "eol", "a_break", "l_neg"}       # (eol: a first break that counts nothing -- Elem::hb == 2)


def walk(pe, fam, text):
    cap = len(text) + 2
    out = (ctypes.c_uint64 * (2 * cap))()
    if fam.pair:
        k = pe.pe_pair_match_all(fam.rx, text, len(text), out, cap)
    else:
        k = pe.pe_run_match_all(fam.rx, text, len(text), out, cap, (ctypes.c_uint32 * 4)())
    assert k >= 0, (fam.rx, k)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(k)]


def test_cpu_walk_equals_oracle_on_the_intra_texts(pe, oracle, intra):
    for i, (name, fam) in enumerate(R.FAMILIES.items()):
        config = R.INTRA_CONFIGS[i % len(R.INTRA_CONFIGS)]
        total = 0
        for c in intra[(config, name)][0]:
            want = oracle.match_all(fam.rx, c.text)
            assert walk(pe, fam, c.text) == want, (name, c.label)
            total += len(want)
        assert total > 1000, (name, total)      # (the dense text alone has thousands)


KIND_SETS = {"runs": ("a.*b", R.RUN_KINDS), "pairs": ("p2", R.pair_kinds(True)), "pairs, no reset": ("p1", R.pair_kinds(False))}


@pytest.mark.parametrize("config", list(R.LEVEL_TILES))
def test_every_kind_pair_across_every_resolve_class(config):
    assert len(R.RUN_KINDS) == 16 and len(R.pair_kinds(True)) == 14 and len(R.pair_kinds(False)) == 6
    for what, (name, kinds) in KIND_SETS.items():
        fam = R.FAMILIES[name]
        assert R.kinds_of(fam) == kinds
        texts = R.level_sequences(config, kinds, fam.pair)
        seen = R.level_coverage(texts)
        req = R.level_requirements(config, kinds)
        uncovered = [r for r in req if (r[1], r[2]) not in seen.get(r[0], ())]
        assert uncovered == [], (config, what, len(uncovered), uncovered[:8])
        # the table names the resolve classes the geometry has, no more, no less
        assert set(seen) & RESOLVE_CLASSES == set(R.LEVEL_CLASSES[config]), (config, set(seen) & RESOLVE_CLASSES)
        full = [c for c in R.LEVEL_CLASSES[config] if c not in R.LEVEL_REDUCED.get(config, {})]
        assert full and all(seen[c] >= {(a, b) for a in kinds for b in kinds} for c in full)
        busy = [k for k in kinds if k != "E"]
        if "chunk" not in R.LEVEL_REDUCED.get(config, {}):
            assert seen["chunk"] >= {(a, b) for a in busy for b in busy}
        if config in ("l1", "l3", "l5"):
            assert seen["block"] >= {(a, b) for a in busy for b in busy}
        for c, how in R.LEVEL_REDUCED.get(config, {}).items():
            if how == "sides":
                assert {a for a, _ in seen[c]} >= set(kinds) and {b for _, b in seen[c]} >= set(kinds), (config, c)
        for geo, seq in texts:
            assert geo.tile_bytes == R.ITER and len(seq) == geo.n_tiles and seq[-1] == "E" and geo.n <= (8 << 20) + 40 * R.ITER
            assert (geo.levels == 2) == config.startswith("l") and set(seq) <= set(kinds)
    geos = [R.level_geo(config, t, pair) for t in R.LEVEL_TILES[config] for pair in (False, True)]
    shapes = {(g.C,) + g.busy_threads() for g in geos}
    if config.startswith("c"):
        want = {"c1": (1, 700, False), "c2": (2, 1024, True), "c3": (3, 1000, False), "c4": (4, 1023, True)}[config]
        assert want in shapes, shapes      # C; threads that own a tile (of 1024); a ragged last thread
    if config == "l1":
        assert all(g.top_C == 5 and g.top_T == 1024 and g.n_blocks > 4096 for g in geos)       # more blocks than threads: pair_resolve_blocks<1024>
    if config in ("l3", "l5"):
        assert all(g.top_C == 1 and g.n_blocks <= 256 for g in geos) and {g.top_T for g in geos} == {256, 1024}
    if config == "l300":
        assert all(g.C == 2 and g.busy_threads()[0] == 150 for g in geos)       # 106 idle threads in a block
    if config == "l1024":
        assert all(g.C == 4 and g.n_blocks == 4 and g.block_size(3) == 500 for g in geos)        # three blocks and a ragged one


def test_classifier_agrees_with_the_generator():
    checked = 0
    groups = list(R.LEVEL_GROUPS.values())
    picks = [(c, groups[i % len(groups)][i % 2]) for i, c in enumerate(R.LEVEL_TILES)]       # a family of every configuration, every family at l3
    picks += [("l3", n) for g in R.LEVEL_GROUPS.values() for n in g]
    for config, name in sorted(set(picks)):
        fam = R.FAMILIES[name]
        seen = set()
        for c in R.level_cases(config, name):
            tb = c.geo.tile_bytes
            for t, kind in enumerate(c.seq[:-1]):
                assert R.classify_tile(fam, c.text[t * tb:(t + 1) * tb]) == kind, (config, name, t, kind)
                seen.add(kind)
                checked += 1
            assert R.classify_tile(fam, c.text[(len(c.seq) - 1) * tb:]) == "E"
        assert seen == set(R.kinds_of(fam)), (config, name)
    assert checked > 50000
    for name in R.ANCHOR_FAMILIES:
        fam = R.FAMILIES[name]
        c = R.anchor_case(name)
        g = c.geo
        assert g.accessor() == (8192, 0, R.ANCHOR_TILES, 1024, 2) and (32 << 20) < c.n < (33 << 20)
        assert all(R.classify_tile(fam, c.text[t * 8192:(t + 1) * 8192]) == k for t, k in enumerate(c.seq[:-1]))
        crossed = {}
        for t in range(g.n_tiles - 2):
            if c.seq[t] != "E" and c.seq[t + 1] != "E":
                for tag in g.boundary_tags(t):
                    crossed[tag] = crossed.get(tag, 0) + 1
        assert crossed["BK"] == 3 and crossed["BKR"] == 1 and min(crossed[t] for t in ("RC", "RI", "TG", "TW", "TC")) >= 4, crossed


@pytest.mark.parametrize("config", R.OWN_CONFIGS)
def test_own_and_carry_cases(oracle, config):
    firsts, blocked, early, far = set(), 0, 0, 0
    for name in R.OWN_FAMILIES:
        fam = R.FAMILIES[name]
        assert not fam.pair         # (the pair kernels take whole texts only: run_pairs)
        cases = R.own_cases(config, name)
        seams = [tag for tag, _ in R.own_seams(R.Geo(cases[0].n, 0, *R.CONFIGS[config]))]
        assert {(c.seam_tag, c.d, c.mode) for c in cases} == ({(s, d, m) for s in seams for d in R.OWN_D for m in R.OWN_MODES}
                                                               | {(s, d, "far") for s in ("TW", "TG") for d in R.OWN_FAR_D})
        assert set(seams) >= {"W", "TW", "TG"} and ("IT" in seams) == (config != "t2")
        if config != "t2" and name not in ("a.*b", "#.+"):
            continue            # (the modes against the oracle: every family at 2-KiB tiles, two at the others)
        for c in cases:
            full = oracle.match_all(fam.rx, c.text)
            cut = c.own[0]
            straddle = [m for m in full if m[0] < cut < m[1]]
            carry = R.carry_of(full, c.own)
            geo = R.own_geo(c, config, carry)
            firsts.add(geo.first_tile > 0)
            if c.mode == "cut":
                assert straddle and cut == c.at, c.label
            elif c.mode == "end":
                assert straddle and straddle[0][1] == c.at == carry["carry_cur"], c.label
            elif c.mode == "begin":
                assert not straddle and cut == c.at and geo.clip_from == c.at + ("lag" in fam.flags), c.label
                assert any(m[0] == cut for m in full) or name in ("acgt+",), c.label        # a match begins AT the own begin
            elif c.mode == "far":
                if fam.has_b and name != "<[^>]*>":      # the carried-in match ends two tiles back; a break behind it; a match begins at the own begin
                    assert not straddle and geo.blocked and carry["carry_prev_end"] == cut - 2 * geo.tile_bytes - 5 and (cut, cut + 3) in full, c.label
                    assert geo.first_tile <= geo.clip_from // geo.tile_bytes - 2, c.label
                    far += 1
            else:
                assert c.own[1] == c.at < c.n and any(m[0] >= c.own[1] for m in full), c.label
            want = [m for m in full if c.own[0] <= m[0] < c.own[1]]
            assert want or c.mode == "oe", c.label
            assert geo.min_start <= geo.clip_from and geo.blocked == (bool(carry) and fam.has_b and name != "<[^>]*>"), c.label
            if geo.blocked:         # the carried-in match ends behind a B that is no break (RunParams::blocked_in): the tiles begin at that B's
                blocked += 1
                assert geo.first_tile == (carry["carry_prev_end"] - 1) // geo.tile_bytes
                early += geo.base(0) < (geo.clip_from // geo.tile_bytes) * geo.tile_bytes
    assert firsts == {False, True}
    assert far >= 2 * len(R.OWN_FAR_D) and blocked >= 2 * len(R.OWN_D) and early >= 4       # (... and at an earlier tile than min_start's: the break in the tile before is seen)
