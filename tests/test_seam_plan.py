"""CPU test of the seam sweep's case planner (tests/seam_sweep.py): its span table against the launch arithmetic of
rejit_amd/csrc/plane_args.h (through tests/support/plane_args_exec.cc, the driver of tests/test_plane_args.py), and the
coverage that keeps tests/test_gpu_seams.py from quietly skipping the hard cases -- every (seam class x offset) pair per
family, every span length as first, interior and last span, waves without a block, the tails."""
import ctypes
import os
import subprocess

import pytest

import seam_sweep as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "support", "plane_args_exec.cc")
DEPS = [SRC, os.path.join(ROOT, "rejit_amd", "csrc", "plane_args.h")]
SO = os.path.join(HERE, "support", "libplane_args_exec.so")
U64 = ctypes.c_uint64
U32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def pa():
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO + ".tmp%d" % os.getpid(), SRC])
        os.replace(SO + ".tmp%d" % os.getpid(), SO)
    lib = ctypes.CDLL(SO)
    u64p = ctypes.POINTER(U64)
    lib.pa_blocks.restype = None
    lib.pa_blocks.argtypes = [U64, U64, U64, U32, U32, U32, u64p]
    lib.pa_split.restype = None
    lib.pa_split.argtypes = [U64, U64, U32, u64p]
    return lib


def all_cases():
    out = {}
    for family in list(S.FAMILIES) + ["own", "busy", "pairs", "pairs_general", "void"]:
        for grid in S.GRIDS:
            out[(family, grid)] = S.cases_of(family, grid)
    return out


@pytest.fixture(scope="module")
def planned():
    return all_cases()


def test_span_table_equals_plane_args(pa, planned):
    """plane_blocks and plane_split of the header give the planner's blocks and spans; the waves tile the blocks in order."""
    out, sp = (U64 * 4)(), (U64 * 3)()
    checked = 0
    plans = [c.plan for cases, _ in planned.values() for c in cases] + [S.anchor_plants()[1], S.anchor_plants()[4]]
    for own in ((5, 4000), (2047, 2049), (4096, 4097), (100000, 100001), (0, 8)):       # (ranges the families do not have)
        for win in ((0, 0, 8), (1, 1, 8), (0, 7, 4), (3, 5, 6)):
            plans.append(S.Plan(123456, own, 2, *win))
            plans.append(S.Plan(own[1] + 3, own, 1, *win))
    for plan in plans:
        lo, hi, n_cmp = plan.window
        pa.pa_blocks(plan.n, plan.sb, plan.se, lo, hi, n_cmp, out)
        assert (plan.wlo, plan.whi, plan.first_block, plan.end_block) == tuple(out), (plan.n, plan.sb, plan.se)
        pa.pa_split(plan.first_block, plan.end_block, plan.n_regions, sp)
        assert (plan.span_blocks, plan.span_extra) == (sp[0], sp[1])
        at = plan.first_block
        for w in plan.waves:
            assert w.c0 == at and w.c0 <= w.fast_end <= w.c1
            at = w.c1
            for c in range(w.c0, w.c1):     # a fast block and the one behind it lie inside the text
                assert (c < w.fast_end) == ((c + 2) * S.BLOCK <= plan.n), (plan.n, c)
        assert at == plan.end_block
        checked += 1
    assert checked > 500


def test_anchor_plan_has_production_spans_and_every_class():
    """Without an override scan_geometry deals a 34 MiB text out in spans of 16 and 17 blocks for the count kernel and of 12
    and 13 for the list kernel -- span lengths the forced grids of the sweep produce too -- and the anchor's plants cover the
    P, B01, B12, BH and S seams of both launches, well apart."""
    n, plan, plants, cover, list_plan = S.anchor_plants()
    assert plan.grid == 272 and {w.length for w in plan.waves} == {16, 17}
    assert list_plan.grid == 362 and {w.length for w in list_plan.waves} == {12, 13}
    assert 48 <= len(plants) <= 800
    tags = {t for p in plants for t in p[2]}
    classes = {"P", "B01", "B12", "BH1", "BH2", "SW", "SG"}
    assert classes | {c + "/list" for c in classes} <= tags, tags
    starts = [p[0] for p in plants]
    assert all(b - a >= 8 + S.MIN_GAP for a, b in zip(starts, starts[1:]))
    for start, s, t, seam in plants:            # every plant lies across the seam it names, in the launch it names
        assert -8 <= start - seam <= 1
        for tag in t:
            p = list_plan if tag.endswith("/list") else plan
            assert any(pos == seam and tag.split("/")[0] in tt for pos, tt in S._anchor_seams(p)), (seam, tag)


@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_every_seam_class_at_every_offset(planned, family):
    lengths = sorted(S.FAMILIES[family].get("cover") or {len(s) for s in S.FAMILIES[family]["plants"]})
    seen = S.Coverage()
    for grid in S.GRIDS:
        cases, cover = planned[(family, grid)]
        for k, v in cover.seen.items():
            seen.seen[k] = seen.seen.get(k, 0) + v
        for c in cases:
            assert len(c.text) <= 70 * S.BLOCK
            assert c.n % S.BLOCK in S.TAILS
            starts = [(p[0], p[0] + len(p[1])) for p in c.plants]
            assert all(b[0] - a[1] >= S.MIN_GAP for a, b in zip(starts, starts[1:])), c.label
            bg = c.text[0] if not c.plants or c.plants[0][0] > 0 else None
            for start, s, tags, seam in c.plants:
                assert c.text[start:start + len(s)] == s and -len(s) <= start - seam <= 1
            assert bg is None or bg not in b"".join(S.FAMILIES[family]["plants"])
    assert seen.missing(lengths) == [], (family, seen.missing(lengths)[:12])


def test_background_is_never_a_candidate():
    """Under every shift a plan can choose, a run of the background differs from every compared piece of a planted string
    in at least two 2-bit codes (three where the set has a class position: a base may hold any byte of the class there)."""
    for name, fam in S.FAMILIES.items():
        bg, worst = S.pick_background(fam["plants"], S.window_of(name)[2])
        has_class = any(b"[" in rx for rx in fam["rx"])
        assert worst >= (3 if has_class else 2), (name, bg, worst)


def test_span_lengths_empty_waves_and_tails(planned):
    for family in S.FAMILIES:
        places = set()
        empty = False
        tails = set()
        for grid in S.GRIDS:
            for c in planned[(family, grid)][0]:
                places |= set(c.plan.span_lengths())
                empty = empty or any(w.length == 0 for w in c.plan.waves)
                tails.add(c.n % S.BLOCK)
        missing = [(length, place) for length in S.SPAN_LENGTHS for place in ("first", "interior", "last") if (length, place) not in places]
        assert not missing, (family, missing)
        assert empty and tails == set(S.TAILS), (family, tails)


def test_variants(planned):
    """Own ranges put first_block > 0 in front of wave 0; the busy ring holds a candidate every ~40 bytes over spans of 8
    and 9 blocks; pairs and chains lie across every class at every offset; the void text has more than 256 candidates
    between two looks at the ring."""
    for grid in S.GRIDS:
        own = planned[("own", grid)][0]
        assert any(c.plan.first_block > 0 for c in own) and any(c.plan.end_block < (c.n + S.BLOCK - 1) // S.BLOCK for c in own)
        assert len(own) >= 30
        void = planned[("void", grid)][0]
        assert void[1].text.count(b"agggtaaa" * 64) >= 1 and void[1].expect_how == 1 and void[0].text == void[2].text
        assert any(w.length == 5 for w in void[1].plan.waves)
    busy = [c for c in planned[("busy", 1)][0]]
    assert {8, 9, 16} <= {w.length for c in busy for w in c.plan.waves}
    for c in busy:
        assert sum(c.text.count(s) for s in S.FAMILIES["dna9"]["near"]) >= c.n // 60
    for family, strings in (("pairs", [15, 22]), ("pairs_general", [6, 7, 8, 10])):
        seen = S.Coverage()
        for grid in S.GRIDS:
            for k, v in planned[(family, grid)][1].seen.items():
                seen.seen[k] = seen.seen.get(k, 0) + v
        assert seen.missing(strings) == [], (family, seen.missing(strings)[:12])


def test_single_pattern_seams():
    for grid in S.GRIDS:
        cases, covers = S.single_cases(grid)
        spans = {int(c.label.split("span=")[1]) for c in cases}
        assert {4, 9} <= spans
        for cover, length in zip(covers, (2, 5, 8, 4)):
            assert cover.missing([length], tags=("LA", "P", "SW")) == [], (grid, length, cover.missing([length], tags=("LA", "P", "SW")))
