"""Seam sweep of the window scan's streaming loop (rejit_amd/csrc/scan_windows.hip: scan_windows<K, TWO, MASKED, TWOLEVEL, NIB>,
scan_windows_body, windows_chunk) and of what runs behind it, on small texts.

Like tests/seam_sweep.py (whose planting machinery it uses) this module is two things.

* A case PLANNER, pure Python, no GPU (tests/test_window_sweep_plan.py asserts its schedule, its coverage and the kernel
  variant of every family).  It restates the launch arithmetic of engine.hip (run_range: wlo, whi, first_chunk, end_chunk),
  scan_geometry under a forced grid, wave_span (kernel_util.h) and the kernel's own fast_end, and returns per wave the
  role of every chunk exactly as scan_windows_body schedules it, and the class of every seam of the text.
* The child DRIVER, `python tests/window_sweep.py FAMILY`, which tests/test_gpu_window_seams.py starts once per
  (family, grid) with RJ_SCAN_GRID and RJ_NO_SMALL=1 in the environment (the library reads both once per process).

Roles of a chunk: S0..S3 a slot of the four-buffer pipeline, E0..E2 its epilogue, P a plain-loop chunk behind the epilogue,
p a plain-loop chunk of a span that never enters the pipeline (fewer than 8 unguarded chunks), G a guarded chunk.

Seam classes (a seam is the boundary before byte `pos`; `X:role` is the class X tagged with a role):
  L             lanes 0|1, 31|32, 62|63 inside a chunk, L:role with the chunk's role
  S01 S12 S23   pipeline slots inside one iteration (the next chunk's buffer was loaded earlier)
  S30           slot 3 -> slot 0 of the next iteration (q0 reloaded in this iteration)
  S3E           the last iteration's slot 3 -> epilogue chunk 0
  E01 E12       inside the epilogue
  E2P           epilogue chunk 2 -> the first plain chunk (q0 = q3; lane 63's own 8-byte load starts here)
  PP / pp       plain -> plain behind a pipeline / in a span that never enters it
  PG / GG       unguarded -> guarded / guarded -> guarded
  SW / SG       a span seam inside a workgroup / between workgroups, SW:role with the role of the chunk before it
  GE            the end of the text
  OWN           sb and se of an own range

GG needs two guarded chunks, that is a tail n % 1024 with window_len <= tail <= 7: a window of 8 bytes cannot have it
(tests/test_window_sweep_plan.py asserts that over every tail, and asserts GG for every family whose window is shorter).
SW:G and SG:G (a span that ends in a guarded chunk with another span behind it) exist in one geometry per grid each; they are
planted wherever they occur and asserted to occur, the full offset rotation is asserted for SW / SG and their P / p tags.

scan_windows_fused is out of scope: rj_multi takes it only in mode 0 for a fusable set that has no plane plan (multi_pattern.hip,
plan_batched: `r.plane = fuse && m->mode == 0 && m->plane.ok`), the nine regexdna patterns have one (tests/seam_sweep.py sweeps
that path), and modes 1 and 2 of the `multi` sweep take scan_windows_train and the separate scans, as the kernel trace shows.
"""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from seam_sweep import (Case, Coverage, DNA9, FAMILIES as PLANE_FAMILIES, GpuBackend, MIN_GAP, Report, first_difference, oracle_spans,   # noqa: E402
                        plant_text, scan_geometry)

CHUNK = 1024
GRIDS = (1, 2, 3)
F_LIST = (1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 16, 17, 33)     # unguarded chunks of a wave
PIPE = ("S0", "S1", "S2", "S3")
EPI = ("E0", "E1", "E2")
ROLES = PIPE + EPI + ("P", "p", "G")
INNER = {("S0", "S1"): "S01", ("S1", "S2"): "S12", ("S2", "S3"): "S23", ("S3", "S0"): "S30", ("S3", "E0"): "S3E", ("E0", "E1"): "E01",
         ("E1", "E2"): "E12", ("E2", "P"): "E2P", ("P", "P"): "PP", ("p", "p"): "pp", ("P", "G"): "PG", ("p", "G"): "PG", ("G", "G"): "GG"}
BASE_CLASSES = ("L", "S01", "S12", "S23", "S30", "S3E", "E01", "E12", "E2P", "PP", "pp", "PG", "SW", "SG", "GE")
TAGGED = tuple("L:" + r for r in ROLES) + ("SW:P", "SW:p", "SG:P", "SG:p")
MAX_TEXT = 140 * 1024


class _Rank(dict):
    """plant_text's order of service: the rare classes first"""

    def __missing__(self, tag):
        base = tag.split(":")[0]
        if base in ("OWN", "SG", "GE", "PG", "GG", "S3E", "E2P", "S30", "E01", "E12") or tag == "SW:G":
            return 0
        if base in ("SW", "S01", "S12", "S23"):
            return 1
        return 2 if base in ("PP", "pp") else 3


RANK = _Rank()


# ------------------------------------------------------------------------------------------------ the arithmetic
def window_range(n, sb, se, offset, length, behind=False):
    """plane_args.h, chunk_range (engine.hip: run_range) -> (wlo, whi, first_chunk, end_chunk); a behind pattern reaches last_w"""
    last_w = n - length + 1 if n >= length else 0
    wlo = sb + offset
    whi = last_w if behind else min(se + offset, last_w)
    whi = max(whi, wlo)
    return wlo, whi, wlo // CHUNK, (whi + CHUNK - 1) // CHUNK


def schedule(c0, c1, fast_end):
    """scan_windows_body: the role of every chunk of the span [c0, c1), in the order the kernel takes them"""
    out = []
    c = c0
    plain = "p"
    if c + 7 < fast_end:
        while c + 7 < fast_end:
            out += [(c + k, PIPE[k]) for k in range(4)]
            c += 4
        out += [(c + k, EPI[k]) for k in range(3)]
        c += 3
        plain = "P"
    while c < fast_end:
        out.append((c, plain))
        c += 1
    for t in range(fast_end, c1):
        out.append((t, "G"))
    return out


class WWave:
    def __init__(self, index, c0, c1, fast_end):
        self.index, self.c0, self.c1, self.fast_end = index, c0, c1, fast_end
        self.roles = schedule(c0, c1, fast_end)

    @property
    def length(self):
        return self.c1 - self.c0

    @property
    def fast(self):
        return self.fast_end - self.c0


class WPlan:
    """The launch of scan_windows over the starts [sb, se) of a text of n bytes for a program with (window_offset, window_len).
    geometry_chunks: the chunk count scan_geometry is asked for when it is not end_chunk - first_chunk (rj_multi's batched
    runs, multi_pattern.hip: plan_batched)."""

    def __init__(self, n, own, grid, offset, length, behind=False, geometry_chunks=None):
        self.n, self.window = n, (offset, length)
        self.sb, self.se = (0, n + 1) if own is None else (own[0], min(own[1], n + 1))
        self.wlo, self.whi, self.first_chunk, self.end_chunk = window_range(n, self.sb, self.se, offset, length, behind)
        self.chunks = max(self.end_chunk - self.first_chunk, 0)
        self.grid, self.n_regions, self.span_chunks = scan_geometry(max(self.chunks if geometry_chunks is None else geometry_chunks, 1), 128, grid)
        fast = (n - 8) // CHUNK if n >= CHUNK + 8 else 0
        self.waves = []
        for w in range(self.n_regions):
            c0 = min(self.first_chunk + w * self.span_chunks, self.end_chunk)
            c1 = min(self.first_chunk + (w + 1) * self.span_chunks, self.end_chunk)
            self.waves.append(WWave(w, c0, c1, max(min(fast, c1), c0)))

    def busy(self):
        return [w for w in self.waves if w.length]

    def f_positions(self):
        """(F, place): place = 'before' for a wave of F unguarded chunks and no other with a busy wave behind it, 'last1' / 'last2'
        for the last wave with one / two guarded chunks behind its F"""
        busy = self.busy()
        out = set()
        for i, w in enumerate(busy):
            g = w.length - w.fast
            if i + 1 < len(busy) and g == 0:
                out.add((w.fast, "before"))
            if i + 1 == len(busy) and g in (1, 2):
                out.add((w.fast, "last%d" % g))
        return out

    def seams(self):
        """[(pos, (class, tagged class))] in text order"""
        out = []
        busy = self.busy()
        for i, w in enumerate(busy):
            for j, (c, role) in enumerate(w.roles):
                base = c * CHUNK
                for lane in (1, 32, 63):
                    out.append((base + 16 * lane, ("L", "L:" + role)))
                if j + 1 < len(w.roles):
                    cls = INNER[(role, w.roles[j + 1][1])]
                    out.append((base + CHUNK, (cls,)))
                elif i + 1 < len(busy):
                    cls = "SG" if (w.index + 1) % 4 == 0 else "SW"
                    out.append((base + CHUNK, (cls, cls + ":" + role)))
        out = [(p, t) for p, t in out if 0 < p < self.n]
        out.append((self.n, ("GE",)))
        return out


    def seams_of(self, w, has_next):
        """the chunk seams of one wave (the anchor plants these and no lane seams)"""
        out = []
        for j, (c, role) in enumerate(w.roles):
            if j + 1 < len(w.roles):
                out.append(((c + 1) * CHUNK, (INNER[(role, w.roles[j + 1][1])],)))
            elif has_next:
                cls = "SG" if (w.index + 1) % 4 == 0 else "SW"
                out.append(((c + 1) * CHUNK, (cls, cls + ":" + role)))
        return out


@functools.lru_cache(maxsize=None)
def guarded_chunks(length, offset, tail):
    """how many guarded chunks the whole-text launch has for the tail n % 1024 (1 or 2)"""
    return sum(w.length - w.fast for w in WPlan(8 * CHUNK + tail, None, 1, offset, length).waves)


# ------------------------------------------------------------------------------------------------ the families
def _fam(rx, plants, near, K, wlen, variant, offset=0, alias=()):
    return dict(rx=rx, plants=plants, near=near, K=K, wlen=wlen, offset=offset, variant=variant, alias=alias)


# variant = (TWO, MASKED, TWOLEVEL, NIB) as launch_scan_windows instantiates it; K = the program's window count (the launcher
# rounds 5 up to 6 and 7 up to 8, the set is padded with copies of its last window); near = strings that must not match:
# one byte off, the class position outside its class, and (alias) a low-nibble alias of a window byte, which the nibble
# filter reports and the verify tail must drop
ONE_M, ONE_U = (False, True, False, False), (False, False, False, False)
TL_U, TL_M = (True, False, True, False), (True, True, True, False)
NIB_U, NIB_M = (True, False, False, True), (True, True, False, True)
PL_U, PL_M = (True, False, False, False), (True, True, False, False)
K7 = b"aaaa1|bbbb2|cccc3|dddd4|eeee5|ffff6|gggg7"
FAMILIES = {
    "m1_k1": _fam(b"qz", [b"qz"], [b"qy", b"Qz"], 1, 2, ONE_M),
    "m1_k3": _fam(b"ab|cd|ef", [b"ab", b"cd", b"ef"], [b"ad", b"cf"], 3, 2, ONE_M),
    "m1_k5": _fam(b"ab|cd|ef|gh|ij", [b"ab", b"cd", b"ef", b"gh", b"ij"], [b"aj", b"ib"], 5, 2, ONE_M),
    "u1_k1": _fam(b"qzvw", [b"qzvw"], [b"qzvx", b"Qzvw"], 1, 4, ONE_U),
    "u1_k2": _fam(b"abab|baba", [b"abab", b"baba"], [b"abaa", b"babb"], 2, 4, ONE_U),
    "u1_k3": _fam(b"qzvw|wvzq|zzqq", [b"qzvw", b"wvzq", b"zzqq"], [b"qzvq", b"zzqw"], 3, 4, ONE_U),
    "u1_k4": _fam(b"abcd|efgh|ijkl|mnop", [b"abcd", b"efgh", b"ijkl", b"mnop"], [b"abcf", b"mnoq"], 4, 4, ONE_U),
    "tl_u8": _fam(b"regexpqz", [b"regexpqz"], [b"regexpqy", b"rfgexpqz"], 1, 8, TL_U),
    "tl_u16": _fam(b"abcdefghijklmnop", [b"abcdefghijklmnop"], [b"abcdefghijklmnoq", b"abcdefgXijklmnop"], 1, 8, TL_U),
    "tl_m5": _fam(b"qzvwx", [b"qzvwx"], [b"qzvwy", b"qzvXx"], 1, 5, TL_M),
    "tl_m_dot": _fam(b"a.cdefgh", [b"abcdefgh", b"aXcdefgh", b"a~cdefgh"], [b"a\ncdefgh", b"abcdefgX"], 1, 8, TL_M),
    "tl_m_k5": _fam(b"abcde|fghij|klmno|pqrst|uvwxy", [b"abcde", b"fghij", b"klmno", b"pqrst", b"uvwxy"], [b"abcdf", b"uvwxz"], 5, 5, TL_M),
    "tl_m_k7": _fam(K7, [b"aaaa1", b"bbbb2", b"cccc3", b"dddd4", b"eeee5", b"ffff6", b"gggg7"], [b"aaaa2", b"gggg1"], 7, 5, TL_M),
    "tl_m_k8": _fam(K7 + b"|hhhh8", [b"aaaa1", b"bbbb2", b"cccc3", b"dddd4", b"eeee5", b"ffff6", b"gggg7", b"hhhh8"], [b"hhhh1", b"aaaa8"], 8, 5, TL_M),
    "nib_u_k1": _fam(b"agggtaaa", [b"agggtaaa"], [b"agggtaac", b"qgggtaaa"], 1, 8, NIB_U, alias=(b"qgggtaaa",)),
    "nib_u_k2": _fam(b"agggtaaa|tttaccct", [b"agggtaaa", b"tttaccct"], [b"agggtaac", b"qgggtaaa", b"tttacccd"], 2, 8, NIB_U, alias=(b"qgggtaaa", b"tttacccd")),
    "nib_u_k3": _fam(b"agggtaaa|tttaccct|ggggaaaa", [b"agggtaaa", b"tttaccct", b"ggggaaaa"], [b"ggggaaac", b"wgggaaaa", b"tttacccd"], 3, 8, NIB_U,
                     alias=(b"wgggaaaa", b"tttacccd")),
    "nib_m_k1": _fam(b"ab.de", [b"abcde", b"abXde", b"ab~de"], [b"ab\nde", b"qbcde", b"abcdf"], 1, 5, NIB_M, alias=(b"qbcde",)),
    "nib_m_k2": _fam(b"agg[act]taaa|ttta[agt]cct", [b"aggataaa", b"aggctaaa", b"aggttaaa", b"tttaacct", b"tttagcct", b"tttatcct"],
                     [b"agggtaaa", b"tttaccct", b"qggataaa"], 2, 8, NIB_M, alias=(b"qggataaa",)),
    "nib_m_k3": _fam(b"acgta|cgtac|gtacg", [b"acgta", b"cgtac", b"gtacg"], [b"acgtc", b"qcgta"], 3, 5, NIB_M, alias=(b"qcgta",)),
    "pl_u_k1": _fam(b"aqaqaqaq", [b"aqaqaqaq"], [b"aqaqaqaa", b"aqaqaqqq"], 1, 8, PL_U),
    "pl_u_k2": _fam(b"aqaqaqaq|qaqaqaqa", [b"aqaqaqaq", b"qaqaqaqa"], [b"aqaqaqaa", b"qaqaqaqq"], 2, 8, PL_U),
    "pl_m_k1": _fam(b"aq.qa", [b"aqaqa", b"aqXqa"], [b"aq\nqa", b"aqaqq"], 1, 5, PL_M),
    "pl_m_k2": _fam(b"aqaqa|qaqaq", [b"aqaqa", b"qaqaq"], [b"aqaqq", b"qaqaa"], 2, 5, PL_M),
    "offset1": _fam(b"[ab]cdefghij", [b"acdefghij", b"bcdefghij"], [b"ccdefghij", b"acdefghiq"], 1, 8, TL_U, offset=1),
    # `abab|baba` again, with strings that hold overlapping candidates: the left-most-longest selection continues across regions
    "chains": _fam(b"abab|baba", [b"ababab", b"abababab", b"bababab"], [b"abaa", b"babb"], 2, 4, ONE_U),
}
K_CLASS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}      # launch_windows_k

OWN_FAMILIES = ("tl_u8", "nib_u_k2", "offset1")
BUSY_FAMILIES = ("tl_u8", "nib_u_k2", "u1_k1")
RUNS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 33, 40)
# whole matches longer than the window; window = (offset, len) as Program.info() reports it, behind: the window lies behind
# an unbounded prefix (a match begins in front of its hit); the driver prints info() and checks these
TAILS = {
    "tail_fwd": dict(rx=b"abcd[0-9]+", plants=[b"abcd" + bytes(48 + (i * 7 + k) % 10 for i in range(k)) for k in RUNS], window=(0, 5), behind=False),
    "tail_bound": dict(rx=b"regexp[0-9]{1,3}", plants=[b"regexp" + d for d in (b"7", b"42", b"365", b"2718", b"31415")], window=(0, 7), behind=False),
    "tail_behind": dict(rx=b"[0-9]+abcd", plants=[bytes(48 + (i * 3 + k) % 10 for i in range(k)) + b"abcd" for k in RUNS], window=(0, 4), behind=True),
    "tail_float": dict(rx=b"ab[0-9]+cd", plants=[b"ab" + bytes(48 + (i + k) % 10 for i in range(k)) + b"cd" for k in RUNS], window=(0, 2), behind=False),
}
SWEEPS = list(FAMILIES) + ["own", "busy", "multi"] + list(TAILS)


def background(fam):
    """a byte that no planted string holds; for the nibble form, whose low nibble no planted byte has either"""
    used = set(b"".join(fam["plants"] + fam["near"]))
    nibbles = {b & 15 for b in used} if fam["variant"][3] else set()
    for x in b"-_=+:;,/!*":
        if x not in used and (x & 15) not in nibbles:
            return x
    raise AssertionError(fam["rx"])


def grid_for(span, rot=0):
    """the largest grid of GRIDS that keeps a text of 4 * grid * span chunks below MAX_TEXT, one smaller every third time"""
    fits = [g for g in GRIDS if 4 * g * span * CHUNK <= MAX_TEXT] or [1]
    return fits[-1] if rot % 3 or len(fits) == 1 else fits[-2]


def tails_of(wlen):
    return sorted({0, 1, 7, 8, 9, wlen - 1, wlen, 1023})


def text_length(chunks, tail, offset, wlen):
    """n = full * 1024 + tail whose whole-text launch has `chunks` chunks"""
    for full in (chunks - 1, chunks):
        n = full * CHUNK + tail
        if full >= 1 and window_range(n, 0, n + 1, offset, wlen)[3] == chunks:
            return n
    raise AssertionError((chunks, tail, wlen))


@functools.lru_cache(maxsize=None)
def geometries(wlen, offset=0):
    """[(grid, n)]: every F of F_LIST as a wave before the last (a span of F chunks), as the last wave with one guarded chunk
    behind it (a span of F + 1) and, where the window allows two guarded chunks, with two (a span of F + 2); every tail;
    spans that do not fill the last wave, and waves without a chunk."""
    tails = tails_of(wlen)
    one = [t for t in tails if guarded_chunks(wlen, offset, t) == 1]
    two = [t for t in tails if guarded_chunks(wlen, offset, t) == 2]
    out = []
    rot = 0
    for span in sorted(set(F_LIST) | {f + 1 for f in F_LIST}):
        g = grid_for(span, rot)
        out.append((g, text_length(4 * g * span, one[rot % len(one)], offset, wlen)))
        rot += 1
    if two:
        for span in sorted(f + 2 for f in F_LIST):
            g = grid_for(span, rot)
            out.append((g, text_length(4 * g * span, two[rot % len(two)], offset, wlen)))
            rot += 1
    # the last wave short (8, 8, 8, 7 and 6 ... 6, 2), three waves without a chunk; and, where the window allows two guarded chunks,
    # a span that ends guarded with a span behind it (SW:G, SG:G)
    out += [(1, text_length(31, 9, offset, wlen)), (2, text_length(44, 1023, offset, wlen)), (3, text_length(25, 8, offset, wlen))]
    small = min(wlen, 7)
    if small >= wlen:       # (the partial chunk has a window position: the chunk before it and it are guarded, each its own span)
        out += [(1, 12 * CHUNK + small), (2, 4 * CHUNK + small), (3, 4 * CHUNK + small)]
    return out


# (grid, span): further texts that plant only the classes that are rare in a text -- one or two per span -- until every family
# has every class at every offset (tests/test_window_sweep_plan.py); tail and string rotate
RARE = ("SG", "SG:P", "SG:p", "SW:P", "SW:p", "PG", "GG", "S3E", "E2P", "S30", "E01", "E12", "L:G", "L:E0", "L:E1", "L:E2", "L:P", "pp", "L:p", "GE")
EXTRA = [(2, 12), (3, 2), (3, 8), (2, 3), (2, 13), (3, 3), (3, 9), (2, 4), (2, 16), (3, 1), (3, 10), (2, 2), (2, 17), (3, 4), (3, 11), (2, 5), (1, 12), (1, 3), (1, 13), (1, 5)]


def _plant_case(label, plan, fam, bg, cover, near_cover, rot, own=None, only=None, extra_seams=()):
    n = plan.n
    seams = plan.seams() + list(extra_seams)
    common = [i for i, s in enumerate(seams) if s[1][0] in ("L", "S01", "S12", "S23", "PP", "pp")]
    near_at = set(common[rot % 7::7]) if only is None else set()
    text, placed = bytearray([bg]) * n, []
    _, near = plant_text(n, [seams[i] for i in sorted(near_at)], fam["near"], bg, near_cover, rot, rare=RANK, text=text, placed=placed)
    data, plants = plant_text(n, [s for i, s in enumerate(seams) if i not in near_at], fam["plants"], bg, cover, rot, only=only, rare=RANK, text=text, placed=placed)
    c = Case(label, plan, data, plants, own=own)
    c.near = near
    return c


@functools.lru_cache(maxsize=None)
def family_cases(name, grid):
    """The texts of one family under a forced grid -> (cases, coverage of the matching plants, coverage of the near misses)."""
    fam = FAMILIES[name]
    bg = background(fam)
    cover, near_cover = Coverage(), Coverage()
    cases = []
    geos = geometries(fam["wlen"], fam["offset"])
    tails = tails_of(fam["wlen"])
    for rot, (g, n) in enumerate(geos):
        if g == grid:
            plan = WPlan(n, None, grid, fam["offset"], fam["wlen"])
            cases.append(_plant_case("%s n=%d" % (name, n), plan, fam, bg, cover, near_cover, rot))
    two = [t for t in tails if guarded_chunks(fam["wlen"], fam["offset"], t) == 2]
    offsets = max(len(s) for s in fam["plants"]) + 2
    for rot, (g, span) in enumerate(EXTRA * ((offsets + 8) // 9)):
        if g == grid:
            tail = two[rot // 2 % len(two)] if two and rot % 2 else tails[rot // 2 % len(tails)]
            n = text_length(4 * g * span, tail, fam["offset"], fam["wlen"])
            plan = WPlan(n, None, grid, fam["offset"], fam["wlen"])
            cases.append(_plant_case("%s n=%d (rare classes)" % (name, n), plan, fam, bg, cover, near_cover, rot + 1, only=RARE))
    return cases, cover, near_cover


@functools.lru_cache(maxsize=None)
def own_cases(grid):
    """Own ranges whose sb / se lie at a seam +- 0..8 -- wlo / whi cut a chunk, first_chunk > 0 --, in the three shapes (x, n + 1),
    (0, x) and (x, x + k * 1024 + r), a third of them per grid."""
    cases = []
    covers = {}
    k = 0
    for name in OWN_FAMILIES:
        fam = FAMILIES[name]
        bg = background(fam)
        cover, near_cover = covers.setdefault(name, (Coverage(), Coverage()))
        for g in GRIDS:
            n = text_length(4 * g * 9 + 3, 9, fam["offset"], fam["wlen"])
            whole = WPlan(n, None, g, fam["offset"], fam["wlen"])
            picks = {}
            for pos, tags in whole.seams():
                if tags[0] in ("S3E", "E2P", "SW", "S12", "pp", "PG") or tags[1:] == ("L:S1",) and pos % CHUNK == 16 * 63:
                    picks.setdefault(tags[0], pos)
            for cls, seam in sorted(picks.items()):
                for d in range(-8, 9):
                    k += 1
                    x = seam + d
                    own = ((x, n + 1), (0, x), (x, x + (2 + k % 5) * CHUNK + (k * 37) % CHUNK))[k % 3]
                    if g != grid:
                        continue
                    plan = WPlan(n, own, grid, fam["offset"], fam["wlen"])
                    edges = [(own[0], ("OWN",))] + ([(own[1], ("OWN",))] if own[1] < n else [])
                    c = _plant_case("own %s n=%d own=%s at %s%+d" % (name, n, own, cls, d), plan, fam, bg, cover, near_cover, k, own=own, extra_seams=edges)
                    c.family = name
                    cases.append(c)
    return cases, covers


@functools.lru_cache(maxsize=None)
def busy_cases(grid):
    """Needles in 6 lanes of one chunk, lanes 0, 62 and 63 among them (the wave-scan branch of RegionHits::push_bits), in a
    chunk of every role; and a needle every 24 bytes over six chunks of one span: more than 64 hits, the first run of a fresh
    scan overflows its regions and runs again, and the next runs of the same text find the hint warm."""
    cases = []
    for name in BUSY_FAMILIES:
        fam = FAMILIES[name]
        bg = background(fam)
        needle = fam["plants"][0]
        for rot, span in enumerate((13, 9)):
            n = text_length(4 * grid * span, (9, 7)[rot], fam["offset"], fam["wlen"])
            plan = WPlan(n, None, grid, fam["offset"], fam["wlen"])
            wave = plan.busy()[min(1 + rot, len(plan.busy()) - 1)]
            dense = [c for c, _ in wave.roles[:6]]
            lanes = {}                      # one chunk per role, outside the dense span
            for w in plan.busy():
                if w is not wave:
                    for c, role in w.roles:
                        lanes.setdefault(role, c)
            clear = [(c * CHUNK, (c + 1) * CHUNK) for c in dense + sorted(lanes.values())]
            c = _plant_case("busy %s n=%d" % (name, n), plan, fam, bg, Coverage(), Coverage(), rot)
            # (plant first, then overwrite the busy chunks whole: nothing planted there survives in part)
            t = bytearray(c.text)
            for lo, hi in clear:
                lo, hi = max(lo - 32, 0), min(hi + 32, n)
                t[lo:hi] = bytes([bg]) * (hi - lo)
            for ch in dense:
                for at in range(ch * CHUNK, (ch + 1) * CHUNK - 24, 24):
                    t[at:at + len(needle)] = needle
            for role, ch in lanes.items():
                if (ch + 1) * CHUNK + 32 > n or ch * CHUNK < 32:
                    continue
                for lane in (0, 62, 63, 7, 31, 32):
                    at = ch * CHUNK + 16 * lane + (lane % 3)
                    t[at:at + len(needle)] = needle
            c.text = bytes(t)
            c.plants = [p for p in c.plants if c.text[p[0]:p[0] + len(p[1])] == p[1]]
            c.family, c.dense, c.lanes = name, dense, lanes
            cases.append(c)
    return cases, None


@functools.lru_cache(maxsize=None)
def tail_cases(name, grid):
    fam = dict(TAILS[name], near=[b"abcQ", b"regexQ"], variant=(False,) * 4)
    off, wlen = fam["window"]
    bg = ord("-")
    cover = Coverage()
    cases = []
    for rot, span in enumerate((13, 9, 12, 2, 8, 17, 3, 10)):
        if 4 * grid * span * CHUNK > MAX_TEXT:
            continue
        n = text_length(4 * grid * span, tails_of(wlen)[rot % len(tails_of(wlen))], off, wlen)
        plan = WPlan(n, None, grid, off, wlen, behind=fam["behind"])
        cases.append(_plant_case("%s n=%d" % (name, n), plan, fam, bg, cover, Coverage(), rot))
    return cases, cover


@functools.lru_cache(maxsize=None)
def multi_cases(grid):
    """The nine regexdna patterns (scan_windows_train, and the separate scans on two streams): the texts of `agggtaaa|tttaccct`
    with the one-off strings of tests/seam_sweep.py; rj_multi asks scan_geometry for every chunk of the text."""
    fam = dict(FAMILIES["nib_u_k2"], plants=PLANE_FAMILIES["dna9"]["plants"], near=PLANE_FAMILIES["dna9"]["near"])
    bg = background(fam)
    cover = Coverage()
    cases = []
    for rot, (g, n) in enumerate(geometries(8)):
        if g == grid:
            plan = WPlan(n, None, grid, 0, 8, geometry_chunks=(n + CHUNK - 1) // CHUNK)
            cases.append(_plant_case("multi n=%d" % n, plan, fam, bg, cover, Coverage(), rot))
    return cases, cover


def cases_of(sweep, grid):
    """the texts of one sweep under one grid (what the child runs, and what the GPU test counts)"""
    if sweep in FAMILIES:
        return family_cases(sweep, grid)[0]
    if sweep in TAILS:
        return tail_cases(sweep, grid)[0]
    return {"own": own_cases, "busy": busy_cases, "multi": multi_cases}[sweep](grid)[0]


def text_count(sweep, grid):
    return len(cases_of(sweep, grid))


# ---- the anchor: the production geometry
ANCHOR_N = 34 * 1024 * CHUNK        # 34816 chunks = 272 workgroups x 128: spans of exactly 32 chunks, F = 32 (7 iterations, epilogue, one plain chunk)
ANCHOR_RX = (b"agggtaaa|tttaccct", b"regexpqz", b"qzvw")
ANCHOR_STRINGS = (b"agggtaaa", b"regexpqz", b"qzvw", b"tttaccct")


@functools.lru_cache(maxsize=None)
def anchor_plants():
    """No override: every chunk seam (S01 ... E2P, PP is not in a span of 32: its one plain chunk ends the span -- SW / SG) of a
    dozen spans spread over the text -> (plans per pattern, [(start, string, tags, seam)], coverage)"""
    plans = {rx: WPlan(ANCHOR_N, None, None, 0, len(rx.split(b"|")[0])) for rx in ANCHOR_RX}
    plan = plans[ANCHOR_RX[0]]
    busy = plan.busy()
    picks = sorted({0, 1, 2, 3, 7, len(busy) // 3 + 1, len(busy) // 3, len(busy) // 3 + 3, len(busy) // 2, len(busy) // 2 + 3, len(busy) - 6, len(busy) - 5, len(busy) - 2, len(busy) - 1})
    cover = Coverage()
    out = []
    used = {}
    k = 0
    for i in picks:
        w = busy[i]
        for pos, tags in plan.seams_of(w, i + 1 < len(busy)):
            s = min(ANCHOR_STRINGS, key=lambda q: (used.get((tags[0], q), 0), (ANCHOR_STRINGS.index(q) + k) % len(ANCHOR_STRINGS)))
            used[(tags[0], s)] = used.get((tags[0], s), 0) + 1
            kk = min(range(len(s) + 2), key=lambda q: (cover.count(tags[0], len(s), q), (q + k) % (len(s) + 2)))
            cover.add(tags, len(s), kk)
            out.append((pos - len(s) + kk, s, tags, pos))
            k += 1
    return plans, out, cover




# ------------------------------------------------------------------------------------------------ the driver
class WReport(Report):
    def miss(self, case, pos, pattern, what, got, want):
        self.mismatches += 1
        cls, off = case.describe(pos) if pos is not None else ("-", 0)
        role = cls.split(":")[1].split("+")[0] if ":" in cls else "-"
        print("MISMATCH %s pattern=%r n=%d grid=%s seam=%s role=%s offset=%+d %s: got %s want %s  [%s]"
              % (self.family, pattern, case.n, self.grid, cls, role, off, what, got, want, case.label), flush=True)
        if self.mismatches >= 10:
            self.done()

    def fail(self, text):
        self.mismatches += 1
        print("MISMATCH %s grid=%s: %s" % (self.family, self.grid, text), flush=True)


def check_info(rep, prog, rx, want):
    info = prog.info()
    got = {k: info[k] for k in want}
    if got != want:
        rep.fail("%r: Program.info() says %s, the family table assumes %s" % (rx, got, want))
    return info


def spans_near(spans, pos):
    return [s for s in spans if pos is not None and abs(s[0] - pos) < 64][:2]


def compare(rep, case, rx, what, got, count, want):
    if got != want or count != len(want):
        pos = first_difference(got, want)
        rep.miss(case, pos, rx, "%s: spans at %s (count %d, %d / %d spans)" % (what, pos, count, len(got), len(want)), spans_near(got, pos), spans_near(want, pos))


def run_spans(scan, t, n, own):
    kw = {} if own is None else {"own_begin": own[0], "own_end": own[1]}
    count = scan.run(t.data_ptr(), n, **kw)
    return (scan.spans() if count else []), count


def check_program(rep, be, oracle, rx, cases, want_info, fresh=False, counts=True):
    prog = be.rj.Program(rx)
    info = check_info(rep, prog, rx, want_info)
    scan, counter = be.rj.Scan(prog), be.rj.Scan(prog)
    for case in cases:
        t = be.device_text(case.text)
        want = oracle_spans(oracle, rx, case.text, case.own)
        rep.texts += 1
        got, count = run_spans(scan, t, case.n, case.own)
        compare(rep, case, rx, "run", got, count, want)
        if counts and case.own is None:
            c = counter.count(t.data_ptr(), case.n)
            if c != len(want):
                rep.miss(case, None, rx, "Scan.count", c, len(want))
    return info


def check_busy(rep, be, oracle, cases):
    for case in cases:
        fam = FAMILIES[case.family]
        prog = be.rj.Program(fam["rx"])
        scan = be.rj.Scan(prog)             # fresh: the first run starts from the smallest regions
        t = be.device_text(case.text)
        want = oracle_spans(oracle, fam["rx"], case.text, None)
        rep.texts += 1
        for attempt in range(3):
            got, count = run_spans(scan, t, case.n, None)
            retries = scan.stats()["retries"]
            compare(rep, case, fam["rx"], "run %d (retries %d)" % (attempt, retries), got, count, want)
            if attempt == 0 and retries < 1:
                rep.miss(case, None, fam["rx"], "retries of the first run", retries, ">= 1")
        c = be.rj.Scan(prog).count(t.data_ptr(), case.n)
        if c != len(want):
            rep.miss(case, None, fam["rx"], "Scan.count", c, len(want))


def check_multi(rep, be, oracle, cases):
    progs = [be.rj.Program(rx) for rx in DNA9]
    multis = []
    for mode in (1, 2):
        m = be.rj.MultiScan(progs)
        m.set_mode(mode)
        multis.append((mode, m))
    for case in cases:
        t = be.device_text(case.text)
        want = [oracle_spans(oracle, rx, case.text, None) for rx in DNA9]
        rep.texts += 1
        for mode, m in multis:
            counts = m.run(t.data_ptr(), case.n)
            for i, rx in enumerate(DNA9):
                got = m.scan(i).spans() if counts[i] else []
                compare(rep, case, rx, "mode %d (how %d)" % (mode, m.how), got, counts[i], want[i])


def check_anchor(rep, be):
    """34 MiB at the geometry scan_geometry picks itself: three patterns across the chunk seams of a dozen spans of 32 chunks,
    checked with an independent sliding compare in torch on the device."""
    torch = be.torch
    assert not os.environ.get("RJ_SCAN_GRID"), "the anchor runs without an override"
    plans, plants, _ = anchor_plants()
    for plan in plans.values():
        assert plan.span_chunks == 32 and plan.grid == 272 and all(w.fast == 32 for w in plan.busy()[:-1]), (plan.span_chunks, plan.grid)
    n = ANCHOR_N
    host = bytearray(b"-") * n
    for start, s, _, _ in plants:
        host[start:start + len(s)] = s
    d = be.device_text(bytes(host))
    case = Case("anchor n=%d" % n, None, b"", plants)
    case.text = host
    rep.texts += 1
    for rx in ANCHOR_RX:
        alts = rx.split(b"|")
        L = len(alts[0])
        hit = torch.zeros(n - L + 1, dtype=torch.bool, device=d.device)
        for alt in alts:
            m = torch.ones(n - L + 1, dtype=torch.bool, device=d.device)
            for k, byte in enumerate(alt):
                m &= d[k:n - L + 1 + k] == byte
            hit |= m
        truth = [(b, b + L) for b in torch.nonzero(hit).flatten().cpu().tolist()]
        planted = sum(1 for p in plants if p[1] in alts)
        if len(truth) != planted:
            rep.miss(case, None, rx, "the sliding compare against the plants", len(truth), planted)
        scan = be.rj.Scan(be.rj.Program(rx))
        got, count = run_spans(scan, d, n, None)
        compare(rep, case, rx, "run", got, count, truth)
    print("anchor: %d plants over spans of %d chunks, grid %d" % (len(plants), plans[ANCHOR_RX[0]].span_chunks, plans[ANCHOR_RX[0]].grid), flush=True)


def family_info(fam):
    return dict(scan_mode=1, n_windows=fam["K"], window_offset=fam["offset"], window_len=fam["wlen"])


def tail_info(name):
    return dict(scan_mode=1, window_offset=TAILS[name]["window"][0], window_len=TAILS[name]["window"][1])


def main(argv):
    sweep = argv[1]
    grid = int(os.environ.get("RJ_SCAN_GRID", "0") or 0)
    from checkers import Oracle
    oracle = Oracle()
    rep = WReport(sweep, grid or "auto")
    be = GpuBackend()
    if sweep == "anchor":
        check_anchor(rep, be)
        rep.done()
    assert grid and os.environ.get("RJ_NO_SMALL"), "RJ_SCAN_GRID and RJ_NO_SMALL must be set"
    if sweep == "dispatch":       # one text of every family: the run whose kernel trace is profiles/window_sweep_kernels.txt
        for name, fam in FAMILIES.items():
            print("dispatch %s %r" % (name, fam["rx"]), flush=True)
            check_program(rep, be, oracle, fam["rx"], family_cases(name, grid)[0][1:2], family_info(fam), counts=False)
        for name in TAILS:
            info = check_program(rep, be, oracle, TAILS[name]["rx"], tail_cases(name, grid)[0][:1], tail_info(name), counts=False)
            print("dispatch %s %r info %s" % (name, TAILS[name]["rx"], info), flush=True)
        check_multi(rep, be, oracle, multi_cases(grid)[0][:1])
    elif sweep in FAMILIES:
        check_program(rep, be, oracle, FAMILIES[sweep]["rx"], cases_of(sweep, grid), family_info(FAMILIES[sweep]))
    elif sweep in TAILS:
        info = check_program(rep, be, oracle, TAILS[sweep]["rx"], cases_of(sweep, grid), tail_info(sweep))
        print("%s %r info %s" % (sweep, TAILS[sweep]["rx"], info), flush=True)
    elif sweep == "own":
        cases = cases_of("own", grid)
        for name in OWN_FAMILIES:
            check_program(rep, be, oracle, FAMILIES[name]["rx"], [c for c in cases if c.family == name], family_info(FAMILIES[name]))
    elif sweep == "busy":
        check_busy(rep, be, oracle, cases_of("busy", grid))
    elif sweep == "multi":
        check_multi(rep, be, oracle, cases_of("multi", grid))
    else:
        raise KeyError(sweep)
    rep.done()


if __name__ == "__main__":
    main(sys.argv)
