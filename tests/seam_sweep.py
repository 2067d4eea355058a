"""Seam sweep of the plane kernels' streaming loop (rejit_amd/csrc/plane_count.hip) on small texts.

Two things live here.

* A case PLANNER, pure Python, no GPU (tests/test_seam_plan.py checks it against tests/support/plane_args_exec.cc and
  asserts its coverage).  It restates the arithmetic of rejit_amd/csrc/plane_args.h (plane_blocks, plane_split), of
  scan_geometry (scan_windows.hip) under a forced grid and of the kernel's own c0 / c1 / full / fast_end, and returns per
  wave the span's blocks with their roles, the seams of the text with their classes, and the texts: a background that can
  neither match nor be a candidate, one planted string at every seam, its start at seam - L ... seam + 1.
* The child DRIVER, `python tests/seam_sweep.py FAMILY`, which tests/test_gpu_seams.py starts once per (family, grid) with
  RJ_SCAN_GRID in the environment (the library reads it once per process).  For every planned text it compares the
  counts-only run (counts, return value, bounds), and the span lists of a default run of the same set, with the oracle.

Seam classes (a seam is the boundary before byte `pos`):
  LA / LB   a 16-byte lane seam inside piece A / piece B, lanes 0|1, 31|32, 62|63
  P         the piece seam, block offset 1024 (lane 63's piece A meets lane 0's piece B)
  B01 / B12 a block seam inside one loop iteration (span-relative even -> odd) / across two iterations (odd -> even)
  BH2 / BH1 behind the span's last fast block when the loop leaves through `c + 2 == fast_end` / through the odd-block arm
  SW / SG   a span seam between two waves of one workgroup / between two workgroups
  GF / GG   fast block -> guarded block / guarded -> guarded, inside one span
  GE        the end of the text
"""
import bisect
import os
import sys

BLOCK = 2048
PIECE = 1024
TAGS = ("LA", "LB", "P", "B01", "B12", "BH2", "BH1", "SW", "SG", "GF", "GG", "GE")
SPAN_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17)
TAILS = (0, 1, 7, 8, 9, 1024, 2047)
MIN_GAP = 24


# ------------------------------------------------------------------------------------------------ the arithmetic
def plane_blocks(n, sb, se, min_offset, max_offset, n_cmp):
    """plane_args.h: plane_blocks -> (wlo, whi, first_block, end_block)"""
    last_w = n - n_cmp + 1 if n >= n_cmp else 0
    wlo = sb + min_offset
    whi = min(se + max_offset, last_w)
    first = wlo // BLOCK
    end = (whi + BLOCK - 1) // BLOCK if whi > wlo else first
    return wlo, whi, first, end


def plane_split(blocks, n_regions):
    """plane_args.h: plane_split -> (span_blocks, span_extra)"""
    return blocks // n_regions, blocks % n_regions


def scan_geometry(chunks, chunks_per_block=128, forced_grid=None):
    """scan_windows.hip: scan_geometry -> (grid, n_regions, span_chunks); forced_grid = RJ_SCAN_GRID"""
    blocks = min(chunks // chunks_per_block, 16384)
    if blocks < 256:
        blocks = min((chunks + 3) // 4, 256)
    blocks = max(blocks, 1)
    if forced_grid:
        blocks = forced_grid
    n_regions = blocks * 4
    return blocks, n_regions, max((chunks + n_regions - 1) // n_regions, 1)


class Wave:
    """One wave's view of a launch: its blocks [c0, c1), of which [c0, fast_end) take the unguarded loop."""

    def __init__(self, index, c0, c1, fast_end):
        self.index, self.c0, self.c1, self.fast_end = index, c0, c1, fast_end

    @property
    def length(self):
        return self.c1 - self.c0

    @property
    def fast(self):
        return self.fast_end - self.c0

    def roles(self, c):
        """the roles of block c of this span"""
        r = {"first": c == self.c0, "odd": bool((c - self.c0) & 1), "guarded": c >= self.fast_end}
        r["last_fast"] = self.fast > 0 and c == self.fast_end - 1
        return r


class Plan:
    """The launch of a plane kernel over the starts [sb, se) of a text of n bytes."""

    def __init__(self, n, own, grid, min_offset, max_offset, n_cmp, chunks_per_block=128):
        self.n, self.window = n, (min_offset, max_offset, n_cmp)
        self.sb, self.se = (0, n + 1) if own is None else (own[0], min(own[1], n + 1))
        self.wlo, self.whi, self.first_block, self.end_block = plane_blocks(n, self.sb, self.se, min_offset, max_offset, n_cmp)
        self.blocks = self.end_block - self.first_block
        self.grid, self.n_regions, _ = scan_geometry(max(self.blocks * 2, 1), chunks_per_block, grid)
        self.span_blocks, self.span_extra = plane_split(self.blocks, self.n_regions)
        full = n // BLOCK
        self.waves = []
        for w in range(self.n_regions):
            c0 = self.first_block + w * self.span_blocks + min(w, self.span_extra)
            c1 = c0 + self.span_blocks + (1 if w < self.span_extra else 0)
            fast_end = full - 1 if full >= 1 else 0
            fast_end = max(min(fast_end, c1), c0)
            self.waves.append(Wave(w, c0, c1, fast_end))

    def span_lengths(self):
        """(length, place) of every wave with blocks: place = 'first', 'interior' or 'last'"""
        busy = [w for w in self.waves if w.length]
        out = []
        for i, w in enumerate(busy):
            if i == 0:
                out.append((w.length, "first"))
            if i == len(busy) - 1:
                out.append((w.length, "last"))
            if 0 < i < len(busy) - 1:
                out.append((w.length, "interior"))
        return out

    def seams(self):
        """[(pos, (tags...))] in text order"""
        out = []
        busy = [w for w in self.waves if w.length]
        for i, w in enumerate(busy):
            for c in range(w.c0, w.c1):
                base = c * BLOCK
                for lane in (1, 32, 63):
                    out.append((base + 16 * lane, ("LA",)))
                out.append((base + PIECE, ("P",)))
                for lane in (1, 32, 63):
                    out.append((base + PIECE + 16 * lane, ("LB",)))
                r = w.roles(c)
                tags = []
                if r["last_fast"]:
                    tags.append("BH1" if w.fast & 1 else "BH2")
                if c + 1 < w.c1:
                    nxt = w.roles(c + 1)
                    if not r["guarded"] and not nxt["guarded"]:
                        tags.append("B12" if r["odd"] else "B01")
                    elif not r["guarded"]:
                        tags.append("GF")
                    else:
                        tags.append("GG")
                elif i + 1 < len(busy):
                    tags.append("SG" if (w.index + 1) % 4 == 0 else "SW")
                else:
                    continue   # the text's last block: its end is the end of the text, or lies behind it
                out.append((base + BLOCK, tuple(tags)))
        out = [(p, t) for p, t in out if p < self.n]
        out.append((self.n, ("GE",)))
        return out

    def tags_at(self, pos, reach=24):
        """the classes of the seam nearest to pos (diagnostics)"""
        best = min(self.seams(), key=lambda s: abs(s[0] - pos))
        return best if abs(best[0] - pos) <= reach else (pos, ("-",))


# ------------------------------------------------------------------------------------------------ the families
def _one_off(bases, letters):
    out = []
    for b in bases:
        out.append(b)
        for j in range(len(b)):
            for c in letters:
                s = b[:j] + bytes([c]) + b[j + 1:]
                if s not in out:
                    out.append(s)
    return out


DNA9 = [b"agggtaaa|tttaccct", b"[cgt]gggtaaa|tttaccc[acg]", b"a[act]ggtaaa|tttacc[agt]t", b"ag[act]gtaaa|tttac[agt]ct", b"agg[act]taaa|ttta[agt]cct",
        b"aggg[acg]aaa|ttt[cgt]ccct", b"agggt[cgt]aa|tt[acg]accct", b"agggta[cgt]a|t[acg]taccct", b"agggtaa[cgt]|[acg]ttaccct"]

# rx: the set; plants: strings that match (or nearly match) a pattern, planted at the seams; near: candidates that classify
# to nothing (the busy ring); window: (min window offset, max window offset, n_cmp) as Program.info() reports them -- the
# driver checks that -- ; kernels: the instantiations the set is expected to dispatch (profiles/seam_sweep_kernels.txt)
FAMILIES = {
    "dna9": dict(rx=DNA9, plants=_one_off([b"agggtaaa", b"tttaccct"], b"acgt"), near=[b"agggxaaa", b"tttaxcct", b"xgggtaaa", b"tttacccx"],
                 window=(0, 0, 8), exact=True, kernels=("ExactShape<2>", "ListShape<2>")),
    "one_base": dict(rx=[b"abcdefgh", b"abc[\x80-\xff]efgh", b"xbcdefgh", b"abcdef[^g]h"],
                     plants=[b"abcdefgh", b"abc\x80efgh", b"abc\xffefgh", b"abcdefxh", b"abcdef\x00h", b"xbcdefgh", b"abcdeggh", b"abcdefgg"],
                     near=[b"abcdeQgh", b"aQcdefgh"], window=(0, 0, 8), kernels=("GeneralShape<1, 8, true>", "GeneralListShape<true>")),
    # (eight distinct bytes in the base: plan_plane, which takes at most four, refuses one_base and the general kernels run it.
    # dna1 is the one-base set the 8-mer table takes: the `agggtaaa` halves of regexdna's nine)
    "dna1": dict(rx=[rx.split(b"|")[0] for rx in DNA9], plants=_one_off([b"agggtaaa"], b"acgt"), near=[b"agggxaaa", b"xgggtaaa"],
                 window=(0, 0, 8), exact=True, kernels=("ExactShape<1>", "ListShape<1>")),
    "kmer6": dict(rx=[b"qwerty", b"asdfgh", b"zxcvbn", b"poiuyt", b"lkjhgf", b"mnbvcx"], plants=[b"qwerty", b"asdfgh", b"zxcvbn", b"poiuyt", b"lkjhgf", b"mnbvcx", b"qwertz"],
                  near=[b"qwertz"], window=(0, 0, 6), kernels=("GeneralShape<1, 8, false>", "GeneralListShape<false>")),
    "kmer6_class": dict(rx=[b"ab[cx]def", b"ab[yz]def"], plants=[b"abcdef", b"abxdef", b"abydef", b"abzdef", b"abqdef"], near=[b"abqdef"],
                        window=(0, 0, 6), kernels=("GeneralShape<1, 8, true>", "GeneralListShape<true>")),
    "alt16": dict(rx=[b"alternation|strings", b"prefix abcd|prefix 1234"], plants=[b"alternation", b"strings", b"prefix abcd", b"prefix 1234", b"prefix abc4", b"stringz"],
                  near=[b"prefix abc4"], window=(0, 1, 7), kernels=("GeneralShape<1, 16, false>", "GeneralListShape<false>")),
    "alt16_class": dict(rx=[b"ab[cx]defghij", b"mno[0-9]pqrstu"], plants=[b"abcdefghij", b"abxdefghij", b"mno5pqrstu", b"mno0pqrstu", b"abqdefghij", b"mnoapqrstu"],
                        near=[b"abqdefghij"], window=(0, 0, 8), kernels=("GeneralShape<1, 16, true>", "GeneralListShape<true>")),
    "wide": dict(rx=[b"abcdefghijkl|mnopqrstuvwx|yz0123456789|9876543210zy", b"0123456789ab|cdefghijklmn|opqrstuvwxyz"],
                 plants=[b"abcdefghijkl", b"mnopqrstuvwx", b"yz0123456789", b"9876543210zy", b"0123456789ab", b"cdefghijklmn", b"opqrstuvwxyz", b"abcdefghijk#"],
                 near=[b"abcdefghijk#"], window=(0, 0, 8), kernels=("GeneralShape<2, 16, false>", "GeneralListShape<false>")),
    # (a class that every 8-byte window of its alternative holds: the plan cannot step round it)
    "wide_class": dict(rx=[b"abcd[ex]fghijkl|mnopqrstuvwx|yz0123456789|9876543210zy"],
                       plants=[b"abcdefghijkl", b"abcdxfghijkl", b"mnopqrstuvwx", b"yz0123456789", b"9876543210zy", b"abcd#fghijkl"],
                       near=[b"abcd#fghijkl"], window=None, kernels=("GeneralShape<2, 16, true>", "GeneralListShape<true>")),
    "prefix": dict(rx=[b"abcd|abcdefgh", b"efgh1234"], plants=[b"abcd", b"abcdefgh", b"abcdefgh1234", b"abcdabcd", b"efgh1234", b"abcdefg1"],
                   near=[b"abcQ"], window=(0, 0, 4), cover=(4, 8), pairs=(b"abcdabcd",), kernels=("GeneralShape<1, 8, false>",)),
    "offset": dict(rx=[b"[ab]cdefghij", b"[xy]cdefghiq"], plants=[b"acdefghij", b"bcdefghij", b"ccdefghij", b"xcdefghiq", b"ycdefghij"],
                   near=[b"ccdefghij"], window=(1, 1, 8), kernels=("GeneralShape<1, 16, false>",)),
}
VARIANTS = ("own", "busy", "pairs", "pairs_general", "void")   # (of dna9, pairs_general of `abab|baba`)
CHAIN_RX = [b"abab|baba", b"ababab"]
SINGLE_RX = [b"qz", b"qzvwx", b"regexpqz", b"[q-s]+z"]           # tests/test_gpu_parity.py's needles, and a pattern the dense walk takes
GRIDS = (1, 2, 3)

# (full blocks, tail): every tail of TAILS, every span length of SPAN_LENGTHS as first, interior and last span over the grids
GEOMETRIES = [(4, 0), (8, 1), (12, 7), (16, 8), (20, 9), (32, 1024), (36, 2047), (64, 0), (68, 1), (7, 8), (35, 9), (67, 1024), (3, 2047), (33, 7),
              (2, 8), (17, 0), (9, 1024), (5, 9), (1, 1), (66, 2047), (24, 8), (40, 7), (10, 0), (6, 1)]


def window_of(name):
    w = FAMILIES[name]["window"]
    return w if w is not None else (0, 0, 8)   # (not known before the program is compiled; over a whole text the blocks do not depend on it)


def pick_background(strings, width):
    """A byte that no planted string holds and whose 2-bit code (byte >> shift) & 3 differs, under every shift a plan can
    choose, from the codes of as many bytes as possible of every `width`-byte piece of a planted string: a run of it is
    never a candidate, exactly or within one code.  Returns (byte, the smallest number of differing codes)."""
    used = set(b"".join(strings))
    best = None
    for x in list(range(0x21, 0x7f)) + [0x0a] + list(range(0x80, 0x100)):
        if x in used:
            continue
        worst = 99
        for sh in range(7):
            cx = (x >> sh) & 3
            for s in strings:
                for i in range(0, max(len(s) - width, 0) + 1):
                    piece = s[i:i + width]
                    worst = min(worst, sum(1 for b in piece if (b >> sh) & 3 != cx) + max(width - len(piece), 0))
        if best is None or worst > best[1]:
            best = (x, worst)
    return best


class Coverage:
    def __init__(self):
        self.seen = {}

    def count(self, tag, length, k):
        return self.seen.get((tag, length, k), 0)

    def add(self, tags, length, k):
        for t in tags:
            self.seen[(t, length, k)] = self.count(t, length, k) + 1

    def missing(self, lengths, tags=TAGS):
        out = []
        for t in tags:
            for length in lengths:
                for k in ([0] if t == "GE" else range(length + 2)):
                    if self.count(t, length, k) == 0:
                        out.append((t, length, k - length))
        return out


class Case:
    def __init__(self, label, plan, text, plants, own=None, expect_how=3):
        self.label, self.plan, self.text, self.plants, self.own, self.expect_how = label, plan, text, plants, own, expect_how

    @property
    def n(self):
        return len(self.text)

    def describe(self, pos):
        """seam class and offset of the plant nearest to pos"""
        if not self.plants:
            return "-", 0
        starts = [p[0] for p in self.plants]
        i = max(bisect.bisect_right(starts, pos) - 1, 0)
        if i + 1 < len(starts) and abs(starts[i + 1] - pos) < abs(starts[i] - pos):
            i += 1
        start, s, tags, seam = self.plants[i]
        return "+".join(tags), start - seam


def plant_text(n, seams, strings, bg, cover, rot, only=None, keep_clear=(), no_cross=(), rare=None, text=None, placed=None):
    """One string at every seam that has room: (text, [(start, string, tags, seam)]).  The (length, offset) pair of a seam is
    the one its classes have seen least so far (`cover`), so the offsets rotate over the seams of a text and over the texts
    of a family; which of two seams closer than a plant + MIN_GAP is served first rotates with `rot`.  `rare` ranks other
    seam classes than this module's (tests/window_sweep.py); `text` and `placed` continue an earlier call's text."""
    text = bytearray([bg]) * n if text is None else text
    by_len = {}
    for s in strings:
        by_len.setdefault(len(s), []).append(s)
    rare = rare if rare is not None else {"OWN": 0, "SG": 0, "GE": 0, "GF": 0, "GG": 0, "BH1": 0, "BH2": 0, "SW": 1, "B01": 2, "B12": 2, "P": 3 + rot % 2, "LA": 3 + (rot + 1) % 2, "LB": 3 + (rot + 1) % 2}
    order = sorted(range(len(seams)), key=lambda i: (min(rare[t] for t in seams[i][1]), seams[i][0]))
    placed = [] if placed is None else placed   # sorted (start, end)
    out = []
    for i in order:
        pos, tags = seams[i]
        if only is not None and not (set(tags) & set(only)):
            continue
        options = []
        for length in by_len:
            for k in ([0] if tags == ("GE",) else range(length + 2)):
                start = pos - length + k
                if start < 0 or start + length > n:
                    continue
                options.append((min(cover.count(t, length, k) for t in tags), sum(cover.count(t, length, k) for t in tags), (k + rot) % (length + 2), length, k))
        for _, _, _, length, k in sorted(options)[:6]:
            start = pos - length + k
            j = bisect.bisect_left(placed, (start, 0))
            if j > 0 and placed[j - 1][1] + MIN_GAP > start:
                continue
            if j < len(placed) and start + length + MIN_GAP > placed[j][0]:
                continue
            if any(lo - MIN_GAP < start + length and start < hi + MIN_GAP for lo, hi in keep_clear):
                continue
            if any(start < x < start + length for x in no_cross):
                continue
            pool = by_len[length]
            s = pool[(sum(cover.count(t, length, kk) for t in tags for kk in range(length + 2)) + rot) % len(pool)]
            text[start:start + length] = s
            placed.insert(j, (start, start + length))
            cover.add(tags, length, k)
            out.append((start, s, tags, pos))
            break
    out.sort()
    return bytes(text), out


def family_cases(name, grid):
    """The texts of one sweep family under a forced grid."""
    fam = FAMILIES[name]
    lo, hi, n_cmp = window_of(name)
    bg, _ = pick_background(fam["plants"], n_cmp)
    cover = Coverage()
    cases = []
    # ... and per grid spans of 2, 3 and 4 blocks at the end of the text, which hold both guarded blocks (GF, GG)
    extra = [(k * 4 * grid - 1, tail) for tail in (8, 9, 1024, 2047) for k in (3, 4, 2)] + [(5 * 4 * grid - 1, 8), (5 * 4 * grid - 1, 1024)]
    for rot, (full, tail) in enumerate(GEOMETRIES + extra):
        n = full * BLOCK + tail
        plan = Plan(n, None, grid, lo, hi, n_cmp)
        text, plants = plant_text(n, plan.seams(), fam["plants"], bg, cover, rot)
        # a planted string that holds two matches of one pattern, cut by a span seam: the documented answer is a void run
        cut = [x for x, tags in plan.seams() if set(tags) & {"SW", "SG"}]
        pair_cut = any(s in fam.get("pairs", ()) and start < x < start + len(s) for start, s, _, _ in plants for x in cut)
        cases.append(Case("%s n=%d" % (name, n), plan, text, plants, expect_how=None if pair_cut else 3))
    return cases, cover


def own_cases(grid):
    """dna9 with own ranges that begin / end at a seam +- 0..8: first_block > 0 and span_base != 0 for wave 0."""
    fam = FAMILIES["dna9"]
    bg, _ = pick_background(fam["plants"], 8)
    cover = Coverage()
    cases = []
    k = 0
    for full, tail in ((36, 9), (33, 1024)):
        n = full * BLOCK + tail
        for seam in (3 * BLOCK, 5 * BLOCK + PIECE, 9 * BLOCK + 16 * 63, 20 * BLOCK):
            for d in range(-8, 9):
                k += 1
                if (k + full) % 2:
                    own = (seam + d, n + 1) if k % 4 < 2 else (0, seam + d)
                else:
                    own = (seam + d, seam + d + 18 * BLOCK + (k % 9))
                plan = Plan(n, own, grid, 0, 0, 8)
                text, plants = plant_text(n, Plan(n, None, grid, 0, 0, 8).seams() + [(own[0], ("OWN",)), (min(own[1], n), ("OWN",))], fam["plants"], bg, cover, k)
                cases.append(Case("own n=%d own=%s" % (n, own), plan, text, plants, own=own))
    return cases[grid - 1::3], cover   # (a third of them per grid)


def busy_cases(grid):
    """dna9: a near-miss (a candidate that classifies to nothing) every 40 bytes, real matches among them: batches of 64
    fire inside the loop and the ring wraps several times per span."""
    fam = FAMILIES["dna9"]
    bg, _ = pick_background(fam["plants"], 8)
    cover = Coverage()
    cases = []
    for rot, (full, tail) in enumerate(((32, 1024), (36, 9), (35, 8), (64, 1), (17, 7))):
        n = full * BLOCK + tail
        plan = Plan(n, None, grid, 0, 0, 8)
        text, plants = plant_text(n, plan.seams(), fam["plants"], bg, cover, rot)
        t = bytearray(text)
        at = 3 + rot
        k = 0
        for start, s, _, _ in plants + [(n + 100, b"", (), 0)]:
            while at + 8 + MIN_GAP <= start and at + 8 <= n:
                t[at:at + 8] = fam["near"][k % len(fam["near"])] if k % 5 else fam["plants"][k % len(fam["plants"])]
                k += 1
                at += 40 - (k % 3)
            at = max(at, start + len(s) + MIN_GAP)
        cases.append(Case("busy n=%d" % n, plan, bytes(t), plants))
    return cases, cover


def pair_cases(grid, general=False):
    """Overlapping pairs and chains across every seam: inside a span the kernel resolves them (return value 3); across a
    span seam (SW, SG) the documented answer is a void run that the span pipeline answers."""
    if general:
        strings, win = [b"ababab", b"abababab", b"bababab", b"ababababab"], (0, 0, 4)
        bg = pick_background(strings, 4)[0]
    else:
        strings, bg, win = [b"agggtaaagggtaaa", b"agggtaaagggtaaagggtaaa", b"tttaccctttaccct"], pick_background(FAMILIES["dna9"]["plants"], 8)[0], (0, 0, 8)
    cover = Coverage()
    cases = []
    R = 4 * grid
    geos = [(3 * R - 1, 1024), (4 * R - 1, 2047), (3 * R - 1, 9), (2 * R + 1, 7), (3 * R - 1, 2047), (5 * R - 1, 1024), (3 * R - 1, 8), (4 * R - 1, 1024)]
    for rot in range(56):
        full, tail = geos[rot % len(geos)]
        n = full * BLOCK + tail
        plan = Plan(n, None, grid, *win)
        seams = plan.seams()
        inner = [s for s in seams if not (set(s[1]) & {"SW", "SG"})]
        outer = [s for s in seams if set(s[1]) & {"SW", "SG"}]
        text, plants = plant_text(n, inner, strings, bg, cover, rot, no_cross=[x for x, _ in outer])   # (a lane seam's string may reach a span seam)
        cases.append(Case("pairs n=%d rot=%d" % (n, rot), plan, text, plants))
        if outer:
            text, plants = plant_text(n, outer, strings, bg, cover, rot)
            cases.append(Case("pairs at span seams n=%d rot=%d" % (n, rot), plan, text, plants, expect_how=None))
    return cases, cover


def void_cases(grid):
    """40 KiB: `agggtaaa` back to back over one span (256 candidates per block, more than the ring takes between two looks at
    it) beside spans with ordinary plants: the run is void (return value 1, the oracle's counts); a clean text follows."""
    fam = FAMILIES["dna9"]
    bg, _ = pick_background(fam["plants"], 8)
    n = 20 * grid * BLOCK      # (spans of five blocks under every grid)
    plan = Plan(n, None, grid, 0, 0, 8)
    wave = next(w for w in plan.waves if w.fast >= 4)
    lo, hi = wave.c0 * BLOCK + 8, (wave.c0 + 3) * BLOCK
    cover = Coverage()
    text, plants = plant_text(n, plan.seams(), fam["plants"], bg, cover, 0, keep_clear=[(lo, hi)])
    clean = Case("void: clean before", plan, text, plants)
    t = bytearray(text)
    t[lo:hi] = b"agggtaaa" * ((hi - lo) // 8)
    return [clean, Case("void n=%d" % n, plan, bytes(t), plants, expect_how=1), Case("void: clean after", plan, text, plants)], cover


# ---- the single-pattern scans (engine.hip takes its geometry from scan_geometry too): 1-KiB chunks, n_regions waves
def single_seams(n, grid):
    chunks = max((n + 1023) // 1024, 1)
    _, n_regions, span = scan_geometry(chunks, 128, grid)
    out = []
    for c in range(chunks):
        base = c * 1024
        for lane in (1, 32, 63):
            out.append((base + 16 * lane, ("LA",)))
        if c:
            out.append((base, ("SW",) if c % span == 0 else ("P",)))
    out = [(p, t) for p, t in out if 0 < p < n]
    out.append((n, ("GE",)))
    return sorted(out), span


def single_cases(grid):
    """One text per needle and geometry with 4- and 9-chunk spans: 16-byte, 1-KiB and span seams."""
    cases = []
    covers = []
    for needle in (b"qz", b"qzvwx", b"regexpqz", b"rsqz"):
        cover = Coverage()
        for rot, chunks in enumerate((4 * 4 * grid, 9 * 4 * grid, 4 * 4 * grid - 1, 9 * 4 * grid - 3)):
            for tail in (0, 7):
                n = chunks * 1024 + tail
                seams, span = single_seams(n, grid)
                text, plants = plant_text(n, seams, [needle], ord("a") + rot, cover, rot + tail)
                c = Case("single %r n=%d span=%d" % (needle, n, span), None, text, plants)
                c.needle = needle
                cases.append(c)
        covers.append(cover)
    return cases, covers


def cases_of(family, grid):
    if family in FAMILIES:
        return family_cases(family, grid)
    if family == "own":
        return own_cases(grid)
    if family in ("busy", "busy7"):
        return busy_cases(grid)
    if family == "pairs":
        return pair_cases(grid)
    if family == "pairs_general":
        return pair_cases(grid, general=True)
    if family == "void":
        return void_cases(grid)
    raise KeyError(family)


def _anchor_seams(plan):
    """the P, block, behind-span and span seams of a dozen spans of a production launch, spread over the text"""
    want = ("P", "B01", "B12", "BH1", "BH2", "SW", "SG")
    busy = [w for w in plan.waves if w.length]
    picks = sorted({0, 1, 2, 3, 4, len(busy) // 3, len(busy) // 3 + 3, len(busy) // 2, len(busy) // 2 + 3, len(busy) - 6, len(busy) - 5, len(busy) - 2})
    seams = []
    for i in picks:
        sub = Plan.__new__(Plan)
        sub.n, sub.waves = plan.n, busy[i:i + 2]
        for pos, tags in Plan.seams(sub):
            t = tuple(x for x in tags if x in want)
            if t and pos < busy[i].c1 * BLOCK + 1 and not (t == ("P",) and (pos // BLOCK) % 5):     # (a P seam in every fifth block)
                seams.append((pos, t))
    return sorted(set(seams))


def anchor_plants(n=34 * 1024 * 1024 + 8 * BLOCK + 9):
    """The production geometry, no override: scan_geometry gives a text of ~34 MiB spans of 16 and 17 blocks by itself (the
    count kernel: 128 chunks per workgroup) and of 12 and 13 blocks for the default run's list kernel (96 chunks per workgroup,
    multi_pattern.hip: plan_batched).  Seams of the classes P, B01, B12, BH1/BH2 and SW/SG of a dozen spans of EACH launch,
    spread over the text -> (n, count plan, [(start, string, tags, seam)], coverage, list plan); the list launch's classes carry
    the suffix `/list`."""
    plan = Plan(n, None, None, 0, 0, 8)
    list_plan = Plan(n, None, None, 0, 0, 8, chunks_per_block=96)
    strings = FAMILIES["dna9"]["plants"]
    seams = {}
    for pos, tags in _anchor_seams(plan):
        seams[pos] = tags
    for pos, tags in _anchor_seams(list_plan):
        seams[pos] = seams.get(pos, ()) + tuple(t + "/list" for t in tags)
    cover = Coverage()
    out = []
    k = 0
    last = -100
    length = 8
    for pos, t in sorted(seams.items()):
        kk = min(range(length + 2), key=lambda q: (min(cover.count(x, length, q) for x in t), (q + k) % 10))
        start = pos - length + kk
        if start < last + MIN_GAP + 8:
            continue
        cover.add(t, length, kk)
        out.append((start, strings[k % len(strings)], t, pos))
        last = start
        k += 1
    return n, plan, out, cover, list_plan


# ------------------------------------------------------------------------------------------------ the driver
class Report:
    def __init__(self, family, grid):
        self.family, self.grid, self.texts, self.mismatches = family, grid, 0, 0

    def miss(self, case, pos, pattern, what, got, want):
        self.mismatches += 1
        cls, off = case.describe(pos) if pos is not None else ("-", 0)
        print("MISMATCH %s n=%d grid=%s seam=%s offset=%+d pattern=%r %s: got %s want %s  [%s]" % (self.family, case.n, self.grid, cls, off, pattern, what, got, want, case.label), flush=True)
        if self.mismatches >= 10:
            self.done()

    def done(self):
        print("checked %d texts, mismatches %d" % (self.texts, self.mismatches), flush=True)
        sys.exit(1 if self.mismatches else 0)


def oracle_spans(oracle, rx, data, own):
    sp = oracle.match_all(rx, data, cap=len(data) // 4 + 16)
    assert not isinstance(sp, int), (rx, sp)
    if own is not None:
        sp = [m for m in sp if own[0] <= m[0] < own[1]]
    return sp


def first_difference(got, want):
    for g, w in zip(got, want):
        if g != w:
            return min(g[0], w[0])
    if len(got) != len(want):
        return (got[len(want)] if len(got) > len(want) else want[len(got)])[0]
    return None


class GpuBackend:
    def __init__(self):
        import numpy as np
        import torch
        assert torch.cuda.is_available(), "the seam sweep needs a GPU"
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import rejit_amd
        rejit_amd.build()
        rejit_amd.load_library()
        self.rj, self.np, self.torch = rejit_amd, np, torch

    def device_text(self, data):
        return self.torch.from_numpy(self.np.frombuffer(data, dtype=self.np.uint8).copy()).cuda()

    def multi(self, rxs, counts_only):
        progs = [self.rj.Program(rx) for rx in rxs]
        m = self.rj.MultiScan(progs)
        took = m.set_counts_only(True) if counts_only else None
        return m, progs, took


def check_multi(rep, be, oracle, rxs, cases, window=None, need_counts_path=True):
    mc, progs, took = be.multi(rxs, True)
    ms, _, _ = be.multi(rxs, False)
    if need_counts_path and not took:
        rep.mismatches += 1
        print("MISMATCH %s: the set does not take the counts path" % rep.family, flush=True)
    if window is not None:
        infos = [p.info() for p in progs]
        got = (min(i["window_offset"] for i in infos), max(i["window_offset"] for i in infos), min(i["window_len"] for i in infos))
        if got != tuple(window):
            rep.mismatches += 1
            print("MISMATCH %s: windows %s, the planner assumes %s" % (rep.family, got, tuple(window)), flush=True)
    for case in cases:
        data, own = case.text, case.own
        t = be.device_text(data)
        kw = {} if own is None else {"own_begin": own[0], "own_end": own[1]}
        want = [oracle_spans(oracle, rx, data, own) for rx in rxs]
        rep.texts += 1
        # the counts-only run: counts, return value, first / last match
        c = mc.run(t.data_ptr(), len(data), **kw)
        how = mc.how
        bounds = mc.bounds()
        for i, rx in enumerate(rxs):
            if c[i] != len(want[i]):
                rep.miss(case, None, rx, "count (how %d)" % how, c[i], len(want[i]))
            wb = (want[i][0][0], want[i][0][1], want[i][-1][0], want[i][-1][1]) if want[i] else None
            if bounds[i] != wb:
                pos = None if wb is None or bounds[i] is None else (wb[0] if wb[:2] != bounds[i][:2] else wb[2])
                rep.miss(case, pos, rx, "bounds (how %d)" % how, bounds[i], wb)
        if case.expect_how is not None and took and how != case.expect_how:
            rep.miss(case, None, b"*", "return value", how, case.expect_how)
        if case.expect_how is None:
            print("note %s: span-seam pairs answered with return value %d" % (case.label, how), flush=True)
        # the default run: every pattern's span list
        s = ms.run(t.data_ptr(), len(data), **kw)
        for i, rx in enumerate(rxs):
            got = ms.scan(i).spans() if s[i] else []
            if got != want[i] or s[i] != len(want[i]):
                pos = first_difference(got, want[i])
                gi = [g for g in got if pos is not None and abs(g[0] - pos) < 32][:2]
                wi = [w for w in want[i] if pos is not None and abs(w[0] - pos) < 32][:2]
                rep.miss(case, pos, rx, "spans at %s (list kernel, how %d; %d / %d spans)" % (pos, ms.how, len(got), len(want[i])), gi, wi)


def check_single(rep, be, oracle, cases):
    scans = {}
    for case in cases:
        rx = b"[q-s]+z" if case.needle == b"rsqz" else case.needle
        if rx not in scans:
            prog = be.rj.Program(rx)
            scans[rx] = be.rj.Scan(prog)
            # the literals scan for their window (scan_windows), `[q-s]+z` has none to scan for: the dense walk
            mode, want_mode = prog.info()["scan_mode"], (0 if case.needle == b"rsqz" else 1)
            if mode != want_mode:
                rep.mismatches += 1
                print("MISMATCH single: %r has scan_mode %d, the family assumes %d" % (rx, mode, want_mode), flush=True)
        t = be.device_text(case.text)
        want = oracle_spans(oracle, rx, case.text, None)
        rep.texts += 1
        count = scans[rx].run_tensor(t)
        got = scans[rx].spans() if count else []
        if got != want:
            pos = first_difference(got, want)
            rep.miss(case, pos, rx, "spans at %s (%d / %d spans)" % (pos, len(got), len(want)), [g for g in got if abs(g[0] - pos) < 32][:2], [w for w in want if abs(w[0] - pos) < 32][:2])


def check_anchor(rep, be):
    """~34 MiB, the production geometry: regexdna strings across seams the planner computes for it, checked with an
    independent sliding compare in torch on the device."""
    torch = be.torch
    n, plan, plants, _, list_plan = anchor_plants()
    assert not os.environ.get("RJ_SCAN_GRID"), "the anchor runs without an override"
    assert plan.span_blocks == 16 and plan.grid >= 256, (plan.span_blocks, plan.grid)
    bg = pick_background(FAMILIES["dna9"]["plants"], 8)[0]
    host = bytearray([bg]) * n
    for start, s, _, _ in plants:
        host[start:start + len(s)] = s
    d = be.device_text(bytes(host))
    case = Case("anchor n=%d" % n, plan, b"", plants)
    case.text = host
    rep.texts += 1
    mc, progs, took = be.multi(DNA9, True)
    ms, _, _ = be.multi(DNA9, False)
    c = mc.run(d.data_ptr(), n)
    how, bounds = mc.how, mc.bounds()
    s = ms.run(d.data_ptr(), n)
    if not took or how != 3:
        rep.miss(case, None, b"*", "return value", how, 3)
    for i, rx in enumerate(DNA9):
        hit = torch.zeros(n - 7, dtype=torch.bool, device=d.device)
        for alt in rx.split(b"|"):
            allowed, j = [], 0
            while j < len(alt):            # (literals and [..] classes of single letters)
                if alt[j:j + 1] == b"[":
                    e = alt.index(b"]", j)
                    allowed.append(alt[j + 1:e])
                    j = e + 1
                else:
                    allowed.append(alt[j:j + 1])
                    j += 1
            assert len(allowed) == 8
            m = torch.ones(n - 7, dtype=torch.bool, device=d.device)
            for k, letters in enumerate(allowed):
                lut = torch.zeros(256, dtype=torch.bool, device=d.device)
                lut[torch.tensor(list(letters), device=d.device)] = True
                m &= lut[d[k:n - 7 + k].long()]
            hit |= m
        truth = torch.nonzero(hit).flatten().cpu().tolist()
        got = [b for b, _ in ms.scan(i).spans()] if s[i] else []
        if c[i] != len(truth):
            rep.miss(case, None, rx, "count", c[i], len(truth))
        wb = (truth[0], truth[0] + 8, truth[-1], truth[-1] + 8) if truth else None
        if bounds[i] != wb:
            rep.miss(case, None, rx, "bounds", bounds[i], wb)
        if got != truth:
            pos = first_difference([(g, 0) for g in got], [(w, 0) for w in truth])
            rep.miss(case, pos, rx, "spans at %s" % pos, len(got), len(truth))
    planted = sorted(p[0] for p in plants)
    print("anchor: %d plants; count kernel grid %d, spans of %d/%d blocks; list kernel grid %d, spans of %d/%d blocks"
          % (len(planted), plan.grid, plan.span_blocks, plan.span_blocks + 1, list_plan.grid, list_plan.span_blocks, list_plan.span_blocks + 1), flush=True)


def main(argv):
    family = argv[1]
    grid = int(os.environ.get("RJ_SCAN_GRID", "0") or 0)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from checkers import Oracle
    oracle = Oracle()
    rep = Report(family, grid or "auto")
    be = GpuBackend()
    if family == "dispatch":      # one text of every family: the run whose kernel trace is profiles/seam_sweep_kernels.txt
        for name in FAMILIES:
            check_multi(rep, be, oracle, FAMILIES[name]["rx"], cases_of(name, grid or 1)[0][3:4], window=FAMILIES[name]["window"])
    elif family == "anchor":
        check_anchor(rep, be)
    elif family == "single":
        assert grid, "RJ_SCAN_GRID must be set"
        check_single(rep, be, oracle, single_cases(grid)[0])
    else:
        assert grid, "RJ_SCAN_GRID must be set"
        cases, _ = cases_of(family, grid)
        if family in FAMILIES:
            check_multi(rep, be, oracle, FAMILIES[family]["rx"], cases, window=FAMILIES[family]["window"])
        elif family == "pairs_general":
            check_multi(rep, be, oracle, CHAIN_RX, cases)
        else:
            check_multi(rep, be, oracle, DNA9, cases)
    rep.done()


if __name__ == "__main__":
    main(sys.argv)
