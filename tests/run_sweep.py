"""Seam and resolve-level sweep of the run and pair kernels (rejit_amd/csrc/run_scan.hip) on small texts.

Two things live here, as in tests/seam_sweep.py and tests/window_sweep.py (whose Case, Coverage, plant_text, Report, GpuBackend
and first_difference are reused).

* A case PLANNER, pure Python, no GPU (tests/test_run_sweep_plan.py asserts its coverage).  `Geo` restates the launch geometry
  of run_tile_bytes, run_tiles, launch_run_summary, launch_run_resolve / launch_pair_resolve (run_scan.hip) and run_params /
  run_runs / run_pairs (engine.hip) for (n, min_start, RJ_RUN_TILE_KB, RJ_RUN_TWO_LEVELS): tile_bytes, first_tile, n_tiles = n //
  tile_bytes - first_tile + 1 (the tile that holds position n exists even when it holds nothing else), the iterations of a tile
  (loaded whole: base + (it + 1) * 2048 <= n; guarded byte by byte; skipped: it_base > n), workgroups of four waves, the one-level
  resolve (T = 1024 threads, C = ceil(n_tiles / 1024) tiles each) and the two-level one (blocks of block_tiles tiles, T = 256
  inside a block, the top level over the blocks with T = 1024 -- the pair kernels' top level: T = 256 up to 1024 blocks).
* The child DRIVER, `python tests/run_sweep.py SWEEP CONFIG`, which tests/test_gpu_run_seams.py starts once per (sweep, config)
  with the configuration's overrides in the environment (the library reads them once per process).  For every text: Scan.run ==
  len(spans()), spans() == the oracle, Scan.count on a fresh and on the reused Scan (whole texts), stats()["run_path"] 1 / 2 and
  linear_path 0, and the library's own geometry (rj_test_run_geometry, run_scan.hip) == the planner's -- without that a mistyped
  or removed override would silently sweep the default geometry.  The accessor is asked for the position the PLANNER counts the
  tiles from (own_geo restates run_runs' rule): the comparison pins the overrides and the tile arithmetic, not where engine.hip
  begins the tiles of an own range -- that is pinned by the spans alone.

Seam classes (a seam is the boundary before byte `pos`; tile-boundary classes also name the boundary before a tile):
  W:loaded / W:guarded   lanes 0|1, 31|32, 62|63 of an iteration that is loaded whole / guarded byte by byte
  IT:first / :middle / :last   iteration k|k+1 inside a tile (a tile of two iterations: its one pair is first and last)
  IG                     a loaded iteration followed by a guarded one
  TW / TG                tile boundary inside a workgroup / between two workgroups
  RC / RI                tile boundary between two threads' chunks of a resolve / inside one thread's chunk (C >= 2)
  R4                     inside a chunk at a multiple of four elements (C > 4: the loads come four at a time)
  BK / BKR               block boundary of the two-level resolve / the boundary into its ragged last block
  TC / TI                block boundary between / inside the top level's thread chunks
  GE, GE:w0 :w1 :w31 :i0 :i1 :i2047 :tile   the text's end, by n mod 32, n mod 2048 and n mod tile_bytes = 0
  MS / OE                (own sweep) min_start -- the own begin, or where a carried-in match ends -- and the own end

The LEVEL sweep plants no strings: its texts are sequences of 2-KiB tiles, each of a KIND defined by what its summary must hold
(RUN_KINDS, pair_kinds), laid out so that every ordered pair of kinds meets across a seam of every resolve class of the
configuration, and once more with a stretch of quiet tiles between the two that covers a whole thread chunk / a whole block.
Where a class has fewer seams than there are pairs within the 8 MiB a text may have -- block boundaries of 300 and 1024 tiles, the
one ragged block of a text -- the requirement is stated smaller (LEVEL_REDUCED) and asserted as stated."""
import bisect
import os
import sys

from seam_sweep import Case, Coverage, GpuBackend, Report, first_difference, plant_text

ITER = 2048
WORD = 32
MAX_TEXT = 140 * 1024
ENV_TILE, ENV_LEVELS = "RJ_RUN_TILE_KB", "RJ_RUN_TWO_LEVELS"
ONE_LEVEL_TILES, BLOCK_TILES = 4096, 1024

# configuration -> (RJ_RUN_TILE_KB, RJ_RUN_TWO_LEVELS); the level configurations run at 2-KiB tiles
CONFIGS = {"t2": (2, None), "t4": (4, None), "default": (None, None), "t32": (32, None),
           "c1": (2, None), "c2": (2, None), "c3": (2, None), "c4": (2, None),
           "l1": (2, 1), "l3": (2, 3), "l5": (2, 5), "l300": (2, 300), "l1024": (2, 1024), "anchor": (None, None)}
# the tile counts of a level configuration's texts (n = (tiles - 1) * 2048 + a tail: the last tile holds the end and little else)
#   c1 .. c4: C = 1 (threads with nothing), 2 and 4 with a ragged last thread, 3 with threads that own nothing
#   l1: more blocks than threads (TI, R4, pair_resolve_blocks<1024>); l3 / l5: small texts, one ragged block each;
#   l300: C = 2 inside a block, idle threads; l1024: the production block, three blocks and a ragged one
LEVEL_TILES = {"c1": (700, 1000), "c2": (2047, 1290), "c3": (3000, 2100), "c4": (4090, 4096), "l1": (4100, 4111), "l3": (602, 32, 35), "l5": (704, 44, 38),
               "l300": (637, 637, 637, 1050), "l1024": (3572,)}
LEVEL_CLASSES = {"c1": ("RC",), "c2": ("RC", "RI"), "c3": ("RC", "RI"), "c4": ("RC", "RI"), "l1": ("BK", "TC", "TI", "R4"),
                 "l3": ("RC", "BK", "BKR", "TC"), "l5": ("RC", "BK", "BKR", "TC"), "l300": ("RC", "RI", "BK", "BKR", "TC"), "l1024": ("RC", "RI", "BK", "BKR", "TC")}
# classes with fewer seams than pairs in texts of this size: "sides" = every kind stands on either side of such a seam once,
# "one" = at least one pair of two kinds that are not quiet
LEVEL_REDUCED = {"l300": {"BK": "sides", "BKR": "sides", "TC": "sides", "block": "one"},
                 "l1024": {"BK": "one", "BKR": "one", "TC": "one", "block": "one"}}
INTRA_CONFIGS = ("t2", "default", "t32")
OWN_CONFIGS = ("t2", "t4", "default")
INTRA_CLASSES = {"t2": ("W:loaded", "W:guarded", "TW", "TG", "RC"),
                 "t4": ("W:loaded", "W:guarded", "IT:first", "IT:last", "IG", "TW", "TG", "RC"),
                 "default": ("W:loaded", "W:guarded", "IT:first", "IT:middle", "IT:last", "IG", "TW", "TG", "RC"),
                 "t32": ("W:loaded", "W:guarded", "IT:first", "IT:middle", "IT:last", "IG", "TW", "TG", "RC")}
GE_CLASSES = ("GE", "GE:w0", "GE:w1", "GE:w31", "GE:i0", "GE:i1", "GE:i2047", "GE:tile")
OWN_D = (-33, -32, -31, -2, -1, 0, 1, 2, 31, 32, 33)
OWN_MODES = ("cut", "end", "begin", "oe")
OWN_FAR_D = (-1, 0, 1, 32)      # the mode `far`, at the TW and TG seams


def config_env(config):
    """the environment of a configuration's child (tests/test_gpu_run_seams.py adds it to a cleaned copy)"""
    tile_kb, two = CONFIGS[config]
    env = {}
    if config != "anchor":
        env["RJ_NO_SMALL"] = "1"        # (texts this small would take the one-workgroup kernel)
        env["RJ_RUNS_FIRST"] = "1"      # (the run shapes: the run kernels before dense_streams and the window scan)
    if tile_kb:
        env[ENV_TILE] = str(tile_kb)
    if two:
        env[ENV_LEVELS] = str(two)
    return env


def ceil_div(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ the arithmetic
class Geo:
    """The launches of a run (pair=True: a pair) call over a text of n bytes looked at from min_start on."""

    def __init__(self, n, min_start=0, tile_kb=None, two_levels=None, pair=False):
        span = n - min(min_start, n)
        forced = (tile_kb // 2) * ITER if tile_kb and tile_kb >= 2 else 0                      # run_tile_bytes
        self.n, self.min_start, self.pair = n, min_start, pair
        self.tile_bytes = forced or (8192 if span <= (256 << 20) else 32768)
        self.first_tile = min_start // self.tile_bytes                                         # run_tiles
        self.n_tiles = n // self.tile_bytes - self.first_tile + 1
        self.iters = self.tile_bytes // ITER
        self.grid = ceil_div(self.n_tiles, 4)                                                  # launch_run_summary: four waves
        self.block_tiles = two_levels if two_levels else BLOCK_TILES                           # launch_run_resolve
        self.levels = 1 if (self.n_tiles <= ONE_LEVEL_TILES and not two_levels) else 2
        if self.levels == 1:
            self.C = ceil_div(self.n_tiles, 1024)
            self.n_blocks = self.top_T = self.top_C = 0
        else:
            self.n_blocks = ceil_div(self.n_tiles, self.block_tiles)
            self.top_T = 256 if (pair and self.n_blocks <= 1024) else 1024
            self.top_C = ceil_div(self.n_blocks, self.top_T)
            self.C = ceil_div(min(self.block_tiles, self.n_tiles), 256)

    def accessor(self):
        """what rj_test_run_geometry returns"""
        return (self.tile_bytes, self.first_tile, self.n_tiles, self.block_tiles, self.levels)

    def base(self, tile):
        return (self.first_tile + tile) * self.tile_bytes

    def iteration(self, tile, it):
        it_base = self.base(tile) + it * ITER
        if it_base > self.n:
            return "skipped"
        return "loaded" if it_base + ITER <= self.n else "guarded"

    def block_size(self, b):
        return min(self.block_tiles, self.n_tiles - b * self.block_tiles)

    def chunk(self, tile):
        """(chunk id, index inside the chunk, C) of the lowest resolve level: one thread's tiles"""
        if self.levels == 1:
            return (0, tile // self.C), tile % self.C, self.C
        b = tile // self.block_tiles
        c = ceil_div(self.block_size(b), 256)
        rel = tile - b * self.block_tiles
        return (b, rel // c), rel % c, c

    def chunk_size(self, cid):
        b, t = cid
        if self.levels == 1:
            return max(min(self.C, self.n_tiles - t * self.C), 0)
        c = ceil_div(self.block_size(b), 256)
        return max(min(c, self.block_size(b) - t * c), 0)

    def busy_threads(self):
        """threads of the one-level resolve (of a full block) that own a tile, and whether the last of them owns fewer than C"""
        n = self.n_tiles if self.levels == 1 else min(self.block_tiles, self.n_tiles)
        return ceil_div(n, self.C), n % self.C != 0

    def boundary_tags(self, t):
        """the classes of the boundary between tile t and tile t + 1 (launch-relative)"""
        tags = ["TG" if (t + 1) % 4 == 0 else "TW"]
        if self.levels == 2 and (t + 1) % self.block_tiles == 0:
            b = (t + 1) // self.block_tiles
            tags.append("BKR" if self.block_size(b) < self.block_tiles else "BK")
            k = b % self.top_C
            tags.append("TC" if k == 0 else "TI")
            if self.top_C > 4 and k and k % 4 == 0:
                tags.append("R4")
        else:
            _, k, c = self.chunk(t + 1)
            tags.append("RC" if k == 0 else "RI")
            if c > 4 and k and k % 4 == 0:
                tags.append("R4")
        return tuple(tags)

    def end_tags(self):
        n = self.n
        tags = ["GE"]
        tags += ["GE:w%d" % (n % WORD)] if n % WORD in (0, 1, 31) else []
        tags += ["GE:i%d" % (n % ITER)] if n % ITER in (0, 1, 2047) else []
        tags += ["GE:tile"] if n % self.tile_bytes == 0 else []
        return tuple(tags)

    def seams(self, w_every=1, rot=0):
        """[(pos, tags)] in text order; the lane seams of every w_every-th iteration only (and of every guarded one)"""
        out = []
        k = 0
        for t in range(self.n_tiles):
            for it in range(self.iters):
                state = self.iteration(t, it)
                if state == "skipped":
                    break
                it_base = self.base(t) + it * ITER
                if it:
                    tags = []
                    if it == 1:
                        tags.append("IT:first")
                    if it == self.iters - 1:
                        tags.append("IT:last")
                    if not tags:
                        tags.append("IT:middle")
                    if state == "guarded" and self.iteration(t, it - 1) == "loaded":
                        tags.append("IG")
                    out.append((it_base, tuple(tags)))
                elif t:
                    out.append((it_base, self.boundary_tags(t - 1)))
                k += 1
                if state == "guarded" or (k + rot) % w_every == 0:
                    for lane in (1, 32, 63):
                        out.append((it_base + WORD * lane, ("W:" + state,)))
        out = [(p, tags) for p, tags in out if self.min_start < p < self.n]
        out.append((self.n, self.end_tags()))
        return out


# ------------------------------------------------------------------------------------------------ the families
class Family:
    """rx; the bytes the symbols of the motifs and tile kinds stand for: l (quiet: in L, in neither A nor B where the shape has
    such a byte), A, B (shapes without a B position: a second quiet byte), r (breaks -- of the pair shape: resets; a pair shape
    without a reset byte: quiet), n (a line break where the shape looks at lines, else r); plan: what make_run_plan must say."""

    def __init__(self, rx, l, A, B, r, n=None, pair=False, has_b=None, nr=None, flags=(), reset=True):
        self.rx, self.pair, self.nr, self.flags, self.reset = rx, pair, nr, tuple(flags), reset
        self.has_b = pair if has_b is None else has_b
        self.sym = {"l": l, "A": A, "B": B, "r": r, "n": n if n is not None else r[:1]}
        # the classes, for the tile classifier (the first that holds a byte names it)
        self.sets = (("A", set(A)), ("B", set(B)), ("r", set() if (pair and not reset) else set(r) | set(self.sym["n"])))

    def byte(self, s, k=0):
        b = self.sym[s]
        return b[k % len(b)]

    def bytes_of(self, motif, k=0):
        return bytes(self.byte(s, k) for s in motif)


def nr_class(nr):
    return 1 if nr <= 1 else 2 if nr <= 2 else 4 if nr <= 4 else 8


FAMILIES = {
    # X+ / A L* / X+ B / A L* B by NR class, with and without B
    "x+": Family(b"x+", b"x", b"x", b"x", b"y", nr=1),
    "acgt+": Family(b"[acgt]+", b"c", b"a", b"g", b"N", nr=4),
    "a[bc]*": Family(b"a[bc]*", b"b", b"a", b"c", b"x", nr=2, flags=("a_break",)),
    "nr8": Family(b"[adgj][behk]*", b"b", b"a", b"e", b"x", nr=8, flags=("a_break",)),
    "[^x]+x": Family(b"[^x]+x", b"c", b"c", b"x", b"x", has_b=True, nr=1, flags=("a_neg", "l_neg", "b_break")),
    "<[^>]*>": Family(b"<[^>]*>", b"c", b"<", b">", b">", has_b=True, nr=2, flags=("l_neg", "b_break")),
    "a.*b": Family(b"a.*b", b"c", b"a", b"b", b"\n\r", has_b=True, nr=4, flags=("l_neg",)),
    "nr8b": Family(b"[adg][^\n\r]*[beh]", b"c", b"a", b"b", b"\n\r", has_b=True, nr=8, flags=("l_neg",)),
    "af09": Family(b"[a-f]+[0-9]", b"c", b"a", b"5", b" ", has_b=True, nr=2),
    "bneg": Family(b"b[b-y]*[^b-y]", b"c", b"b", b"z", b"z", has_b=True, nr=2, flags=("b_neg", "b_break")),
    # A L+ / A L+ B
    "#.+": Family(b"#.+", b"c", b"#", b"d", b"\n\r", nr=4, flags=("lag", "l_neg")),
    "a.+b": Family(b"a.+b", b"c", b"a", b"b", b"\n\r", has_b=True, nr=4, flags=("lag", "l_neg")),
    "<[^>]+>": Family(b"<[^>]+>", b"c", b"<", b">", b">", has_b=True, nr=2, flags=("lag", "l_neg", "b_break")),
    # ^ / $
    "^#.*": Family(b"^#.*", b"c", b"#", b"d", b"\n\r", nr=4, flags=("bol", "l_neg")),
    "#.*$": Family(b"#.*$", b"c", b"#", b"d", b"\n\r", nr=4, flags=("eol", "l_neg")),
    "a[b ]*$": Family(b"a[b ]*$", b"b", b"a", b" ", b"\nx", n=b"\n", nr=4, flags=("eol", "a_break")),
    "^AB+$": Family(b"^[AB][ab]+$", b"a", b"A", b"b", b"\n ", n=b"\n", nr=2, flags=("lag", "bol", "eol", "a_break")),
    "^a.*b": Family(b"^a.*b", b"c", b"a", b"b", b"\n\r", has_b=True, nr=4, flags=("bol", "l_neg")),
    # a range in 0x80 .. 0xff (this dialect has no escapes inside brackets: the bytes themselves)
    "high+": Family(b"[\x80-\xff]+", b"\x90", b"\x81", b"\xfe", b"a", nr=1, flags=("high",)),
    "highb": Family(b"\xe0[\x80-\xbf]*\xff", b"\x90", b"\xe0", b"\xff", b"a", has_b=True, nr=4, flags=("high", "a_break", "b_break")),
    # the pair shape: NR 1, 2, 4, 8, with and without a reset byte
    "p1": Family(b"\"[^\"]*\"", b"c", b"\"", b"\"", b"c", pair=True, nr=1, flags=("l_neg",), reset=False),
    "p2": Family(b"\"[^\"\n]*\"", b"c", b"\"", b"\"", b"\n", pair=True, nr=2, flags=("l_neg",)),
    "p4": Family(b"[\"'][^\"'\n\r]*[\"']", b"c", b"\"'", b"'\"", b"\n\r", pair=True, nr=4, flags=("l_neg",)),
    "p8": Family(b"[\"'%|][^\"'%|\n]*[\"'%|]", b"c", b"\"'%|", b"|%'\"", b"\n", pair=True, nr=8, flags=("l_neg",)),
    "p8n": Family(b"[\"'%|@][^\"'%|@]*[\"'%|@]", b"c", b"\"'%|@", b"@|%'\"", b"c", pair=True, nr=8, flags=("l_neg",), reset=False),
    "p%": Family(b"%[a-z]*%", b"c", b"%", b"%", b" \n", pair=True, nr=2),
    "phigh": Family(b"[\x80][^\x80]*[\x80]", b"c", b"\x80", b"\x80", b"c", pair=True, nr=1, flags=("l_neg", "high"), reset=False),
}
INTRA_GROUPS = {"t2": 4, "default": 4, "t32": 8}       # children per configuration: every n-th family (a child's time: tests/test_gpu_run_seams.py)
OWN_GROUPS = 2
LEVEL_SPLIT = ("l3", "l5")
LEVEL_MERGED = {"c1": ("runsA+runsB+pairs",), "c2": ("runsA", "runsB+pairs"), "c3": ("runsA", "runsB+pairs")}     # (few small texts: fewer children)
OWN_FAMILIES = ("a.*b", "<[^>]*>", "a[bc]*", "acgt+", "#.+", "a.+b", "^#.*", "a[b ]*$")
LEVEL_GROUPS = {"runsA": ("a.*b", "a[bc]*", "a[b ]*$"), "runsB": ("a.+b", "^#.*", "^AB+$"), "pairs": ("p2", "p1", "p8")}
# every internal boundary of a motif falls on every class of seam once: `r A l l B l r`, `r A r`, A on the break, two breaks in
# one word with a match between them, a B before and a B behind the seam, `\n A l` for `^`, A then l for `A L+`
MOTIFS = ("rAllBlr", "AlBlBlr", "rArAlBr", "rAlBr", "nAllr", "lBAlB", "rAr", "AlB", "nAl", "AAl")
MOTIF_LENGTHS = (3, 5, 7)
DENSE_UNIT = "AlrABrArlBrBrAArlrABnlr"       # a break every two to three bytes; 23 bytes: the unit drifts through the 32-byte words


class _Rank(dict):
    """plant_text's order of service: the classes one text has few seams of first"""
    ORDER = {"GE": -1, "IG": 0, "W:guarded": 0, "TG": 0, "MS": 0, "OE": 0, "TW": 1, "IT:last": 1, "IT:first": 2, "IT:middle": 2, "W:loaded": 3}

    def __missing__(self, tag):
        return self.ORDER.get(tag.split(":")[0] if tag.startswith("GE") else tag, 1)


def missing(cover, classes, lengths=MOTIF_LENGTHS):
    out = []
    for t in classes:
        for length in lengths:
            for k in ([0] if t.startswith("GE") else range(length + 2)):
                if cover.count(t, length, k) == 0:
                    out.append((t, length, k - length))
    return out


def intra_geometries(config):
    """n of a configuration's intra-tile texts, in the order they are tried: every GE class, texts of a few iterations (cheap:
    IG, W:guarded and GE need a text each per offset) and texts of more than four tiles (TG)"""
    tb = Geo(1, 0, CONFIGS[config][0]).tile_bytes
    iters = tb // ITER
    out = []
    tails = (0, 1, 31, 32, 33, 1000, 2047, 64, 2017)
    most = MAX_TEXT // tb
    for k in range(36):
        tiles = (0, 1, 4, 0, 2, most, 1, 5 if most >= 5 else most, 0, 3)[k % 10]
        tiles = min(tiles, most)
        it = (k * 3 + 1) % iters if iters > 1 else 0
        tail = tails[k % len(tails)]
        n = tiles * tb + min(it * ITER + tail, MAX_TEXT - tiles * tb)
        out.append(max(n, ITER + tail))
    out += [tb, 4 * tb, 2 * tb, 2 * tb + 1, 4 * tb + 31]          # (n mod tile_bytes = 0: the last tile holds only the end position)
    return out


def intra_cases(config, name):
    """The intra-tile texts of one family under one configuration -> (cases, coverage); a dense text first."""
    fam = FAMILIES[name]
    tile_kb, two = CONFIGS[config]
    cover = Coverage()
    cases = []
    strings = [fam.bytes_of(m, k) for k, m in enumerate(MOTIFS)]
    bg = fam.byte("l")
    classes = INTRA_CLASSES[config] + GE_CLASSES
    tb = Geo(1, 0, tile_kb).tile_bytes
    n = min(3 * tb + ITER + 77, MAX_TEXT)
    unit = b"".join(fam.bytes_of(DENSE_UNIT, k) for k in range(4))
    cases.append(RunCase("%s dense n=%d" % (name, n), Geo(n, 0, tile_kb, two, fam.pair), (unit * (n // len(unit) + 1))[:n], [], name))
    geos = intra_geometries(config)
    for rot in range(160):
        if rot >= len(geos) and not missing(cover, classes):
            break
        n = geos[rot % len(geos)]
        geo = Geo(n, 0, tile_kb, two, fam.pair)
        text, plants = plant_text(n, geo.seams(w_every=3, rot=rot), strings, bg, cover, rot, rare=_Rank())
        cases.append(RunCase("%s n=%d" % (name, n), geo, text, plants, name))
    return cases, cover


class RunCase(Case):
    def __init__(self, label, geo, text, plants, family, own=None, carry=None, seq=None, whole=True):
        Case.__init__(self, label, geo, text, plants, own=own)
        self.geo, self.family, self.carry, self.seq, self.whole = geo, family, carry, seq, whole

    def where(self, pos):
        """the address of a mismatch at pos: seam class and offset, or the tile and its neighbours' kinds"""
        if self.seq is not None:
            t = max(min(pos // self.geo.tile_bytes, len(self.seq) - 1), 0)
            tags = "+".join(self.geo.boundary_tags(t - 1)) if t else "-"
            return "tile %d (%s | %s | %s) seam before it %s" % (t, self.seq[t - 1] if t else "-", self.seq[t], self.seq[t + 1] if t + 1 < len(self.seq) else "-", tags)
        cls, off = self.describe(pos)
        return "seam=%s offset=%+d" % (cls, off)


# ------------------------------------------------------------------------------------------------ own ranges and carries
def own_seams(geo):
    """one W, IT, TW and TG seam each (W in the first tile: first_tile = 0; the others behind it)"""
    tb = geo.tile_bytes
    return (("W", WORD * 32), ("IT" if geo.iters > 1 else "W63", 2 * tb + (ITER if geo.iters > 1 else WORD * 63)), ("TW", 3 * tb), ("TG", 4 * tb))


def own_cases(config, name):
    """Cuts at pos + d around a W, IT, TW and TG seam.  Modes: `cut` -- a full-text match straddles the cut at pos + d; `end` -- the
    straddling match ENDS at pos + d (min_start: where the carried-in match ends); `begin` -- nothing straddles, the own range begins
    at pos + d; `oe` -- the own range ENDS at pos + d, before the text's end.  The caller takes the carry from the last full-text
    match before the cut and expects the full text's matches that begin in the range.  `far` (TW and TG, OWN_FAR_D): see below."""
    fam = FAMILIES[name]
    tile_kb, two = CONFIGS[config]
    tb = Geo(1, 0, tile_kb).tile_bytes
    n = 5 * tb + ITER + 77
    unit = fam.bytes_of("llrAllBllll")
    base = (unit * (n // len(unit) + 1))[:n]
    cases = []
    for tag, pos in own_seams(Geo(n, 0, tile_kb, two)):
        for d in OWN_D:
            at = pos + d
            for mode in ("cut", "end", "begin"):
                t = bytearray(base)
                if mode == "begin":
                    cut = at
                    t[cut - 2:cut + 5] = fam.bytes_of("lrAlBlr")
                    owns = [(mode, (cut, n + 1)), ("oe", (tb + 100 if pos > 2 * tb else 40, cut))]
                else:
                    length = 9 + abs(d) % 5
                    mb, e = (at - 5 - abs(d) % 3, at - 5 - abs(d) % 3 + length) if mode == "cut" else (at - length, at)
                    cut = at if mode == "cut" else e - 3
                    if fam.has_b:      # r A l .. l B, then an A without a B behind it in the same segment
                        ov = fam.bytes_of("rA" + "l" * (length - 2) + "BlAlr")
                    else:              # r A l .. l, the match ends at the break
                        ov = fam.bytes_of("rA" + "l" * (length - 1) + "r")
                    t[mb - 1:mb - 1 + len(ov)] = ov
                    owns = [(mode, (cut, n + 1))]
                for m, own in owns:
                    c = RunCase("%s own %s %s%+d own=%s" % (name, m, tag, d, own), None, bytes(t), [(at, b"", ("OE" if m == "oe" else "MS", tag), pos)], name, own=own, whole=False)
                    c.mode, c.seam_tag, c.d, c.at = m, tag, d, at
                    cases.append(c)
        if tag in ("TW", "TG"):
            # `far`: the carried-in match ends two tiles before the own begin at pos + d, a break a few bytes behind it, nothing
            # but quiet bytes from there to the own begin, where a match begins
            for d in OWN_FAR_D:
                at = pos + d
                e = at - 2 * tb - 5
                t = bytearray(base)
                t[e - 9:at + 5] = fam.bytes_of("rAllllllB" + "lllr") + bytes([fam.byte("l")]) * (at - e - 4) + fam.bytes_of("AlBlr")
                c = RunCase("%s own far %s%+d own=%s" % (name, tag, d, (at, n + 1)), None, bytes(t), [(at, b"", ("MS", tag), pos)], name, own=(at, n + 1), whole=False)
                c.mode, c.seam_tag, c.d, c.at = "far", tag, d, at
                cases.append(c)
    return cases


def carry_of(full, own):
    """the selection state at own[0] from the full text's matches, as tests/test_gpu_runs.py: test_run_own_ranges_and_carry"""
    before = [m for m in full if m[0] < own[0]]
    if not before:
        return {}
    b, e = before[-1]
    return dict(carry_cur=e if e > b else b + 1, carry_prev_end=e, have_prev=True)


def own_geo(case, config, carry):
    """run_runs (engine.hip): min_start = max(own begin, carry_cur) + lag; the tiles begin with min_start's -- or, when the carried-in
    match ended behind a B that is no break (blocked_in: its segment goes on and has had its match), with the tile of that B, so
    that the kernels see the break that lifts the block.  -> Geo from the first tile's position on; .clip_from = min_start."""
    fam = FAMILIES[case.family]
    lag = 1 if "lag" in fam.flags else 0
    tile_kb, two = CONFIGS[config]
    min_start = max(case.own[0], carry.get("carry_cur", 0)) + lag
    e = carry.get("carry_prev_end", 0)
    blocked = bool(carry) and fam.has_b and 1 <= e <= case.n and case.text[e - 1] not in fam.sets[2][1]
    geo = Geo(case.n, min(min_start, e - 1) if blocked else min_start, tile_kb, two)
    geo.clip_from, geo.blocked = min_start, blocked
    return geo


# ------------------------------------------------------------------------------------------------ the level sweep
# a tile's kind: what its summary must hold -- (symbol, place): a fraction of the tile (moved a little from tile to tile), 0 = the
# tile's first byte, -1 = its last
RUN_KINDS = {"E": (), "A": (("A", .5),), "B": (("B", .5),), "AB": (("A", .3), ("B", .6)), "BA": (("B", .3), ("A", .6)), "r": (("r", .5),),
             "Ar": (("A", .3), ("r", .6)), "rA": (("r", .3), ("A", .6)), "Br": (("B", .3), ("r", .6)), "ABr": (("A", .2), ("B", .5), ("r", .8)),
             "rAB": (("r", .2), ("A", .5), ("B", .8)), "rMr": (("r", .1), ("A", .3), ("B", .6), ("r", .8)),
             "r0": (("r", 0),), "rZ": (("r", -1),), "AZ": (("A", -1),), "B0": (("B", 0),)}


def pair_kinds(reset):
    """0 / 1 / 2 / 3 Q bytes before the first reset, without a reset / with one and an even / odd Q count behind the last, Q at
    the tile's first / last byte"""
    kinds = {"E": ()}
    for k in range(4):
        before = tuple(("A", f) for f in (.1, .2, .3)[:k])
        if k:
            kinds["q%d" % k] = tuple(("A", f) for f in (.3, .5, .7)[:k])
        if reset:
            kinds["q%dr0" % k] = before + (("r", .5), ("A", .7), ("A", .8))
            kinds["q%dr1" % k] = before + (("r", .5), ("r", .6), ("A", .7))
    kinds["Q0"] = (("A", 0),)
    kinds["QZ"] = (("A", -1),)
    return kinds


def kinds_of(fam):
    return pair_kinds(fam.reset) if fam.pair else RUN_KINDS


def make_tile(fam, kind, index, tb=ITER):
    t = bytearray([fam.byte("l")]) * tb
    for j, (s, place) in enumerate(kinds_of(fam)[kind]):
        at = 0 if place == 0 else tb - 1 if place == -1 else int(place * tb) + (index * 37 + j) % 101
        t[at] = fam.byte(s, index + j)
    return bytes(t)


def classify_tile(fam, tile):
    """The kind of a tile from its bytes and the family's classes alone (not from make_tile)."""
    if not hasattr(fam, "_table"):
        table = bytearray(256)
        for s, members in reversed(fam.sets):       # (the first class that holds a byte names it)
            for b in members:
                table[b] = ord(s)
        fam._table = bytes(table)
    marks = tile.translate(fam._table)
    sig = marks.replace(b"\0", b"").decode()
    first, last = marks[:1] != b"\0", marks[-1:] != b"\0"
    if fam.pair:
        if sig == "":
            return "E"
        if sig == "A" and (first or last):
            return "Q0" if first else "QZ"
        if "r" not in sig:
            return "q%d" % len(sig)
        return "q%dr%d" % (sig.index("r"), (len(sig) - 1 - sig.rindex("r")) & 1)
    if sig == "":
        return "E"
    if sig == "r" and (first or last):
        return "r0" if first else "rZ"
    if sig == "A" and last:
        return "AZ"
    if sig == "B" and first:
        return "B0"
    return "rMr" if sig == "rABr" else sig


def level_geo(config, tiles, pair):
    tile_kb, two = CONFIGS[config]
    tb = Geo(1, 0, tile_kb).tile_bytes
    return Geo((tiles - 1) * tb + 100 + tiles % 7, 0, tile_kb, two, pair)


def level_requirements(config, kinds):
    """(class, a, b) for the adjacent pairs, ("chunk" | "block" | "top", a, b) for the pairs with a quiet stretch between them"""
    names = list(kinds)
    busy = [k for k in names if k != "E"]
    reduced = LEVEL_REDUCED.get(config, {})
    req = []
    for cls in LEVEL_CLASSES[config]:
        how = reduced.get(cls)
        if how == "one":
            req.append((cls, busy[3 % len(busy)], busy[4 % len(busy)]))
        elif how == "sides":
            req += [(cls, a, busy[(i + 3) % len(busy)]) for i, a in enumerate(busy)] + [(cls, "E", busy[0]), (cls, busy[0], "E")]
        else:
            req += [(cls, a, b) for a in names for b in names]
    stretches = ["chunk"] + (["block"] if CONFIGS[config][1] else []) + (["top"] if config == "l1" else [])
    for what in stretches:
        how = reduced.get(what)
        if how == "one":
            req.append((what, busy[5 % len(busy)], busy[6 % len(busy)]))
        elif how == "sides":
            req += [(what, a, busy[(i + 5) % len(busy)]) for i, a in enumerate(busy)]
        else:
            req += [(what, a, b) for a in busy for b in busy]
    return req


def level_sequences(config, kinds, pair):
    """The texts of a level configuration as sequences of kinds, laid out requirement after requirement: [(geo, [kind per tile])].
    (Deterministic.  What the sequences cover is measured from them afterwards: level_coverage.)"""
    req = level_requirements(config, kinds)
    sizes = LEVEL_TILES[config]
    out = []
    todo = list(req)
    placed = set()                                # (class, a, b) of the pairs laid out so far: a seam has several classes
    while todo:
        tiles = sizes[len(out)] if len(out) < len(sizes) else sizes[1 + (len(out) - 1) % (len(sizes) - 1)] if len(sizes) > 1 else sizes[0]
        geo = level_geo(config, tiles, pair)
        last = geo.n_tiles - 2                    # (the tile that holds the text's end stays quiet)
        tags = [geo.boundary_tags(t) for t in range(last)]       # tags[t]: between tile t and t + 1
        by_class = {}
        for t, tg in enumerate(tags):
            for c in tg:
                by_class.setdefault(c, []).append(t)
        seq = ["E"] * geo.n_tiles
        cursor = 1                                # the first tile that is still free
        rest = []
        for what, a, b in todo:
            if (what, a, b) in placed:
                continue
            if what in ("chunk", "block", "top"):
                unit = {"chunk": geo.C, "block": geo.block_tiles, "top": geo.block_tiles * max(geo.top_C, 1)}[what]
                if what == "block" and unit > 8:  # aligned: a at a block's last tile, the next block quiet, b behind it
                    first = ceil_div(cursor + 1, unit) * unit - 1
                    ta, tb_ = first, first + unit + 1
                else:
                    ta, tb_ = cursor, cursor + 2 * unit
                if tb_ > last:
                    rest.append((what, a, b))
                    continue
                seq[ta], seq[tb_] = a, b
                cursor = tb_ + 2
                placed.add((what, a, b))
                continue
            places = by_class.get(what, [])
            i = bisect.bisect_left(places, cursor)
            if i == len(places) or places[i] + 1 > last:
                rest.append((what, a, b))
                continue
            t = places[i]
            seq[t], seq[t + 1] = a, b
            cursor = t + 3
            placed |= {(c, a, b) for c in tags[t]}
        assert len(rest) < len(todo), (config, rest[:4])
        out.append((geo, seq))
        todo = rest
        assert len(out) <= 400, config
    return out


def level_coverage(texts):
    """What sequences of kinds cover, read from them: {class: {(a, b)}} of the adjacent pairs, and under "chunk" / "block" / "top" the
    pairs of kinds (not quiet) with a quiet stretch between them that holds a whole thread chunk / block / top-level chunk."""
    seen = {}
    for geo, seq in texts:
        for t in range(len(seq) - 1):
            for c in geo.boundary_tags(t):
                seen.setdefault(c, set()).add((seq[t], seq[t + 1]))
        busy = [t for t, k in enumerate(seq) if k != "E"]
        for i, j in zip(busy, busy[1:]):
            if j - i < 2:
                continue
            pairs = (seq[i], seq[j])
            chunks, blocks = {}, {}
            for t in range(i + 1, j):
                cid = geo.chunk(t)[0]
                chunks[cid] = chunks.get(cid, 0) + 1
                if geo.levels == 2:
                    b = t // geo.block_tiles
                    blocks[b] = blocks.get(b, 0) + 1
            if any(v == geo.chunk_size(cid) for cid, v in chunks.items()):
                seen.setdefault("chunk", set()).add(pairs)
            whole = sorted(b for b, v in blocks.items() if v == geo.block_size(b))
            if whole:
                seen.setdefault("block", set()).add(pairs)
            if geo.levels == 2 and geo.top_C > 1 and any(all(b + k in whole for k in range(geo.top_C)) for b in whole if b % geo.top_C == 0):
                seen.setdefault("top", set()).add(pairs)
    return seen


def level_cases(config, name):
    fam = FAMILIES[name]
    cases = []
    for geo, seq in level_sequences(config, kinds_of(fam), fam.pair):
        tb = geo.tile_bytes
        text = bytearray(b"".join(make_tile(fam, k, t, tb) for t, k in enumerate(seq)))
        del text[geo.n:]
        cases.append(RunCase("%s level %s tiles=%d" % (name, config, geo.n_tiles), geo, bytes(text), [], name, seq=seq))
    return cases


# ------------------------------------------------------------------------------------------------ the anchor
ANCHOR_TILES = 4101          # just above 32 MiB at 8-KiB tiles: the two-level resolve with blocks of 1024 tiles from the code itself
ANCHOR_FAMILIES = ("a.*b", "p2")


def anchor_case(name):
    """No override.  Tile kinds across every BK / BKR seam and across RC, RI and TG seams spread over the text."""
    fam = FAMILIES[name]
    geo = level_geo("anchor", ANCHOR_TILES, fam.pair)
    assert geo.levels == 2 and geo.block_tiles == BLOCK_TILES and geo.tile_bytes == 8192
    busy = [k for k in kinds_of(fam) if k != "E"]
    seq = ["E"] * geo.n_tiles
    seams = [t for t in range(geo.n_tiles - 2) if set(geo.boundary_tags(t)) & {"BK", "BKR"}]
    seams += [t for t in range(5, geo.n_tiles - 2, 61)]        # (61: every residue modulo 4 -- RC, RI, TW and TG)
    for k, t in enumerate(sorted(set(seams))):
        if seq[t - 1] == "E" and seq[t] == "E":
            seq[t], seq[t + 1] = busy[k % len(busy)], busy[(k * 5 + 2) % len(busy)]
    text = bytearray(b"".join(make_tile(fam, k, t, geo.tile_bytes) for t, k in enumerate(seq)))
    del text[geo.n:]
    return RunCase("%s anchor tiles=%d" % (name, geo.n_tiles), geo, bytes(text), [], name, seq=seq)


# ------------------------------------------------------------------------------------------------ what a child runs
def sweeps():
    """[(sweep, config)] of tests/test_gpu_run_seams.py, the anchor apart"""
    out = [("intra:%d" % g, c) for c in INTRA_CONFIGS for g in range(INTRA_GROUPS[c])]
    out += [("own:%d" % g, c) for c in OWN_CONFIGS for g in range(OWN_GROUPS)]
    for c in LEVEL_TILES:
        for g in LEVEL_MERGED.get(c, LEVEL_GROUPS):
            if c in LEVEL_SPLIT and g != "pairs":     # (hundreds of small texts a family: two children a group)
                out += [("level:%s/%d" % (g, h), c) for h in range(2)]
            else:
                out.append(("level:" + g, c))
    return out


def families_of(sweep, config):
    kind, _, group = sweep.partition(":")
    if kind == "intra":
        return list(FAMILIES)[int(group)::INTRA_GROUPS[config]]
    if kind == "own":
        return list(OWN_FAMILIES)[int(group)::OWN_GROUPS]
    if kind == "level":
        group, _, half = group.partition("/")
        names = [n for g in group.split("+") for n in LEVEL_GROUPS[g]]
        return names if not half else names[:2] if half == "0" else names[2:]
    if kind == "anchor":
        return list(ANCHOR_FAMILIES)
    raise KeyError(sweep)


def cases_of(sweep, config, name):
    kind = sweep.partition(":")[0]
    if kind == "intra":
        return intra_cases(config, name)[0]
    if kind == "own":
        return own_cases(config, name)
    if kind == "level":
        return level_cases(config, name)
    return [anchor_case(name)]


def text_count(sweep, config):
    kind = sweep.partition(":")[0]
    if kind == "anchor":
        return len(ANCHOR_FAMILIES)
    if kind == "level":     # (no need to build the texts)
        return sum(len(level_sequences(config, kinds_of(FAMILIES[n]), FAMILIES[n].pair)) for n in families_of(sweep, config))
    return sum(len(cases_of(sweep, config, n)) for n in families_of(sweep, config))


# ------------------------------------------------------------------------------------------------ the driver
class RunReport(Report):
    def note(self, case, rx, pos, what, got, want):
        self.mismatches += 1
        print("MISMATCH config=%s family=%s pattern=%r n=%d %s %s: got %s want %s  [%s]"
              % (self.grid, case.family, rx, case.n, case.where(pos) if pos is not None else "-", what, got, want, case.label), flush=True)
        if self.mismatches >= 10:
            self.done()


def near(spans, pos):
    return [m for m in spans if pos is not None and abs(m[0] - pos) < 64][:2]


def check_family(rep, be, oracle, config, name, cases, geometry):
    fam = FAMILIES[name]
    rx = fam.rx
    path = 2 if fam.pair else 1
    prog = be.rj.Program(rx)
    reused = be.rj.Scan(prog)
    for case in cases:
        data, n = case.text, case.n
        t = be.device_text(data)
        rep.texts += 1
        cap = n // 2 + 16 if n <= (1 << 20) else n // 64        # (a match and the break behind it take two bytes; the level texts are sparse)
        full = oracle.match_all(rx, data, cap=cap)
        assert not isinstance(full, int) and len(full) < cap, (rx, n)
        if case.own is None:
            kw, want, geo = {}, full, case.geo
            sc = be.rj.Scan(prog)
        else:
            carry = carry_of(full, case.own)
            kw = dict(own_begin=case.own[0], own_end=case.own[1], **carry)
            want = [m for m in full if case.own[0] <= m[0] < case.own[1]]
            geo = own_geo(case, config, carry)
            sc = reused
        lib_geo = geometry(n, geo.min_start)       # (the position the tiles are counted from)
        if lib_geo != geo.accessor():
            rep.note(case, rx, None, "geometry (tile_bytes, first_tile, n_tiles, block_tiles, levels)", lib_geo, geo.accessor())
        k = sc.run(t.data_ptr(), n, **kw)
        st = sc.stats()
        got = sc.spans() if k else []
        if got != want or k != len(want):
            pos = first_difference(got, want)
            rep.note(case, rx, pos, "spans at %s (run returned %d; %d / %d spans)" % (pos, k, len(got), len(want)), near(got, pos), near(want, pos))
        if st["run_path"] != path or st["linear_path"] != 0:
            rep.note(case, rx, None, "path", (st["run_path"], st["linear_path"]), (path, 0))
        if case.whole:
            fresh = be.rj.Scan(prog)
            for what, s in (("count, fresh scan", fresh), ("count, reused scan", sc), ("count, the family's scan", reused)):
                c = s.count(t.data_ptr(), n)
                # (no override, few matches: the scan object may send a window-mode shape's next call to the window scan)
                if c != len(want) or (s.stats()["run_path"] != path and config != "anchor"):
                    rep.note(case, rx, None, what + " (run_path %d)" % s.stats()["run_path"], c, len(want))


def main(argv):
    sweep, config = argv[1], argv[2]
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    import ctypes
    from checkers import Oracle
    want_env = config_env(config)
    for key in (ENV_TILE, ENV_LEVELS, "RJ_NO_SMALL", "RJ_RUNS_FIRST"):
        assert os.environ.get(key) == want_env.get(key), "%s=%r, the configuration %s needs %r" % (key, os.environ.get(key), config, want_env.get(key))
    oracle = Oracle()
    rep = RunReport(sweep, config)
    be = GpuBackend()
    lib = be.rj.load_library()
    lib.rj_test_run_geometry.restype = None
    lib.rj_test_run_geometry.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]

    def geometry(n, min_start):
        out = (ctypes.c_uint64 * 5)()
        lib.rj_test_run_geometry(n, min_start, out)
        return tuple(int(x) for x in out)

    for name in families_of(sweep, config):
        check_family(rep, be, oracle, config, name, cases_of(sweep, config, name), geometry)
    rep.done()


if __name__ == "__main__":
    main(sys.argv)
