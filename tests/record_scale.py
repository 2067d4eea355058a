"""Tables for the four row-layer record calls -- rj_scan_records_group, _sort, _lookup, _parse -- with MORE rows than one pass
of their persistent grids covers, and what the calls must answer for them.  Pure numpy: no torch, no GPU, no library
(tests/test_record_scale_plan.py checks this module on the CPU, tests/test_gpu_record_scale.py runs its tables on the GPU).

The kernels walk units of kThreads = 256 rows, `for (unit = blockIdx.x; unit < n_units; unit += gridDim.x)`:

    unit_grid() of rejit_amd/csrc/record_frame.h allows at most 1024 workgroups           one pass = 1024 x 256 rows  = K0
    kParseGrid  of rejit_amd/csrc/record_parse.hip is 256 * 8 = 2048 workgroups           one pass = 2048 x 256 rows  = 2 K0
    the wave-tier kernels stride by gridDim.x * kWaves = 1024 x 4 waves                   one pass = 4096 long rows

A table of a million rows cannot be written row by row in Python, and its expectation must not come from the library.  So
every table is DRAWN from a small pool of strings -- `pick`, k entries of the pool -- and every expectation is gathered, in a
few numpy lines, from a plain reference over the pool: a dict for `canon` (the first pool entry with an entry's bytes),
Python's sorted() over the pool's distinct strings for `rank`, parse_cases.meaning per pool string.  test_record_scale_plan.py
holds each of them against a row-by-row loop written there.

A pick gives two tables: the DIRECT one (rec_begin = pool.rb[pick], rec_end = pool.re[pick], no index list: rows alias the
same bytes, which the calls allow) and the INDEXED one (the pool's own records and `pick` as the index list)."""
import functools

import numpy as np

import parse_cases as pc

# ------------------------------------------------------------------------------------------------ the sizes
UNIT_ROWS = 256                      # record_frame.h: kThreads, the rows of a unit
UNIT_GRID_CAP = 1024                 # record_frame.h: unit_grid(), the most workgroups of a persistent unit loop
PARSE_GRID = 256 * 8                 # record_parse.hip: kParseGrid
WAVE_STRIDE = UNIT_GRID_CAP * 4      # the wave tier: gridDim.x * kWaves rows of the long list per pass
K0 = UNIT_GRID_CAP * UNIT_ROWS       # 262144: the rows ONE pass of a unit_grid() launch covers
assert K0 == 1024 * 256 and PARSE_GRID * UNIT_ROWS == 2 * K0
# exactly one pass; one row into the second pass (one more unit); a whole unit and one row of another into it; into the THIRD pass
KS = (K0, K0 + 1, K0 + 257, 2 * K0 + 65)
# the parse call has two grids: its check kernel takes unit_grid() (passes end at K0, 2 K0, ...), its parse kernel kParseGrid
# (passes end at 2 K0, 4 K0): one row behind the check's first pass; exactly one parse pass; one row behind it; the parse
# kernel's third pass and the check's fifth
PARSE_KS = (K0 + 1, 2 * K0, 2 * K0 + 1, 4 * K0 + 65)
LOOKUP_SIZES = ((K0 + 257, 2 * K0 + 65), (2 * K0 + 65, K0 + 1), (300, 2 * K0 + 65))      # (set rows, probe rows)
SMALL_KS = (0, 1, 257, 5000)         # what the CPU test walks row by row besides one k beyond K0

LENS = (0, 1, 15, 16, 17, 40, 700)
WINDOW = 7                           # record_sort.h: kWindow, the bytes of a row a round's key holds
FORCED_LONG = 16                     # RJ_GROUP_LONG_BYTES / RJ_SORT_LONG_BYTES as the GPU test forces them
SHORT_ROWS = 96                      # the rows of a pick that are shorter than WINDOW bytes (they close in the sort's first round)
SMALL_POOL = 40                      # distinct strings under RJ_GROUP_HASH_BITS=2
NONE = -1                            # RJ_LOOKUP_NONE as int64


def units(k):
    return (k + UNIT_ROWS - 1) // UNIT_ROWS


# ------------------------------------------------------------------------------------------------ pools
class Pool:
    """P strings in one text: text (uint8), rb / re (int64, a record per string), strings (bytes), lens, and canon[p]: the
    first entry with p's bytes"""

    def __init__(self, text, rb, re_, strings):
        self.text = np.frombuffer(bytes(text), dtype=np.uint8).copy()
        self.rb, self.re = np.array(rb, dtype=np.int64), np.array(re_, dtype=np.int64)
        self.strings = list(strings)
        self.lens = self.re - self.rb
        first = {}
        self.canon = np.array([first.setdefault(s, p) for p, s in enumerate(self.strings)], dtype=np.int64)
        self.ids = np.unique(self.canon)                  # one entry per distinct string: its first
        self.P = len(self.strings)

    @functools.lru_cache(maxsize=None)
    def rank(self):
        """rank()[p]: the dense rank of entry p's string among the pool's distinct strings, in Python's bytes order"""
        of = {s: r for r, s in enumerate(sorted(set(self.strings)))}
        return np.array([of[s] for s in self.strings], dtype=np.int64)

    @functools.lru_cache(maxsize=None)
    def parsed(self, kind, trim):
        """parse_cases.meaning of every entry -> (status as uint8, bits as uint64)"""
        want = [pc.meaning(s, kind, trim) for s in self.strings]
        return np.array([w[0] for w in want], dtype=np.uint8), np.array([w[1] for w in want], dtype=np.uint64)


def _distinct_strings(d, rng):
    """d distinct strings of lower-case letters with lengths from LENS: among them strings that share everything but their
    last byte, strings that are prefixes of one another (the sort needs a third round for those) and strings that differ in
    one byte behind the first WINDOW"""
    pool, seen, tries = [], set(), 0
    while len(pool) < d:
        kind = tries % 5
        tries += 1
        last = pool[-1] if pool else b""
        if kind == 1 and len(last) > 0:
            s = last[:-1] + bytes([ord("a") + (last[-1] - ord("a") + 1) % 26])
        elif kind == 2 and len(last) > 1:
            s = last[:int(rng.choice([n for n in sorted(set(LENS) | {1}) if n < len(last)]))]
        elif kind == 4 and len(last) > 16:
            at = int(rng.choice([8, len(last) // 2]))
            s = last[:at] + bytes([ord("a") + (last[at] - ord("a") + 7) % 26]) + last[at + 1:]
        else:
            s = rng.randint(ord("a"), ord("z") + 1, int(rng.choice(LENS))).astype(np.uint8).tobytes()
        if s not in seen:
            seen.add(s)
            pool.append(s)
    return pool


@functools.lru_cache(maxsize=None)
def string_pool(seed=20, d=1000):
    """The pool of the group, sort and lookup tables: d distinct strings, every one laid out TWICE -- entries p and d + p have
    equal bytes at different offsets and different misalignments, so equal rows live at different addresses (`cb == rb` is
    a shortcut in the kernels) -- with 0..3 filler bytes between neighbours."""
    rng = np.random.RandomState(seed)
    distinct = _distinct_strings(d, rng)
    text, rb, re_ = bytearray(b"abcde"), [0] * (2 * d), [0] * (2 * d)
    for p in range(d):
        text += b"z" * int(rng.randint(0, 4))
        rb[p] = len(text)
        text += distinct[p]
        re_[p] = len(text)
    text += b"|" * 7
    for p in rng.permutation(d).tolist():                 # the second copies, in another order
        seam = int(rng.randint(0, 4))
        if (len(text) + seam) % 16 == rb[p] % 16:
            seam = (seam + 1) % 4
        text += b"y" * seam
        rb[d + p] = len(text)
        text += distinct[p]
        re_[d + p] = len(text)
    text += b"tail"
    return Pool(text, rb, re_, distinct + distinct)


@functools.lru_cache(maxsize=None)
def parse_pool():
    """every named family of tests/parse_cases.py and its seeded mix, laid out by parse_cases.lay"""
    rows = pc.all_case_rows() + pc.random_rows(900, 31)
    text, records = pc.lay(rows)
    return Pool(text, [b for b, _ in records], [e for _, e in records], rows)


# ------------------------------------------------------------------------------------------------ picks
def pick(pool, k, seed, ids=None, short_rows=SHORT_ROWS):
    """k entries of the pool (of the entries whose string is one of `ids`, when given), seeded.  Three strings appear ONCE:
    two at the rows either side of the first pass's end, K0 - 1 and K0 (of the first unit's end, 255 and 256, in a table of
    at most K0 rows), one only at the last row.  With short_rows a number: all rows but that many are at least WINDOW bytes
    long (short_rows=None: no such rule, the parse tables)."""
    rng = np.random.RandomState(seed)
    entries = np.arange(pool.P) if ids is None else np.nonzero(np.isin(pool.canon, ids))[0]
    if k == 0:
        return np.zeros(0, dtype=np.int64)
    is_short = pool.lens[entries] < WINDOW if short_rows is not None else np.zeros(len(entries), dtype=bool)
    body, short = entries[~is_short], entries[is_short]
    strings = np.unique(pool.canon[body])
    singles = rng.choice(strings, min(3, len(strings) - 1), replace=False)
    body = body[~np.isin(pool.canon[body], singles)]
    out = body[rng.randint(0, len(body), k)]
    seam = K0 if k > K0 else UNIT_ROWS if k > UNIT_ROWS else 0
    places = ([seam - 1, seam] if seam else []) + ([k - 1] if k - 1 > seam else [])
    if len(short) and k >= 16:       # the short rows in pairs of one string, so that none of them appears once
        at = rng.choice(k, min(short_rows, k // 8), replace=False)
        at = at[~np.isin(at, places)]
        at = at[:len(at) // 2 * 2]
        half = short[rng.randint(0, len(short), len(at) // 2)]
        out[at] = np.concatenate([half, half])
    for row, string in zip(places, singles.tolist()):
        copies = np.nonzero(pool.canon == string)[0]
        out[row] = copies[rng.randint(0, len(copies))]
    return out.astype(np.int64)


def small_ids(pool, most=SMALL_POOL):
    return pool.ids[:most]


def lookup_sides(pool):
    """-> (the strings of the set, the strings of the probe): the set takes one half of the pool's strings, the probe the
    other half, and one quarter -- of the set's half -- belongs to both: a third of the probe's strings is found, half of the
    set's strings are hit by no probe"""
    quarter = np.arange(len(pool.ids)) % 4
    return pool.ids[quarter <= 1], pool.ids[quarter >= 1]


def group_pick(pool, k):
    return pick(pool, k, 1000 + k % 9973)


def group_small_pick(pool, k):
    return pick(pool, k, 1500 + k % 9973, ids=small_ids(pool))


def sort_pick(pool, k):
    return pick(pool, k, 2000 + k % 9973)


def lookup_picks(pool, ks, kp):
    set_ids, probe_ids = lookup_sides(pool)
    return pick(pool, ks, 3000 + ks % 9973, ids=set_ids), pick(pool, kp, 4000 + kp % 9973, ids=probe_ids)


def parse_pick(pool, k):
    return pick(pool, k, 5000 + k % 9973, short_rows=None)


def direct(pool, pk):
    """-> (rec_begin, rec_end, indices = None): the rows as records of their own"""
    return pool.rb[pk], pool.re[pk], None


def indexed(pool, pk):
    """-> (rec_begin, rec_end, indices): the pool's records and the pick as the index list"""
    return pool.rb, pool.re, pk


# ------------------------------------------------------------------------------------------------ meanings
def group_meaning(pool, pk):
    """-> (group, rep, count): the distinct strings numbered in order of first appearance"""
    if len(pk) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    _, first, inverse, count = np.unique(pool.canon[pk], return_index=True, return_inverse=True, return_counts=True)
    by_appearance = np.argsort(first, kind="stable")
    number = np.empty(len(first), dtype=np.int64)
    number[by_appearance] = np.arange(len(first))
    return number[inverse.reshape(-1)].astype(np.int64), first[by_appearance].astype(np.int64), count[by_appearance].astype(np.int64)


def sort_meaning(pool, pk):
    """-> order: THE stable permutation into byte order"""
    return np.argsort(pool.rank()[pk], kind="stable").astype(np.int64)


def lookup_meaning(pool, set_pk, probe_pk, long_bytes=64):
    """-> (index, set_hits, stats)"""
    first_row = np.full(pool.P, NONE, dtype=np.int64)
    strings, first = (np.unique(pool.canon[set_pk], return_index=True) if len(set_pk) else (np.zeros(0, dtype=np.int64),) * 2)
    first_row[strings] = first
    index = first_row[pool.canon[probe_pk]]
    hits = np.bincount(index[index >= 0], minlength=len(set_pk)).astype(np.int64)
    stats = {"n_found": int((index >= 0).sum()), "n_set_distinct": len(strings), "n_set_hit": int((hits > 0).sum()),
             "long_rows": int((pool.lens[probe_pk] > long_bytes).sum())}
    return index, hits, stats


PARSE_STATS = ("n_ok", "n_empty", "n_malformed", "n_range", "n_inexact")


def parse_meaning(pool, pk, kind, trim):
    """-> (status, bits, stats)"""
    status, bits = pool.parsed(kind, trim)
    counts = np.bincount(status[pk], minlength=5)
    return status[pk], bits[pk], dict(zip(PARSE_STATS, (int(c) for c in counts)))


# ------------------------------------------------------------------------------------------------ what the inputs reach
def open_after_round_one(pool, pk):
    """the rows of at least WINDOW bytes whose first WINDOW bytes another row has too: what the sort's second round lists"""
    window = {}
    key = np.array([window.setdefault(s[:WINDOW], len(window)) if len(s) >= WINDOW else -1 for s in pool.strings], dtype=np.int64)
    rows = key[pk]
    rows = rows[rows >= 0]
    return int((np.bincount(rows, minlength=1)[rows] >= 2).sum())


def longer_than(pool, pk, long_bytes=FORCED_LONG):
    return int((pool.lens[pk] > long_bytes).sum())


# ------------------------------------------------------------------------------------------------ one string, bad rows
def one_string_table(k, string):
    """k rows of ONE string, laid out twice at different misalignments: even rows name one copy, odd rows the other
    -> (text as uint8, rec_begin, rec_end)"""
    text = b"#" * 3 + string + b"#" * 6 + string + b"#"
    a, b = 3, 3 + len(string) + 6
    rb = np.where(np.arange(k) % 2 == 0, a, b).astype(np.int64)
    return np.frombuffer(text, dtype=np.uint8).copy(), rb, rb + len(string)


BAD_K = 2 * K0 + 65
BAD_ROWS = (K0 + 5, 2 * K0 + 1)      # in the second and in the third pass of a unit_grid() launch: the FIRST is named


def bad_index_list(pool, pk):
    """the pick with an index == n_records at the first of BAD_ROWS and -1 at the second"""
    out = pk.copy()
    out[BAD_ROWS[0]], out[BAD_ROWS[1]] = pool.P, -1
    return out
