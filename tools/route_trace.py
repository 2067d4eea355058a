#!/usr/bin/env python3
"""Which route answers which call?  A fixed list of (pattern, texts, calls) over the shapes tests/test_gpu_sequences.py uses --
window, floating, behind and dense plans, run shapes, the pair shape, assertions, an at-risk pattern, automata of more than
128 positions, a walk that outlives max_walk, own ranges with a carry -- three rounds per object, so that the hints turn
warm.  Prints per call the match count and every rj_stats field but the two times.  Two builds that route alike print the
same lines:
    python tools/route_trace.py > after.txt     (and the same in the tree before; diff the two)"""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rejit_amd


def mix(alphabet, n, seed, plant=b"", every=0):
    rng = np.random.default_rng(seed)
    t = bytearray(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes())
    for p in range(every // 2, max(n - len(plant), 0), every or n):
        t[p:p + len(plant)] = plant
    return bytes(t)


def groups(n, seed):      # floating windows: matches that overlap the next group's candidates (test_no_local_select_...)
    rng, parts, size = random.Random(seed), [], 0
    while size < n:
        p = rng.choice([b"axyzababxyzb", b"bbxyzaxyzab", b"xyz", b"ab", b"c", b" ", b"abab"]) + bytes(rng.choice(b"abc xyz") for _ in range(rng.randrange(40)))
        parts.append(p)
        size += len(p)
    return b"".join(parts)[:n]


N = 400000
_rng = random.Random(9)       # a wide cyclic automaton over its own words: one candidate that outlives every walk (the carry scan)
CYCLE = ["".join(_rng.choice("abcd") for _ in range(_rng.randint(6, 10))) for _ in range(40)]
LOG = mix(b"abcdefgh <>#()\n \"", N, 1)
WORDS = mix(b"acgtacgtacgtacgtN\xf0", N, 2)
LONG_RUN = WORDS[:100000] + mix(b"acgt", 280000, 3) + WORDS[:20000]
TEXTS = {
    "log": LOG, "sparse": mix(b"cdefgh\n", N, 4, b"a cd b <x> # y", 190000), "words": WORDS, "long_run": LONG_RUN,
    "regexp": mix(b"regxp ab\n\x80", 1 << 20, 5, b"regexp", 40000), "regexp_dense": b"regexp" * 60000, "groups": groups(N, 6),
    "digits": mix(b"abcd0123456789 \n", N, 7, b"271828abcd", 3000), "mail": mix(b"abcdx \nAB@.", 300000, 8, b"ab@cd@ef", 9000),
    "xy": mix(b"xxxy", 50000, 9), "lines": mix(b"abc \n", N, 10), "few": mix(b"abc \n", 60000, 11, b"qzvwab ", 5000),
    "many": mix(b"abc \n", 60000, 12, b"qzvwab ", 8), "float_wide": mix(b"ab c\n", 200000, 13, b"babxyzab", 600),
    "cycle": ("".join(_rng.choice(CYCLE) for _ in range(12000)) + "x" + "".join(_rng.choice(CYCLE) for _ in range(500)) + "ab").encode(),
    "risk": mix(b"abcd \n", N, 14), "small": mix(b"abcdefgh <>#()\n \"regxp", 20000, 15, b"regexp", 900),
}
# (pattern, [text names]): every text is run whole, as two halves with the selection carried over the cut, and counted
CASES = [
    (b"regexp", ["regexp", "regexp_dense", "small"]), (b"agggtaaa|tttaccct", ["words"]), (b"[ab]{1,4}xyz[ab]+", ["groups", "float_wide"]),
    (b"(ab|b){2,5}xyz[ab]{1,140}", ["float_wide", "groups"]), (b"[0-9]+abcd", ["digits", "log"]), (b"[a-z]+@[a-z]+", ["mail", "lines"]),
    (b"[acgt]+", ["words", "long_run", "words"]), (b"(x|y)y", ["xy"]), (b"x*", ["xy"]), (b"[A-Z][a-z]+", ["log"]),
    (b"a.*b", ["log", "sparse", "sparse", "log"]), (b"#.*", ["log", "sparse"]), (b"<[^>]*>", ["sparse", "log"]), (b" +", ["log", "long_run"]),
    (b'"[^"]*"', ["log", "small"]), (b"^", ["lines"]), (b"$", ["lines", "small"]), (b".{0,2}(ab|cd)", ["risk", "small"]),
    (b"qzvw[a-z]{1,140}", ["many", "few"]), (("(" + "|".join(CYCLE) + ")+").encode(), ["cycle", "lines", "cycle"]),
]
FIELDS = ("n_hits", "n_candidates", "n_matches", "retries", "large_path", "exact_path", "linear_path", "stream_path", "slow_starts",
          "count_path", "run_path")


def main():
    device = {name: torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for name, t in TEXTS.items()}
    for rx, names in CASES:
        scan = rejit_amd.Scan(rejit_amd.Program(rx))

        def call(what, name, k):
            st = scan.stats()
            print(rx.decode()[:40], name, what, k, " ".join("%s=%d" % (f, st[f]) for f in FIELDS), flush=True)
        for rnd in range(3):
            for name in names:
                p, n = device[name].data_ptr(), len(TEXTS[name])
                call("run%d" % rnd, name, scan.run(p, n))
                cut = n // 3 + 17
                k = scan.run(p, n, own_begin=0, own_end=cut)
                call("head%d" % rnd, name, k)
                carry = {}
                if k:
                    b, e = scan.spans()[-1]
                    carry = dict(carry_cur=e if e > b else b + 1, carry_prev_end=e, have_prev=True)
                call("tail%d" % rnd, name, scan.run(p, n, own_begin=cut, own_end=n + 1, **carry))
                call("count%d" % rnd, name, scan.count(p, n))


if __name__ == "__main__":
    main()
