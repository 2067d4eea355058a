"""At-risk patterns past the limits of the exact replay (rejit_amd/csrc/exact_replay.hip), their seeded texts, and what the
engine's routing makes of them -- shared by tests/golden/make_golden.py (wide_artefact_vectors.json), the CPU fixture test
(test_wide_artefact_fixture.py) and the GPU test (test_gpu_wide_artefact.py).

Three classes, by what decides the path a whole-text MatchAll of an at-risk pattern takes when the reference's ring artefact
applies:
  A  <= 1024 positions and a ring of <= 448 slots (times x n_states): the parallel replay          (the control)
  B  <= 1024 positions, a ring of more than 448 slots: one lane per stretch between synchronisation points
  C  more than 1024 positions: no synchronisation points; one lane over the whole text
Texts are generated from a seed, never stored: 'adjacent' plants the pattern's words back to back over a background that
matches on its own (the artefact arises), 'spread' puts them on lines of their own (no candidate begins where another ends:
the reference's answer is the documented one)."""
import random
import zlib

SEED = 20261016
SIZES = (1 << 10, 1 << 14, 1 << 16)
KINDS = ("adjacent", "spread")
WALK_SLOTS = 448        # exact_replay.hip: kWalkSlots
WALK_WORDS = 32         # exact_replay.hip: exact_replay_fits (1024 positions)


def words(k, seed, lo=6, hi=10, alphabet="abcd"):
    rng = random.Random(seed)
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(k)]


def literals(m, length, seed, alphabet="ab"):
    rng = random.Random(seed)
    return ["".join(rng.choice(alphabet) for _ in range(length)) for _ in range(m)]


def _case(name, cls, head, pieces, tail="", background="abcd\n"):
    return dict(name=name, cls=cls, regex=head + "(" + "|".join(pieces) + ")" + tail, pieces=pieces, background=background)


def patterns():
    """The fixture's patterns: `.{0,k}(word alternation)` of several widths, long literals behind a short class run (times
    near 65: rings of B size with few positions), nested groups with `^` / `$` inside repetitions, nullable ones."""
    return [
        _case("A_words40", "A", ".{0,2}", words(40, 1)),
        _case("A_words110", "A", ".{0,3}", words(110, 2)),
        _case("A_lit2", "A", "[ab]{0,2}", literals(2, 64, 3), background="ab\n"),
        _case("A_words20_nullable", "A", ".{0,2}", words(20, 12), tail="?"),
        _case("B_dot8_lit4", "B", ".{0,8}", literals(4, 64, 4), background="ab\n"),
        _case("B_class6_lit6", "B", "[ab]{0,6}", literals(6, 64, 5), background="ab\n"),
        _case("B_dot7_lit3_nullable", "B", ".{0,7}", literals(3, 64, 6), tail="?", background="ab\n"),
        _case("B_class5_lit5", "B", "[ab]{0,5}", literals(5, 64, 13), background="ab\n"),
        _case("B_dot10_lit3", "B", ".{0,10}", literals(3, 64, 14), background="ab\n"),
        _case("B_nested_anchors", "B", "(^[ab]{1,2}.|[ab]?b\\n*|\\nb\\nb+){,2}^{1,2}", literals(3, 64, 7), tail="$", background="ab\n"),
        _case("C_words140", "C", ".{0,2}", words(140, 1)),
        _case("C_words220", "C", ".{0,2}", words(220, 1)),
        _case("C_dot5_words140", "C", ".{0,5}", words(140, 8)),
        _case("C_class2_lit20", "C", "[ab]{0,2}", literals(20, 64, 9), background="ab\n"),
        _case("C_anchored_words140", "C", "(^.{0,2}|\\n)", words(140, 10), tail="$"),
    ]


def text_seed(name, size, kind):
    return zlib.crc32(("%d/%s/%d/%s" % (SEED, name, size, kind)).encode())


def make_text(case, size, kind, seed=None):
    """Bytes of `size`: 'adjacent' -- random background, pieces planted at random, half of them followed at once by
    another; 'spread' -- every piece on a line of its own between empty lines."""
    rng = random.Random(text_seed(case["name"], size, kind) if seed is None else seed)
    pieces = case["pieces"]
    if kind == "spread":
        out = bytearray()
        while len(out) < size:
            out += b"\n" * rng.randint(3, 12) + rng.choice(pieces).encode()
        out = out[:size]
        # (a piece cut by the end of the text must not end it: a match of a prefix would then end at n)
        cut = out.rfind(b"\n")
        out[cut:] = b"\n" * (size - cut)
        return bytes(out)
    bg = case["background"]
    buf = bytearray("".join(rng.choice(bg) for _ in range(size)).encode())
    longest = max(len(p) for p in pieces)
    for _ in range(max(1, size // (4 * longest))):
        at = rng.randrange(0, max(1, size - 2 * longest - 1))
        for _k in range(1 + (rng.random() < 0.5)):
            w = rng.choice(pieces).encode()
            buf[at:at + len(w)] = w
            at += len(w)
    return bytes(buf[:size])


def classify(n_pos, n_words, slots):
    if n_words > WALK_WORDS:
        return "C"
    return "B" if slots > WALK_SLOTS else "A"
