"""The meaning of rj_scan_records_zip, written in Python independently of the library (tests/test_record_zip.py on the CPU,
tests/test_gpu_record_zip.py on the device): line j is sep.join(column c's row j, rjust / ljust to |width| with the pad
byte), and the layout is the pack's -- `lead` fill bytes, every line, `gap` fill bytes behind each."""
import random

EMIT_CHUNK = 4096      # rejit_amd/csrc/record_zip.h: kEmitChunk
STREAM_BYTES = 32      # rejit_amd/csrc/record_zip.h: kStreamBytes, the tier threshold T
SEAM_LENGTHS = (0, 1, 15, 16, 17, 33)


def pieces(text, begins, ends, indices=None):
    """-> the rows of a column as bytes"""
    rows = range(len(begins)) if indices is None else indices
    return [bytes(text[begins[r]:ends[r]]) for r in rows]


def field(piece, width, pad):
    p = bytes([pad])
    return piece.rjust(width, p) if width > 0 else piece.ljust(-width, p)


def lines(columns, sep=b"", widths=None, pad=32):
    """columns: a list of lists of bytes, all of one length -> the lines"""
    widths = [0] * len(columns) if widths is None else widths
    return [sep.join(field(col[j], w, pad) for col, w in zip(columns, widths)) for j in range(len(columns[0]))]


def layout(rows, fill=10, lead=0, gap=1):
    """-> (text, begins, ends)"""
    f = bytes([fill])
    out, begins, ends = [f * lead], [], []
    at = lead
    for row in rows:
        begins.append(at)
        ends.append(at + len(row))
        out.append(row + f * gap)
        at += len(row) + gap
    return b"".join(out), begins, ends


def table(lengths, seed, junk=3, alphabet=None):
    """a text with one record per length, `junk` other bytes (at most) between two records and in front -> (text, begins, ends);
    a record's bytes tell its number and place (no two records are alike by accident)"""
    rng = random.Random(seed)
    alphabet = alphabet or bytes(range(0x21, 0x7F))
    out, begins, ends = bytearray(), [], []
    for length in lengths:
        out += b"~" * rng.randrange(junk + 1)
        begins.append(len(out))
        out += bytes(alphabet[(len(out) + 7 * i + length) % len(alphabet)] for i in range(length))
        ends.append(len(out))
    out += b"~" * rng.randrange(junk + 1)
    return bytes(out), begins, ends


def seam_columns(rows=600, seed=14):
    """the seam test's fixed table: `rows` rows x 3 columns over three texts, piece lengths drawn from SEAM_LENGTHS"""
    rng = random.Random(seed)
    return [table([rng.choice(SEAM_LENGTHS) for _ in range(rows)], seed + 1 + c) for c in range(3)]


def segments(columns, sep, widths, pad, lead, gap):
    """-> every segment of the output as (kind, begin, end): kind in piece, pad, sep, row, gap (empty ones included)"""
    out = []
    at = lead
    for j in range(len(columns[0])):
        row0 = at
        for c, (col, w) in enumerate(zip(columns, widths)):
            if c:
                out.append(("sep", at, at + len(sep)))
                at += len(sep)
            padding = max(abs(w) - len(col[j]), 0)
            if w > 0:
                out.append(("pad", at, at + padding))
                at += padding
            out.append(("piece", at, at + len(col[j])))
            at += len(col[j])
            if w < 0:
                out.append(("pad", at, at + padding))
                at += padding
        out.append(("row", row0, at))
        out.append(("gap", at, at + gap))
        at += gap
    return out


def seam_coverage(columns, sep, widths, pad, leads, gap, chunk=EMIT_CHUNK):
    """over the sweep of `leads`: per kind, the offsets inside a 16-byte group at which a non-empty segment of the kind BEGAN (for
    a row: at which it ENDED), and how often a chunk's end fell inside one -> ({kind: set of offsets}, {kind: count})"""
    kinds = ("piece", "pad", "sep", "row", "gap")
    offsets, crossed = {kind: set() for kind in kinds}, {kind: 0 for kind in kinds}
    for lead in leads:
        for kind, a, b in segments(columns, sep, widths, pad, lead, gap):
            if a == b:
                continue
            offsets[kind].add((b if kind == "row" else a) % 16)
            if (b - 1) // chunk != a // chunk:      # a chunk ends behind the segment's first byte and before its last
                crossed[kind] += 1
    return offsets, crossed
