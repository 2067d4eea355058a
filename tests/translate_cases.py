"""The meaning of rj_scan_records_translate, written in Python independently of the library (tests/test_record_translate.py on
the CPU, tests/test_gpu_record_translate.py on the device): row j is bytes.translate(table, delete) of the record it names, and
the layout is the pack's -- `lead` fill bytes, every row, `gap` fill bytes behind each."""
import random

SLAB = 4096        # rejit_amd/csrc/record_translate.h: kSlab, positions of the virtual stream per slab
IMAGE = 4096       # rejit_amd/csrc/record_translate.h: kImage, output bytes per turn of the emit
GROUP = 16         # positions a lane takes at a time

IDENTITY = bytes(range(256))
LOWER = bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in range(256))
UPPER = bytes(b - 32 if 0x61 <= b <= 0x7A else b for b in range(256))


def drop_bits(delete):
    """the 32-byte drop set: bit (b & 7) of byte b >> 3"""
    bits = bytearray(32)
    for b in delete:
        bits[b >> 3] |= 1 << (b & 7)
    return bytes(bits)


def rows_of(text, begins, ends, indices=None):
    order = range(len(begins)) if indices is None else indices
    return [bytes(text[begins[r]:ends[r]]) for r in order]


def translate(rows, table=None, delete=b""):
    return [row.translate(table, delete) for row in rows]


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


def stats(rows, table=None, delete=b""):
    table = IDENTITY if table is None else table
    joined = b"".join(rows)
    kept = joined.translate(None, delete)
    changing = bytes(b for b in range(256) if table[b] != b)
    return {"bytes_in": len(joined), "bytes_dropped": len(joined) - len(kept), "bytes_changed": len(kept) - len(kept.translate(None, changing))}


def table(lengths, seed, junk=3, alphabet=None):
    """a text with one record per length, `junk` other bytes (at most) between two records and in front -> (text, begins, ends)"""
    rng = random.Random(seed)
    alphabet = alphabet or bytes(range(256))
    out, begins, ends = bytearray(), [], []
    for length in lengths:
        out += b"~" * rng.randrange(junk + 1)
        begins.append(len(out))
        out += bytes(rng.choice(alphabet) for _ in range(length))
        ends.append(len(out))
    out += b"~" * rng.randrange(junk + 1)
    return bytes(out), begins, ends


def stream_places(lengths):
    """the rows' places in the virtual stream (a row's bytes, then one terminator) -> (sb, S)"""
    sb, at = [], 0
    for length in lengths:
        sb.append(at)
        at += length + 1
    return sb, at


def seam_lengths(slab, n_slabs, reach, rng):
    """row lengths whose begins and terminators fall at every offset within +-reach of every slab seam of a stream of about
    n_slabs slabs -- one table per call cannot hold them all, so -> a list of length lists, one per offset"""
    tables = []
    for off in range(-reach, reach + 1):
        lengths, at = [], 0
        for seam in range(1, n_slabs):
            target = seam * slab + off           # a row's terminator stands here, the next row begins behind it
            while target - at > slab // 2:
                step = rng.randrange(1, slab // 4)
                lengths.append(step - 1)
                at += step
            lengths.append(target - at)
            at = target + 1
        lengths.append(slab // 2 + rng.randrange(0, 40))      # the last slab, half full
        tables.append(lengths)
    return tables
