"""The meaning of rj_scan_records_format_csv, written in Python independently of the library and with bytes, not with the csv
module (tests/test_record_csv_format.py on the CPU, tests/test_gpu_record_csv_format.py on the device): line j is the columns'
rows j joined with the delimiter, a field between two quote bytes where it holds a special byte (or its column is in `always`,
or it is the lone empty field), the quote bytes inside doubled unless the column is raw; the layout is the pack's
(zip_cases.layout).  python_lines runs csv.writer over latin-1 for the agreement check."""
import csv
import io
import random

from zip_cases import layout, pieces, table  # noqa: F401  (the layout arithmetic and the tables are the zip's)

EMIT_CHUNK = 4096      # rejit_amd/csrc/record_csv_format.h: kEmitChunk
STREAM_BYTES = 32      # kStreamBytes: a shorter piece is written byte by byte
WAVE_STEP = 1024       # kWaveStep: source bytes a wave takes at a time
WAVE_BYTES = 1024      # kWaveBytes: a piece this long is classified by its wave
MAX_EXPAND = 128       # kMaxExpand
CHECKPOINT_BYTES = 8192 # kCheckpointBytes: an expanding piece this long leaves checkpoints
TIER_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)


def need(piece, d, q, always, lone):
    return always or any(b in piece for b in (bytes([d]), bytes([q]), b"\r", b"\n")) or (lone and not piece)


def field(piece, d=44, q=34, always=False, raw=False, lone=False):
    if not need(piece, d, q, always, lone):
        return piece
    qq = bytes([q])
    return qq + (piece if raw else piece.replace(qq, qq + qq)) + qq


def lines(columns, d=44, q=34, always=(), raw=()):
    """columns: a list of lists of bytes, all of one length -> the lines"""
    lone = len(columns) == 1
    return [bytes([d]).join(field(col[j], d, q, c in always, c in raw, lone) for c, col in enumerate(columns)) for j in range(len(columns[0]))]


def stats(columns, d=44, q=34, always=(), raw=()):
    """-> (n_quoted, n_doubled)"""
    lone = len(columns) == 1
    quoted = doubled = 0
    for c, col in enumerate(columns):
        for piece in col:
            if need(piece, d, q, c in always, lone):
                quoted += 1
                doubled += 0 if c in raw else piece.count(bytes([q]))
    return quoted, doubled


def python_lines(columns, d=44, q=34, quote_all=False):
    """the same lines from csv.writer over latin-1, without its terminator (rows without NUL: Python before 3.11 cannot write one)"""
    out = []
    for j in range(len(columns[0])):
        buf = io.StringIO(newline="")
        w = csv.writer(buf, delimiter=chr(d), quotechar=chr(q), lineterminator="\r\n", quoting=csv.QUOTE_ALL if quote_all else csv.QUOTE_MINIMAL)
        w.writerow([col[j].decode("latin-1") for col in columns])
        text = buf.getvalue()
        assert text.endswith("\r\n")
        out.append(text[:-2].encode("latin-1"))
    return out


def column_of(rows_bytes, seed=0, junk=3):
    """a column's rows (bytes) as a table: (text, begins, ends), up to `junk` other bytes between two records"""
    rng = random.Random(seed)
    out, begins, ends = bytearray(), [], []
    for piece in rows_bytes:
        out += b"~" * rng.randrange(junk + 1)
        begins.append(len(out))
        out += piece
        ends.append(len(out))
    out += b"~" * rng.randrange(junk + 1)
    return bytes(out), begins, ends


def random_rows(count, n_cols, seed, d=44, q=34, upto=8, nul=False):
    """random fields of 0..upto bytes over an alphabet with d, q, \\r, \\n, a space and a high byte -> columns (lists of bytes)"""
    rng = random.Random(seed)
    alphabet = bytes([d, q, 13, 10, 32, 0xE9, 0x61, 0x62]) + (b"\0" if nul else b"")
    return [[bytes(rng.choice(alphabet) for _ in range(rng.randint(0, upto))) for _ in range(count)] for _ in range(n_cols)]


def tier_pieces(q=34, lengths=TIER_LENGTHS, body=0x61):
    """every length with no quote, with one quote at EVERY position, and all quotes"""
    out = []
    for n in lengths:
        out.append(bytes([body]) * n)
        for i in range(n):
            out.append(bytes([body]) * i + bytes([q]) + bytes([body]) * (n - i - 1))
        if n:
            out.append(bytes([q]) * n)
    return out


def seam_cases(boundary, d=44, q=34):
    """-> [(name, columns, lead)]: two-column one-row calls whose `lead` puts a chosen output byte at boundary - 2 .. boundary + 2:
    the opening quote, the first and the second byte of a doubled quote, the closing quote, a delimiter -- for a short piece
    (bytes tier) and a long one (expand tier)"""
    out = []
    for long_piece in (False, True):
        stem = b"x" * (40 if long_piece else 3)
        first = stem + bytes([q]) + b"yz"            # line: q stem q q y z q d w
        cols = [[first], [b"w" * 5]]
        marks = {"open": 0, "double0": 1 + len(stem), "double1": 2 + len(stem), "close": len(stem) + 5, "delimiter": len(stem) + 6}
        for name, at in marks.items():
            for off in (-2, -1, 0, 1, 2):
                lead = boundary + off - at
                if lead >= 0:
                    out.append(("%s%s%+d" % (name, "-long" if long_piece else "", off), cols, lead))
    return out
