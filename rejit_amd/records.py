"""Record tables for Scan.run_records (rj_scan_records, include/rejit_hip.h): torch plumbing only -- every table is built
from device tensors, the matching and the join are the library's kernels."""
from __future__ import annotations

from typing import List, Sequence, Tuple

from .api import Program, Scan


def line_records(text_tensor, stream=None):
    """(rec_begin, rec_end): the lines of `text_tensor` (contiguous uint8 on the GPU) as int64 device tensors.  The begins
    are the matches of `^` (a MatchAll on the device, emit_scan.hip: the line table of a grep-like caller); a line ends
    before its line break, the last one at the end of the text.  A text that ends in a line break has a last, empty line
    behind it, exactly as `^` sees it."""
    import torch

    n = int(text_tensor.numel())
    scan = Scan(Program(b"^"))
    scan.run_tensor(text_tensor, stream=stream)
    begins = scan.spans_tensor(text_tensor.device)[:, 0].contiguous()
    ends = torch.empty_like(begins)
    if begins.numel():
        ends[:-1] = begins[1:] - 1     # (the byte before the next line's begin is this line's break)
        ends[-1] = n
    return begins, ends


def pack_records(texts: Sequence[bytes], sep: int, device, lead: int = 0, gap: int = 1):
    """(text_tensor, rec_begin, rec_end) on `device`: the packed layout of rj_match_all_packed -- `lead` separator bytes, then
    every text followed by `gap` >= 1 bytes of `sep` (Program.batch_separator()), so that no match crosses a record."""
    import numpy as np
    import torch

    assert gap >= 1 and 0 <= sep < 256
    sizes = np.array([len(t) for t in texts], dtype=np.int64)
    begins = lead + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]]).astype(np.int64) if len(texts) else np.zeros(0, dtype=np.int64)
    total = lead + int(sizes.sum()) + gap * len(texts)
    buf = np.full(max(total, 1), sep, dtype=np.uint8)
    for b, t in zip(begins, texts):
        buf[b:b + len(t)] = np.frombuffer(t, dtype=np.uint8)
    text = torch.from_numpy(buf[:total].copy() if total else buf[:0].copy()).to(device)
    return text, torch.from_numpy(begins).to(device), torch.from_numpy(begins + sizes).to(device)


def offsets_records(offsets):
    """(rec_begin, rec_end) of an Arrow-style offsets tensor (k + 1 ascending offsets of k strings that touch): views of it
    when it is a contiguous int64 tensor (rec_begin = offsets[:-1], rec_end = offsets[1:]), else of an int64 copy (Arrow's
    default offsets are int32).  The records touch, so a match can run from one string into the next: Scan.pack_records
    with the program's separator makes them independent."""
    import torch

    assert offsets.dim() == 1 and offsets.numel() >= 1
    o = offsets.to(torch.int64).contiguous()
    return o[:-1], o[1:]


def relative_spans(spans, result, rec_begin, i: int):
    """Record i's matches relative to its begin: an (count, 2) int64 tensor -- spans = the scan's spans_tensor after
    run_records, result = what run_records returned."""
    f, c = int(result.first[i]), int(result.counts[i]) & 0xFFFFFFFF
    return spans[f:f + c] - rec_begin[i]


def all_relative_spans(spans, result, rec_begin) -> List[List[Tuple[int, int]]]:
    """Every record's matches relative to its begin, as Python lists (tests, small tables)."""
    sp = spans.cpu().tolist()
    out = []
    for f, c, b in zip(result.first.cpu().tolist(), result.counts.cpu().tolist(), rec_begin.cpu().tolist()):
        out.append([(x - b, y - b) for x, y in sp[f:f + (c & 0xFFFFFFFF)]])
    return out


def field_records(piece_begin, piece_end, piece_first, f: int):
    """(begin, end, present): field f (0-based; negative: counted from the row's end) of every row of a piece table
    (Scan.split_records) as a record table -- int64 tensors of k rows -- and a bool tensor that says which rows have such a
    field.  A row with fewer fields gets the empty record at its last piece's end (a row without any piece, and a table
    without pieces: the empty record at 0)."""
    import torch

    lo, hi = piece_first[:-1], piece_first[1:]
    at = lo + f if f >= 0 else hi + f
    present = (at >= lo) & (at < hi)
    n_pieces = int(piece_begin.numel())
    if n_pieces == 0:
        zero = torch.zeros_like(lo)
        return zero, zero.clone(), present
    last = (hi - 1).clamp(min=0)
    has_any = hi > lo
    fallback = torch.where(has_any, piece_end[last], torch.zeros_like(lo))
    pick = torch.where(present, at, torch.zeros_like(at))
    begin = torch.where(present, piece_begin[pick], fallback)
    end = torch.where(present, piece_end[pick], fallback)
    return begin.contiguous(), end.contiguous(), present


def nonempty_pieces(piece_begin, piece_end):
    """The indices (int64, ascending) of the pieces with end > begin: with Scan.pack_records over the piece table, the
    fields or matches that have bytes."""
    import torch

    return torch.nonzero(piece_end > piece_begin).reshape(-1).contiguous()


def top_groups(count, rep, top: int):
    """(count, rep, group) of the `top` most frequent groups of Scan.group_records: by descending count, ties in order of
    first appearance (a stable sort over the G groups: `sort -rn | head` over `uniq -c`).  group: the groups' numbers."""
    import torch

    _, order = torch.sort(count, descending=True, stable=True)
    order = order[:max(int(top), 0)].contiguous()
    return count[order].contiguous(), rep[order].contiguous(), order


def sorted_groups(scan, text, rec_begin, rec_end, indices=None):
    """Scan.group_records followed by Scan.sort_records over the distinct rows: (rep_sorted, count_sorted, group_sorted).
    rep_sorted is the dictionary in byte order (`sort -u`; pack_records over the rows rep_sorted, indices[rep_sorted] when
    there are indices, prints it), count_sorted its counts (`sort | uniq -c`), group_sorted[j] row j's number in that order
    -- a dictionary encoding whose codes compare as the strings do.  The sort sees G rows, not k."""
    import torch

    group, rep, count = scan.group_records(text, rec_begin, rec_end, indices=indices)
    rows = rep if indices is None else indices[rep].contiguous()
    order = scan.sort_records(text, rec_begin, rec_end, indices=rows)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), dtype=torch.int64, device=order.device)
    return rep[order].contiguous(), count[order].contiguous(), rank[group].contiguous()


def join_rows(index, set_group, set_count):
    """(probe_row, set_row): ALL pairs of the inner join of a probe table with a set table on their rows' bytes, int64 tensors
    of equal length on index's device.  index: Scan.lookup_records of the probe rows against the set's dictionary -- the rows
    `rep` of Scan.group_records over the set table as set_indices --, so a group number per probe row, or -1; set_group and
    set_count: that group call's `group` and `count`.  The pairs are ordered by probe row, then by ascending set row.  Torch
    only and device-agnostic: a stable argsort of set_group lists every group's set rows in ascending order, an exclusive
    cumsum of set_count says where a group's run begins, repeat_interleave expands every probe row by its group's count."""
    import torch

    found = torch.nonzero(index >= 0).reshape(-1)
    groups = index[found]
    by_group = torch.argsort(set_group, stable=True)
    first = torch.cumsum(set_count, 0) - set_count
    counts = set_count[groups]
    probe_row = torch.repeat_interleave(found, counts)
    begin = torch.cumsum(counts, 0) - counts                      # where a probe row's pairs begin in the output
    within = torch.arange(probe_row.numel(), dtype=torch.int64, device=index.device) - torch.repeat_interleave(begin, counts)
    set_row = by_group[torch.repeat_interleave(first[groups], counts) + within]
    return probe_row.contiguous(), set_row.contiguous()


def group_sums(group, values, ok, n_groups: int):
    """The per-group sum of the OK rows' values: `awk '{s[$1] += $2}'` behind Scan.group_records (group: its `group`, n_groups:
    the length of its `rep`) and Scan.parse_records (values; ok: status == PARSE_OK, a bool tensor) over the same rows.  A
    tensor of n_groups entries of values' dtype on its device: int64 sums wrap as int64 does, float64 sums are added in
    index_add_'s order of the rows (on a GPU that order is not fixed: the last bits may differ from run to run).  Rows that
    are not ok add 0; a group without an ok row sums to 0 (group_counts_ok tells it from a sum of 0).  Torch only and
    device-agnostic."""
    import torch

    sums = torch.zeros(int(n_groups), dtype=values.dtype, device=values.device)
    return sums.index_add_(0, group, torch.where(ok, values, torch.zeros_like(values)))


def group_counts_ok(group, ok, n_groups: int):
    """The number of OK rows per group (int64, n_groups entries): the divisor of a mean, and what tells an empty sum from 0."""
    import torch

    counts = torch.zeros(int(n_groups), dtype=torch.int64, device=group.device)
    return counts.index_add_(0, group, ok.to(torch.int64))


def time_buckets(values, status, width: int):
    """(bucket_start, ok) of Scan.parse_time_records' (values, status): bucket_start[j] = floor(values[j] / width) x width, the
    floor toward minus infinity, so an instant before 1970 lies in the bucket that begins at or before it (-1 with width 60 is
    in the bucket -60); ok = status == PARSE_OK, a bool tensor -- the rows that are not ok have the value 0 and must be left
    out by it.  `width` is a positive count of the values' unit: "requests per minute" is time_buckets(..., 60) over seconds,
    then torch.unique(bucket_start[ok], return_counts=True).  Torch only and device-agnostic."""
    import torch

    width = int(width)
    if width < 1:
        raise ValueError("time_buckets: width is a positive number of units, not %r" % (width,))
    start = torch.div(values, width, rounding_mode="floor") * width
    return start, status == 0


# ---- byte tables for Scan.translate_records (rj_scan_records_translate): bytes plumbing only
class DropSet(bytes):
    """the 32-byte (256-bit) drop set of rj_scan_records_translate: byte b is dropped when bit (b & 7) of self[b >> 3] is set
    (a type of its own, so that translate_records can tell it from the bytes to delete)"""


def byte_map(src: bytes = b"", dst: bytes = b"") -> bytes:
    """The 256-byte table that maps src[i] to dst[i] and every other byte to itself (bytes.maketrans with one rule more: where
    a byte stands in src twice, the later pair wins)."""
    if len(src) != len(dst):
        raise ValueError("byte_map: src has %d bytes, dst %d" % (len(src), len(dst)))
    table = bytearray(range(256))
    for a, b in zip(src, dst):
        table[a] = b
    return bytes(table)


def drop_set(delete: bytes) -> DropSet:
    """The drop set that holds the bytes of `delete`."""
    bits = bytearray(32)
    for b in delete:
        bits[b >> 3] |= 1 << (b & 7)
    return DropSet(bits)


ASCII_LOWER = byte_map(bytes(range(0x41, 0x5B)), bytes(range(0x61, 0x7B)))   # str.lower over ASCII, Arrow's ascii_lower
ASCII_UPPER = byte_map(bytes(range(0x61, 0x7B)), bytes(range(0x41, 0x5B)))   # str.upper over ASCII, Arrow's ascii_upper


# ---- the tables of Scan.csv_records (rj_scan_records_csv): torch plumbing only
def csv_column(row_first, c: int):
    """(field_index, present): the number of the field in column c (0-based; negative: counted from the row's end) of every
    row of Scan.csv_records' row_first -- an int64 tensor of n_rows entries, the `indices` of every other record call over
    (field_begin, field_end) -- and a bool tensor that says which rows have such a column.  A ragged row that lacks it is
    not present, and its index is its own first field's (every row has one), so that the index stays valid: leave those rows
    out with `present`."""
    import torch

    lo, hi = row_first[:-1], row_first[1:]
    at = lo + c if c >= 0 else hi + c
    present = (at >= lo) & (at < hi)
    return torch.where(present, at, lo).contiguous(), present


def csv_bad_rows(row_first, field_flags):
    """A bool tensor of n_rows entries: does the row hold a field with a CSV_MALFORMED flag (its values are the rule's, not a
    CSV reader's: include/rejit_hip.h)."""
    import torch
    from .api import CSV_MALFORMED

    bad = ((field_flags & CSV_MALFORMED) != 0).to(torch.int64)
    upto = torch.cat([torch.zeros(1, dtype=torch.int64, device=bad.device), torch.cumsum(bad, 0)])
    return upto[row_first[1:]] > upto[row_first[:-1]]


def csv_cut(scan, text, csv_result, cols, delimiter: bytes = b",", quote: bytes = b'"', rows=None, fill: int = 10, lead: int = 0, gap: int = 1):
    """(out_text, out_begin, out_end): the columns `cols` (0-based; negative: counted from the row's end, as csv_column) of the
    rows of Scan.csv_records' result -- all of them, or those the int64 tensor `rows` names -- written as CSV lines again by
    Scan.format_csv_records, in that order, as a packed device text with its record table.  The fields go in as RAW columns
    straight from the original text -- their interiors as csv_records delimits them, `""` still in place: no pack, no
    unescape --, so a field comes out quoted exactly when its value needs it.  A ragged row's absent column is written as an
    empty field.  Rows with a CSV_MALFORMED field are the caller's to leave out (csv_bad_rows).  `scan` lends scratch only."""
    import torch

    columns = []
    for c in cols:
        index, present = csv_column(csv_result.row_first, int(c))
        if rows is not None:
            index, present = index[rows], present[rows]
        begin = csv_result.field_begin[index].contiguous()
        end = torch.where(present, csv_result.field_end[index], begin).contiguous()
        columns.append((text, begin, end))
    return scan.format_csv_records(columns, delimiter=delimiter, quote=quote, raw=range(len(columns)), fill=fill, lead=lead, gap=gap)


def csv_values(scan, text, field_begin, field_end, field_flags, indices=None, quote: bytes = b'"', fill: int = 10):
    """(out_text, out_begin, out_end): the VALUES of the fields of Scan.csv_records -- all of them, or those `indices` names
    (csv_column) -- as a packed device text with its record table, a doubled quote read as one.  When no chosen field is
    CSV_ESCAPED that is scan.pack_records; otherwise the pack, then a scan for the doubled quote over the PACKED text, then
    replace_records with the single one.  (Never a scan of the original text: in a field whose value begins with a quote (three quote bytes, then `a`, then one) the leftmost match would pair the
    opening quote with the first byte of the escape and cross the field's begin; in the packed text the separator `fill`,
    which must not be the quote, makes the fields independent.)  `scan` lends scratch only."""
    import torch
    from .api import CSV_ESCAPED

    chosen = field_flags if indices is None else field_flags[indices]
    packed, ob, oe = scan.pack_records(text, field_begin, field_end, indices=indices, fill=fill)
    if not bool(((chosen & CSV_ESCAPED) != 0).any()):
        return packed, ob, oe
    q = bytes(quote)
    assert len(q) == 1 and q[0] != fill
    finder = getattr(scan, "_csv_unescape", None)
    if finder is None or finder[0] != q:
        lit = b"\\x%02x" % q[0]
        finder = (q, Scan(Program(lit + lit)))
        scan._csv_unescape = finder
    found = finder[1].run_records(packed, ob, oe)
    return finder[1].replace_records(packed, ob, oe, found, q, fill=fill)
