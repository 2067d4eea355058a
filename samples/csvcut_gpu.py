#!/usr/bin/env python3
"""csvcut_gpu.py FILE (-c COLS | -C COLS | -g N -a M) [-d DELIM] -- columns of a CSV file with quoted fields, with everything between
the upload and the answer on the GPU:

    the file is uploaded once; rj_scan_records_csv (Scan.csv_records) reads its rows and fields -- a delimiter or a line break
    inside quotes is data --; records.csv_column picks a column's field of every row, records.csv_values packs the fields'
    values (`""` read as `"`), and rj_scan_records_zip puts the columns side by side: that text is the only download.

  -c COLS   print the columns COLS (1-based, comma separated, in that order) of every row, tab-separated, one row per line;
            a row without such a column prints an empty value (`csvcut -c`, values unquoted)
  -C COLS   print the same columns as CSV again, with the input's delimiter: a field that holds the delimiter, a quote or a line
            break stands in quotes, as Python's csv.writer writes it (records.csv_cut: rj_scan_records_format_csv over the
            fields' interiors in the uploaded text -- no pack, no unescape; `csvcut -c`)
  -g N -a M   print every distinct value of column N, in order of first appearance, a tab, and the int64 sum of column M over
            its rows (rj_scan_records_group, rj_scan_records_parse, records.group_sums, rj_scan_records_format); a value of M
            that is not an integer [+-]?[0-9]+ (spaces and tabs around it dropped) adds 0
  -d DELIM  the delimiter, one byte (default `,`)

A row with malformed quoting (a quote inside an unquoted field, bytes behind a closing quote, a bare \\r, an unterminated last
field) is named on stderr by its 1-based number and left out.  Exit status 0, 1 when a row was malformed, 2 on errors."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def option(argv, name):
    if name in argv[:-1]:
        at = argv.index(name)
        return argv[at + 1], argv[:at] + argv[at + 2:]
    return None, argv


def main(argv):
    cols, argv = option(argv, "-c")
    csv_cols, argv = option(argv, "-C")
    group, argv = option(argv, "-g")
    agg, argv = option(argv, "-a")
    delim, argv = option(argv, "-d")
    delim = b"," if delim is None else os.fsencode(delim)
    numbers = lambda s: s is not None and all(x.isdigit() and int(x) >= 1 for x in s.split(","))
    if len(argv) != 1 or len(delim) != 1 or (cols is not None) + (csv_cols is not None) + (group is not None) != 1 or (group is None) != (agg is None) or (
            cols is not None and not numbers(cols)) or (csv_cols is not None and not numbers(csv_cols)) or (group is not None and not (group.isdigit() and agg.isdigit() and int(group) >= 1 and int(agg) >= 1)):
        sys.stderr.write(__doc__)
        return 2
    import numpy as np
    import torch

    import rejit_amd
    from rejit_amd import records

    if not torch.cuda.is_available():
        sys.stderr.write("csvcut_gpu: no GPU\n")
        return 2
    rejit_amd.build()
    data = np.fromfile(argv[0], dtype=np.uint8)
    if data.size == 0:
        return 0
    text = torch.from_numpy(data).to("cuda:0")                       # the only upload
    scan = rejit_amd.Scan(rejit_amd.Program(b" "))                   # (the record calls borrow a scan's scratch)
    try:
        table = scan.csv_records(text, delimiter=delim, rows=False)
    except rejit_amd.RejitError as err:
        sys.stderr.write("csvcut_gpu: %s\n" % err.message)
        return 2
    bad = records.csv_bad_rows(table.row_first, table.field_flags)
    good = torch.nonzero(~bad).reshape(-1)
    for r in torch.nonzero(bad).reshape(-1).cpu().tolist():
        sys.stderr.write("csvcut_gpu: row %d is malformed\n" % (r + 1))
    status = 1 if int(bad.sum()) else 0
    if good.numel() == 0:
        return status

    def column(c):
        """column c of the good rows as a record table of values; a row without it has the empty value"""
        index, present = records.csv_column(table.row_first, c - 1)
        vt, vb, ve = records.csv_values(scan, text, table.field_begin, table.field_end, table.field_flags, indices=index[good].contiguous())
        return vt, vb, torch.where(present[good], ve, vb).contiguous()
    if csv_cols is not None:
        printed, _, _ = records.csv_cut(scan, text, table, [int(c) - 1 for c in csv_cols.split(",")], delimiter=delim, rows=good)
    elif cols is not None:
        printed, _, _ = scan.zip_records([column(int(c)) for c in cols.split(",")], sep=b"\t")
    else:
        kt, kb, ke = column(int(group))
        groups, rep, _count = scan.group_records(kt, kb, ke)
        at, ab, ae = column(int(agg))
        values, parsed = scan.parse_records(at, ab, ae, kind="int64", trim=True)
        sums = records.group_sums(groups, values, parsed == rejit_amd.PARSE_OK, int(rep.numel()))
        printed, _, _ = scan.zip_records([(kt, kb, ke, rep), scan.format_records(sums.contiguous())], sep=b"\t")
    sys.stdout.flush()
    sys.stdout.buffer.write(printed.cpu().numpy().tobytes())         # the only download
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
