#!/usr/bin/env python3
"""linegrep_gpu.py FILE PATTERN [-c] [-v] [-n] [-p] [-s WITH] [-o] [-f N] [-u [-t K] [-a M | -A M]] [-b] [-k KEYS] [-i] [-D] [-Z] [-T FORMAT -w UNITS [-F OUTFORMAT]] -- count, number or print the lines of FILE in which a match of PATTERN
begins, the way `grep -E -c` / `grep -E -n | cut -d: -f1` / plain `grep -E` do, with everything between the upload and the
answer on the GPU:

    the file is uploaded once; `^` over it is the line table (rejit_amd/records.py: line_records), PATTERN over it the match
    list, rj_scan_records joins the two on the device and rj_scan_records_select lists the lines -- only the four-word
    summary (-c) or the selected line numbers (-n) come back.  -p: rj_scan_records_pack gathers the selected lines, a line
    break behind each, into one new device text -- the program's output, and the only download.

  -c   print the number of selected lines (the default)
  -n   print their 1-based numbers, one per line
  -p   print the selected lines themselves (grep's default output)
  -v   select the lines WITHOUT a match
  -s WITH   print every line -- with -p / -v: every selected line -- with its matches replaced by WITH (rj_scan_records_replace:
       the new text is made on the device and is the only download): `sed -E 's/PATTERN/WITH/g'`, respectively `grep ... | sed ...`
  -o   print every non-empty match of every line -- with -p / -v: of every selected line -- on a line of its own (`grep -E -o`):
       rj_scan_records_split lists the matches per line as a piece table, rj_scan_records_pack gathers the non-empty ones
  -f N   PATTERN is the field separator: print field N (1-based) of every line -- with -p / -v: of every selected line --, an
       empty line where a line has fewer fields (`awk -F PATTERN '{print $N}'`): the fields are rj_scan_records_split's pieces
       between the matches, field N of every row a torch gather over its offsets, the packed fields the only download
  -u   with -o or -f N: print each DISTINCT match or field once, in order of first appearance, with the number of its
       occurrences in front as "%7d %s" (`... | sort | uniq -c` without the sort's order): rj_scan_records_group groups the pieces
       by their bytes on the device; only the packed dictionary and the counts come back
  -t K   with -u: only the K most frequent, by descending count, ties in order of first appearance (`| sort -rn | head -K`)
  -a M   with -f N -u: behind each distinct value of field N also print the SUM of field M (1-based) over its lines, as
       "%7d %s %d" (`awk -F PATTERN '{c[$N]++; s[$N] += $M} END {...}'`): rj_scan_records_parse reads field M of every line as an
       int64 on the device (spaces and tabs around the number are dropped), records.group_sums adds the values per group; only
       the dictionary, the counts and the sums come back.  NOT awk's numeric-prefix rule: awk reads "12abc" as 12, "1.9" as 1.9
       and "1e3" as 1000; here a field adds its value only when ALL of it is an integer [+-]?[0-9]+ inside int64 -- a line whose
       field M is missing, empty, "12abc", "1.9", "1e3" or out of range adds 0 --, and the sum wraps as int64 does
  -A M   as -a M, but the sum is a float64, printed as Python's repr() writes it ("%7d %s %r"): field M is read as a double
       with RJ_PARSE_TRIM | RJ_PARSE_WIDE -- [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?, correctly rounded, so "1.9", "1e3" and
       "0.30000000000000004" add their values --; a field that is missing, malformed, infinite as a double or (more than 64 bits
       of mantissa, rarely) INEXACT adds 0.  The order in which a group's values are added is not fixed, as for any float sum on
       the device.  Not together with -a
  -b   byte order (`LC_ALL=C sort`), made on the device by rj_scan_records_sort: with -u the distinct values print in the
       order of their bytes with their counts (`... | sort | uniq -c`; with -t K the K most frequent, ties in byte order);
       with -p, -o or -f N and no -u the selected lines, the matches or the fields print sorted (`... | sort`)
  -k KEYS   select the lines that have a match of PATTERN AND are equal to a line of the file KEYS (`grep -E PATTERN FILE |
       grep -F -x -f KEYS`); with -f N, where PATTERN is the separator, the lines whose field N is a line of KEYS (`awk -F
       PATTERN 'NR==FNR{s[$0];next} $N in s' KEYS FILE`; a line with fewer fields is not selected).  -v inverts the whole
       selection.  KEYS is uploaded as a second device text; its rows are its lines (without the last, empty one when it ends
       in a line break, as `grep -f` reads it), and rj_scan_records_lookup looks the lines or the fields up in them on the
       device: only the count (-c), the numbers (-n) or the packed lines (-p) come back.  Beside -k only -c, -n, -p, -v and
       -f N are allowed.
  -i   ignore ASCII case: the file's lines are lowered ONCE on the device (rj_scan_records_translate with the A-Z -> a-z table:
       a new device text with its own line table, no download) before the scan and before any grouping or sorting, so a
       lower-case PATTERN is `grep -i`.  With -c / -n / -p the selected row numbers index the original table and the ORIGINAL
       lines are printed; with -u it is `uniq -ci`, with -b `sort -f` (ties aside), and every other option that prints parts of
       lines (-o, -f N, -s WITH) prints them lowered.  Not together with -k
  -D   numbers as text from the device: with -n the 1-based line numbers, with -a M / -A M the sums, are written as decimal
       text by rj_scan_records_format -- str(int) / repr(float), byte for byte -- and only that packed text is downloaded,
       not the values; the output is the output without -D
  -Z   (implies -D) with -u: the printed lines themselves are made on the device -- rj_scan_records_zip puts the counts
       (rj_scan_records_format's text, width 7), the distinct values (their rows straight from the file's text) and, with
       -a M / -A M, the formatted sums side by side with a space between -- and that one text is the only download; the output
       is the output without -Z
  -T FORMAT -w UNITS   with -f N: field N of every line -- with -p / -v: of every selected line -- is read as a TIMESTAMP under
       the strptime-style FORMAT (rj_scan_records_parse_time, in seconds, spaces and tabs around the field dropped; the
       directives are %Y %m %b %d %H %M %S %f %z %%, every other byte a literal; without %z the fields are UTC), and the lines
       are counted per bucket of UNITS seconds: "%7d %d" -- the count and the bucket's first second since 1970-01-01T00:00:00Z,
       the floor toward minus infinity -- in ascending bucket order (`awk '{c[int(t($N)/w)*w]++}'` with a t() awk does not
       have): records.time_buckets and a torch.unique over the int64 values; only the buckets and the counts come back.  A
       line whose field N is missing, not in FORMAT, out of range (month 13, 30 February, a second of 60) or, under %f, has a
       non-zero fraction of a second is counted nowhere.  Only -p and -v go with it; a FORMAT the library refuses (an unknown directive, no %Y / %d /
       month, more than 64 bytes) is an error.  Exit status 0 when a line was counted, else 1
  -F OUTFORMAT   with -T FORMAT -w UNITS: the bucket is printed as a TIMESTAMP under the strftime-style OUTFORMAT (the directives
       of -T; `%Y-%m-%dT%H:%M` for requests per minute) instead of as a number of seconds -- "%7d %s".  The printed lines are
       made on the device: rj_scan_records_format_time writes the buckets, rj_scan_records_format the counts (width 7),
       rj_scan_records_zip puts them side by side with a space between, and that one text is the only download.  An
       OUTFORMAT the library refuses is an error

Exit status 0 when a line was selected, 1 when none was, 2 on errors -- grep's.  The engine's line breaks are \\n and \\r, and
its dialect is the library's (include/rejit.h), not POSIX: for patterns that mean the same in both and cannot match across a
line break the output is grep's.  samples/jrep_gpu.* is the full grep (files, context, -H); this is the per-record API in
forty lines."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(argv):
    repl = None
    if "-s" in argv[:-1]:
        at = argv.index("-s")
        repl, argv = os.fsencode(argv[at + 1]), argv[:at] + argv[at + 2:]
    field = None
    if "-f" in argv[:-1]:
        at = argv.index("-f")
        field, argv = argv[at + 1], argv[:at] + argv[at + 2:]
    top = None
    if "-t" in argv[:-1]:
        at = argv.index("-t")
        top, argv = argv[at + 1], argv[:at] + argv[at + 2:]
    keys = None
    if "-k" in argv[:-1]:
        at = argv.index("-k")
        keys, argv = argv[at + 1], argv[:at] + argv[at + 2:]
    agg = None
    if "-a" in argv[:-1]:
        at = argv.index("-a")
        agg, argv = argv[at + 1], argv[:at] + argv[at + 2:]
    agg_float = False
    if "-A" in argv[:-1] and agg is None:
        at = argv.index("-A")
        agg, agg_float, argv = argv[at + 1], True, argv[:at] + argv[at + 2:]
    time_format = width = None
    if "-T" in argv[:-1]:
        at = argv.index("-T")
        time_format, argv = os.fsencode(argv[at + 1]), argv[:at] + argv[at + 2:]
    if "-w" in argv[:-1]:
        at = argv.index("-w")
        width, argv = argv[at + 1], argv[:at] + argv[at + 2:]
    out_format = None
    if "-F" in argv[:-1]:
        at = argv.index("-F")
        out_format, argv = os.fsencode(argv[at + 1]), argv[:at] + argv[at + 2:]
    matches_out, unique, byte_order, device_zip, fold = "-o" in argv, "-u" in argv, "-b" in argv, "-Z" in argv, "-i" in argv
    device_text = "-D" in argv or device_zip
    argv = [a for a in argv if a not in ("-o", "-u", "-b", "-D", "-Z", "-i")]
    flags = [a for a in argv if a in ("-c", "-v", "-n", "-p")]
    rest = [a for a in argv if a not in ("-c", "-v", "-n", "-p")]
    if len(rest) != 2 or (field is not None and (not field.isdigit() or int(field) < 1)) or (top is not None and (not top.isdigit() or not unique)) or (
            unique and not matches_out and field is None) or (byte_order and not matches_out and field is None and "-p" not in flags) or (
            keys is not None and (repl is not None or top is not None or matches_out or unique or byte_order or agg is not None or fold)) or (
            agg is not None and (not agg.isdigit() or int(agg) < 1 or not unique or field is None or matches_out)) or (
            (time_format is None) != (width is None)) or (out_format is not None and time_format is None) or (time_format is not None and (
                not width.isdigit() or int(width) < 1 or field is None or matches_out or unique or byte_order or device_text or repl is not None
                or keys is not None or agg is not None or top is not None or "-n" in flags or "-c" in flags)):
        sys.stderr.write(__doc__)
        return 2
    path, pattern = rest
    invert, numbers = "-v" in flags, "-n" in flags and "-c" not in flags
    lines_out = "-p" in flags and "-c" not in flags and not numbers
    import numpy as np
    import torch

    import rejit_amd
    from rejit_amd import records

    if not torch.cuda.is_available():
        sys.stderr.write("linegrep_gpu: no GPU\n")
        return 2
    rejit_amd.build()
    data = np.fromfile(path, dtype=np.uint8)
    if data.size == 0:
        if not numbers and not lines_out and repl is None and not matches_out and field is None:
            print(0)
        return 1
    text = torch.from_numpy(data).to("cuda:0")                       # the only upload
    begins, ends = records.line_records(text)
    if data[-1] in (10, 13):                                         # `^` also matches behind the file's last line break: not a line
        begins, ends = begins[:-1].contiguous(), ends[:-1].contiguous()
    scan = rejit_amd.Scan(rejit_amd.Program(pattern))
    original = (text, begins, ends)
    if fold:                                                         # the lowered lines: a new device text, the same row numbers
        text, begins, ends = scan.translate_records(text, begins, ends, table=records.ASCII_LOWER, fill=10, lead=0, gap=1)
    result = scan.run_records(text, begins, ends)
    selected = result.n_records - result.n_matching if invert else result.n_matching
    if time_format is not None:
        every = not invert and "-p" not in flags
        lines = None if every else scan.select_records(invert=invert)
        counted = 0
        if every or selected:
            pb, pe, pf = scan.split_records(begins, ends, result, int(text.numel()), indices=lines, what="between")
            tb, te, _ = records.field_records(pb, pe, pf, int(field) - 1)     # (a missing field is an empty record: RJ_PARSE_EMPTY)
            try:
                values, status = scan.parse_time_records(text, tb, te, time_format, unit="s", trim=True)
            except rejit_amd.RejitError as err:
                sys.stderr.write("linegrep_gpu: -T: %s\n" % err.message)
                return 2
            start, ok = records.time_buckets(values, status, int(width))
            buckets, counts = torch.unique(start[ok], return_counts=True)     # ascending; the only downloads
            counted = int(buckets.numel())
            if out_format is not None and counted:
                try:
                    stamps = scan.format_time_records(buckets.contiguous(), out_format, unit="s")
                except rejit_amd.RejitError as err:
                    sys.stderr.write("linegrep_gpu: -F: %s\n" % err.message)
                    return 2
                printed, _, _ = scan.zip_records([scan.format_records(counts.contiguous()), stamps], sep=b" ", widths=[7, 0])
                sys.stdout.flush()
                sys.stdout.buffer.write(printed.cpu().numpy().tobytes())     # the only download
                return 0
            sys.stdout.write("".join("%7d %d\n" % (c, b) for b, c in zip(buckets.cpu().tolist(), counts.cpu().tolist())))
        return 0 if counted else 1
    if keys is not None:
        key_data = np.fromfile(keys, dtype=np.uint8)
        key_text = torch.from_numpy(key_data if key_data.size else np.zeros(1, dtype=np.uint8)).to("cuda:0")     # the second upload
        if key_data.size:
            kb, ke = records.line_records(key_text)
            if key_data[-1] in (10, 13):                             # (the empty record behind the last line break is not a key)
                kb, ke = kb[:-1].contiguous(), ke[:-1].contiguous()
        else:
            kb = ke = torch.empty(0, dtype=torch.int64, device="cuda:0")
        if field is None:
            rows, rb, re_ = scan.select_records(), begins, ends      # the lines with a match, looked up whole
        else:
            pb, pe, pf = scan.split_records(begins, ends, result, int(text.numel()), what="between")
            rb, re_, present = records.field_records(pb, pe, pf, int(field) - 1)
            rows = torch.nonzero(present).reshape(-1).contiguous()   # the lines that have a field N, looked up by it
        index = scan.lookup_records(key_text, kb, ke, text, rb, re_, indices=rows)
        lines = rows[index >= 0]
        if invert:
            keep = torch.ones(result.n_records, dtype=torch.bool, device="cuda:0")
            keep[lines] = False
            lines = torch.nonzero(keep).reshape(-1)
        lines = lines.contiguous()
        selected = int(lines.numel())
        if numbers and device_text:
            sys.stdout.flush()
            sys.stdout.buffer.write(scan.format_records(lines + 1)[0].cpu().numpy().tobytes())
        elif numbers:
            sys.stdout.write("".join("%d\n" % (i + 1) for i in lines.cpu().tolist()))
        elif lines_out:
            if selected:
                packed, _, _ = scan.pack_records(text, begins, ends, indices=lines, fill=10, lead=0, gap=1)
                sys.stdout.flush()
                sys.stdout.buffer.write(packed.cpu().numpy().tobytes())
        else:
            print(selected)
        return 0 if selected else 1
    if repl is not None:
        every = not invert and "-p" not in flags
        lines = None if every else scan.select_records(invert=invert)
        if every or selected:
            new, _, _ = scan.replace_records(text, begins, ends, result, repl, indices=lines, fill=10, lead=0, gap=1)
            if every and data[-1] not in (10, 13):                   # (sed adds no line break to a last line without one)
                new = new[:-1]
            sys.stdout.flush()
            sys.stdout.buffer.write(new.cpu().numpy().tobytes())     # the only download besides the summary
        return 0 if every or selected else 1
    if matches_out or field is not None:
        every = not invert and "-p" not in flags
        lines = None if every else scan.select_records(invert=invert)
        if every or selected:
            pb, pe, pf = scan.split_records(begins, ends, result, int(text.numel()), indices=lines, what="matches" if matches_out else "between")
            if matches_out:
                keep = records.nonempty_pieces(pb, pe)
            else:
                if agg is not None:
                    ab, ae, _ = records.field_records(pb, pe, pf, int(agg) - 1)      # (a missing field is an empty record: RJ_PARSE_EMPTY)
                pb, pe, _ = records.field_records(pb, pe, pf, int(field) - 1)
                keep = None
            if unique and (keep is None or keep.numel()):
                if byte_order:
                    rep, count, group = records.sorted_groups(scan, text, pb, pe, indices=keep)
                else:
                    group, rep, count = scan.group_records(text, pb, pe, indices=keep)
                sums = None
                if agg is not None:
                    values, status = scan.parse_records(text, ab, ae, kind="float64" if agg_float else "int64", trim=True, wide=agg_float)
                    sums = records.group_sums(group, values, status == rejit_amd.PARSE_OK, int(rep.numel()))
                if top is not None:
                    count, rep, order = records.top_groups(count, rep, int(top))
                    sums = None if sums is None else sums[order]
                if device_zip:                                          # the lines as one text: the only download
                    columns = [scan.format_records(count.to(torch.int64).contiguous()), (text, pb, pe, (rep if keep is None else keep[rep]).contiguous())]
                    if sums is not None:
                        columns.append(scan.format_records(sums.contiguous()))
                    zipped, _, _ = scan.zip_records(columns, sep=b" ", widths=[7] + [0] * (len(columns) - 1))
                    sys.stdout.flush()
                    sys.stdout.buffer.write(zipped.cpu().numpy().tobytes())
                    return 0 if selected or (every and field is not None) else 1
                packed, _, _ = scan.pack_records(text, pb, pe, indices=rep if keep is None else keep[rep], fill=10, lead=0, gap=1)
                words = packed.cpu().numpy().tobytes().split(b"\n")     # the dictionary and the counts: the only downloads
                sys.stdout.flush()
                if sums is not None and device_text:                    # the sums as one packed text: its lines are the third column
                    sum_words = scan.format_records(sums.contiguous())[0].cpu().numpy().tobytes().split(b"\n")
                    sys.stdout.buffer.write(b"".join(b"%7d %s %s\n" % (c, w, a) for c, w, a in zip(count.cpu().tolist(), words, sum_words)))
                elif sums is None:
                    sys.stdout.buffer.write(b"".join(b"%7d %s\n" % (c, w) for c, w in zip(count.cpu().tolist(), words)))
                elif agg_float:
                    sys.stdout.buffer.write(b"".join(b"%7d %s %s\n" % (c, w, repr(a).encode()) for c, w, a in zip(count.cpu().tolist(), words, sums.cpu().tolist())))
                else:
                    sys.stdout.buffer.write(b"".join(b"%7d %s %d\n" % (c, w, a) for c, w, a in zip(count.cpu().tolist(), words, sums.cpu().tolist())))
            elif keep is None or keep.numel():
                if byte_order:
                    order = scan.sort_records(text, pb, pe, indices=keep)
                    keep = order if keep is None else keep[order].contiguous()
                packed, _, _ = scan.pack_records(text, pb, pe, indices=keep, fill=10, lead=0, gap=1)
                sys.stdout.flush()
                sys.stdout.buffer.write(packed.cpu().numpy().tobytes())   # the only download besides the summary
        return 0 if selected or (every and field is not None) else 1
    if numbers and device_text:
        lines = scan.select_records(invert=invert)
        sys.stdout.flush()
        sys.stdout.buffer.write(scan.format_records(lines + 1)[0].cpu().numpy().tobytes())   # the only download besides the summary
    elif numbers:
        lines = scan.select_records(invert=invert)                   # the only download besides the summary
        sys.stdout.write("".join("%d\n" % (i + 1) for i in lines.cpu().tolist()))
    elif lines_out:
        if selected:
            lines = scan.select_records(invert=invert)
            if byte_order:
                lines = lines[scan.sort_records(text, begins, ends, indices=lines)].contiguous()
            else:
                text, begins, ends = original                        # (-i: the rows' numbers are the original table's)
            packed, _, _ = scan.pack_records(text, begins, ends, indices=lines, fill=10, lead=0, gap=1)
            sys.stdout.flush()
            sys.stdout.buffer.write(packed.cpu().numpy().tobytes())   # the only download besides the summary
    else:
        print(selected)
    return 0 if selected else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
