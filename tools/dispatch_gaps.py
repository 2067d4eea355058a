"""The gaps between consecutive dispatches of one kernel in a rocprofv3 results database (rocprofv3 --kernel-trace writes
<name>_results.db): from one dispatch's end to the next one's begin, for the launches of the steady loop (gaps beyond
--max-gap-us, the breaks between the loops of a run, are left out), as a whole and split by the dispatch's parity -- the
headline loop of bench.py alternates two objects, of which one carries the scan's start event.

usage: dispatch_gaps.py r_results.db [kernel-name substring] [--max-gap-us 50]"""
import sqlite3
import statistics
import sys


def gaps(path, needle="plane_count<rejit_amd::ExactShape<2>", max_gap_us=50.0):
    db = sqlite3.connect(path)
    cur = db.cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    cols = [r[1] for r in cur.execute(f"pragma table_info({ks})")]
    name_col = "display_name" if "display_name" in cols else "kernel_name"
    rows = cur.execute(f"select d.start, d.end from {kd} d join {ks} s on d.kernel_id = s.id where s.{name_col} like ? order by d.start",
                       ("%" + needle + "%",)).fetchall()
    out = []
    for k in range(1, len(rows)):
        g = (rows[k][0] - rows[k - 1][1]) / 1e3
        if g <= max_gap_us:
            out.append((k, g, (rows[k][1] - rows[k][0]) / 1e3))
    return len(rows), out


def line(label, v):
    if not v:
        return "%-28s none" % label
    v = sorted(v)
    return "%-28s n %6d  median %7.2f  mean %7.2f  p10 %7.2f  p90 %7.2f us" % (label, len(v), statistics.median(v), statistics.fmean(v), v[len(v) // 10], v[len(v) * 9 // 10])


def main(argv):
    path = argv[1]
    needle = argv[2] if len(argv) > 2 and not argv[2].startswith("--") else "plane_count<rejit_amd::ExactShape<2>"
    max_gap = float(argv[argv.index("--max-gap-us") + 1]) if "--max-gap-us" in argv else 50.0
    n, g = gaps(path, needle, max_gap)
    print("%s: %d dispatches of *%s*, %d gaps <= %.0f us" % (path, n, needle, len(g), max_gap))
    print(line("all gaps", [x[1] for x in g]))
    print(line("before even dispatches", [x[1] for x in g if x[0] % 2 == 0]))
    print(line("before odd dispatches", [x[1] for x in g if x[0] % 2 == 1]))
    print(line("kernel duration", [x[2] for x in g]))


if __name__ == "__main__":
    main(sys.argv)
