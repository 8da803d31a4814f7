"""Per-kernel durations and inter-kernel idle time from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats -d OUT -- python3 bench.py --gpus 1 --steps 20 --warmup 3
    python3 tools/trace_gaps.py OUT [--min-count 500]

Reads every *kernel_trace.csv (--output-format csv) or *_results.db (the default rocpd database) under OUT.  Prints,
for each kernel that ran at least --min-count times (the rebuild passes of the timed loop; one-off setup launches drop
out), the median duration, and for each consecutive pair of such kernels on a queue the median idle time between the
end of the first and the start of the second.  Times in us.
"""
import argparse
import collections
import csv
import glob
import os
import re
import sqlite3
import statistics


def short(name):
    """Kernel name without namespace and argument list, template arguments kept."""
    name = re.sub(r"\(.*\)$", "", name.strip())
    name = re.sub(r"^(void )?(abz::)?", "", name)
    return name.replace("abz::", "")


def load(path):
    rows = []
    for f in sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r.get("Queue_Id", 0) or 0), int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                             short(r["Kernel_Name"])))
    for f in sorted(glob.glob(os.path.join(path, "**", "*_results.db"), recursive=True)):
        with sqlite3.connect(f) as db:
            for q, t0, t1, name in db.execute("select queue_id, start, end, name from kernels"):
                rows.append((int(q), int(t0), int(t1), short(name)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--min-count", type=int, default=500)
    a = ap.parse_args()
    rows = load(a.trace_dir)
    if not rows:
        raise SystemExit("no kernel trace under " + a.trace_dir)
    count = collections.Counter(r[3] for r in rows)
    keep = {k for k, n in count.items() if n >= a.min_count}
    dur = collections.defaultdict(list)
    gap = collections.defaultdict(list)
    byq = collections.defaultdict(list)
    for r in rows:
        byq[r[0]].append(r)
    for q in byq.values():
        q.sort(key=lambda r: r[1])
        for i, (_, t0, t1, k) in enumerate(q):
            if k in keep:
                dur[k].append((t1 - t0) / 1e3)
            if i and k in keep and q[i - 1][3] in keep:
                gap[(q[i - 1][3], k)].append((t0 - q[i - 1][2]) / 1e3)
    print("kernel durations (median us, launches)")
    for k in sorted(dur, key=lambda k: -statistics.median(dur[k])):
        print("  %9.2f  %6d  %s" % (statistics.median(dur[k]), len(dur[k]), k))
    print("idle between consecutive kernels (median us, pairs)")
    for (p, k) in sorted(gap, key=lambda pk: -len(gap[pk])):
        v = gap[(p, k)]
        if len(v) >= a.min_count:
            print("  %9.2f  %6d  %s -> %s" % (statistics.median(v), len(v), p, k))


if __name__ == "__main__":
    main()
