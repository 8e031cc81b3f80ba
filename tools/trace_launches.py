"""Per-kernel dispatch counts and per-stream dispatch order of a rocprofv3
kernel trace, in a form that two commits' runs can be diffed in.

usage: trace_launches.py <run_kernel_trace.csv> <counts.txt> <order.txt> [<skip prefix>]

counts.txt: one line per kernel name, "k<i> <count> <name>", sorted by name.
order.txt:  the kernels (as k<i>) of every stream in dispatch order, without the
kernels whose name starts with <skip prefix> (the runtime's own copy and fill
kernels, say).  A stream is a (launching thread, stream id) pair: the runtime
hands the id of a destroyed stream to the next one created, and ranks that
run as threads race for them.  For the same reason a stream is named by its
place among the streams ordered by content (s0, s1, ...), not by its id: the
same launches give the same file.
"""
import collections
import csv
import sys


def main(trace, counts_out, order_out, skip=None):
    rows = list(csv.DictReader(open(trace)))
    key = next((k for k in ("Stream_Id", "Queue_Id") if rows and k in rows[0]), None)
    if key is None:
        sys.exit("the trace names neither streams nor queues")
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    counts = collections.Counter(r["Kernel_Name"] for r in rows)
    with open(counts_out, "w") as f:
        for i, name in enumerate(sorted(counts)):
            f.write(f"k{i:02d} {counts[name]} {name}\n")
    short = {name: f"k{i:02d}" for i, name in enumerate(sorted(counts))}
    streams = collections.defaultdict(list)
    for r in rows:
        if not (skip and r["Kernel_Name"].startswith(skip)):
            streams[(r.get("Agent_Id", ""), r.get("Thread_Id", ""), r[key])].append(short[r["Kernel_Name"]])
    with open(order_out, "w") as f:
        for i, seq in enumerate(sorted(streams.values())):
            f.write(f"== s{i}: {len(seq)} dispatches\n")
            f.writelines(name + "\n" for name in seq)
    print(f"{len(rows)} dispatches of {len(counts)} kernels on {len(streams)} streams (by {key})")


if __name__ == "__main__":
    main(*sys.argv[1:5])
