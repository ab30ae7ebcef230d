#!/usr/bin/env python3
"""Which launch chains shared a hardware queue?  Reads a kernel trace (Start / End / Queue_Id rows) and prints, per queue id, the
number of launches, the busy time and how many distinct launch chains interleave on it; then the distinct queue ids, how many chains
share one, and the mean kernels in flight (summed kernel time / traced time).

usage: queue_share.py <trace> [skip]
  trace  rocprofv3's kernel_trace.csv, or a compact trace (.csv or .csv.gz) with the columns queue, kernel, start ns, end ns,
         workgroups [, thread id [, stream id]] (tools/prof_bench.sh writes the first five)
  skip   fraction of the traced time to drop at the start (warm-up), default 0

A chain is one in-order stream of launches: the trace's stream id where it has one, else the launching host thread (the library
gives every host thread one stream).  A trace with neither can only be estimated: streams that share a queue multiply its launches,
so the chains of a queue are taken as its launches over the median launches of the queues that carry at least 1 % of all launches."""
import collections
import csv
import gzip
import sys


def read(path):
    """[(queue, chain or None, start, end, kernel)]"""
    op = gzip.open if path.endswith(".gz") else open
    rows = []
    with op(path, "rt") as f:
        first = f.readline()
        f.seek(0)
        if "Queue_Id" in first:
            for r in csv.DictReader(f):
                chain = r.get("Stream_Id") or r.get("Thread_Id") or None
                rows.append((r["Queue_Id"], chain, int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0]))
        else:
            for line in f:
                c = line.rstrip("\n").split(",")
                if len(c) < 5:
                    continue
                chain = (c[6] if len(c) > 6 and c[6] else c[5] if len(c) > 5 and c[5] else None)
                rows.append((c[0], chain, int(c[2]), int(c[3]), c[1]))
    return rows


def summarise(rows, skip=0.0):
    lo = min(r[2] for r in rows)
    hi = max(r[3] for r in rows)
    cut = lo + skip * (hi - lo)
    rows = [r for r in rows if r[2] >= cut]
    lo = min(r[2] for r in rows)
    have_chain = all(r[1] is not None for r in rows)
    q = collections.OrderedDict()
    for qid, chain, s, e, name in sorted(rows, key=lambda r: r[2]):
        d = q.setdefault(qid, {"n": 0, "busy": 0, "chains": collections.Counter(), "switch": 0, "last": None})
        d["n"] += 1
        d["busy"] += e - s
        if have_chain:
            d["chains"][chain] += 1
            if d["last"] is not None and d["last"] != chain:
                d["switch"] += 1
            d["last"] = chain
    total = sum(d["n"] for d in q.values())
    if not have_chain:
        big = sorted(d["n"] for d in q.values() if d["n"] >= 0.01 * total)
        med = big[(len(big) - 1) // 2] if big else 1
        for d in q.values():
            d["est"] = max(1, int(round(d["n"] / float(med)))) if d["n"] >= 0.01 * total else 1
    # a chain counts for a queue when it put at least 1 % of the queue's launches there (a few set-up launches do not make a sharer)
    for d in q.values():
        d["nchains"] = sum(1 for c in d["chains"].values() if c >= 0.01 * d["n"]) if have_chain else d["est"]
    return {"rows": len(rows), "wall": hi - lo, "sum": sum(r[3] - r[2] for r in rows), "queues": q, "have_chain": have_chain, "total": total}


def main(argv):
    rows = read(argv[1])
    S = summarise(rows, float(argv[2]) if len(argv) > 2 else 0.0)
    how = "by stream / thread id" if S["have_chain"] else "ESTIMATED from launch counts (the trace has no stream or thread ids)"
    print("%d launches over %.3f s; chains %s" % (S["rows"], S["wall"] / 1e9, how))
    print("%-8s %9s %10s %7s %9s" % ("queue", "launches", "busy ms", "chains", "switches"))
    for qid, d in sorted(S["queues"].items(), key=lambda kv: -kv[1]["n"]):
        print("%-8s %9d %10.1f %7d %9s" % (qid, d["n"], d["busy"] / 1e6, d["nchains"], d["switch"] if S["have_chain"] else "-"))
    work = [d for d in S["queues"].values() if d["n"] >= 0.01 * S["total"]]
    shared = [d for d in work if d["nchains"] > 1]
    print("distinct queue ids: %d (%d with at least 1 %% of the launches); queues that carry more than one chain: %d (%d chains on them); "
          "most chains on one queue: %d" % (len(S["queues"]), len(work), len(shared), sum(d["nchains"] for d in shared),
                                          max(d["nchains"] for d in S["queues"].values())))
    print("mean kernels in flight (summed kernel time / traced time): %.2f" % (S["sum"] / float(max(S["wall"], 1))))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv)
