#!/usr/bin/env python3
"""`variant -a` / consensus qualities for R regions, timed three ways in ONE process on the GPU:

    (a) a loop of `PSAlign.ScorePoints()` over the regions (the scored list exported as string pools, one MutationScore per edit)
    (b) one `RegionBatch.PointTable(table=True)` over the regions' resident AlignData (ps_batch_point_table, k_point_table)
    (c) the same with table=False (the 16-byte records only)

    python3 tools/gpu_point_table.py [--length 10000] [--events 10] [--regions 1,20] [--repeats 3]

For every R all routes are warmed up once, then alternated; every route ends synchronised (each returns host data), and (b) must
hold (a)'s scores exactly.  A last, untimed pass of (b) under the library's profile gives the kernel time by class.  Prints one JSON
line per R.  (a) uses nothing this tool's commit added, so it runs the same way on the parent commit (--loop-only)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from poreseq_amd import _capi, synth  # noqa: E402
from poreseq_amd.batch import RegionBatch  # noqa: E402
from poreseq_amd.poreseqcpp import PSAlign, swalign  # noqa: E402
from poreseq_amd.util import DEFAULT_PARAMS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--events", type=int, default=10)
ap.add_argument("--regions", default="1,20")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--loop-only", action="store_true")
args = ap.parse_args()

api = _capi.load_hip()
P = dict(DEFAULT_PARAMS, verbose=0)
counts = [int(v) for v in args.regions.split(",")]
pas = []
for k in range(max(counts)):
    pa = PSAlign()
    pa.sequence, pa.events, _ = synth.make_region(args.length, args.events, 1002 + k, swalign, P)
    pa.params = dict(P)
    pas.append(pa)


def timed(fn, *a):
    t = time.perf_counter()
    out = fn(*a)
    return time.perf_counter() - t, out


def loop(regs):
    return [pa.ScorePoints() for pa in regs]


for R in counts:
    regs = pas[:R]
    _, la = timed(loop, regs)
    if args.loop_only:
        ta = [timed(loop, regs)[0] for _ in range(args.repeats)]
        print(json.dumps({"regions": R, "length": args.length, "events": args.events, "loop_s": [round(t, 4) for t in ta]}), flush=True)
        continue
    rb = RegionBatch(regs).load()
    _, full = timed(rb.PointTable)
    _, lean = timed(rb.PointTable, None, False)
    for ms, (table, margin, slot, npos), (_, m2, s2, n2) in zip(la, full, lean):
        assert np.array_equal(table[~np.isnan(table)], np.array([m.score for m in ms])), "the two routes disagree"
        assert np.array_equal(margin, m2) and np.array_equal(slot, s2) and np.array_equal(npos, n2)
    del la
    ta, tb, tc = [], [], []
    for _ in range(args.repeats):
        ta.append(timed(loop, regs)[0])
        tb.append(timed(rb.PointTable)[0])
        tc.append(timed(rb.PointTable, None, False)[0])
    api.prof_enable(1)
    api.prof_reset()
    rb.PointTable()
    prof = {k: api.prof_get(k) for k in ("fill", "sweep", "score", "point_table", "slab")}
    api.prof_enable(0)
    rb.drop()
    rb.close()
    npos_tot = sum(len(pa.sequence) - 4 for pa in regs)
    print(json.dumps({"regions": R, "length": args.length, "events": args.events,
                      "loop_s": [round(t, 4) for t in ta], "table_s": [round(t, 4) for t in tb], "records_s": [round(t, 4) for t in tc],
                      "batched_below_loop": max(tb) < min(ta), "batched_not_above_loop_slowest": max(tb) <= max(ta),
                      "kernel_ms": {k: round(prof[k][0], 2) for k in ("fill", "sweep", "score", "point_table")},
                      "point_table_launches": prof["point_table"][1], "point_table_alg_bytes": prof["point_table"][2],
                      "dense_calls": prof["slab"][1],
                      "bytes_back_table": 88 * npos_tot, "bytes_back_records": 16 * npos_tot}), flush=True)
