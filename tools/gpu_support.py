#!/usr/bin/env python3
"""Per-edit read support of R regions' point-edit lists, timed two ways in ONE process on the GPU:

    (a) per region `PSAlign.ScorePoints()` plus `ScoreMutationDeltas` of the same list reduced on the host (`util.support_from_deltas`
        needs the events x edits matrix and the re-aligned refs: two scoring passes and E x M doubles copied back)
    (b) one `RegionBatch.ScoreMutationSupport(None)` over the regions (ps_batch_score_mutation_support, k_support)

    python3 tools/gpu_support.py [--length 10000] [--events 10] [--regions 1,8] [--repeats 3]

Both routes are warmed up once, then alternated; (b) must hold (a)'s scores and sums exactly.  A last, untimed pass of (b) under the
library's profile gives the kernel time by class.  Prints one JSON line per R."""
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
from poreseq_amd.util import DEFAULT_PARAMS, MutationInfo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--events", type=int, default=10)
ap.add_argument("--regions", default="1,8")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

api = _capi.load_hip()
P = dict(DEFAULT_PARAMS, verbose=0)
P["scoring_width"] = P["point_width"]     # (route (a) scores a given list: at scoring_width)
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


def host_route(regs):
    out = []
    for pa in regs:
        scored = pa.ScorePoints()
        muts = []
        for s in scored:
            mi = MutationInfo()
            mi.start, mi.orig, mi.mut = s.start, s.orig, s.mut
            muts.append(mi)
        deltas = pa.ScoreMutationDeltas(muts)
        grp = np.array([1 if ev.model.complement else 0 for ev in pa.events])
        sums = np.stack([np.add.reduce(deltas[grp == g], axis=0) if np.any(grp == g) else np.zeros(deltas.shape[1]) for g in (0, 1)], axis=1)
        out.append((np.array([s.score for s in scored]), sums))
    return out


for R in counts:
    regs = pas[:R]
    rb = RegionBatch(regs, resident=False)
    _, a = timed(host_route, regs)
    _, b = timed(rb.ScoreMutationSupport, None)
    for (sc, _sums), (sc2, sup, _l) in zip(a, b):
        assert np.array_equal(sc, sc2), "the two routes disagree"
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(timed(host_route, regs)[0])
        tb.append(timed(rb.ScoreMutationSupport, None)[0])
    api.prof_enable(1)
    api.prof_reset()
    rb.ScoreMutationSupport(None)
    prof = {k: api.prof_get(k) for k in ("fill", "sweep", "score", "support")}
    api.prof_enable(0)
    rb.close()
    M = sum(len(x[0]) for x in a)
    print(json.dumps({"regions": R, "length": args.length, "events": args.events, "edits": M,
                      "scores_plus_deltas_s": [round(t, 4) for t in ta], "support_s": [round(t, 4) for t in tb],
                      "kernel_ms": {k: round(prof[k][0], 3) for k in prof}, "support_launches": prof["support"][1],
                      "support_alg_bytes": prof["support"][2], "bytes_back_support": (8 + 24 * 2) * M,
                      "bytes_back_deltas": 8 * args.events * M}), flush=True)
