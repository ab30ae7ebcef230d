#!/usr/bin/env python3
"""What the alignment census costs beside the alignment it reads, and what recalibration does to a synthetic consensus, in ONE process
on the GPU:

    (a) `RegionBatch.ScoreEvents()`                    (ps_batch_score_alignments: the fills and the backtraces)
    (b) `RegionBatch.AlignStats()`                     (ps_batch_align_stats: the same chain, then k_align_stats)
    (c) `RegionBatch.AlignStats(realign=False)`        (k_align_stats alone, over the refs the handles hold)

    python3 tools/gpu_align_stats.py [--regions 20] [--length 10000] [--events 10] [--consensus 1000]

over one resident lock-step batch.  Every route is warmed up, timed once on the wall clock and run once more under the library's
profile for the kernel time by class.  Then `consensus_region` with and without `recalibrate=True` on one region of `--consensus`
bases (0: skip), as it is and with every read's model distorted by a random (scale 0.93 .. 1.07, shift -2 .. 2): identity against the
truth.  Synthetic data only — what recalibration does on real reads is unmeasured.  Prints one JSON line per result."""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from poreseq_amd import _capi, synth  # noqa: E402
from poreseq_amd.batch import RegionBatch  # noqa: E402
from poreseq_amd.consensus import consensus_region  # noqa: E402
from poreseq_amd.poreseqcpp import PSAlign, swalign  # noqa: E402
from poreseq_amd.util import DEFAULT_PARAMS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--regions", type=int, default=20)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--events", type=int, default=10)
ap.add_argument("--consensus", type=int, default=1000)
args = ap.parse_args()

api = _capi.load_hip()
P = dict(DEFAULT_PARAMS, verbose=0)
CLASSES = ("fill", "sweep", "align_stats")


def make_pa(seq, events):
    pa = PSAlign()
    pa.sequence, pa.events, pa.params = seq, events, dict(P)
    return pa


pas = [make_pa(*synth.make_region(args.length, args.events, 9100 + k, swalign, P)[:2]) for k in range(args.regions)]
levels = sum(ev.mean.size for pa in pas for ev in pa.events)
rb = RegionBatch(pas)
rb.load()
routes = (("ScoreEvents", rb.ScoreEvents), ("AlignStats", rb.AlignStats), ("AlignStats(realign=False)", lambda: rb.AlignStats(realign=False)))
for _, call in routes:
    call()
for name, call in routes:
    t0 = time.time()
    call()
    wall = time.time() - t0
    api.prof_enable(1)
    api.prof_reset()
    call()
    prof = {k: dict(zip(("ms", "launches"), api.prof_get(k)[:2])) for k in CLASSES}
    api.prof_enable(0)
    print(json.dumps(dict(route=name, regions=args.regions, events=args.regions * args.events, levels=levels, wall_ms=1e3 * wall, kernels=prof)), flush=True)
rb.drop()
rb.close()

if args.consensus:
    rng = np.random.default_rng(77)
    draft, events, truth = synth.make_region(args.consensus, args.events, 9201, swalign, P)
    bent = copy.deepcopy(events)
    for ev in bent:
        a, b = rng.uniform(0.93, 1.07), rng.uniform(-2.0, 2.0)
        ev.model.level_mean = (ev.model.level_mean - b) / a
    for tag, evs in (("undistorted", events), ("distorted", bent)):
        for rec in (None, True):
            api.srand(1)
            log = []
            seq, _ = consensus_region(make_pa(draft, copy.deepcopy(evs)), reps=4, log=log, recalibrate=rec)
            print(json.dumps(dict(models=tag, recalibrate=bool(rec), identity_vs_truth=swalign(seq, truth)[0], draft_identity=swalign(draft, truth)[0],
                                  reads_recalibrated=log[0][1] if rec else 0, calls=len(log))), flush=True)
