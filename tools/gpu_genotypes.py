#!/usr/bin/env python3
"""What the genotype likelihoods cost on top of the support call, on one region's point-edit list, in ONE process on the GPU:

    (a) `RegionBatch.ScoreMutationSupport(None)`                          (ps_batch_score_mutation_support: k_support)
    (b) `RegionBatch.ScoreMutationGenotypes(None, alt_frac=K fractions)`   (ps_batch_score_mutation_genotypes: k_support + k_genotype)

    python3 tools/gpu_genotypes.py [--length 10000] [--events 10] [--fractions 1,8] [--repeats 3]

Both routes are warmed up once, then alternated; (b) must hold (a)'s scores and records exactly.  A last, untimed pass of (b) under
the library's profile gives the kernel time by class.  Prints one JSON line per K."""
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
ap.add_argument("--fractions", default="1,8")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

api = _capi.load_hip()
P = dict(DEFAULT_PARAMS, verbose=0)
pa = PSAlign()
pa.sequence, pa.events, _ = synth.make_region(args.length, args.events, 1002, swalign, P)
pa.params = dict(P)


def timed(fn, *a, **kw):
    t = time.perf_counter()
    out = fn(*a, **kw)
    return time.perf_counter() - t, out


for K in [int(v) for v in args.fractions.split(",")]:
    fr = [(k + 1) / (K + 1) for k in range(K)]
    rb = RegionBatch([pa], resident=False)
    _, a = timed(rb.ScoreMutationSupport, None)
    _, b = timed(rb.ScoreMutationGenotypes, None, alt_frac=fr)
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[0][1].tobytes() == b[0][1].tobytes(), "the two routes disagree"
    assert np.array_equal(b[0][4], b[0][1]["cover"].sum(axis=1))
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(timed(rb.ScoreMutationSupport, None)[0])
        tb.append(timed(rb.ScoreMutationGenotypes, None, alt_frac=fr)[0])
    api.prof_enable(1)
    api.prof_reset()
    rb.ScoreMutationGenotypes(None, alt_frac=fr)
    prof = {k: api.prof_get(k) for k in ("fill", "sweep", "score", "support", "genotype")}
    api.prof_enable(0)
    rb.close()
    M = len(a[0][0])
    print(json.dumps({"fractions": K, "length": args.length, "events": args.events, "edits": M,
                      "support_s": [round(t, 4) for t in ta], "genotypes_s": [round(t, 4) for t in tb],
                      "kernel_ms": {k: round(prof[k][0], 3) for k in prof}, "genotype_launches": prof["genotype"][1],
                      "genotype_alg_bytes": prof["genotype"][2], "bytes_back_support": (8 + 24 * 2) * M,
                      "bytes_back_genotypes": (8 + 24 * 2 + 8 * (K + 1) + 4) * M}), flush=True)
