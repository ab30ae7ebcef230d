#!/usr/bin/env python3
"""What phasing costs behind the genotype call, on one region, in ONE process on the GPU:

    (a) `RegionBatch.ScoreMutationGenotypes(sites, alt_frac=(0.5,))`   (ps_batch_score_mutation_genotypes: k_support + k_genotype)
    (b) `RegionBatch.ScoreMutationPhase(sites, window=W)`              (ps_batch_score_mutation_phase: k_link + k_phase + k_haptag)

    python3 tools/gpu_phase.py [--length 10000] [--events 10] [--sites 64,0] [--windows 2,8] [--repeats 3]

`--sites N` takes N point edits spread evenly over the region's point list, 0 the whole list (where the serial scan of k_phase is
longest).  Both routes are warmed up once, then alternated — (b) is the second call of `variant_support(phase=True)`, (a) the one it
follows; (b) must hold (a)'s scores exactly.  A last, untimed pass of each under the library's profile gives the kernel time by
class.  Prints one JSON line per (sites, window)."""
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
ap.add_argument("--sites", default="64,0")
ap.add_argument("--windows", default="2,8")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

api = _capi.load_hip()
P = dict(DEFAULT_PARAMS, verbose=0)
pa = PSAlign()
pa.sequence, pa.events, _ = synth.make_region(args.length, args.events, 1002, swalign, P)
pa.params = dict(P)


def point_list(seq):
    out = []
    for i in range(max(len(seq) - 4, 0)):
        for orig, mut in [(seq[i], "")] + [(seq[i], b) for b in "ACGT" if b != seq[i]] + [("", b) for b in "ACGT"]:
            m = MutationInfo()
            m.start, m.orig, m.mut = i, orig, mut
            out.append(m)
    return out


def timed(fn, *a, **kw):
    t = time.perf_counter()
    out = fn(*a, **kw)
    return time.perf_counter() - t, out


points = point_list(pa.sequence)
for n in [int(v) for v in args.sites.split(",")]:
    sites = points if n == 0 else [points[int(k * len(points) / n)] for k in range(n)]
    for W in [int(v) for v in args.windows.split(",")]:
        rb = RegionBatch([pa], resident=False)
        _, a = timed(rb.ScoreMutationGenotypes, [sites], alt_frac=(0.5,))
        _, b = timed(rb.ScoreMutationPhase, [sites], window=W)
        assert a[0][0].tobytes() == b[0][0].tobytes(), "the two routes disagree"
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(timed(rb.ScoreMutationGenotypes, [sites], alt_frac=(0.5,))[0])
            tb.append(timed(rb.ScoreMutationPhase, [sites], window=W)[0])
        api.prof_enable(1)
        api.prof_reset()
        rb.ScoreMutationGenotypes([sites], alt_frac=(0.5,))
        rb.ScoreMutationPhase([sites], window=W)
        prof = {k: api.prof_get(k) for k in ("fill", "sweep", "score", "support", "genotype", "link", "phase", "haptag")}
        api.prof_enable(0)
        rb.close()
        M = len(sites)
        print(json.dumps({"sites": M, "window": W, "length": args.length, "events": args.events, "n_sets": b[0][4],
                          "genotypes_s": [round(t, 4) for t in ta], "phase_s": [round(t, 4) for t in tb],
                          "kernel_ms": {k: round(prof[k][0], 4) for k in prof},
                          "launches": {k: prof[k][1] for k in ("link", "phase", "haptag")},
                          "alg_bytes": {k: prof[k][2] for k in ("link", "phase", "haptag")},
                          "bytes_back_phase": (8 + 32 * W + 16) * M + 24 * 4 * args.events + 8}), flush=True)
