#!/usr/bin/env python3
"""Start selection of the `test` mode (Mutate.py:59-65) for a lock-step batch, timed two ways in ONE process on the GPU:

    (a) one `swalign` per (read, draft) pair, as the only public route was before `swalign_summaries`
    (b) one `swalign_summaries` call over all pairs

    python3 tools/gpu_start_select.py [--regions 20] [--length 10000] [--events 10] [--repeats 3]

Both are warmed up once, then alternated; both end synchronised (each returns host data).  The picks must agree.  A last,
untimed pass of (b) under the library's profile says how many launch chains ("sw" launches: one per chunk and per fall-back
batch) it took, and the band counters how many pairs ran banded / fell back.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from poreseq_amd import _capi, consensus, synth  # noqa: E402
from poreseq_amd.poreseqcpp import swalign, swalign_summaries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--regions", type=int, default=20)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--events", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

api = _capi.load_hip()
rng = np.random.default_rng(20)
regions = []
for r in range(args.regions):          # reads and draft as synth.make_region corrupts them (no event levels needed here)
    truth = synth.random_sequence(rng, args.length)
    draft = synth.corrupt(rng, truth, 0.04, 0.04, 0.04)
    reads = [synth.corrupt(rng, truth, 0.05, 0.05, 0.05) for _ in range(args.events)]
    regions.append((draft, reads))


class Ev:
    def __init__(self, s):
        self.sequence = s


def by_swalign():
    picks = []
    for draft, reads in regions:
        seq = ""
        for s in reads:
            pairs = swalign(s, draft)[1]
            if pairs[-1][1] - pairs[0][1] > len(seq):
                seq = s[pairs[0][0]:pairs[-1][0]]
        picks.append(seq)
    return picks


def by_summaries():
    sums = swalign_summaries([(s, draft) for draft, reads in regions for s in reads])
    picks, k = [], 0
    for draft, reads in regions:
        picks.append(consensus.test_start([Ev(s) for s in reads], draft, sums[k:k + len(reads)])[0])
        k += len(reads)
    return picks


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


_, pa = timed(by_swalign)
_, pb = timed(by_summaries)
assert pa == pb, "the two routes picked different starts"
ta, tb = [], []
for _ in range(args.repeats):
    ta.append(timed(by_swalign)[0])
    tb.append(timed(by_summaries)[0])
c0 = api.debug_sw_band()
api.prof_enable(1)
api.prof_reset()
by_summaries()
ms, launches, _ = api.prof_get("sw")
api.prof_enable(0)
c1 = api.debug_sw_band()
print(json.dumps({"pairs": args.regions * args.events, "length": args.length, "swalign_loop_s": [round(t, 4) for t in ta],
                  "summaries_s": [round(t, 4) for t in tb], "sw_launches": launches, "sw_kernel_ms": round(ms, 2),
                  "banded": c1["banded"] - c0["banded"], "fell_back": c1["fell_back"] - c0["fell_back"],
                  "start_identity": [round(s.accuracy, 1) for s in swalign_summaries([(p, d) for p, (d, _) in zip(pb, regions)])][:5]}))
