#!/usr/bin/env python3
"""`variant -v` for V candidate sequences of one region, timed two ways in ONE process on the GPU:

    (a) the reference's loop through existing entry points: per variant Copy(), RealignTo() (one `swalign`, numpy `mapaligns` per
        event) and ScoreEvents() (a fresh AlignData per call)
    (b) one `PSAlign.ScoreSequences` call (ps_score_sequences: batched Smith-Waterman in map form, k_remap, one chain of alignments)

    python3 tools/gpu_variant_seqs.py [--length 10000] [--events 10] [--variants 1,4,16,64] [--repeats 3]

For every V both are warmed up once, then alternated; both end synchronised (each returns host data) and must agree exactly.  A
last, untimed pass of (b) under the library's profile gives its kernel time by class, its Smith-Waterman launches and alignment
chunks, and the band counters say how many pairs ran banded / fell back.  Prints one JSON line per V.  (a) uses nothing this tool's
commit added, so it runs the same way on the parent commit (--loop-only)."""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from poreseq_amd import _capi, synth  # noqa: E402
from poreseq_amd.poreseqcpp import PSAlign, swalign  # noqa: E402
from poreseq_amd.util import DEFAULT_PARAMS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--events", type=int, default=10)
ap.add_argument("--variants", default="1,4,16,64")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--loop-only", action="store_true")
args = ap.parse_args()

api = _capi.load_hip()
P = dict(DEFAULT_PARAMS, verbose=0)
draft, events, truth = synth.make_region(args.length, args.events, 20, swalign, P)
pa = PSAlign()
pa.sequence, pa.events, pa.params = draft, events, dict(P)
rng = np.random.default_rng(21)


def variants(n):
    """haplotype-like candidates: the draft with ~0.5 % of SNVs and short indels, and every eighth one with a 30-base deletion"""
    out = []
    for k in range(n):
        s = synth.corrupt(rng, draft, 0.001, 0.003, 0.001)
        if k % 8 == 7:
            at = int(rng.integers(100, len(s) - 200))
            s = s[:at] + s[at + 30:]
        out.append(s)
    return out


def literal_loop(seqs):
    rows = []
    for s in seqs:
        pav = pa.Copy()
        pav.RealignTo(s)
        rows.append(pav.ScoreEvents())
    return rows


def timed(fn, *a):
    t = time.perf_counter()
    out = fn(*a)
    return time.perf_counter() - t, out


for V in [int(v) for v in args.variants.split(",")]:
    seqs = variants(V)
    _, ra = timed(literal_loop, seqs)
    if args.loop_only:
        ta = [timed(literal_loop, seqs)[0] for _ in range(args.repeats)]
        print(json.dumps({"variants": V, "length": len(draft), "events": len(events), "loop_s": [round(t, 4) for t in ta]}), flush=True)
        continue
    _, rb = timed(pa.ScoreSequences, seqs)
    assert rb.tolist() == ra, "the two routes disagree"
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(timed(literal_loop, seqs)[0])
        tb.append(timed(pa.ScoreSequences, seqs)[0])
    c0 = api.debug_sw_band()
    api.prof_enable(1)
    api.prof_reset()
    pa.ScoreSequences(seqs)
    prof = {k: api.prof_get(k) for k in ("sw", "sweep", "fill", "sw_map", "remap", "variant_chunks")}
    api.prof_enable(0)
    c1 = api.debug_sw_band()
    print(json.dumps({"variants": V, "length": len(draft), "events": len(events),
                      "loop_s": [round(t, 4) for t in ta], "batched_s": [round(t, 4) for t in tb],
                      "batched_below_loop": max(tb) < min(ta),
                      "kernel_ms": {k: round(prof[k][0], 2) for k in ("sw", "sweep", "fill")},
                      "sw_launches": prof["sw_map"][1], "remap_launches": prof["remap"][1], "chunks": prof["variant_chunks"][1],
                      "banded": c1["banded"] - c0["banded"], "fell_back": c1["fell_back"] - c0["fell_back"]}), flush=True)
