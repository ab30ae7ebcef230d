#!/usr/bin/env python3
"""What counting the backtrace's moves costs, in ONE process on the GPU, from the library's profile (ps_prof):

    (a) `RegionBatch.ScoreEvents()`                  (ps_batch_score_alignments: the chain the others add to)
    (b) `RegionBatch.MoveStats()`                    (ps_batch_move_stats: the same chain with k_move_stats behind the walk)
    (c) `RegionBatch.MoveStats(levels=True)`         (the same with the per-level step codes and columns written and copied back)
    (d) `RegionBatch.AlignStats(realign=False)`      (k_align_stats on the same batch, in the same run: 16 B / level against 8)

    python3 tools/gpu_move_stats.py [--regions 20] [--length 10000] [--events 10] [--repeat 5]

Synthetic regions with their drafts' alignments on one resident lock-step batch.  Every route is warmed up, timed once by the
wall clock and then run `--repeat` times under the profile; the kernel time is the mean per launch.  `stream_fraction` is the
8 B / level the kernel reads (13 with the per-level arrays written) over the kernel time and the device's peak memory bandwidth
(--peak, GB/s).  Prints one JSON line per route."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poreseq_amd import _capi, synth  # noqa: E402
from poreseq_amd.batch import RegionBatch  # noqa: E402
from poreseq_amd.poreseqcpp import PSAlign, swalign  # noqa: E402
from poreseq_amd.util import DEFAULT_PARAMS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--regions", type=int, default=20)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--events", type=int, default=10)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--peak", type=float, default=8000.0, help="peak memory bandwidth in GB/s for stream_fraction")
args = ap.parse_args()

api = _capi.load_hip()
P = dict(DEFAULT_PARAMS, verbose=0)


def make_pa(seq, events):
    pa = PSAlign()
    pa.sequence, pa.events, pa.params = seq, events, dict(P)
    return pa


pas = [make_pa(*synth.make_region(args.length, args.events, 9100 + k, swalign, P)[:2]) for k in range(args.regions)]
levels = sum(ev.mean.size for pa in pas for ev in pa.events)
rb = RegionBatch(pas)
rb.load()
routes = (("ScoreEvents", None, 0.0, rb.ScoreEvents),
          ("MoveStats", "move_stats", 8.0, rb.MoveStats),
          ("MoveStats(levels=True)", "move_stats", 13.0, lambda: rb.MoveStats(levels=True)),
          ("AlignStats(realign=False)", "align_stats", 16.0, lambda: rb.AlignStats(realign=False)))
for name, cls, per_level, call in routes:
    call()
    walls = []
    for _ in range(args.repeat):
        t0 = time.time()
        call()
        walls.append(1e3 * (time.time() - t0))
    api.prof_enable(1)
    api.prof_reset()
    for _ in range(args.repeat):
        call()
    ms, launches, alg_bytes = api.prof_get(cls) if cls else (0.0, 0, 0.0)
    fill_ms = api.prof_get("fill")[0] + api.prof_get("sweep")[0]
    api.prof_enable(0)
    per = ms / max(launches, 1)
    out = dict(route=name, regions=args.regions, events=sum(len(pa.events) for pa in pas), levels=levels, launches=launches, kernel_ms=per,
               wall_ms=sorted(walls), fill_ms_per_call=fill_ms / args.repeat, alg_bytes_per_launch=alg_bytes / max(launches, 1))
    if cls and per > 0:
        out["stream_fraction"] = per_level * levels / (per * 1e-3) / (args.peak * 1e9)
    print(json.dumps(out), flush=True)
rb.drop()
rb.close()
