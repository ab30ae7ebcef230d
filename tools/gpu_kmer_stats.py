#!/usr/bin/env python3
"""What the per-k-mer model statistics cost, in ONE process on the GPU, from the library's profile (ps_prof):

    (a) k_kmer_stats for one region                          (`RegionBatch.KmerStats(realign=False)` over one resident handle)
    (b) k_kmer_stats for a lock-step batch of `--regions`    (one launch over all regions)
    (c) k_align_stats on the same batch, in the same run     (the reduction that reads the same refs: 16 B / level against 24)

    python3 tools/gpu_kmer_stats.py [--regions 20] [--length 10000] [--events 10] [--repeat 5]

Synthetic regions with their drafts' alignments, grouped by strand (two groups).  Every route is warmed up and then run `--repeat`
times under the profile; the kernel time is the mean per launch.  `stream_fraction` is the 24 B / level the definition reads, over
the kernel time and the device's peak memory bandwidth (--peak, GB/s) — the kernel stages every level once per k-mer block and is
bound by its serial walk, not by that stream; the number says how far.  Prints one JSON line per route."""
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
rb = RegionBatch(pas)
rb.load()
everything = list(range(args.regions))
routes = (("kmer_stats, one region", "kmer_stats", [0], lambda: rb.KmerStats([0], realign=False)),
          ("kmer_stats, batch", "kmer_stats", everything, lambda: rb.KmerStats(realign=False)),
          ("align_stats, batch", "align_stats", everything, lambda: rb.AlignStats(realign=False)))
for name, cls, idx, call in routes:
    call()
    t0 = time.time()
    call()
    wall = time.time() - t0
    api.prof_enable(1)
    api.prof_reset()
    for _ in range(args.repeat):
        call()
    ms, launches, alg_bytes = api.prof_get(cls)
    api.prof_enable(0)
    levels = sum(ev.mean.size for i in idx for ev in pas[i].events)
    per = ms / max(launches, 1)
    out = dict(route=name, regions=len(idx), events=sum(len(pas[i].events) for i in idx), levels=levels, launches=launches, kernel_ms=per,
               wall_ms=1e3 * wall, alg_bytes_per_launch=alg_bytes / max(launches, 1), tile=_capi.KMER_TILE, kmer_blocks=4, groups=2)
    if cls == "kmer_stats" and per > 0:
        out["stream_fraction"] = 24.0 * levels / (per * 1e-3) / (args.peak * 1e9)
    print(json.dumps(out), flush=True)
rb.drop()
rb.close()
