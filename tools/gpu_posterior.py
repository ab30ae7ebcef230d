#!/usr/bin/env python3
"""What the sum-product fill of the bands costs, in ONE process on the GPU, from the library's profile (ps_prof: HIP event pairs
around every launch):

    (a) `RegionBatch.PosteriorStats()`               (ps_batch_posterior_stats: k_post_fwd, k_post_bwd)
    (b) `RegionBatch.PosteriorStats(levels=True)`    (the same with the per-level emit / col arrays written and copied back)
    (c) `RegionBatch.ScoreEvents()` on k_fill        (the max-plus forward fill of the same bands, same run: the same cells)

    python3 tools/gpu_posterior.py [--regions 20] [--length 10000] [--events 10] [--repeat 3]

for one region and for a lock-step batch of `--regions`, synthetic reads on their drafts' alignments.  Every route is warmed up,
timed by the wall clock and then run `--repeat` times under the profile; kernel times are means per launch.  The band cells are
the records' own n_cells.  Prints one JSON line per (batch size, route), with ns per band cell and, for (a), the ratio to k_fill.
The static instruction counts per cell come from the ISA: tools/isa_sweep_count.py on ps_post.hip's assembly (k_post_fwd /
k_post_bwd: one barrier per loop body, one cell per lane and step)."""
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
ap.add_argument("--repeat", type=int, default=3)
args = ap.parse_args()

api = _capi.load_hip()
api.set_sweep_min(1 << 30)      # forward-only batches of every size on k_fill: the fill that covers the same cells in the same layout
P = dict(DEFAULT_PARAMS, verbose=0)


def make_pa(seq, events):
    pa = PSAlign()
    pa.sequence, pa.events, pa.params = seq, events, dict(P)
    return pa


def profiled(call, names):
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
    got = {n: api.prof_get(n) for n in names}
    api.prof_enable(0)
    return sorted(walls), {n: (ms / max(k, 1), k) for n, (ms, k, _) in got.items()}


all_pas = [make_pa(*synth.make_region(args.length, args.events, 9100 + k, swalign, P)[:2]) for k in range(args.regions)]
for count in sorted({1, args.regions}):
    pas = all_pas[:count]
    rb = RegionBatch(pas)
    rb.load()
    cells = sum(int(r["n_cells"].sum()) for r in rb.PosteriorStats())
    base = dict(regions=count, events=sum(len(pa.events) for pa in pas), levels=sum(ev.mean.size for pa in pas for ev in pa.events), band_cells=cells)
    walls, k = profiled(rb.ScoreEvents, ("fill",))
    fill_ms = k["fill"][0]
    print(json.dumps(dict(base, route="ScoreEvents (k_fill)", wall_ms=walls, fill_ms=fill_ms, fill_launches=k["fill"][1],
                          fill_ns_per_cell=1e6 * fill_ms / cells)), flush=True)
    for name, call in (("PosteriorStats", rb.PosteriorStats), ("PosteriorStats(levels=True)", lambda: rb.PosteriorStats(levels=True))):
        walls, k = profiled(call, ("post_fwd", "post_bwd"))
        fwd, bwd = k["post_fwd"][0], k["post_bwd"][0]
        print(json.dumps(dict(base, route=name, wall_ms=walls, post_fwd_ms=fwd, post_bwd_ms=bwd, launches=[k["post_fwd"][1], k["post_bwd"][1]],
                              fwd_ns_per_cell=1e6 * fwd / cells, bwd_ns_per_cell=1e6 * bwd / cells,
                              fwd_over_fill=fwd / fill_ms if fill_ms else None, bwd_over_fill=bwd / fill_ms if fill_ms else None)), flush=True)
    rb.drop()
    rb.close()
