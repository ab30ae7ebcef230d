#!/usr/bin/env python3
"""Golden vectors of partial-span reads (tests/tiled_cases.py), build container only: the outputs of the reference build
(oracle/_ref/libps_ref.so through RefPSAlign) on

  gap     (loader)     stored with its inputs
  single  (truncated)  stored with its inputs
  pinned  (truncated)  inputs regenerated from the seed by the tests and checked against a SHA-256 (golden_util.input_digest)

The stored cases keep their 1024-entry model tables as float16: their inputs ARE the crafted case with every model entry rounded
to float16 (tiled_cases.golden_inputs), so nothing is lost on the way back.  Outputs: tiled_cases.golden_outputs.
Nothing of the reference is written anywhere but its results.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tiled.py
"""
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import backends as B  # noqa: E402
import golden_util as G  # noqa: E402
import tiled_cases as TC  # noqa: E402


def main():
    assert B.have_ref(), "build the reference shim first (make -C oracle)"
    out = {}
    for name in TC.GOLDEN_CASES:
        draft, events, par = TC.golden_inputs(name)
        rec = {"params_keys": np.array(sorted(par)), "params_vals": np.array([par[k] for k in sorted(par)])}
        if name in TC.GOLDEN_STORED:
            rec["sequence"], rec["n_events"] = np.array(draft), np.array(len(events))
            for e, ev in enumerate(events):
                m = ev.model
                tables = np.array([m.level_mean, m.level_stdv, m.sd_mean, m.sd_stdv])
                assert np.array_equal(tables.astype(np.float16).astype(np.float64), tables)
                rec["ev%d_model" % e] = tables.astype(np.float16)
                rec["ev%d_trans" % e] = np.array([m.prob_skip, m.prob_stay, m.prob_extend, m.prob_insert])
                rec["ev%d_complement" % e] = np.array(m.complement)
                for k in ("mean", "stdv", "ref_align", "ref_like"):
                    rec["ev%d_%s" % (e, k)] = getattr(ev, k)
                rec["ev%d_sequence" % e] = np.array(ev.sequence)
        else:
            rec["input_sha256"] = np.array(G.input_digest(draft, events, ""))
        rec.update(TC.golden_outputs(B.RefPSAlign, name, draft, events, par))
        print(name, TC.GOLDEN_CASES[name], rec["nbases"].tolist(), flush=True)
        out.update({name + "/" + k: v for k, v in rec.items()})
    path = os.path.join(HERE, "tiled.npz")
    np.savez_compressed(path, **out)
    print("wrote tiled.npz,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
