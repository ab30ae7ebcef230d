#!/usr/bin/env python3
"""Golden vectors of `poreseq variant -v` (poreseq/Variant.py:42-63), build container only:

  the statements of Variant.py:48-61, read from /root/reference at generation time, compiled in memory and run as they stand on a
  PSAlign served by the reference build (oracle/_ref/libps_ref.so, RefPSAlign), with stand-ins for the FASTA records, on the cases
  of tests/variant_cases.py: per variant the accuracy RealignTo saw, the E scores of ScoreEvents, the dscore and the printed line

Nothing of the reference is written anywhere; only digests and results are stored (tests/golden/variant_seqs.json; Python's JSON
round-trips doubles, so the numbers are exact).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_variant_seqs.py
"""
import copy
import io
import json
import os
import sys
import types

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import backends as B  # noqa: E402
import variant_cases as VC  # noqa: E402

REF = os.environ.get("PORESEQ_REFERENCE", "/root/reference")


class Logged(B.RefPSAlign):
    """RefPSAlign that notes what ScoreEvents returned (the copies made by Copy() share the class and so the log)"""
    log = []

    def ScoreEvents(self):
        r = B.RefPSAlign.ScoreEvents(self)
        Logged.log.append(list(r))
        return r


def reference_variant_loop(pa, vs):
    """Variant.py:48-61 as it stands -> ({id: dscore}, printed text, [scores of every ScoreEvents call])"""
    lines = open(os.path.join(REF, "poreseq", "Variant.py")).read().splitlines()[47:61]
    body = "\n".join(l[8:] for l in lines)
    variants = {vid: types.SimpleNamespace(id=vid, seq=s) for vid, s in vs}   # SeqIO.index: a mapping id -> record
    out = io.StringIO()
    env = {"pa": pa, "variants": variants, "np": np, "sys": types.SimpleNamespace(stdout=out, stderr=sys.stderr)}
    Logged.log = []
    exec(compile(body, "Variant.py:48-61", "exec"), env)
    return env["variantscores"], out.getvalue(), Logged.log


def main():
    assert B.have_ref(), "build the reference shim first (make -C oracle)"
    res = {}
    for name in VC.CASES:
        draft, events, p, vs = VC.case(name, B.ref_swalign)
        ids = [vid for vid, _ in vs]
        assert len(set(ids)) == len(ids)
        pa = B.make_pa(Logged, draft, copy.deepcopy(events), p)
        scores, text, log = reference_variant_loop(pa, vs)
        assert len(log) == len(vs) + 1 and list(scores) == ids            # the base call, then one per variant in order
        rec = {"inputs": VC.inputs_digest(draft, events, vs), "base": log[0], "variants": {}}
        printed = text.splitlines(keepends=True)
        for k, (vid, s) in enumerate(vs):
            rec["variants"][vid] = {"accuracy": B.ref_swalign(draft, s)[0], "scores": log[k + 1], "dscore": float(scores[vid]), "line": printed[k]}
            print(name, vid, len(s), rec["variants"][vid]["accuracy"], scores[vid], flush=True)
        # the AlignData the loop ran on is as it was
        assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))
        res[name] = rec
    with open(os.path.join(HERE, "variant_seqs.json"), "w") as f:
        json.dump(res, f, indent=1)
    print("wrote variant_seqs.json")


if __name__ == "__main__":
    main()
