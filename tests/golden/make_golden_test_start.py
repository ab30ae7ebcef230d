#!/usr/bin/env python3
"""Golden vectors of the consensus driver's `test` start mode (poreseq/Mutate.py:59-68), build container only:

  selection  the statements of Mutate.py:60-65, read from /root/reference at generation time, compiled in memory and run as they
             stand with the reference build's swalign (oracle/_ref/libps_ref.so), on the regions of tests/start_cases.py
  schedules  the consensus schedule from that start (Mutate('self'), then {Mutate('viterbi'), Refine()}) through the reference
             C++ (RefPSAlign), srand(1): per call (name, bases changed, SHA-256 of the sequence), final digest and accuracy

Nothing of the reference is written anywhere; only seeds, digests and results are stored (tests/golden/test_start.json).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_test_start.py
"""
import copy
import json
import os
import sys
import types

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import backends as B  # noqa: E402
import start_cases as SC  # noqa: E402
from poreseq_amd import consensus  # noqa: E402

REF = os.environ.get("PORESEQ_REFERENCE", "/root/reference")


class Sliced(str):
    """a read's sequence string that notes the slice taken from it"""
    def __getitem__(self, sl):
        self.log.append((self.k, sl.start, sl.stop))
        return str.__getitem__(self, sl)


def reference_selection(draft, events):
    """Mutate.py:60-65 as it stands -> (sequence, event index, slice start, slice stop)"""
    lines = open(os.path.join(REF, "poreseq", "Mutate.py")).read().splitlines()[59:65]
    body = "\n".join(l[8:] for l in lines)
    log = []
    evs = []
    for k, ev in enumerate(events):
        s = Sliced(ev.sequence)
        s.k, s.log = k, log
        evs.append(types.SimpleNamespace(sequence=s))
    pa = types.SimpleNamespace(events=evs, sequence=None)
    env = {"pa": pa, "refseq": draft, "poreseqcpp": types.SimpleNamespace(swalign=B.ref_swalign)}
    exec(compile(body, "Mutate.py:60-65", "exec"), env)
    k, a, b = log[-1]
    assert str(pa.sequence) == events[k].sequence[a:b]
    return str(pa.sequence), k, a, b


def main():
    assert B.have_ref(), "build the reference shim first (make -C oracle)"
    out = {"selection": {}, "schedules": {}}
    for name, (length, ne, seed, cut) in SC.SELECTION.items():
        draft, events = SC.region(length, ne, seed, cut, B.ref_swalign, tie=name in SC.TIES)
        seq, k, a, b = reference_selection(draft, events)
        out["selection"][name] = {"inputs": SC.inputs_digest(draft, events), "event": k, "first": a, "last": b, "sequence": SC.digest(seq)}
        print(name, "event", k, "slice", a, b, flush=True)
    for name, (length, ne, seed, cut) in SC.SCHEDULES.items():
        draft, events = SC.region(length, ne, seed, cut, B.ref_swalign)
        start, k, _, _ = reference_selection(draft, events)
        pa = B.make_pa(B.RefPSAlign, draft, copy.deepcopy(events), SC.P0)
        log = []
        B.reset_rand()
        seq, acc = consensus.consensus_region(pa, test=True, log=log, verbose=-1)
        rec = {"inputs": SC.inputs_digest(draft, events), "event": k, "start": SC.digest(start), "start_len": len(start),
               "calls": [[c, int(n), SC.digest(s)] for c, n, s in log], "final": SC.digest(seq), "final_len": len(seq), "accuracy": acc}
        # the start the driver took is the reference's own statement of it
        assert (log[0][2] is not None) and rec["start"] == SC.digest(start)
        out["schedules"][name] = rec
        print(name, "event", k, "start", len(start), "calls", [(c, n) for c, n, _ in log], "final", len(seq), acc, flush=True)
    with open(os.path.join(HERE, "test_start.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote test_start.json")


if __name__ == "__main__":
    main()
