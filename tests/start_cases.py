"""Inputs of the `test` start-mode fixtures (tests/golden/test_start.json), rebuilt from seeds: used by the generator
(tests/golden/make_golden_test_start.py) and by the tests, which check the SHA-256 of what they rebuilt against the stored one."""
import hashlib

import numpy as np

from poreseq_amd import synth
from poreseq_amd.util import DEFAULT_PARAMS

P0 = dict(DEFAULT_PARAMS, verbose=0)

# name -> (length, events, region seed, cut seed or None)
SELECTION = {
    "whole_300": (300, 5, 4101, None), "whole_400": (400, 6, 4102, None), "whole_1000": (1000, 10, 4103, None),
    "cut_300": (300, 5, 4101, 51), "cut_400": (400, 6, 4102, 52), "cut_400b": (400, 7, 4104, 53), "cut_1000": (1000, 10, 4103, 54),
    "cut_1000b": (1000, 12, 4105, 55), "cut_1500": (1500, 10, 4106, 56), "tie_300": (300, 6, 4107, 58), "tie_400": (400, 7, 4108, 59),
}
TIES = ("tie_300", "tie_400")   # regions whose reads mostly carry one and the same sequence string (region(..., tie=True))
SCHEDULES = {
    "whole_1000": (1000, 10, 4103, None), "cut_1000": (1000, 10, 4103, 54), "cut_1500": (1500, 10, 4106, 56),
    "cut_400": (400, 6, 4102, 52),
}


def digest(s):
    return hashlib.sha256(s.encode("ascii")).hexdigest()


def region(length, n_events, seed, cut_seed, swalign, tie=False):
    """(draft, events): a synth.make_region region as it comes, or (cut_seed) with every read's sequence string cut to a random
    sub-range, one read's string copied over its neighbour's and the events shuffled.  tie: event 0 then gets the first half of
    event 1's string and every later event the whole of it, so all spans from event 1 on are equal"""
    draft, events, _ = synth.make_region(length, n_events, seed, swalign, P0)
    if cut_seed is not None:
        rng = np.random.default_rng(cut_seed)
        for ev in events:
            n = len(ev.sequence)
            a, b = int(rng.integers(0, n // 3)), int(rng.integers(2 * n // 3, n + 1))
            ev.sequence = ev.sequence[a:b]
        k = int(rng.integers(0, len(events) - 1))
        events[k + 1].sequence = events[k].sequence
        events = [events[int(k)] for k in rng.permutation(len(events))]
    if tie:
        s = events[1].sequence
        events[0].sequence = s[:len(s) // 2]
        for ev in events[2:]:
            ev.sequence = s
    return draft, events


def inputs_digest(draft, events):
    return digest(draft + "|" + "|".join(ev.sequence for ev in events))
