"""Inputs of the `variant -v` fixtures (tests/golden/variant_seqs.json), rebuilt from seeds: used by the generator
(tests/golden/make_golden_variant_seqs.py) and by the tests, which check the SHA-256 of what they rebuilt against the stored one."""
import hashlib
import io
import json
import os

import numpy as np

from poreseq_amd import consensus, synth
from poreseq_amd.util import DEFAULT_PARAMS

# name -> (length, events, region seed, realign_width, variant seed)
CASES = {"L600": (600, 6, 5101, 40, 61), "L3000": (3000, 8, 5102, 300, 62), "L10000": (10000, 10, 5103, 300, 63)}
_B = "ACGT"


def params(name):
    return dict(DEFAULT_PARAMS, verbose=0, realign_width=float(CASES[name][3]))


def _snvs(rng, seq, rate):
    s = list(seq)
    for k in np.flatnonzero(rng.random(len(s)) < rate):
        s[k] = _B[(_B.index(s[k]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def variants(draft, truth, width, seed):
    """[(id, sequence)]: the kinds of candidate a `variant -v` run meets, and the ones that are hard for the re-mapping and the
    band-following fills: the first Smith-Waterman index of a clipped variant with an insertion is an interpolation point of
    PSEvent.mapaligns (EventData.py:250-253), and an indel longer than 2 * realign_width + 32 moves the band centre by more rows than
    a band holds between two adjacent columns"""
    rng = np.random.default_rng(seed)
    n = len(draft)
    big = 150 if width <= 40 else 700
    assert big > 2 * width + 32 and n > 3 * big
    mid = n // 2
    ins8 = synth.random_sequence(rng, 8)
    clip_a, clip_b = 7 + n // 50, n - 9 - n // 40
    out = [("draft", draft), ("truth", truth), ("snv", _snvs(rng, draft, 0.01)), ("indel1", synth.corrupt(rng, draft, 0.005, 0.0, 0.005)),
           ("clip_ins", draft[clip_a:mid] + ins8 + draft[mid:clip_b]),
           ("clip_del", draft[clip_a:mid] + draft[mid + 5:clip_b]),
           ("long_del", draft[:n // 3] + draft[n // 3 + big:]),
           ("long_ins", draft[:2 * n // 3] + synth.random_sequence(rng, big) + draft[2 * n // 3:]),
           ("diverged", synth.corrupt(rng, draft, 0.10, 0.10, 0.10))]
    out.append(("dup", out[2][1]))   # the same string twice: aligned and scored once, reported twice
    return out


def case(name, swalign):
    """(draft, events, params, [(id, sequence)])"""
    length, ne, seed, width, vseed = CASES[name]
    p = params(name)
    draft, events, truth = synth.make_region(length, ne, seed, swalign, p)
    return draft, events, p, variants(draft, truth, width, vseed)


def many_variants(draft, vs, n):
    """the sequences of `vs`, then haplotype-like candidates (the draft with ~1 % of edits) up to n in all: a call large enough to be cut into chunks"""
    rng = np.random.default_rng(811)
    out = [s for _, s in vs]
    while len(out) < n:
        out.append(synth.corrupt(rng, draft, 0.004, 0.004, 0.004))
    return out


def inputs_digest(draft, events, vs):
    h = hashlib.sha256()
    h.update(draft.encode("ascii"))
    for ev in events:
        h.update(b"|" + ev.sequence.encode("ascii"))
        for a in (ev.mean, ev.stdv, ev.ref_align):
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    for vid, s in vs:
        h.update(("|%s=%s" % (vid, s)).encode("ascii"))
    return h.hexdigest()


# the stored reference run (tests/golden/make_golden_variant_seqs.py) and the comparison every backend is held to
_GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variant_seqs.json")
GOLD = json.load(open(_GOLD_PATH)) if os.path.exists(_GOLD_PATH) else {}   # (absent only while the generator makes it)


def check_against_fixture(name, pa, vs, rows=None):
    """variant_sequences on `pa` equals the stored reference run: scores, printed lines and the E scores of every variant"""
    want = GOLD[name]
    out = io.StringIO()
    got = consensus.variant_sequences(pa, vs, out=out)
    assert list(got) == [vid for vid, _ in vs]
    for vid, _ in vs:
        assert got[vid] == want["variants"][vid]["dscore"], vid
    assert out.getvalue() == "".join(want["variants"][vid]["line"] for vid, _ in vs)
    rows = pa.ScoreSequences([s for _, s in vs]) if rows is None else rows
    assert rows.shape == (len(vs), len(pa.events)) and rows.dtype == np.float64
    for (vid, _), row in zip(vs, rows):
        assert row.tolist() == want["variants"][vid]["scores"], vid
    assert pa.ScoreEvents() == want["base"]
