"""The `test` start mode on the GPU: `ps_batch_sw_summary` (the summary build of the Smith-Waterman traceback, ps_sw.hip) against the
records derived from the library's own `ps_swfull` lists and from the oracle's, and the consensus drivers in that mode against the
stored reference schedules (tests/golden/test_start.json), the region-by-region runs and the oracle.  Tolerance 0 everywhere."""
import copy
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import backends as B
import start_cases as SC
from poreseq_amd import _capi, consensus, synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign, swalign, swalign_summaries

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(B.ROOT, "tests", "golden", "test_start.json")))
P = SC.P0


class _env:
    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in self.kv:
            os.environ.pop(k, None)


def _same(a, b):
    return tuple(a[:9]) == tuple(b[:9]) and (a.accuracy == b.accuracy or (math.isnan(a.accuracy) and math.isnan(b.accuracy)))


def _from_hip_lists(pairs):
    api = _capi.load_hip()
    return [_capi.summary_from_lists(a, b, *api.swfull(a, b)) for a, b in pairs]


def _check(got, pairs, with_oracle=True):
    assert len(got) == len(pairs)
    own = _from_hip_lists(pairs)
    orc = B.oracle_api().sw_summaries(pairs) if with_oracle else own
    for k, (g, o, c) in enumerate(zip(got, own, orc)):
        assert _same(g, o), (k, len(pairs[k][0]), len(pairs[k][1]), g, o)
        assert _same(g, c), (k, len(pairs[k][0]), len(pairs[k][1]), g, c)


def _short_pairs():
    rng = np.random.default_rng(515)
    base = synth.random_sequence(rng, 80)
    other = synth.corrupt(rng, base, 0.04, 0.04, 0.04) + synth.random_sequence(rng, 10)
    pairs = [(base[:n1], other[:n2]) for n1 in (0, 1, 63, 64, 65) for n2 in (0, 1, 63, 64, 65)]
    pairs.append(("AAAA" * 20, "CCCC" * 20))                               # no match: nothing scores above 0
    for _ in range(6):
        n = int(rng.integers(66, 3001))
        s = synth.random_sequence(rng, n)
        e = float(rng.uniform(0.0, 0.08))
        pairs.append((s, synth.corrupt(rng, s, e, e, e)))
    s = synth.random_sequence(rng, 2900)
    pairs += [(s[300:1500], s), (s, s[1000:2700]), (synth.random_sequence(rng, 1500), synth.random_sequence(rng, 1600))]
    return pairs


@pytest.mark.parametrize("cols,packed", [("4", None), ("8", None), ("8", "0")])
def test_summaries_of_short_and_ragged_pairs(cols, packed):
    """lengths around the 64-wide tiles, empty strings, a pair with no match, random lengths up to 3 kb: 4 columns per lane, 8 on the
    packed fill, 8 on the 32-bit fill"""
    pairs = _short_pairs()
    with _env(PORESEQ_SW_K=cols, PORESEQ_SW_PK=packed):
        got = _capi.load_hip().sw_summaries(pairs)
    _check(got, pairs)
    assert sum(1 for g in got if g.n_pairs == 0) >= 10


def _long_pairs():
    rng = np.random.default_rng(616)
    pairs = []
    for n, e in [(10000, 0.05), (9800, 0.05), (10000, 0.003), (10400, 0.004), (3000, 0.002), (2000, 0.06)]:
        s = synth.random_sequence(rng, n)
        pairs.append((synth.corrupt(rng, s, e, e, e), s))                  # read (or Viterbi-like seed) against draft
    s = synth.random_sequence(rng, 2500)                                   # these three cannot pass a 128-wide band's certificate
    pairs += [(s, s[:40] + s[290:]), (s[250:], s), (synth.random_sequence(rng, 120) + s, s + synth.random_sequence(rng, 120))]
    pairs.append((s[:700], s[:700]))
    return pairs


@pytest.mark.parametrize("band,width", [("off", None), ("auto", None), ("force", "128")])
def test_summaries_of_long_pairs_full_matrix_banded_and_fallen_back(band, width):
    pairs = _long_pairs()
    api = _capi.load_hip()
    with _env(PORESEQ_SW_BAND="off"):
        own = _from_hip_lists(pairs)
    with _env(PORESEQ_SW_BAND=band, PORESEQ_SW_BAND_W=width):
        c0 = api.debug_sw_band()
        got = api.sw_summaries(pairs)
        c1 = api.debug_sw_band()
    d = {k: c1[k] - c0[k] for k in c0}
    if band == "off":
        assert d["banded"] == 0
    elif band == "auto":
        assert 2 <= d["banded"] < len(pairs) and d["fell_back"] == 0       # the ~99 % pairs band, the ~85 % reads do not
    else:
        assert d["banded"] == len(pairs) and d["fell_back"] >= 3           # redone on the full matrix, in summary form
        assert d["fell_back"] < len(pairs)
    orc = B.oracle_api().sw_summaries(pairs)
    for k, (g, o, c) in enumerate(zip(got, own, orc)):
        assert _same(g, o) and _same(g, c), (k, g, o, c)


_CHUNK_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
from poreseq_amd import _capi, synth
api = _capi.load_hip()
api.set_device_fraction(0.1)          # the runtime's share drops to its floor: 250 MB of Smith-Waterman checkpoints per launch
rng = np.random.default_rng(717)
distinct = []
for _ in range(12):
    s = synth.random_sequence(rng, 10000)
    distinct.append((synth.corrupt(rng, s, 0.05, 0.05, 0.05), s))
pairs = distinct * 4
api.prof_enable(1)
api.prof_reset()
got = api.sw_summaries(pairs)
ms, launches, nbytes = api.prof_get("sw")
api.prof_enable(0)
print("RESULT " + json.dumps({"records": [list(g) for g in got], "launches": launches, "bytes": nbytes,
                              "cells5": sum(5.0 * len(a) * len(b) for a, b in pairs)}))
"""


def test_a_large_batch_is_cut_into_chunks_by_the_device_share():
    """48 pairs of 10 kb (12.6 MB of checkpoints each) under a tenth of the device: several launches, the same records; the "sw"
    profile class counts one launch per chunk and 5 bytes per cell, as for the list form.  A process of its own: the fraction is
    set before the first compute call, as ranks that share a GPU do."""
    code = _CHUNK_CHILD % {"root": B.ROOT, "tests": os.path.join(B.ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res["launches"] >= 3
    assert res["bytes"] == res["cells5"]
    rng = np.random.default_rng(717)
    distinct = []
    for _ in range(12):
        s = synth.random_sequence(rng, 10000)
        distinct.append((synth.corrupt(rng, s, 0.05, 0.05, 0.05), s))
    own = _from_hip_lists(distinct)
    got = [_capi.SwSummary(*g) for g in res["records"]]
    assert len(got) == 48
    for k, g in enumerate(got):
        assert _same(g, own[k % 12]), (k, g, own[k % 12])
    for k in (0, 5, 11):
        assert _same(got[k], B.oracle_api().sw_summaries([distinct[k]])[0])


def test_python_surface_on_the_gpu_dedups_and_keeps_order():
    pairs = _short_pairs()[20:30]
    many = pairs + pairs[::-1] + pairs[:3]
    got = swalign_summaries(many)
    want = _from_hip_lists(pairs)
    want = want + want[::-1] + want[:3]
    assert all(_same(g, w) for g, w in zip(got, want)) and len(got) == len(many)


# the four fill families of tests/conftest.py's `fwd_kernel`, for this module
_FILLS = {"sweep": 1, "sweep_w2": 2, "sweep_w4": 4, "fill": 0}


@pytest.fixture(params=list(_FILLS))
def fills(request):
    api = _capi.load_hip()
    nw = _FILLS[request.param]
    api.set_sweep_min(0 if nw else 1 << 30)
    api.set_sweep2_min(0 if nw else 1 << 30)
    api.set_sparse_min(0 if nw else 1 << 30)
    api.set_sweep_form(0, nw)
    yield request.param
    api.set_sweep_min(-1)
    api.set_sweep2_min(-1)
    api.set_sparse_min(-1)
    api.set_sweep_form(0, 0)


@pytest.mark.parametrize("name", sorted(SC.SCHEDULES))
def test_stored_schedules_replayed_on_the_gpu(name, fills):
    """band centres from a ref_align that belongs to another sequence, heavy edits: digest for digest with the reference C++"""
    draft, events = SC.region(*SC.SCHEDULES[name], B.oracle_swalign)
    want = GOLD["schedules"][name]
    assert SC.inputs_digest(draft, events) == want["inputs"]
    pa = B.make_pa(PSAlign, draft, copy.deepcopy(events), P)
    log = []
    B.reset_rand()
    seq, acc = consensus.consensus_region(pa, test=True, log=log, verbose=-1)
    got = [[c, int(n), SC.digest(s)] for c, n, s in log]
    for k, (g, w) in enumerate(zip(got, want["calls"])):
        assert g == w, (fills, k, g, w)
    assert len(got) == len(want["calls"])
    assert (SC.digest(seq), len(seq), acc) == (want["final"], want["final_len"], want["accuracy"])


def _cases():
    cases = [SC.region(*SC.SELECTION["cut_300"], B.oracle_swalign), SC.region(*SC.SELECTION["whole_300"], B.oracle_swalign)]
    d3, e3, _ = synth.make_region(220, 3, 4190, B.oracle_swalign, P)        # below the five-event threshold
    cases.insert(1, (d3, e3))
    cases.append(SC.region(260, 6, 4191, 57, B.oracle_swalign))
    cases.append(SC.region(*SC.SELECTION["cut_400b"], B.oracle_swalign))
    return cases


def _one_by_one(cls, api, cases):
    res, logs, accs = [], [], []
    for draft, events in cases:
        B.reset_rand()
        pa = B.make_pa(cls, draft, copy.deepcopy(events), P)
        log = []
        res.append(consensus.consensus_region(pa, test=True, log=log, verbose=-1))
        logs.append(log)
        accs.append([swalign(s, draft, api)[0] for c, _, s in log if c in ("Mutate:self", "Refine")])
    return res, logs, accs


_WANT = {}


@pytest.mark.parametrize("preloaded", [False, True])
def test_lock_step_in_test_mode_equals_region_by_region_and_the_oracle(preloaded):
    cases = _cases()
    if "want" not in _WANT:
        _WANT["want"] = _one_by_one(PSAlign, _capi.load_hip, cases)
        _WANT["oracle"] = _one_by_one(B.OraclePSAlign, B.oracle_api, cases)
    want = _WANT["want"]
    assert want == _WANT["oracle"]
    pas = [B.make_pa(PSAlign, d, copy.deepcopy(ev), P) for d, ev in cases]
    logs, accs = [[] for _ in cases], [[] for _ in cases]
    batch = RegionBatch(pas).load() if preloaded else None               # resident AlignData that still hold the loaded sequence
    got = consensus.consensus_regions(pas, test=True, logs=logs, accuracies=accs, batch=batch)
    assert (got, logs, accs) == want
    assert got[1] == (cases[1][0], 100)


def test_train_in_test_mode_lock_step_equals_replica_by_replica():
    draft, events, truth = synth.make_region(300, 5, 4195, B.oracle_swalign, P)

    def loader(cls):
        def make_pa(p):
            evs = copy.deepcopy(events)
            for e in evs:
                e.setparams(p)
            return B.make_pa(cls, draft, evs, p)
        return make_pa

    sets = [dict(P), dict(P, skip_t=0.6, skip_c=0.6, stay_t=0.5, stay_c=0.5), dict(P, insert_t=0.3, insert_c=0.3),
            dict(P, skip_t=0.2, skip_c=0.2)]
    best, accs = consensus.train(loader(PSAlign), P, truth, iters=1, reps=2, paramlists=[sets], lock_step=True, test=True)
    each = []
    for p in sets:
        B.reset_rand()
        each.append(consensus.consensus_region(loader(B.OraclePSAlign)(p), p, reps=2, refseq=truth, test=True, verbose=-1)[1])
    assert accs[0] == max(each) and best == sets[int(np.argmax(each))]
