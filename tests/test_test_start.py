"""The consensus driver's `test` start mode (poreseq/Mutate.py:59-68) on the CPU checkers: the start selection restated on
Smith-Waterman summaries against the reference's own statements (tests/golden/test_start.json, made by
tests/golden/make_golden_test_start.py), the schedule from that start call for call, the lock-step driver and `train` in that mode,
and the summary records a checker library serves from `swfull` when it lacks `ps_batch_sw_summary`.  All comparisons are exact.
"""
import copy
import ctypes
import json
import math
import os

import numpy as np
import pytest

import backends as B
import start_cases as SC
from poreseq_amd import _capi, consensus, synth
from poreseq_amd.poreseqcpp import swalign, swalign_summaries

GOLD = json.load(open(os.path.join(B.ROOT, "tests", "golden", "test_start.json")))
P = SC.P0


def _same_float(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _records_from_lists(s1, s2, score, acc, i1, i2):
    """the summary of one pair, written out from swfull's lists (the table of include/poreseq_hip.h)"""
    pairs = list(zip(i1.tolist(), i2.tolist()))
    if not pairs:
        return (score, 0, 0, 0, 0, 0, 0, 0, 0)
    nm = sum(1 for a, b in pairs if a > 0 and b > 0 and s1[a - 1] == s2[b - 1])
    return (score, len(pairs), nm, pairs[0][0], pairs[0][1], pairs[-1][0], pairs[-1][1],
            sum(1 for a, _ in pairs if a == 0), sum(1 for _, b in pairs if b == 0))


def _sw_pairs():
    rng = np.random.default_rng(99)
    s = synth.random_sequence(rng, 700)
    return [("", "ACGT"), ("ACGT", ""), ("", ""), ("AAAA", "CCCC"), ("A", "A"), ("ACGTACGT", "ACGTACGT"),
            (s, synth.corrupt(rng, s, 0.05, 0.05, 0.05)), (s[100:400], s), (s, s[200:650]),
            (synth.random_sequence(rng, 90), synth.random_sequence(rng, 120))]


def test_an_oracle_library_without_the_summary_symbol_still_loads():
    api = B.oracle_api()
    assert "ps_batch_sw_summary" in api.missing and api.missing <= _capi.OPTIONAL
    assert "ps_batch_sw_summary" in _capi.SYMBOLS
    assert hasattr(ctypes.CDLL(_capi.HIP_LIB), "ps_batch_sw_summary")      # the product exports it
    assert _capi.load_hip().missing == set()


def test_summary_fallback_equals_the_lists_it_is_derived_from():
    api = B.oracle_api()
    pairs = _sw_pairs()
    got = swalign_summaries(pairs, B.oracle_api)
    assert len(got) == len(pairs)
    empty = 0
    for (s1, s2), g in zip(pairs, got):
        score, acc, i1, i2 = api.swfull(s1, s2)
        assert tuple(g[:9]) == _records_from_lists(s1, s2, score, acc, i1, i2)
        assert _same_float(g.accuracy, acc)
        if g.n_pairs:
            assert g.accuracy == 100.0 * g.n_match / float(g.n_pairs)
        else:
            empty += 1
            assert math.isnan(g.accuracy)
    assert empty >= 4                                                       # the empty strings and the pair with no positive score


def test_identical_pairs_are_aligned_once():
    calls = []

    class Counting:
        def sw_summaries(self, pairs):
            calls.append(list(pairs))
            return B.oracle_api().sw_summaries(pairs)

    pairs = [("ACGTTGCA", "ACGTGCA"), ("ACGT", "ACGT"), ("ACGTTGCA", "ACGTGCA"), ("ACGT", "ACGT"), ("ACGT", "ACGA")]
    got = swalign_summaries(pairs, Counting)
    assert len(calls) == 1 and len(calls[0]) == 3
    assert got == B.oracle_api().sw_summaries(pairs)


@pytest.mark.parametrize("name", sorted(SC.SELECTION))
def test_start_selection_equals_the_reference_statements(name):
    draft, events = SC.region(*SC.SELECTION[name], B.oracle_swalign, tie=name in SC.TIES)
    want = GOLD["selection"][name]
    assert SC.inputs_digest(draft, events) == want["inputs"]
    sums = swalign_summaries([(ev.sequence, draft) for ev in events], B.oracle_api)
    seq, k = consensus.test_start(events, draft, sums)
    assert k == want["event"]
    assert seq == events[k].sequence[want["first"]:want["last"]]
    assert (sums[k].first1, sums[k].last1) == (want["first"], want["last"])
    assert SC.digest(seq) == want["sequence"]


def test_selection_vectors_cover_the_quirks():
    """a winner that is not event 0, a tie the first of equals wins, and a slice whose off-by-one shows"""
    assert any(v["event"] != 0 for v in GOLD["selection"].values())
    for name in SC.TIES:
        draft, events = SC.region(*SC.SELECTION[name], B.oracle_swalign, tie=True)
        k = GOLD["selection"][name]["event"]
        assert k >= 1 and sum(ev.sequence == events[k].sequence for ev in events) >= 3      # the winner's span is shared by other events
    assert all(v["first"] >= 1 for v in GOLD["selection"].values())         # 1-based index as a 0-based bound: a base is dropped


def test_start_of_an_empty_alignment_raises_like_the_reference():
    draft, events = SC.region(*SC.SELECTION["whole_300"], B.oracle_swalign)
    events[2].sequence = ""
    sums = swalign_summaries([(ev.sequence, draft) for ev in events], B.oracle_api)
    with pytest.raises(IndexError):
        consensus.test_start(events, draft, sums)


def _replay(cls, name):
    draft, events = SC.region(*SC.SCHEDULES[name], B.oracle_swalign)
    want = GOLD["schedules"][name]
    assert SC.inputs_digest(draft, events) == want["inputs"]
    pa = B.make_pa(cls, draft, copy.deepcopy(events), P)
    log = []
    B.reset_rand()
    seq, acc = consensus.consensus_region(pa, test=True, log=log, verbose=-1)
    got = [[c, int(n), SC.digest(s)] for c, n, s in log]
    assert got == want["calls"]
    assert (SC.digest(seq), len(seq), acc) == (want["final"], want["final_len"], want["accuracy"])


@pytest.mark.parametrize("name", sorted(SC.SCHEDULES))
def test_schedule_from_the_start_on_the_oracle_equals_the_reference(name):
    _replay(B.OraclePSAlign, name)


@pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("name", ["cut_400", "whole_1000"])
def test_schedule_from_the_start_on_the_live_reference_build(name):
    _replay(B.RefPSAlign, name)


def test_the_start_is_assigned_without_realignment_and_verbose_is_raised(capsys):
    draft, events = SC.region(*SC.SELECTION["cut_300"], B.oracle_swalign)

    class Stop(Exception):
        pass

    class Probe(B.OraclePSAlign):
        def Mutate(self, seqs='self', reps=4):
            raise Stop()

    pa = B.make_pa(Probe, draft, copy.deepcopy(events), P)
    with pytest.raises(Stop):
        consensus.consensus_region(pa, test=True)
    want = GOLD["selection"]["cut_300"]
    assert SC.digest(pa.sequence) == want["sequence"]
    for a, b in zip(pa.events, events):
        assert np.array_equal(a.ref_align, b.ref_align)                     # as loaded: no RealignTo
    err = capsys.readouterr().err
    assert "starting from event %d" % want["event"] in err                  # test turned verbose 0 into 1 (Mutate.py:45-46)
    # the shortcut comes first: fewer than five events, nothing selected, nothing run
    pa = B.make_pa(Probe, draft, copy.deepcopy(events[:4]), P)
    assert consensus.consensus_region(pa, test=True) == (draft, 100)


def test_lock_step_driver_in_test_mode_equals_region_by_region_oracle():
    cases = [SC.region(*SC.SELECTION["cut_300"], B.oracle_swalign), SC.region(*SC.SELECTION["whole_300"], B.oracle_swalign)]
    d3, e3, _ = synth.make_region(220, 3, 4190, B.oracle_swalign, P)        # below the five-event threshold
    cases.insert(1, (d3, e3))
    cases.append(SC.region(260, 6, 4191, 57, B.oracle_swalign))
    want, wlogs, wacc = [], [], []
    for draft, events in cases:
        B.reset_rand()
        pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P)
        log = []
        want.append(consensus.consensus_region(pa, test=True, log=log, verbose=-1))
        wlogs.append(log)
        wacc.append([swalign(s, draft, B.oracle_api)[0] for c, _, s in log if c in ("Mutate:self", "Refine")])
    pas = [B.make_pa(B.OraclePSAlign, d, copy.deepcopy(ev), P) for d, ev in cases]
    logs, accs = [[] for _ in cases], [[] for _ in cases]
    got = consensus.consensus_regions(pas, test=True, logs=logs, accuracies=accs)
    assert got == want
    assert logs == wlogs and accs == wacc
    assert got[1] == (d3, 100) and logs[1] == [] and accs[1] == []


def test_lock_step_final_accuracies_are_those_of_single_swalign_calls():
    """the default mode: the batched summaries return the very doubles `swalign` gave per region"""
    cases = [SC.region(*SC.SELECTION["whole_300"], B.oracle_swalign), SC.region(260, 6, 4191, None, B.oracle_swalign)]
    pas = [B.make_pa(B.OraclePSAlign, d, copy.deepcopy(ev), P) for d, ev in cases]
    accs, logs = [[] for _ in cases], [[] for _ in cases]
    got = consensus.consensus_regions(pas, accuracies=accs, logs=logs)
    for (seq, acc), (draft, _), a, log in zip(got, cases, accs, logs):
        assert acc == swalign(seq, draft, B.oracle_api)[0]
        assert a == [swalign(s, draft, B.oracle_api)[0] for c, _, s in log if c in ("Mutate:self", "Refine")]   # (before end_trim)


def test_train_in_test_mode_picks_the_winner_of_its_candidates_run_one_by_one():
    draft, events, truth = synth.make_region(300, 5, 4195, B.oracle_swalign, P)

    def make_pa(p):
        evs = copy.deepcopy(events)
        for e in evs:
            e.setparams(p)
        return B.make_pa(B.OraclePSAlign, draft, evs, p)

    sets = [dict(P), dict(P, skip_t=0.6, skip_c=0.6, stay_t=0.5, stay_c=0.5), dict(P, insert_t=0.3, insert_c=0.3)]
    B.reset_rand()
    each = [consensus.consensus_region(make_pa(p), p, reps=2, refseq=truth, test=True, verbose=-1)[1] for p in sets]
    B.reset_rand()
    best, accs = consensus.train(make_pa, P, truth, iters=1, reps=2, paramlists=[sets], test=True)
    assert best == sets[int(np.argmax(each))] and accs == [max(each)]
    # lock-step: every replica is a fresh process
    fresh = []
    for p in sets:
        B.reset_rand()
        fresh.append(consensus.consensus_region(make_pa(p), p, reps=2, refseq=truth, test=True, verbose=-1)[1])
    best, accs = consensus.train(make_pa, P, truth, iters=1, reps=2, paramlists=[sets], test=True, lock_step=True)
    assert best == sets[int(np.argmax(fresh))] and accs == [max(fresh)]


def test_refine_regions_hands_the_flag_to_the_lock_step_driver():
    from poreseq_amd import dist as psdist
    cases = [SC.region(*SC.SELECTION["cut_300"], B.oracle_swalign), SC.region(260, 6, 4191, 57, B.oracle_swalign)]
    regs = [(0, len(cases[0][0])), (1000, 1000 + len(cases[1][0]))]
    by_start = {a: c for (a, _), c in zip(regs, cases)}

    def make_region_pa(a, b):
        draft, events = by_start[a]
        return B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P)

    want = []
    for draft, events in cases:
        B.reset_rand()
        want.append(consensus.consensus_region(B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P), test=True, verbose=-1))
    assert psdist.refine_regions(regs, make_region_pa, batch=2, test=True) == want
    assert psdist.refine_regions(regs, make_region_pa, batch=2) != want
