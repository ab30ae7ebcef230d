"""Alignment census and scaling fit on the CPU checkers: the fallback path (util.align_stats_from_refs behind PSAlign.AlignStats /
RegionBatch.AlignStats on a library without ps_align_stats) against the plain loops of stats_cases, util.fit_scaling / apply_scaling
against the exact-WLS bounds on simulated reads with a known distortion, PSEvent.getrefstats, and the `recalibrate` argument of the
consensus drivers.  The same cases run on k_align_stats in test_hip_align_stats.py."""
import copy
import ctypes
import os
import re

import numpy as np

import backends as B
import stats_cases as S
from poreseq_amd import _capi, consensus, synth, util
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import consensus_region, consensus_regions

NEW = ("ps_align_stats", "ps_batch_align_stats")
P = S.P0


def test_new_symbols_are_declared_optional_and_exported_by_the_product():
    hdr = open(os.path.join(B.ROOT, "include", "poreseq_hip.h")).read()
    declared = set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _capi.SYMBOLS and name in _capi.OPTIONAL
    api = B.oracle_api()                             # the checker lacks them and still loads
    assert set(NEW) <= api.missing and api.missing <= _capi.OPTIONAL
    lib = ctypes.CDLL(_capi.HIP_LIB)                 # the product exports them
    for name in NEW:
        assert hasattr(lib, name), name
    assert _capi.load_hip().missing == set()
    assert _capi.EVENT_STATS.itemsize == 112
    assert [_capi.EVENT_STATS.fields[k][1] for k in ("n_levels", "reserved", "n_gap_cols", "sw", "swrr")] == [0, 52, 56, 64, 104]


def test_fallback_equals_the_plain_loops_on_every_crafted_case():
    for name, (seq, events) in S.crafted().items():
        st = S.states_of(seq)
        got = np.zeros(len(events), dtype=_capi.EVENT_STATS)
        for e, ev in enumerate(events):
            got[e] = util.align_stats_from_refs(st, ev.mean, ev.ref_align, ev.model.level_mean, ev.model.level_stdv)
        S.check(got, S.want(seq, events), name)
    w = S.want(*S.crafted()["mixed16"])[0]           # the case's purpose, by hand: stay, extend, extend, a stay across an insert ...
    assert [w[k] for k in ("n_aligned", "n_insert", "n_unaligned", "n_stay", "n_extend", "n_step", "n_jump", "n_gap_cols", "n_back",
                           "first_col", "last_col")] == [10, 3, 3, 2, 3, 1, 2, 3, 1, 3, 8]
    w = S.want(*S.crafted()["seven"])[4]             # 300 inserted levels between two levels on column 20: one stay, then an extend
    assert w["n_insert"] == 300 and w["n_levels"] == 600
    w = S.want(*S.crafted()["past_S"])[0]
    assert w["n_nostate"] == 8 and w["n_fit"] == 6 and w["last_col"] == 1
    seq, events = S.crafted()["non_acgt"]
    assert min(S.states_of(seq)) < 0 and S.want(seq, events)[0]["n_nostate"] > 0


def test_align_stats_through_the_oracle_on_the_crafted_cases():
    """PSAlign.AlignStats(realign=False) and the lock-step RegionBatch on a library without the entry point"""
    cases = S.crafted()
    for name, (seq, events) in cases.items():
        scores, got = S.pa_of(B.OraclePSAlign, seq, events).AlignStats(realign=False)
        assert scores is None
        S.check(got, S.want(seq, events), name)
    pas = [S.pa_of(B.OraclePSAlign, *cases[n]) for n in S.BATCH]
    for resident in (True, False):
        rb = RegionBatch(pas, resident=resident)
        try:
            res = rb.AlignStats(realign=False)
            back = rb.AlignStats(idx=[2, 1], realign=False)
            rb.drop()
        finally:
            rb.close()
        for n, (sc, got) in zip(S.BATCH, res):
            assert sc is None
            S.check(got, S.want(*cases[n]), "lock-step " + n)
        assert back[0][1].tobytes() == res[2][1].tobytes() and back[1][1].tobytes() == res[1][1].tobytes()


def _getrefstats(ra):
    """EventData.py:264-286, restated"""
    ra = np.asarray(ra, dtype=np.float64)
    counts = {}
    for x in ra:
        if x >= 0:
            counts[int(x)] = counts.get(int(x), 0) + 1
    top = max(counts) if counts else 0
    skips = sum(1 for c in range(1, top + 1) if c not in counts)
    stays = sum(n - 1 for c, n in counts.items() if c >= 1)
    total = float(sum(1 for x in ra if x != 0))
    return skips / total, stays / total, sum(1 for x in ra if x < 0) / total


def test_getrefstats_is_the_reference_definition():
    n = 0
    for name, (seq, events) in S.crafted().items():
        for ev in events:
            if np.isnan(ev.ref_align).any() or not np.any(ev.ref_align != 0) or ev.ref_align.max() > 1e6:
                continue                             # (the reference's bincount has no answer for these)
            got = ev.getrefstats()
            assert tuple(float(g) for g in got) == _getrefstats(ev.ref_align), name
            n += 1
    assert n >= 6
    ev = S.crafted()["mixed16"][1][0]
    assert ev.getrefstats() == (4 / 13, 5 / 13, 3 / 13)


def test_fallback_on_the_oracle_after_a_realignment():
    draft, events = synth.make_region(260, 6, 8821, B.oracle_swalign, P)[:2]
    pa = S.pa_of(B.OraclePSAlign, draft, events)
    scores, got = pa.AlignStats()
    assert np.asarray(scores, dtype=np.float64).tobytes() == np.asarray(S.pa_of(B.OraclePSAlign, draft, events).ScoreEvents(), dtype=np.float64).tobytes()
    api = B.oracle_api()
    h = api.align_create(draft, copy.deepcopy(events), P)
    try:
        api.score_alignments(h, len(events))
        refs = api.align_event_refs(h, len(events))
    finally:
        api.align_destroy(h)
    assert any(not np.array_equal(r, ev.ref_align) for r, ev in zip(refs, events))       # the call did realign
    S.check(got, S.want(draft, events, refs), "after a realignment")
    assert all(np.array_equal(a.ref_align, b.ref_align) and np.array_equal(a.ref_like, b.ref_like) for a, b in zip(pa.events, events))
    assert pa.sequence == draft


def test_fit_recovers_a_known_distortion():
    for a, b in S.DISTORTIONS:
        seq, events = S.recovery_region(a, b)
        _, stats = S.pa_of(B.OraclePSAlign, seq, events).AlignStats(realign=False)
        S.check(stats, S.want(seq, events), "recovery")                                   # the sums are the yardstick's
        S.check_recovery(stats, util.fit_scaling(stats), a, b)


def test_fit_guards_and_apply():
    seq, events = S.recovery_region(1.05, -1.5)
    _, stats = S.pa_of(B.OraclePSAlign, seq, events).AlignStats(realign=False)
    f = util.fit_scaling(stats[0])
    assert f.ok and util.fit_scaling(stats)[0] == f
    ident = (1.0, 0.0, 1.0, False)
    assert tuple(util.fit_scaling(stats[0], min_levels=10 ** 6))[:4] == ident
    assert tuple(util.fit_scaling(stats[0], scale_limits=(0.99, 1.01)))[:4] == ident
    assert tuple(util.fit_scaling(stats[0], var_limits=(2.0, 4.0)))[:4] == ident
    assert tuple(util.fit_scaling(stats[0], min_spread=0.999))[:4] == ident
    assert tuple(util.fit_scaling(np.zeros((), dtype=_capi.EVENT_STATS)))[:4] == ident
    ev = copy.deepcopy(events[0])
    before = copy.deepcopy(ev)
    util.apply_scaling(ev, f, var=False)
    assert np.array_equal(ev.model.level_mean, before.model.level_mean * f.scale + f.shift)
    assert np.array_equal(ev.model.level_stdv, before.model.level_stdv)
    util.apply_scaling(ev, f)
    assert np.array_equal(ev.model.level_stdv, before.model.level_stdv * f.var)
    for k in ("sd_mean", "sd_stdv"):
        assert np.array_equal(getattr(ev.model, k), getattr(before.model, k))
    assert np.array_equal(ev.mean, before.mean) and np.array_equal(ev.ref_align, before.ref_align)


def check_score_can_only_improve(cls, seq, events):
    """s0 = the scores of AlignStats(); the mean scaling of every read with an ok fit applied (var=False); s1 = ScoreEvents(): no
    event scores worse.  The band of both calls comes from the Python ref_align, which neither writes; the path that scored s0 is in
    the band of the second call, its transitions and stdv terms are unchanged, and the fit minimises the Gaussian part over exactly
    the levels that carry an emission."""
    pa = S.pa_of(cls, seq, events)
    s0, st = pa.AlignStats()
    fits = util.fit_scaling(st)
    for ev, f in zip(pa.events, fits):
        if f.ok:
            util.apply_scaling(ev, f, var=False)
    s1 = pa.ScoreEvents()
    for e, (x0, x1) in enumerate(zip(np.asarray(s0).tolist(), s1)):
        print("event %d: %.6f -> %.6f (%s)" % (e, x0, x1, fits[e]))
        assert x1 >= x0 - 1e-9 * max(1.0, abs(x0)), (e, x0, x1, fits[e])
    return fits


def test_score_can_only_improve_on_the_oracle():
    for a, b in S.DISTORTIONS:
        fits = check_score_can_only_improve(B.OraclePSAlign, *S.recovery_region(a, b))
        assert all(f.ok for f in fits)
    check_score_can_only_improve(B.OraclePSAlign, *synth.make_region(300, 6, 8822, B.oracle_swalign, P)[:2])


def _models(events):
    return [(ev.model.level_mean.tobytes(), ev.model.level_stdv.tobytes()) for ev in events]


def test_consensus_drivers_with_and_without_recalibrate():
    regs = [synth.make_region(300, 8, 8831, B.oracle_swalign, P)[:2], synth.make_region(200, 5, 8832, B.oracle_swalign, P)[:2]]
    runs = {}
    for key, kw in (("plain", {}), ("none", dict(recalibrate=None)), ("on", dict(recalibrate=True))):
        out = []
        for draft, events in regs:
            B.reset_rand()
            pa, log = S.pa_of(B.OraclePSAlign, draft, events), []
            res = consensus_region(pa, reps=2, log=log, **kw)
            out.append((res, log, _models(pa.events)))
        runs[key] = out
    assert runs["none"] == runs["plain"] and consensus._recalibrate_kw(False) is None and consensus._recalibrate_kw(True) == {}
    for (draft, events), (res, log, models), (_, plain_log, _) in zip(regs, runs["on"], runs["plain"]):
        fits = S.pa_of(B.OraclePSAlign, draft, events).Recalibrate()
        ok = [f.ok for f in fits]
        assert log[0] == ("Recalibrate", sum(ok), draft) and [l[0] for l in log[1:]][:1] == ["Mutate:self"]
        assert sum(1 for l in log if l[0] == "Recalibrate") == 1 and plain_log[0][0] == "Mutate:self"
        assert [m != m0 for m, m0 in zip(models, _models(events))] == ok and any(ok)
        want = copy.deepcopy(events)
        for ev, f in zip(want, fits):
            if f.ok:
                util.apply_scaling(ev, f)
        assert models == _models(want)
    for key, kw, modes in (("plain", {}, (True,)), ("on", dict(recalibrate=dict(var=True, min_levels=100)), (True, False))):
        for resident in modes:
            pas, logs = [S.pa_of(B.OraclePSAlign, d, ev) for d, ev in regs], [[], []]
            res = consensus_regions(pas, reps=2, logs=logs, resident=resident, **kw)
            for k in range(2):
                assert res[k][0] == runs[key][k][0][0] and res[k][1] == runs[key][k][0][1], (key, resident, k)
                assert logs[k] == runs[key][k][1] and _models(pas[k].events) == runs[key][k][2]
