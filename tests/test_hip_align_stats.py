"""Alignment census and scaling fit on the GPU (k_align_stats; ps_align_stats / ps_batch_align_stats): `PSAlign.AlignStats`,
`RegionBatch.AlignStats` / `Recalibrate` against the plain loops of stats_cases — ints equal, the six sums byte for byte — on the
crafted ref arrays (realign=0) and on the refs a realignment leaves in the handle under every fill; the keep_refs contract of a
resident batch; and the recovery and score tests of test_align_stats.py on the HIP path."""
import copy
import ctypes as C

import numpy as np
import pytest

import backends as B
import stats_cases as S
from poreseq_amd import _capi, synth, util
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign
from test_align_stats import check_score_can_only_improve

pytestmark = pytest.mark.gpu
P = S.P0
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]      # conftest's fwd_kernel fixture
_MADE = {}


def region260():
    if "r" not in _MADE:
        _MADE["r"] = synth.make_region(260, 6, 8821, B.oracle_swalign, P)[:2]
    return _MADE["r"]


def launches(api):
    return api.prof_get("align_stats")[1]


@pytest.mark.parametrize("name", list(S.crafted()))
def test_crafted_ref_arrays_without_a_realignment(name):
    seq, events = S.crafted()[name]
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        scores, got = S.pa_of(PSAlign, seq, events).AlignStats(realign=False)
        n = launches(api)
        fill = [api.prof_get(k)[1] for k in ("fill", "sweep")]
    finally:
        api.prof_enable(0)
    assert scores is None and n == (1 if events else 0) and fill == [0, 0]      # one launch, no DP; nothing for a region without events
    S.check(got, S.want(seq, events), name)
    assert not got["reserved"].any()


@pytest.mark.parametrize("resident", [True, False])
def test_lock_step_batch_of_crafted_regions(resident):
    cases = S.crafted()
    pas = [S.pa_of(PSAlign, *cases[n]) for n in S.BATCH]
    api = _capi.load_hip()
    rb = RegionBatch(pas, resident=resident)
    try:
        rb.load()
        api.prof_enable(1)
        api.prof_reset()
        try:
            res = rb.AlignStats(realign=False)
            n = launches(api)
        finally:
            api.prof_enable(0)
        back = rb.AlignStats(idx=[2, 1], realign=False)
        rb.drop()
    finally:
        rb.close()
    assert n == 1                                                               # 0 + 1 + 7 events: one launch
    for name, (sc, got) in zip(S.BATCH, res):
        assert sc is None
        S.check(got, S.want(*cases[name]), "lock-step " + name)
    assert back[0][1].tobytes() == res[2][1].tobytes() and back[1][1].tobytes() == res[1][1].tobytes()
    for pa, name in zip(pas, S.BATCH):
        assert all(np.array_equal(a.ref_align, b.ref_align, equal_nan=True) for a, b in zip(pa.events, cases[name][1]))


@pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)
def test_realignment_under_every_fill(fwd_kernel):
    draft, events = region260()
    api = _capi.load_hip()
    E = len(events)
    h = api.align_create(draft, copy.deepcopy(events), P)
    api.prof_enable(1)
    api.prof_reset()
    try:
        scores, got = api.align_stats(h, E, True)
        n = launches(api)
        refs = api.align_event_refs(h, E)
    finally:
        api.prof_enable(0)
        api.align_destroy(h)
    assert n == 1
    assert scores.tobytes() == np.asarray(S.pa_of(PSAlign, draft, events).ScoreEvents(), dtype=np.float64).tobytes()
    assert any(not np.array_equal(r, ev.ref_align) for r, ev in zip(refs, events))
    S.check(got, S.want(draft, events, refs), "realigned, " + fwd_kernel)
    if "oracle" not in _MADE:
        _MADE["oracle"] = S.pa_of(B.OraclePSAlign, draft, events).AlignStats()
    assert got.tobytes() == _MADE["oracle"][1].tobytes() and scores.tobytes() == np.asarray(_MADE["oracle"][0]).tobytes()
    pa = S.pa_of(PSAlign, draft, events)                                        # the Python call: same bits, events untouched
    s2, g2 = pa.AlignStats()
    assert s2.tobytes() == scores.tobytes() and g2.tobytes() == got.tobytes()
    assert all(np.array_equal(a.ref_align, b.ref_align) and np.array_equal(a.ref_like, b.ref_like) for a, b in zip(pa.events, events))


def _state(pas):
    return [(pa.sequence, [(ev.ref_align.tobytes(), ev.ref_like.tobytes()) for ev in pa.events]) for pa in pas]


def test_resident_batch_keeps_its_refs_and_rebuilds_after_recalibrate():
    regs = [region260(), synth.make_region(200, 5, 8823, B.oracle_swalign, P)[:2]]
    mk = lambda: [S.pa_of(PSAlign, d, ev) for d, ev in regs]
    alone = mk()
    with RegionBatch(alone) as rb:
        nb_alone = rb.Refine()
    pas = mk()
    with RegionBatch(pas) as rb:
        first = rb.AlignStats()
        again = rb.AlignStats()
        nb = rb.Refine()
    assert nb == nb_alone and _state(pas) == _state(alone)                      # AlignStats left nothing behind in the handles
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(first, again))
    for (d, ev), (sc, st) in zip(regs, first):
        one = S.pa_of(PSAlign, d, ev).AlignStats()
        assert one[0].tobytes() == sc.tobytes() and one[1].tobytes() == st.tobytes()
    pas = mk()
    rb = RegionBatch(pas)
    try:
        rb.load()
        fits = rb.Recalibrate()
        scores = rb.ScoreEvents()
        rb.drop()
    finally:
        rb.close()
    for (d, ev), pa, f, sc in zip(regs, pas, fits, scores):
        want = copy.deepcopy(ev)
        for e, one in zip(want, f):
            if one.ok:
                util.apply_scaling(e, one)
        assert any(one.ok for one in f)
        assert [e.model.level_mean.tobytes() for e in pa.events] == [e.model.level_mean.tobytes() for e in want]
        assert sc == S.pa_of(PSAlign, d, want).ScoreEvents()                    # a fresh PSAlign carrying the recalibrated models
        assert sc != S.pa_of(PSAlign, d, ev).ScoreEvents()


def test_fit_recovers_a_known_distortion_on_the_device():
    for a, b in S.DISTORTIONS:
        seq, events = S.recovery_region(a, b)
        _, stats = S.pa_of(PSAlign, seq, events).AlignStats(realign=False)
        S.check(stats, S.want(seq, events), "recovery")
        S.check_recovery(stats, util.fit_scaling(stats), a, b)


def test_score_can_only_improve_on_the_device():
    for a, b in S.DISTORTIONS:
        fits = check_score_can_only_improve(PSAlign, *S.recovery_region(a, b))
        assert all(f.ok for f in fits)
    check_score_can_only_improve(PSAlign, *synth.make_region(300, 6, 8822, B.oracle_swalign, P)[:2])


def test_bad_arguments_of_the_c_abi():
    api = _capi.load_hip()
    draft, events = region260()
    E = len(events)
    h = api.align_create(draft, copy.deepcopy(events), P)
    h0 = api.align_create(draft, [], P)
    try:
        st, sc = np.zeros(E, dtype=_capi.EVENT_STATS), np.zeros(E)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*scores without a realignment"):      # PS_ERR_BAD_ARG
            api.check(api.lib.ps_align_stats(h, 0, _capi._dp(sc), vp(st)))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null stats"):
            api.check(api.lib.ps_align_stats(h, 1, _capi._dp(sc), None))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null stats"):
            api.check(api.lib.ps_align_stats(h0, 0, None, None))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\)"):
            api.check(api.lib.ps_align_stats(None, 0, None, vp(st)))
        api.prof_enable(1)
        api.prof_reset()
        try:
            api.check(api.lib.ps_align_stats(h0, 1, None, vp(st)))              # no events: PS_OK, nothing launched
            api.check(api.lib.ps_align_stats(h0, 0, None, vp(st)))
            assert launches(api) == 0
            api.check(api.lib.ps_align_stats(h, 1, None, vp(st)))               # scores may be NULL with a realignment
            assert launches(api) == 1
        finally:
            api.prof_enable(0)
        assert st["n_levels"].tolist() == [ev.mean.size for ev in events] and (st["n_fit"] > 0).all()
    finally:
        api.align_destroy(h)
        api.align_destroy(h0)
