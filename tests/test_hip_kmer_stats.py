"""Per-k-mer model statistics on the GPU (k_kmer_stats; ps_kmer_stats / ps_batch_kmer_stats): `PSAlign.KmerStats`,
`RegionBatch.KmerStats` / `RefitKmers` against the plain loops of kmer_cases — counts equal, the five sums byte for byte — on the
crafted ref arrays (realign=0), on ragged lock-step batches and on the refs a realignment leaves in the handle; the invariant
against ps_align_stats' n_fit; resident and rebuilt batches; one launch per call; poisoned scratch; and the refit end to end."""
import copy
import ctypes as C

import numpy as np
import pytest

import backends as B
import golden_util as G
import kmer_cases as K
import poison_cases as PC
import sweep_cases
import tiled_cases
from poreseq_amd import _capi, util
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import consensus_region
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu
P = K.P0


def launches(api):
    return api.prof_get("kmer_stats")[1]


@pytest.mark.parametrize("name", list(K.crafted()))
def test_crafted_ref_arrays_without_a_realignment(name):
    seq, events, grp, G_ = K.crafted()[name]
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        scores, got = K.pa_of(PSAlign, seq, events).KmerStats(grp, G_, realign=False)
        n = launches(api)
        fill = [api.prof_get(k)[1] for k in ("fill", "sweep", "align_stats")]
    finally:
        api.prof_enable(0)
    assert scores is None and n == (1 if events else 0) and fill == [0, 0, 0]      # one launch, no DP; nothing for a region without events
    K.check(got, K.want(seq, events, grp, G_), name)
    if name == "nonfinite":
        fin = np.ones(got.shape, dtype=bool)
        for cell in K.nonfinite_cells():
            fin[cell] = False
        assert all(np.isfinite(got[k][fin]).all() for k in K.SUMS) and not np.isfinite(got["sz"][~fin]).any()
    if name == "order_ab":                                                          # the other event order: other bits, also on the device
        other = K.pa_of(PSAlign, *K.crafted()["order_ba"][:2]).KmerStats([0, 0], 1, realign=False)[1]
        assert other.tobytes() != got.tobytes() and (other["n"] == got["n"]).all()


@pytest.mark.parametrize("resident", [True, False])
def test_ragged_lock_step_batch(resident):
    cases = K.crafted()
    pas = [K.pa_of(PSAlign, *cases[n][:2]) for n in K.BATCH]
    grp, ng = [cases[n][2] for n in K.BATCH], [cases[n][3] for n in K.BATCH]
    api = _capi.load_hip()
    rb = RegionBatch(pas, resident=resident)
    try:
        rb.load()
        api.prof_enable(1)
        api.prof_reset()
        try:
            res = rb.KmerStats(groups=grp, n_groups=ng, realign=False)
            n = launches(api)
        finally:
            api.prof_enable(0)
        back = rb.KmerStats(idx=[2, 1], groups=[grp[2], grp[1]], n_groups=[ng[2], ng[1]], realign=False)
        rb.drop()
    finally:
        rb.close()
    assert n == 1 and [t.shape[0] for _, t in res] == [2, 1, 3]                     # 0 + 1 + 7 events, 2 + 1 + 3 groups: one launch
    for name, (sc, got) in zip(K.BATCH, res):
        assert sc is None
        K.check(got, K.want(*cases[name]), "lock-step " + name)
        alone = K.pa_of(PSAlign, *cases[name][:2]).KmerStats(cases[name][2], cases[name][3], realign=False)[1]
        assert got.tobytes() == alone.tobytes(), name                                # the table of a call on its own, by bytes
    assert res[0][1].tobytes() == bytes(2 * 1024 * 48)
    assert back[0][1].tobytes() == res[2][1].tobytes() and back[1][1].tobytes() == res[1][1].tobytes()
    for pa, name in zip(pas, K.BATCH):
        assert all(np.array_equal(a.ref_align, b.ref_align, equal_nan=True) for a, b in zip(pa.events, cases[name][1]))


def _region260():
    seed = min(sweep_cases.SEEDS, key=lambda s: (abs(len(sweep_cases.case(s)[0]) - 260), s))
    draft, holed, _, par, _ = sweep_cases.case(seed)
    return draft, K.quantised(holed), par


def _single():
    draft, events, par = tiled_cases.crafted("single", "truncated")
    return draft, K.quantised(events), par


@pytest.mark.parametrize("region", [_region260, _single], ids=["sweep260", "tiled_single"])
def test_realignment_scores_table_and_invariant(region):
    draft, events, par = region()
    api = _capi.load_hip()
    E = len(events)
    grp, G_ = util.kmer_groups(events)
    h = api.align_create(draft, copy.deepcopy(events), par)
    api.prof_enable(1)
    api.prof_reset()
    try:
        scores, got = api.kmer_stats(h, E, grp, G_, True)
        n = launches(api)
        refs = api.align_event_refs(h, E)
        _, st = api.align_stats(h, E, False)                                        # the same handle, the refs the call left
    finally:
        api.prof_enable(0)
        api.align_destroy(h)
    assert n == 1
    assert scores.tobytes() == np.asarray(K.pa_of(PSAlign, draft, events, par).ScoreEvents(), dtype=np.float64).tobytes()
    assert any(not np.array_equal(r, ev.ref_align, equal_nan=True) for r, ev in zip(refs, events))
    K.check(got, K.want(draft, events, grp.tolist(), G_, refs=refs), "realigned")
    assert int(got["n"].sum()) == int(st["n_fit"].sum()) > 0
    pa = K.pa_of(PSAlign, draft, events, par)                                       # the Python call: same bits, events untouched
    s2, g2 = pa.KmerStats()
    assert s2.tobytes() == scores.tobytes() and g2.tobytes() == got.tobytes()
    assert all(np.array_equal(a.ref_align, b.ref_align, equal_nan=True) and np.array_equal(a.ref_like, b.ref_like, equal_nan=True)
               for a, b in zip(pa.events, events))


def test_n_fit_invariant_on_the_crafted_cases():
    for name, (seq, events, grp, G_) in K.crafted().items():
        pa = K.pa_of(PSAlign, seq, events)
        _, tb = pa.KmerStats(grp, G_, realign=False)
        _, st = pa.AlignStats(realign=False)
        assert int(tb["n"].sum()) == int(st["n_fit"].sum()), name


def _state(pas):
    return [(pa.sequence, [(ev.ref_align.tobytes(), ev.ref_like.tobytes()) for ev in pa.events]) for pa in pas]


def test_resident_and_rebuilt_batches_agree_and_one_launch_per_call():
    d1, e1, p1 = _region260()
    d2, e2 = K.true_region(200, 5, 9912)
    regs = [(d1, e1, p1), (d2, e2, P)]
    mk = lambda: [K.pa_of(PSAlign, d, ev, par) for d, ev, par in regs]
    api = _capi.load_hip()
    out = {}
    for resident in (True, False):
        pas = mk()
        with RegionBatch(pas, resident=resident) as rb:
            rb.load()
            api.prof_enable(1)
            api.prof_reset()
            try:
                first = rb.KmerStats()
                n1 = launches(api)
                again = rb.KmerStats()
                n2 = launches(api)
            finally:
                api.prof_enable(0)
            nb = rb.Refine()
        assert (n1, n2) == (1, 2)                                                   # once per batch call
        assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(first, again))
        out[resident] = (first, nb, _state(pas))
    (ra, nba, sa), (rb_, nbb, sb) = out[True], out[False]
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(ra, rb_))
    assert nba == nbb and sa == sb                                                  # KmerStats left nothing behind in the resident handles
    alone = mk()
    with RegionBatch(alone) as rb:
        assert rb.Refine() == nba
    assert _state(alone) == sa
    for (d, ev, par), (sc, tb) in zip(regs, ra):
        one = K.pa_of(PSAlign, d, ev, par).KmerStats()
        assert one[0].tobytes() == sc.tobytes() and one[1].tobytes() == tb.tobytes()


@pytest.mark.parametrize("pattern", PC.PATTERN_IDS)
def test_poisoned_scratch_changes_no_byte(pattern):
    d1, e1, p1 = _region260()
    seq, events, grp, G_ = K.crafted()["seven"]
    plain = (K.pa_of(PSAlign, d1, e1, p1).KmerStats(), K.pa_of(PSAlign, seq, events).KmerStats(grp, G_, realign=False))
    cls = PC.CLASSES[pattern]
    calls = PC.api(pattern).calls
    got = (K.pa_of(cls, d1, e1, p1).KmerStats(), K.pa_of(cls, seq, events).KmerStats(grp, G_, realign=False))
    assert PC.api(pattern).calls > calls
    assert PC.same_bytes(got, plain)


def test_bad_arguments_of_the_c_abi():
    api = _capi.load_hip()
    seq, events, _, _ = K.crafted()["one_group"]
    E = len(events)
    h = api.align_create(seq, copy.deepcopy(events), P)
    h0 = api.align_create(seq, [], P)
    try:
        tb, sc = np.ones((3, 1024), dtype=_capi.KMER_STATS), np.zeros(E)
        grp = np.array([0, 2, 0, 2], dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ip = lambda a: a.ctypes.data_as(_capi.c_i32p)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*scores without a realignment"):      # PS_ERR_BAD_ARG
            api.check(api.lib.ps_kmer_stats(h, 0, ip(grp), 3, _capi._dp(sc), vp(tb)))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null table"):
            api.check(api.lib.ps_kmer_stats(h, 0, ip(grp), 3, None, None))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null groups"):
            api.check(api.lib.ps_kmer_stats(h, 0, None, 3, None, vp(tb)))
        for bad in (0, 257, -1):
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*n_groups"):
                api.check(api.lib.ps_kmer_stats(h, 0, ip(grp), bad, None, vp(tb)))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*event 1 has group 2"):
            api.check(api.lib.ps_kmer_stats(h, 0, ip(grp), 2, None, vp(tb)))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*has group -1"):
            api.check(api.lib.ps_kmer_stats(h, 0, ip(np.array([0, 0, -1, 0], dtype=np.int32)), 2, None, vp(tb)))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\)"):
            api.check(api.lib.ps_kmer_stats(None, 0, ip(grp), 3, None, vp(tb)))
        assert (tb["n"] == 1).all()                                                 # a refused call writes nothing
        api.prof_enable(1)
        api.prof_reset()
        try:
            api.check(api.lib.ps_kmer_stats(h0, 1, None, 3, None, vp(tb)))          # no events: PS_OK, nothing launched, all zero
            assert launches(api) == 0 and tb.tobytes() == bytes(3 * 1024 * 48)
            api.check(api.lib.ps_kmer_stats(h, 1, ip(grp), 3, None, vp(tb)))        # scores may be NULL with a realignment
            assert launches(api) == 1
        finally:
            api.prof_enable(0)
        assert tb["n"][0].any() and tb["n"][2].any() and not tb["n"][1].any()
        big = api.kmer_stats(h, E, [0, 255, 3, 3], 256, False)[1]                   # the most groups the ABI takes
        refs = api.align_event_refs(h, E)                                           # (the realignment above stays in the handle)
        K.check(big, K.want(seq, events, [0, 255, 3, 3], 256, refs=refs), "256 groups")
    finally:
        api.align_destroy(h)
        api.align_destroy(h0)


def test_refit_recovers_shifted_kmers_end_to_end():
    """a 450-base, 6-read region with true alignments; on the template reads' models the 20 most frequent k-mers of the sequence are
    shifted by 3 level_stdv.  RefitKmers must raise the total score; how close it comes to the undistorted models is what the
    shrinkage (prior 8) leaves, printed and not bounded"""
    seq, events = K.true_region()
    ks = np.array(K.top_kmers(seq, 20))
    bent = copy.deepcopy(events)
    for ev in bent:
        if not ev.model.complement:
            ev.model.level_mean = ev.model.level_mean.copy()
            ev.model.level_mean[ks] = ev.model.level_mean[ks] + 3.0 * ev.model.level_stdv[ks]
    clean = sum(K.pa_of(PSAlign, seq, events).ScoreEvents())
    pa = K.pa_of(PSAlign, seq, bent)
    before = sum(pa.ScoreEvents())
    fits = pa.RefitKmers()
    after = sum(pa.ScoreEvents())
    print("sum of scores: before %.3f, after %.3f, clean %.3f; template dmean on the shifted k-mers %s"
          % (before, after, clean, np.round(fits[0].dmean[ks], 2).tolist()))
    assert before < after
    assert len(fits) == 2 and np.median(fits[0].dmean[ks]) < -0.5                   # the template group moves back towards its levels
    with RegionBatch([K.pa_of(PSAlign, seq, bent), K.pa_of(PSAlign, seq, bent)]) as rb:      # the lock-step form on resident handles
        rb.load()
        each = rb.RefitKmers(pool=False)
        sc = rb.ScoreEvents()
    assert each[0][0].dmean.tobytes() == fits[0].dmean.tobytes() and sum(sc[0]) == after and sum(sc[1]) == after
    out = consensus_region(K.pa_of(PSAlign, seq, bent), reps=1, refit_kmers=True)
    assert isinstance(out[0], str) and len(out[0]) > 100                            # (end_trim takes 150 bases off either end)


def test_refit_kmers_off_is_the_golden_schedule():
    z = G.load("consensus_L400_E6")
    B.reset_rand()
    pa, log = G.make(PSAlign, z), []
    consensus_region(pa, params={}, reps=4, log=log, refit_kmers=False)
    assert [l[0] for l in log] == [str(c) for c in z["calls"]]
    assert [l[1] for l in log] == [int(n) for n in z["nbases"]] and [l[2] for l in log] == [str(s) for s in z["sequences"]]
    for e, ev in enumerate(pa.events):
        assert np.array_equal(ev.ref_align, z["final_ev%d_ref_align" % e]) and np.array_equal(ev.ref_like, z["final_ev%d_ref_like" % e])
