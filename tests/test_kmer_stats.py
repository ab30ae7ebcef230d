"""Per-k-mer model statistics on the CPU checkers: the fallback path (util.kmer_stats_from_refs behind PSAlign.KmerStats /
RegionBatch.KmerStats on a library without ps_kmer_stats) against the plain loops of kmer_cases, and the host side of the refit —
util.kmer_groups, fit_kmers, fit_scaling_sd, apply_kmers, apply_scaling_sd, add_kmer_stats — by its algebraic identities; the
`refit_kmers` argument of the consensus drivers.  The same cases run on k_kmer_stats in test_hip_kmer_stats.py."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import backends as B
import kmer_cases as K
from poreseq_amd import _capi, consensus, synth, util
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import consensus_region, consensus_regions

NEW = ("ps_kmer_stats", "ps_batch_kmer_stats")
P = K.P0


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
    assert _capi.KMER_STATS.itemsize == 48
    assert [_capi.KMER_STATS.fields[k][1] for k in ("n", "sz", "szz", "sp", "spu", "spv")] == [0, 8, 16, 24, 32, 40]
    src = open(os.path.join(B.ROOT, "poreseq_amd", "csrc", "ps_internal.h")).read()      # the tile the cases straddle is the kernel's
    assert int(re.search(r"constexpr int KMER_TILE = (\d+);", src).group(1)) == _capi.KMER_TILE == K.T
    assert int(re.search(r"#define PS_KMER_MAX_GROUPS (\d+)", hdr).group(1)) == _capi.KMER_MAX_GROUPS == util.KMER_MAX_GROUPS == 256


@pytest.mark.parametrize("name", list(K.crafted()))
def test_fallback_equals_the_plain_loops_on_every_crafted_case(name):
    seq, events, grp, G = K.crafted()[name]
    scores, got = K.pa_of(B.OraclePSAlign, seq, events).KmerStats(grp, G, realign=False)
    assert scores is None
    K.check(got, K.want(seq, events, grp, G), name)
    if name == "nonfinite":
        fin = np.ones(got.shape, dtype=bool)
        for cell in K.nonfinite_cells():
            fin[cell] = False
        assert all(np.isfinite(got[k][fin]).all() for k in K.SUMS) and not np.isfinite(got["sz"][~fin]).any()


def test_lock_step_batch_on_the_oracle_equals_the_single_calls():
    cases = K.crafted()
    pas = [K.pa_of(B.OraclePSAlign, *cases[n][:2]) for n in K.BATCH]
    grp, ng = [cases[n][2] for n in K.BATCH], [cases[n][3] for n in K.BATCH]
    for resident in (True, False):
        rb = RegionBatch(pas, resident=resident)
        try:
            res = rb.KmerStats(groups=grp, n_groups=ng, realign=False)
            back = rb.KmerStats(idx=[2, 1], groups=[grp[2], grp[1]], n_groups=[ng[2], ng[1]], realign=False)
            rb.drop()
        finally:
            rb.close()
        assert [t.shape[0] for _, t in res] == [2, 1, 3]
        for n, (sc, got) in zip(K.BATCH, res):
            assert sc is None
            K.check(got, K.want(*cases[n]), "lock-step " + n)
            assert got.tobytes() == K.pa_of(B.OraclePSAlign, *cases[n][:2]).KmerStats(cases[n][2], cases[n][3], realign=False)[1].tobytes()
        assert back[0][1].tobytes() == res[2][1].tobytes() and back[1][1].tobytes() == res[1][1].tobytes()
    assert not res[0][1]["n"].any() and res[0][1].tobytes() == bytes(2 * 1024 * 48)      # no events: an all-zero table


def test_fallback_after_a_realignment_and_the_n_fit_invariant():
    draft, events = synth.make_region(260, 6, 8821, B.oracle_swalign, P)[:2]
    events = K.quantised(events)
    pa = K.pa_of(B.OraclePSAlign, draft, events)
    scores, got = pa.KmerStats()
    assert np.asarray(scores, dtype=np.float64).tobytes() == np.asarray(K.pa_of(B.OraclePSAlign, draft, events).ScoreEvents(), dtype=np.float64).tobytes()
    api = B.oracle_api()
    h = api.align_create(draft, copy.deepcopy(events), P)
    try:
        api.score_alignments(h, len(events))
        refs = api.align_event_refs(h, len(events))
    finally:
        api.align_destroy(h)
    assert any(not np.array_equal(r, ev.ref_align) for r, ev in zip(refs, events))       # the call did realign
    K.check(got, K.want(draft, events, refs=refs), "after a realignment")
    assert all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events)) and pa.sequence == draft
    _, st = K.pa_of(B.OraclePSAlign, draft, events).AlignStats()
    assert int(got["n"].sum()) == int(st["n_fit"].sum()) > 0
    for name, (seq, ev, grp, G) in K.crafted().items():
        _, tb = K.pa_of(B.OraclePSAlign, seq, ev).KmerStats(grp, G, realign=False)
        _, st = K.pa_of(B.OraclePSAlign, seq, ev).AlignStats(realign=False)
        assert int(tb["n"].sum()) == int(st["n_fit"].sum()), name


def test_argument_errors():
    seq, events = K.crafted()["one_group"][:2]
    pa = K.pa_of(B.OraclePSAlign, seq, events)
    for bad in (dict(groups=[0, 1, 0]), dict(groups=[0, 1, 0, 2], n_groups=2), dict(groups=[0, -1, 0, 0]), dict(n_groups=0),
                dict(n_groups=257), dict(groups=[0, 0, 0, 256])):
        with pytest.raises(ValueError, match="kmer_stats"):
            pa.KmerStats(realign=False, **bad)
    grp, G = util.kmer_groups(events, [0, 255, 3, 3])
    assert G == 256 and grp.dtype == np.int32
    assert util.kmer_groups(events)[0].tolist() == [0, 1, 0, 1] and util.kmer_groups(events)[1] == 2
    assert util.kmer_groups([], None, None)[1] == 2 and util.kmer_groups([], [], None)[1] == 1
    _, tb = pa.KmerStats([0, 255, 3, 3], realign=False)
    assert tb.shape == (256, 1024) and tb["n"][255].any() and not tb["n"][254].any()
    with pytest.raises(ValueError, match="one grouping per region"):
        RegionBatch([pa], resident=False).KmerStats(groups=[[0] * 4, [0]], realign=False)
    with pytest.raises(ValueError, match="different numbers of groups"):
        RegionBatch([pa, K.pa_of(B.OraclePSAlign, seq, events)], resident=False).RefitKmers(groups=[[0, 0, 0, 0], [0, 1, 2, 0]])
    with pytest.raises(ValueError, match="no tables"):
        util.add_kmer_stats([])


# ---- the fits -------------------------------------------------------------------------------------------------------------------------
def _table(seq, events, groups=None, n_groups=None):
    return K.pa_of(B.OraclePSAlign, seq, events).KmerStats(groups, n_groups, realign=False)[1]


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert (err <= 1e-9).all(), (what, float(err.max()))


def test_fit_kmers_is_equivariant():
    """algebraic identities of the statistics, prior=0 and no limits in the way: no statistical bound to choose"""
    seq, events = K.true_region()
    E = len(events)
    one = [0] * E
    wide = dict(prior=0, mean_limit=1e9, var_limits=(0.0, 1e9), sd_limits=(0.0, 1e9))
    f0 = util.fit_kmers(_table(seq, events, one, 1), **wide)[0]
    ks = np.array(K.top_kmers(seq, 20))
    assert (f0.n[ks] >= 2).all() and not f0.kept[ks].any() and not f0.clamped.any()
    rng = np.random.default_rng(9921)
    d = rng.uniform(-2.0, 2.0, ks.size)
    moved = copy.deepcopy(events)
    for ev in moved:
        ev.model.level_mean = ev.model.level_mean.copy()
        ev.model.level_mean[ks] = ev.model.level_mean[ks] - d * ev.model.level_stdv[ks]
    f1 = util.fit_kmers(_table(seq, moved, one, 1), **wide)[0]
    _close(f1.dmean[ks], f0.dmean[ks] + d, "dmean rises by d_k")
    rest = np.setdiff1d(np.arange(1024), ks)
    assert f1.dmean[rest].tobytes() == f0.dmean[rest].tobytes() and f1.sd_scale.tobytes() == f0.sd_scale.tobytes()
    _close(f1.vscale[ks], f0.vscale[ks], "a shift leaves the variance alone")
    q = 1.25
    moved = copy.deepcopy(events)
    for ev in moved:
        ev.model.level_stdv = ev.model.level_stdv.copy()
        ev.model.level_stdv[ks] = ev.model.level_stdv[ks] / q
    f2 = util.fit_kmers(_table(seq, moved, one, 1), **wide)[0]
    _close(f2.vscale[ks], f0.vscale[ks] * q * q, "vscale is multiplied by q^2")
    _close(f2.dmean[ks], f0.dmean[ks] * q, "dmean is in units of level_stdv")
    a = 1.5
    moved = copy.deepcopy(events)
    for ev in moved:
        ev.model.sd_mean = ev.model.sd_mean / a
    t0, t3 = _table(seq, events, one, 1), _table(seq, moved, one, 1)
    f3 = util.fit_kmers(t3, **wide)[0]
    fitted = ~f0.kept
    _close(f3.sd_scale[fitted], f0.sd_scale[fitted] * a, "sd_scale is multiplied by a")
    s0, s3 = util.fit_scaling_sd(t0[0], a_limits=(0.0, 1e9), var_limits=(0.0, 1e9)), util.fit_scaling_sd(t3[0], a_limits=(0.0, 1e9), var_limits=(0.0, 1e9))
    assert s0.ok and s3.ok and s0.n == s3.n == int(t0["n"].sum())
    _close(s3.a, s0.a * a, "fit_scaling_sd's a is multiplied by a")


def _row(**cells):
    t = np.zeros(1024, dtype=_capi.KMER_STATS)
    for k, v in cells.items():
        t[k][:len(v)] = v
    return t


def test_shrinkage_clamps_and_flags():
    # k-mer 0: n = 8 levels whose residuals have mean 1 and variance 3 about it, spu / sp = 1.5; k-mer 1: one level; 2: none; 3: NaN
    t = _row(n=[8, 1, 0, 4], sz=[8.0, 0.5, 0.0, np.nan], szz=[32.0, 0.25, 0.0, 1.0], sp=[4.0, 1.0, 0.0, 1.0], spu=[6.0, 1.0, 0.0, 1.0], spv=[4.0, 1.0, 0.0, 1.0])
    f = util.fit_kmers(t, prior=8.0)
    assert (f.dmean[0], f.vscale[0], f.sd_scale[0]) == (0.5, 2.0, 1.25)                   # n = prior: halfway to (1, 3, 1.5)
    assert f.kept.tolist()[:4] == [False, False, True, True] and f.kept[4:].all() and not f.clamped.any() and f.n_fitted == 2
    assert (f.dmean[2:4] == 0).all() and (f.vscale[2:4] == 1).all() and (f.sd_scale[2:4] == 1).all()
    f = util.fit_kmers(t, prior=0.0)
    assert (f.dmean[0], f.vscale[0], f.sd_scale[0]) == (1.0, 3.0, 1.5) and (f.dmean[1], f.vscale[1]) == (0.5, 0.25) and f.clamped.tolist()[:2] == [False, True]      # (one level: variance 0, cut at the limit)
    f = util.fit_kmers(t, prior=0.0, min_count=2)
    assert f.kept.tolist()[:2] == [False, True] and f.dmean[1] == 0.0
    f = util.fit_kmers(t, prior=0.0, mean_limit=0.75, var_limits=(0.5, 2.5), sd_limits=(0.5, 1.25))
    assert (f.dmean[0], f.vscale[0], f.sd_scale[0]) == (0.75, 2.5, 1.25) and (f.dmean[1], f.vscale[1]) == (0.5, 0.5)
    assert f.clamped.tolist()[:4] == [True, True, False, False]
    two = util.fit_kmers(np.stack([t, t]), prior=8.0)
    assert len(two) == 2 and two[1].dmean[0] == 0.5
    pooled = util.add_kmer_stats([t, t, t])
    assert pooled["n"][0] == 24 and pooled["sz"][0] == 24.0 and pooled["spu"][0] == 18.0 and t["n"][0] == 8
    bad = util.fit_scaling_sd(t)
    assert tuple(bad)[:3] == (1.0, 1.0, False)                                            # a NaN-free row, but fewer than min_levels
    ok = util.fit_scaling_sd(_row(n=[60, 60], sp=[30.0, 30.0], spu=[33.0, 33.0], spv=[60.0, 60.0]))
    assert ok.ok and ok.a == 1.1 and ok.n == 120 and abs(ok.D - (120.0 - 3600.0 / 66.0) / 120.0) < 1e-15
    assert not util.fit_scaling_sd(_row(n=[60, 60], sp=[30.0, 30.0], spu=[33.0, 33.0], spv=[60.0, 60.0]), a_limits=(0.95, 1.05)).ok
    assert not util.fit_scaling_sd(_row(n=[60, 60], sp=[30.0, 30.0], spu=[33.0, 33.0], spv=[60.0, np.nan])).ok


def test_apply_and_a_second_fit():
    seq, events = K.true_region()
    E = len(events)
    one = [0] * E
    off = copy.deepcopy(events)
    for ev in off:                                                                        # a stdv channel that is off by a known factor
        ev.model.sd_mean = ev.model.sd_mean / 1.125
    free = dict(a_limits=(0.0, 1e9), var_limits=(0.0, 1e9))
    s = util.fit_scaling_sd(_table(seq, off, one, 1)[0], **free)
    assert s.ok and abs(s.a / util.fit_scaling_sd(_table(seq, events, one, 1)[0], **free).a - 1.125) < 1e-9
    fixed = copy.deepcopy(off)
    before = copy.deepcopy(off[0])
    for ev in fixed:
        util.apply_scaling_sd(ev, s.a, s.D)
    assert np.array_equal(fixed[0].model.sd_mean, before.model.sd_mean * s.a) and np.array_equal(fixed[0].model.sd_stdv, before.model.sd_stdv * (s.a ** 1.5 * s.D ** 0.5))
    assert np.array_equal(fixed[0].model.level_mean, before.model.level_mean) and np.array_equal(fixed[0].model.level_stdv, before.model.level_stdv)
    tb = util.kmer_stats_from_refs(K.states_of(seq), fixed, [ev.ref_align for ev in fixed], one, 1)      # (off the grid now: the numpy path)
    s2 = util.fit_scaling_sd(tb[0], **free)
    print("first fit %r, second fit %r" % (s, s2))
    assert abs(s2.a - 1.0) <= 1e-9 and abs(s2.D - 1.0) <= 1e-9
    only_a = copy.deepcopy(off)
    for ev in only_a:
        util.apply_scaling_sd(ev, s.a)
    s3 = util.fit_scaling_sd(util.kmer_stats_from_refs(K.states_of(seq), only_a, [ev.ref_align for ev in only_a], one, 1)[0], **free)
    assert abs(s3.a - 1.0) <= 1e-9 and abs(s3.D - s.D) <= 1e-9 * max(1.0, s.D)           # without D the deviance stays what it was
    # apply_kmers, a group per read (one model per fit): a second fit of the refitted models finds nothing left to move
    own = list(range(E))
    wide = dict(prior=0, min_count=2, mean_limit=1e9, var_limits=(0.0, 1e9), sd_limits=(0.0, 1e9))
    fits = util.fit_kmers(_table(seq, events, own, E), **wide)
    done = copy.deepcopy(events)
    lam0 = util.model_lambda(done[0].model.sd_mean, done[0].model.sd_stdv)
    for ev, f in zip(done, fits):
        util.apply_kmers(ev, f)
    _close(util.model_lambda(done[0].model.sd_mean, done[0].model.sd_stdv), lam0, "lambda stays where it was")
    assert np.array_equal(done[0].model.level_mean, events[0].model.level_mean + fits[0].dmean * events[0].model.level_stdv)
    assert np.array_equal(done[0].model.level_stdv, events[0].model.level_stdv * np.sqrt(fits[0].vscale))
    again = util.fit_kmers(util.kmer_stats_from_refs(K.states_of(seq), done, [ev.ref_align for ev in done], own, E), **wide)
    for f, f2 in zip(fits, again):
        sure = ~f.kept & (f.vscale >= 1e-3)
        assert sure.sum() > 50 and (f2.kept == f.kept).all()
        _close(f2.dmean[sure], 0.0 * f.dmean[sure], "no shift left")
        _close(f2.vscale[sure], 1.0 + 0.0 * f.dmean[sure], "no variance factor left")
        _close(f2.sd_scale[sure], 1.0 + 0.0 * f.dmean[sure], "no stdv-channel factor left")


def _models(events):
    return [tuple(np.asarray(getattr(ev.model, k)).tobytes() for k in ("level_mean", "level_stdv", "sd_mean", "sd_stdv")) for ev in events]


def test_refit_kmers_and_the_consensus_drivers():
    draft, events = synth.make_region(240, 6, 8841, B.oracle_swalign, P)[:2]
    events = K.quantised(events)
    pa = K.pa_of(B.OraclePSAlign, draft, events)
    fits = pa.RefitKmers()
    assert len(fits) == 2 and all(f.n_fitted > 0 for f in fits) and pa.sequence == draft
    _, tb = K.pa_of(B.OraclePSAlign, draft, events).KmerStats()
    want = copy.deepcopy(events)
    for ev in want:
        util.apply_kmers(ev, util.fit_kmers(tb)[1 if ev.model.complement else 0])
    assert _models(pa.events) == _models(want) and _models(pa.events) != _models(events)
    assert all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))
    for resident in (True, False):                                                        # the lock-step form, pooled and not
        pas = [K.pa_of(B.OraclePSAlign, draft, events), K.pa_of(B.OraclePSAlign, draft, events)]
        with RegionBatch(pas, resident=resident) as rb:
            each = rb.RefitKmers(pool=False)
        assert _models(pas[0].events) == _models(want) and _models(pas[1].events) == _models(want) and len(each) == 2
        pas = [K.pa_of(B.OraclePSAlign, draft, events), K.pa_of(B.OraclePSAlign, draft, events)]
        with RegionBatch(pas, resident=resident) as rb:
            pooled = rb.RefitKmers(pool=True)
        both = util.fit_kmers(util.add_kmer_stats([tb, tb]))
        assert pooled[0] is pooled[1] and all(p.dmean.tobytes() == b.dmean.tobytes() and (p.n == 2 * f.n).all() for p, b, f in zip(pooled[0], both, fits))
    runs = {}
    for key, kw in (("plain", {}), ("off", dict(refit_kmers=False)), ("on", dict(refit_kmers=True))):
        B.reset_rand()
        p1, log = K.pa_of(B.OraclePSAlign, draft, events), []
        res = consensus_region(p1, reps=1, log=log, **kw)
        runs[key] = (res, log, _models(p1.events))
    assert runs["off"] == runs["plain"] and consensus._refit_kmers_kw(False) is None and consensus._refit_kmers_kw(True) == {}
    res, log, models = runs["on"]
    assert log[0] == ("RefitKmers", sum(f.n_fitted for f in fits), draft) and log[1][0] == "Mutate:self" and models == _models(want)
    assert isinstance(res[0], str) and len(res[0]) > 100
    for key, kw in (("plain", {}), ("on", dict(refit_kmers={}))):
        pas, logs = [K.pa_of(B.OraclePSAlign, draft, events)], [[]]
        out = consensus_regions(pas, reps=1, logs=logs, **kw)
        assert out[0][0] == runs[key][0][0] and logs[0] == runs[key][1] and _models(pas[0].events) == runs[key][2]
