"""ps_posterior_stats on the CPU: util.posterior_from_emissions — the definition — against an explicit enumeration of all paths of
small lattices, against the oracle's max-plus tables (semiring='max'), its sum mode against bounds that follow from the recursion,
its counts against derivatives of logz; util.fit_transitions_soft; and the drivers (PosteriorStats, RefitTransitions(posterior=True),
consensus_region(refit_transitions={'posterior': True}), train(estimate='posterior')) on the oracle through the fallback path.

Bounds used here and where they come from:
  BRUTE_ULPS   64 units of 2^-63 (longdouble): an enumeration has at most 2 809 paths (pairwise sums: 12 roundings), the recursion
               nests at most n0 + C = 7 log-sums of at most 6 terms, each an exp, a sum and a log of about one rounding each, on either
               side: below 64 in all.  (Worst seen: 5.5.)
  K0           the max-mode tables against the oracle's debug_fill: only emission rounding could separate the two.  Measured on the
               CPU over every case: 0 — util.fill_emissions forms every emission bit for bit as the oracle does — so twice the worst
               value seen is 0 and the tables are asserted EQUAL (K0 = 0 in K0 2^-52 (n0 + C) max(1, |v|)).
  sum mode     F >= the max-plus tables up to the rounding of one log-sum per anti-diagonal (SUM_ULPS 2^-52 (n0 + C) max(1, |v|) with
               SUM_ULPS = 4: an exp, a sum of at most 7 terms and a log per level of nesting); score <= logz <= score +
               (n0 + C) log 7 + log n_cells: every (+) has at most 7 terms, so every cell is at most its max-plus value plus
               log 7 per anti-diagonal, and logz adds n_cells of them.
  derivatives  see test_counts_are_derivatives_of_logz."""
import copy
import math

import numpy as np
import pytest

import backends as B
import move_cases as M
import post_cases as PC
from poreseq_amd import _capi, consensus, synth, util
from poreseq_amd.batch import RegionBatch
from poreseq_amd.events import PSEvent

P = M.P0
LD = np.longdouble
BRUTE_ULPS = 64
SUM_ULPS = 4
RATE_KEYS = tuple(r + s for r in util.TRANSITION_RATES for s in ("_t", "_c"))
LIKS = (math.log(0.14), math.log(0.04), math.log(0.07), math.log(0.02))


def test_record_layout():
    assert _capi.EVENT_POSTERIOR.itemsize == 80
    assert [_capi.EVENT_POSTERIOR.fields[k][1] for k in ("n_cells", "logz", "e_extend")] == [16, 24, 72]
    assert {"ps_posterior_stats", "ps_batch_posterior_stats", "ps_debug_posterior"} <= _capi.OPTIONAL <= set(_capi.SYMBOLS)


def test_restatement_equals_the_enumeration_of_all_paths():
    rng = np.random.default_rng(8950)
    worst, n, most = 0.0, 0, 0
    for n0, bands, valid in PC.small_lattices():
        obs, mask, va = PC.small_arrays(n0, bands, valid, rng)
        logz, counts, npaths = PC.enumerate_paths(n0, bands, valid, obs, LIKS)
        res = util.posterior_from_emissions(obs, mask, va, *LIKS, dtype=LD)
        errs = [PC.rel_err(res.logz, logz)] + [PC.rel_err(res.counts[k], counts[k]) for k in PC.COUNTS]
        worst, n, most = max(worst, float(max(errs)) / 2.0 ** -63), n + 1, max(most, npaths)
        assert res.n_cells == sum(b - a + 1 for (a, b), v in zip(bands, valid) if v) and res.n_cols == sum(valid)
    print("%d lattices, at most %d paths, worst error %.1f units of 2^-63" % (n, most, worst))
    assert n == 5454 and worst <= BRUTE_ULPS


def test_a_lattice_written_by_hand():
    """one level, one column: M = 0 (+) lik_skip (+) obs (+) (lik_insert: ignore); no stay.  Two levels: the stay floor shows"""
    obs = np.array([[0.0, 0.0], [0.0, 1.5]])
    mask = np.ones((2, 2), dtype=bool)
    mask[0, 1] = False
    res = util.posterior_from_emissions(obs, mask, [False, True], *LIKS, levels=True)
    lsk, lst, lex, lin = LIKS
    z = 1.0 + math.exp(lsk) + math.exp(1.5) + math.exp(lin)
    assert abs(res.logz - math.log(z)) < 1e-15 and res.n_cells == 1 and res.n_cols == 1
    assert abs(res.counts["e_match"] - math.exp(1.5) / z) < 1e-15 and abs(res.counts["e_skip"] - math.exp(lsk) / z) < 1e-15
    assert abs(res.counts["e_ignore"] - math.exp(lin) / z) < 1e-15 and res.counts["e_stay"] == 0 and res.counts["e_insert"] == 0
    assert abs(res.emit[0] - math.exp(1.5) / z) < 1e-15 and res.col[0] == 1.0 and np.isneginf(res.stay[1, 1])
    assert util.posterior_from_emissions(obs, mask, [False, True], *LIKS, semiring="max").stay[1, 1] == -1e300
    dead = util.posterior_from_emissions(obs, mask, [False, False], *LIKS, levels=True)
    assert dead.logz == 0 and dead.n_cells == 0 and not any(dead.counts.values()) and dead.main[1, 1] == 0 and np.isnan(dead.col[0])
    with pytest.raises(ValueError):
        util.posterior_from_emissions(obs, mask, [False, True], *LIKS, semiring="min")


@pytest.mark.parametrize("name", PC.NAMES)
def test_max_mode_is_the_oracles_lattice(name):
    worst = 0.0
    for e in range(PC.n_events(name)):
        main, stay = PC.oracle_tables(name, e)
        res = PC.restated(name, e, "max")
        n0, C = PC.lattice(name, e)[4:]
        assert np.array_equal(np.isnan(res.main), np.isnan(main)) and np.array_equal(np.isnan(res.stay), np.isnan(stay)), (name, e)
        if main.size:
            worst = max(worst, float(max(PC.rel_err(res.main, main).max(), PC.rel_err(res.stay, stay).max())) / (PC.EPS * max(1, n0 + C)))
        with np.errstate(invalid="ignore"):
            score = max(0.0, float(np.nanmax(np.where(np.isnan(main[:, 1:]), -np.inf, main[:, 1:])))) if C else 0.0
        assert float(res.logz) == score, (name, e)
    print("%s: worst |restatement - oracle| / (2^-52 (n0 + C) max(1, |v|)) = %g" % (name, worst))
    assert worst == 0.0


def test_the_n_cases_have_columns_without_a_state():
    for name, want in ((PC.N_COLUMN, 1), (PC.N_RUN, 5)):
        valid = PC.lattice(name, 0)[2]
        mask = PC.lattice(name, 0)[1]
        dead = np.nonzero(~valid[1:])[0] + 1
        assert dead.size == want and np.all(np.diff(dead) == 1) and mask[:, dead].sum() >= 3 * want
        assert PC.restated(name, 0).n_cols == valid.size - 1 - want
        assert np.all(PC.restated(name, 0).main[:, dead][mask[:, dead]] == 0)


@pytest.mark.parametrize("name", PC.NAMES)
def test_sum_mode_dominates_the_best_path_and_is_bounded_by_it(name):
    for e in range(PC.n_events(name)):
        mx, sm = PC.restated(name, e, "max"), PC.restated(name, e, "sum")
        n0, C = PC.lattice(name, e)[4:]
        live = ~np.isnan(mx.main)
        slack = SUM_ULPS * PC.EPS * max(1, n0 + C)
        for a, b in ((sm.main, mx.main), (sm.stay, mx.stay)):
            fin = live & np.isfinite(b) & (b > -1e299)
            assert np.all(a[fin] >= b[fin] - slack * np.maximum(1.0, np.abs(b[fin]))), (name, e)
        assert np.array_equal(np.isneginf(sm.stay), mx.stay == -1e300)
        score, logz = float(mx.logz), float(sm.logz)
        if sm.n_cells == 0:
            assert PC.inert(name, e) and logz == 0.0 and not any(sm.counts.values())
            continue
        assert score <= logz <= score + (n0 + C) * math.log(7.0) + math.log(sm.n_cells), (name, e, score, logz)
        assert all(v >= 0 for v in sm.counts.values())
        ld = PC.restated(name, e, "sum", LD)
        assert float(PC.rel_err(sm.logz, ld.logz)) <= 64 * PC.EPS * (n0 + C)


DERIV = (("narrow", 0), ("narrow", 3), (PC.N_RUN, 2), ("column0", 0), ("untouched", 0), ("wide", 1))


@pytest.mark.parametrize("name,e", DERIV)
def test_counts_are_derivatives_of_logz(name, e):
    """logz(x) = log sum over paths of exp(w_p + x n_p), n_p the number of times path p uses the moves the parameter enters: the
    first derivative at 0 is the posterior mean of n — the expected count — and the third is its third cumulant, |k3| <= N^3 for
    0 <= n_p <= N (N = C for skips, one per column at most; N = n0 for the others, each of which consumes a level).  A central
    difference with step h is off by at most h^2 N^3 / 6 from truncation and d / h from rounding, d the absolute error of one logz:
    d <= 16 (n0 + C) 2^-64 max(1, logz) in longdouble (at most 16 roundings per level of nesting).  h = (6 d / N^3)^(1/3) balances
    the two; the tolerance is their sum at that h, plus the same d-sized relative error for the count itself."""
    obs, mask, valid, lk, n0, C = PC.lattice(name, e)
    ref = PC.restated(name, e, "sum", LD)
    d = 16.0 * (n0 + C) * 2.0 ** -64 * max(1.0, float(ref.logz))

    def logz(dlk=(0, 0, 0, 0), dobs=0):
        with np.errstate(invalid="ignore"):
            o = np.asarray(obs, dtype=LD) + LD(dobs)
        liks = [LD(v) + LD(x) for v, x in zip(lk, dlk)]
        return util.posterior_from_emissions(o, mask, valid, *liks, dtype=LD, counts=False).logz

    c = ref.counts
    emitting = c["e_match"] + c["e_stay"] + c["e_extend"]
    wants = (("lik_skip", (1, 0, 0, 0), 0, c["e_skip"], C), ("lik_insert", (0, 0, 0, 1), 0, c["e_insert"] + c["e_ignore"], n0),
             ("lik_stay", (0, 1, 0, 0), 0, c["e_stay"], n0), ("lik_extend", (0, 0, 1, 0), 0, c["e_extend"], n0),
             ("lik_offset", (0, 0, 0, 0), 1, emitting, n0))
    for what, dlk, dobs, want, N in wants:
        h = (6.0 * d / N ** 3) ** (1.0 / 3.0)
        tol = h * h * N ** 3 / 6.0 + d / h + 16.0 * (n0 + C) * 2.0 ** -64 * max(1.0, float(want))
        got = (logz(tuple(h * x for x in dlk), h * dobs) - logz(tuple(-h * x for x in dlk), -h * dobs)) / LD(2 * h)
        print("%s[%d] d logz / d %s = %.12g, expected count %.12g, |difference| %.3g, tolerance %.3g (h = %.3g)"
              % (name, e, what, float(got), float(want), abs(float(got - want)), tol, h))
        assert abs(float(got - want)) <= tol, (name, e, what)
    assert abs(float(np.sum(ref.emit) - emitting)) <= 64 * 2.0 ** -63 * n0 * max(1.0, float(emitting))
    with np.errstate(invalid="ignore"):
        on = ref.emit > 0
    assert np.all(np.isnan(ref.col[~on])) and np.all((ref.col[on] >= 1) & (ref.col[on] <= C))


# ---- fit_transitions_soft ------------------------------------------------------------------------------------------------------------
def _pair(rows):
    mv, ps = np.zeros(len(rows), dtype=_capi.EVENT_MOVES), np.zeros(len(rows), dtype=_capi.EVENT_POSTERIOR)
    for k, r in enumerate(rows):
        for a, b in zip(("n_match", "n_ignore", "n_insert", "n_stay", "n_extend", "n_skip_cols"),
                        ("e_match", "e_ignore", "e_insert", "e_stay", "e_extend", "e_skip")):
            mv[a][k], ps[b][k] = r[a], float(r[a])
    return mv, ps


def test_soft_fit_on_integer_counts_is_the_fit_of_the_counts():
    rows = [dict(n_match=60, n_ignore=4, n_insert=6, n_stay=10, n_extend=20, n_skip_cols=16),
            dict(n_match=40, n_ignore=0, n_insert=0, n_stay=10, n_extend=0, n_skip_cols=0),
            dict(n_match=90, n_ignore=5, n_insert=5, n_stay=0, n_extend=0, n_skip_cols=5)]
    mv, ps = _pair(rows)
    for kw in (dict(prior=0.0, lo=0.0, hi=1.0), dict(), dict(prior=80.0, lo=0.15)):
        a, b = util.fit_transitions(mv, [0, 0, 1], P, **kw), util.fit_transitions_soft(ps, [0, 0, 1], P, **kw)
        assert a.params == b.params and a.rates == b.rates and a.flags == b.flags
        assert {k: (float(n), float(d)) for k, (n, d) in a.counts.items()} == b.counts
    ps["e_stay"][0] = 10.5
    soft = util.fit_transitions_soft(ps, [0, 0, 1], P, prior=0.0, lo=0.0, hi=1.0)
    assert soft.params["stay_t"] == 20.5 / 150.5 and soft.params["extend_t"] == 20 / 40.5
    empty = util.fit_transitions_soft(ps[:0], [], P)
    assert empty.params == P and set(empty.flags.values()) == {"empty"}
    with pytest.raises(ValueError):
        util.fit_transitions_soft(ps, [0, 1], P)


P20 = dict(P, realign_width=20.0)


def _simulated(p_stay, p_skip, seed):
    rng = np.random.default_rng(seed)
    seq = synth.random_sequence(rng, 300)
    events = []
    for _ in range(4):
        model = synth.make_model(rng, False)
        mean, stdv, ral = synth.simulate_event(rng, synth.states_of(seq), model, p_stay=p_stay, p_skip=p_skip)
        ev = PSEvent(mean, stdv, ral, np.zeros(mean.size), sequence=seq, model=model)
        ev.setparams(P20)
        events.append(ev)
    return B.make_pa(B.OraclePSAlign, seq, events, P20)


def test_soft_fit_orders_two_simulations_as_they_were_made():
    fits = []
    for k, (p_stay, p_skip) in enumerate(((0.15, 0.02), (0.02, 0.20))):
        rec = _simulated(p_stay, p_skip, 8930 + k).PosteriorStats()
        fits.append(util.fit_transitions_soft(rec, [0] * len(rec), P20))
        print("simulated stay %.2f skip %.2f: fitted stay_t %.4f skip_t %.4f" % (p_stay, p_skip, fits[-1].params["stay_t"], fits[-1].params["skip_t"]))
    assert fits[0].params["stay_t"] > fits[1].params["stay_t"] and fits[0].params["skip_t"] < fits[1].params["skip_t"]


# ---- the drivers on the oracle, through the fallback ------------------------------------------------------------------------------------
def _state(events):
    return [(ev.mean.tobytes(), ev.ref_align.tobytes(), ev.ref_like.tobytes(), ev.model.level_mean.tobytes(), ev.model.level_stdv.tobytes(),
             ev.model.sd_mean.tobytes(), ev.model.sd_stdv.tobytes()) for ev in events]


def _rates(events):
    return [tuple(float(getattr(ev.model, "prob_" + r)) for r in util.TRANSITION_RATES) for ev in events]


@pytest.mark.parametrize("name", ("narrow", "all_unaligned", "empty_read", PC.N_RUN))
def test_posterior_stats_through_the_fallback(name):
    draft, events, par = PC.case(name)
    pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
    assert "ps_posterior_stats" in B.oracle_api().missing
    rec, emit, col = pa.PosteriorStats(levels=True)
    assert rec.dtype == _capi.EVENT_POSTERIOR and rec.shape == (len(events),)
    for e, ev in enumerate(events):
        want = PC.restated(name, e)
        assert int(rec["n_levels"][e]) == ev.mean.size and int(rec["inert"][e]) == int(PC.inert(name, e))
        assert int(rec["n_cells"][e]) == want.n_cells and float(rec["logz"][e]) == float(want.logz)
        assert int(rec["n_cols"][e]) == (0 if PC.inert(name, e) else want.n_cols)
        assert all(float(rec[k][e]) == float(want.counts[k]) for k in PC.COUNTS)
        assert emit[e].tobytes() == np.asarray(want.emit, dtype=np.float64).tobytes() and col[e].tobytes() == np.asarray(want.col).tobytes()
    assert _state(pa.events) == _state(events) and pa.sequence == draft
    assert pa.PosteriorStats().tobytes() == rec.tobytes()
    with RegionBatch([pa, B.make_pa(B.OraclePSAlign, *M.case(M.NO_EVENTS))], resident=False) as rb:
        both = rb.PosteriorStats(levels=True)
    assert both[0][0].tobytes() == rec.tobytes() and M.same(both[0][1], emit) and both[1][0].shape == (0,) and both[1][1] == []


def test_posterior_refit_changes_the_rates_and_nothing_else():
    draft, events, par = M.case("narrow")
    pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
    rec = pa.PosteriorStats()
    want = util.fit_transitions_soft(rec, util.strand_groups(events), par)
    fit = pa.RefitTransitions(posterior=True)
    assert fit.params == want.params and fit.flags == want.flags and fit.logz == [math.fsum(rec["logz"].tolist())]
    assert _state(pa.events) == _state(events) and pa.sequence == draft and pa.params == par
    assert _rates(pa.events) != _rates(events)
    # two rounds: the second starts from the first one's rates, and its logz is that of the events as the first round left them
    two = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
    fit2 = two.RefitTransitions(posterior=True, iters=2)
    again = util.fit_transitions_soft(pa.PosteriorStats(), util.strand_groups(events), fit.params)
    assert len(fit2.logz) == 2 and fit2.logz[0] == fit.logz[0] and fit2.logz[1] != fit2.logz[0]
    assert fit2.params == again.params and fit2.params != fit.params
    assert pa.RefitTransitions().logz is None                                             # the best-path fit: as it was
    with pytest.raises(ValueError):
        two.RefitTransitions(posterior=True, iters=0)
    # lock-step, pooled over two regions and region by region
    regs = [M.case("narrow"), PC.case(PC.N_COLUMN)]
    pas = [B.make_pa(B.OraclePSAlign, d, copy.deepcopy(ev), p) for d, ev, p in regs]
    with RegionBatch(pas) as rb:
        recs = rb.PosteriorStats()
        fits = rb.RefitTransitions(pool=True, params=P, posterior=True)
    pooled = util.fit_transitions_soft(np.concatenate(recs), [g for _, ev, _ in regs for g in util.strand_groups(ev)], P)
    assert fits[0] is fits[1] and fits[0].params == pooled.params
    assert all(_state(pa.events) == _state(ev) for pa, (_, ev, _) in zip(pas, regs))
    pas = [B.make_pa(B.OraclePSAlign, d, copy.deepcopy(ev), p) for d, ev, p in regs]
    with RegionBatch(pas) as rb:
        own = rb.RefitTransitions(pool=False, posterior=True)
    assert own[0].params == fit.params and own[1].params != own[0].params


P20S = dict(P, realign_width=20.0)


def test_consensus_region_with_the_posterior_refit():
    draft, events, _ = synth.make_region(220, 5, 8940, B.oracle_swalign, P20S)
    runs = {}
    for key, kw in (("plain", {}), ("path", dict(refit_transitions=True)), ("post", dict(refit_transitions=dict(posterior=True))),
                    ("post2", dict(refit_transitions=dict(posterior=True, iters=2)))):
        B.reset_rand()
        pa, log = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P20S), []
        res = consensus.consensus_region(pa, reps=1, log=log, **kw)
        runs[key] = (res, log, _rates(pa.events))
    assert runs["plain"][2] == _rates(events)
    assert runs["post"][1][0] == ("RefitTransitions", 8, draft) and [c for c, _, _ in runs["post"][1][1:]] == [c for c, _, _ in runs["plain"][1]]
    assert len({tuple(runs[k][2]) for k in runs}) == 4
    fit = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P20S).RefitTransitions(posterior=True)
    assert runs["post"][2][0] == tuple(fit.params[r + "_t"] for r in util.TRANSITION_RATES)
    B.reset_rand()
    pas, logs = [B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P20S)], [[]]
    res = consensus.consensus_regions(pas, reps=1, logs=logs, refit_transitions=dict(posterior=True))
    assert res[0] == runs["post"][0] and logs[0] == runs["post"][1] and _rates(pas[0].events) == runs["post"][2]


def test_train_starts_from_the_posterior_estimate(monkeypatch):
    draft, events, truth = synth.make_region(220, 5, 8941, B.oracle_swalign, P20S)
    seen = []

    def make_pa(p):
        evs = copy.deepcopy(events)
        for e in evs:
            e.setparams(p)
        return B.make_pa(B.OraclePSAlign, draft, evs, p)

    def one_candidate(params):
        seen.append(dict(params))
        return [dict(params)]

    monkeypatch.setattr(util, "VaryParams", one_candidate)
    B.reset_rand()
    best, _ = consensus.train(make_pa, dict(P20S), truth, iters=1, reps=1, estimate='posterior')
    fit = make_pa(P20S).RefitTransitions(params=P20S, posterior=True)
    path = make_pa(P20S).RefitTransitions(params=P20S)
    assert seen[0] == fit.params and best == fit.params and fit.params != path.params
    assert {k: v for k, v in seen[0].items() if k not in RATE_KEYS} == {k: v for k, v in P20S.items() if k not in RATE_KEYS}
