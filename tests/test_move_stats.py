"""ps_move_stats on the CPU: util.moves_from_tables — the definition — against the backtrace of the oracle and, where it is built,
of the live reference (the ref_align / ref_like their ScoreEvents leaves, bit for bit, on every case of move_cases); what each
case family is there for; the invariants of include/poreseq_hip.h; util.fit_transitions; and the drivers (MoveStats,
RefitTransitions, consensus_region(refit_transitions=True), train(estimate=True)) on the oracle through the fallback path."""
import copy

import numpy as np
import pytest

import backends as B
import move_cases as M
from poreseq_amd import _capi, consensus, synth, util
from poreseq_amd.batch import RegionBatch
from poreseq_amd.events import PSEvent

P = M.P0
RATE_KEYS = tuple(r + s for r in util.TRANSITION_RATES for s in ("_t", "_c"))


def test_record_layout():
    assert _capi.EVENT_MOVES.itemsize == 64 and _capi.EVENT_MOVES.names == M.INTS
    assert _capi.EVENT_MOVES.fields["n_skip_cols"][1] == 56
    assert {"ps_move_stats", "ps_batch_move_stats"} <= set(_capi.SYMBOLS) and {"ps_move_stats", "ps_batch_move_stats"} <= _capi.OPTIONAL


def test_walk_of_a_table_written_by_hand():
    """3 levels, 5 columns; the path, from the best cell (3, 5): MATCH to (2, 4), a skip to (2, 3), the main matrix' STAY hands over to
    the stay matrix, whose STAY records level 2 and returns to the main matrix on (1, 3), two skips to (1, 1), INSERT records level
    1 and the walk stops on row 0"""
    nan = float("nan")
    main = np.full((4, 6), nan)
    stay = np.full((4, 6), nan)
    sm, ss = np.zeros((4, 6), dtype=np.uint8), np.zeros((4, 6), dtype=np.uint8)
    main[0, :] = 0.0
    for (i, j), (v, s) in {(3, 5): (9.0, 1), (2, 4): (7.0, 0), (2, 3): (6.5, 4), (1, 3): (4.0, 0), (1, 2): (3.0, 0), (1, 1): (2.0, 2),
                           (3, 4): (8.0, 1), (2, 5): (1.0, 255)}.items():      # (the last two: cells off the path)
        main[i, j], sm[i, j] = v, s
    stay[2, 3], ss[2, 3] = 6.5, 4
    rec, step, col, ra, rl = util.moves_from_tables(main, stay, sm, ss)
    assert M.as_dict(rec) == dict(n_levels=3, inert=0, top_level=3, top_col=5, low_level=1, low_col=1, end_kind=0, n_match=1, n_ignore=0,
                                  n_insert=1, n_stay=1, n_extend=0, n_skip_runs=2, max_skip=2, n_skip_cols=3)
    assert step.tolist() == [2, 4, 1] and col.tolist() == [1, 3, 5]
    assert ra.tolist() == [-1.0, 3.0, 5.0] and rl.tolist() == [2.0, 6.5, 9.0]
    # the first maximum: smallest column, then row
    main[2, 2], sm[2, 2] = 9.0, 255
    rec = util.moves_from_tables(main, stay, sm, ss)[0]
    assert (int(rec["top_level"]), int(rec["top_col"]), int(rec["low_level"]), int(rec["low_col"]), int(rec["end_kind"])) == (2, 2, 0, 2, 1)
    # no score > 0: nothing is walked
    rec, step, col, ra, rl = util.moves_from_tables(np.where(main > 0, -1.0, main), stay, sm, ss)
    assert not any(int(rec[k]) for k in M.INTS if k != "n_levels") and not step.any() and not ra.any()


@pytest.mark.parametrize("name", M.NAMES)
def test_restated_walk_leaves_the_oracles_refs(name):
    walk = M.oracle_walk(name)
    scores, ras, rls = M.oracle_scored(name)
    assert M.same([w[3] for w in walk], ras) and M.same([w[4] for w in walk], rls)
    assert any(w[0]["top_level"] > 0 for w in walk)
    for w, sc in zip(walk, scores.tolist()):                # the score of an event is that of the cell the walk starts from
        assert (sc > 0) == (w[0]["top_level"] > 0)
        if w[0]["top_level"]:
            assert w[4][w[0]["top_level"] - 1] == sc or w[0]["low_level"] == 0


@pytest.mark.skipif(not B.have_ref(), reason="the reference build is not here")
@pytest.mark.parametrize("name", M.NAMES)
def test_restated_walk_leaves_the_references_refs(name):
    api = B.ref_api()
    walk = M.oracle_walk(name, api)
    scores, ras, rls = M.scored(api, name)
    assert M.same([w[3] for w in walk], ras) and M.same([w[4] for w in walk], rls)
    want = M.oracle_walk(name)
    assert [w[0] for w in walk] == [w[0] for w in want]
    assert M.same([w[1] for w in walk], [w[1] for w in want]) and M.same([w[2] for w in walk], [w[2] for w in want])


@pytest.mark.parametrize("name", sorted(M.REACH))
def test_families_reach_what_they_are_there_for(name):
    assert M.REACH[name](M.oracle_walk(name)), [w[0] for w in M.oracle_walk(name)]


def test_cases_cover_the_tile_edges_and_every_branch():
    recs = [w[0] for name in M.NAMES for w in M.oracle_walk(name)]
    assert set(M.LEVEL_COUNTS) <= set(r["n_levels"] for r in recs)
    live = [r for r in recs if not r["inert"]]
    for k in M.RECORDED:
        assert any(r[k] > 0 for r in live), k
    assert any(r["max_skip"] >= 2 for r in live) and any(r["inert"] for r in recs)
    assert {0, 1} == set(r["end_kind"] for r in live if r["low_level"] > 1)      # both ends, below a recorded level
    assert any(r["top_level"] > 0 and r["low_level"] == 0 for r in live)          # a walk that records nothing
    assert any(r["top_level"] > 256 and r["low_level"] == 1 for r in live)        # a path through more than one tile


@pytest.mark.parametrize("name", M.NAMES)
def test_invariants_against_the_census_of_the_refs(name):
    draft, events, _ = M.case(name)
    states = B.oracle_api().seq_to_states(draft)
    for e, (ev, w) in enumerate(zip(events, M.oracle_walk(name))):
        stats = util.align_stats_from_refs(states, ev.mean, w[3], ev.model.level_mean, ev.model.level_stdv)
        M.check_invariants(w[0], stats, "%s event %d" % (name, e))
        rec, step, col = w[0], w[1], w[2]
        on = step != 0
        assert int(on.sum()) == sum(rec[k] for k in M.RECORDED) and not col[~on].any()
        if on.any():
            idx = np.flatnonzero(on)
            assert idx[0] == rec["low_level"] - 1 and idx[-1] == rec["top_level"] - 1 and idx.size == idx[-1] - idx[0] + 1
            assert [int((step == c).sum()) for c in (1, 3, 2, 4, 5)] == [rec[k] for k in M.RECORDED]
            aligned = np.isin(step, (1, 4, 5))
            assert np.array_equal(col[aligned].astype(np.float64), w[3][aligned]) and (w[3][on & ~aligned] == -1).all()
            # the header's skip rule, from the per-level arrays
            dj = np.isin(step, (1, 3)).astype(np.int64)
            c = col.astype(np.int64)
            gaps = [rec["top_col"] - c[idx[-1]]] + [int(c[i + 1] - dj[i + 1] - c[i]) for i in idx[:-1]] + [int(c[idx[0]] - dj[idx[0]] - rec["low_col"])]
            assert min(gaps) >= 0 and sum(gaps) == rec["n_skip_cols"] and max(gaps) == rec["max_skip"]
            assert sum(1 for g in gaps if g > 0) == rec["n_skip_runs"]


# ---- fit_transitions ------------------------------------------------------------------------------------------------------------------
def _records(rows):
    rec = np.zeros(len(rows), dtype=_capi.EVENT_MOVES)
    for r, row in zip(rec, rows):
        for k, v in row.items():
            r[k] = v
    return rec


def test_fit_in_closed_form():
    rec = _records([dict(n_match=60, n_ignore=4, n_insert=6, n_stay=10, n_extend=20, n_skip_cols=16),
                    dict(n_match=40, n_ignore=0, n_insert=0, n_stay=10, n_extend=0, n_skip_cols=0),
                    dict(n_match=90, n_ignore=5, n_insert=5, n_stay=0, n_extend=0, n_skip_cols=5)])
    fit = util.fit_transitions(rec, [0, 0, 1], P, prior=0.0, lo=0.0, hi=1.0)
    # template: L = 150, Ccol = 60 + 4 + 40 + 16 = 120
    assert fit.params["skip_t"] == 16 / 120 and fit.params["stay_t"] == 20 / 150 and fit.params["extend_t"] == 20 / 40
    assert fit.params["insert_t"] == 10 / 150
    # complement: L = 100, Ccol = 100; no stay to extend
    assert fit.params["skip_c"] == 5 / 100 and fit.params["stay_c"] == 0.0 and fit.params["insert_c"] == 10 / 100
    assert fit.params["extend_c"] == P["extend_c"] and fit.flags == {"extend_c": "empty"} and not fit.ok
    assert fit.counts["skip_t"] == (16, 120) and fit.counts["extend_c"] == (0, 0)
    assert {k: v for k, v in fit.params.items() if k not in RATE_KEYS} == {k: v for k, v in P.items() if k not in RATE_KEYS}
    assert set(fit.rates) == set(RATE_KEYS)


def test_fit_shrinks_clamps_and_flags():
    rec = _records([dict(n_match=60, n_ignore=4, n_insert=6, n_stay=10, n_extend=20, n_skip_cols=16)])
    fit = util.fit_transitions(rec, [0], P, prior=80.0, lo=0.0, hi=1.0)
    assert fit.params["skip_t"] == (16 + 80.0 * P["skip_t"]) / 160.0      # halfway between 16 / 80 and the given rate at prior = Ccol = 80
    assert fit.params["stay_t"] == (10 + 80.0 * P["stay_t"]) / (100 + 80.0)
    for k in ("skip", "stay", "extend", "insert"):                                         # an empty group keeps what it had
        assert fit.params[k + "_c"] == P[k + "_c"] and fit.flags[k + "_c"] == "empty"
    huge = util.fit_transitions(rec, [0], P, prior=1e12)
    assert all(abs(huge.params[k] - P[k]) < 1e-9 for k in RATE_KEYS)
    cl = util.fit_transitions(rec, [0], P, prior=0.0, lo=0.15, hi=0.5)
    assert cl.params["skip_t"] == 16 / 80 and "skip_t" not in cl.flags                                              # 0.2: inside
    assert cl.params["stay_t"] == 0.15 and cl.rates["stay_t"] == 10 / 100 and cl.flags["stay_t"] == "clamped"       # 0.1 < lo
    assert cl.params["extend_t"] == 0.5 and cl.rates["extend_t"] == 20 / 30 and cl.flags["extend_t"] == "clamped"   # 0.667 > hi
    assert cl.params["insert_t"] == 0.15 and cl.flags["insert_t"] == "clamped" and not cl.ok
    none = util.fit_transitions(_records([]), [], P)
    assert all(none.params[k] == P[k] for k in RATE_KEYS) and set(none.flags.values()) == {"empty"} and len(none.flags) == 8
    inert = util.fit_transitions(_records([dict(n_levels=200, inert=1)]), [0], P)
    assert inert.flags == none.flags and inert.params == none.params
    bare = util.fit_transitions(rec, [0], {}, prior=10.0)                                   # what params lacks: the defaults
    assert bare.params["skip_t"] == (16 + 10.0 * util.DEFAULT_PARAMS["skip_t"]) / 90.0
    with pytest.raises(ValueError):
        util.fit_transitions(rec, [0, 1], P)
    with pytest.raises(ValueError):
        util.fit_transitions(rec, [2], P)
    with pytest.raises(ValueError):
        util.fit_transitions(rec, [0], P, lo=0.5, hi=0.1)


def _simulated(p_stay, p_skip, seed):
    rng = np.random.default_rng(seed)
    seq = synth.random_sequence(rng, 300)
    events = []
    for _ in range(4):
        model = synth.make_model(rng, False)
        mean, stdv, ral = synth.simulate_event(rng, synth.states_of(seq), model, p_stay=p_stay, p_skip=p_skip)
        ev = PSEvent(mean, stdv, ral, np.zeros(mean.size), sequence=seq, model=model)
        ev.setparams(P)
        events.append(ev)
    return B.make_pa(B.OraclePSAlign, seq, events, P)


def test_fit_orders_two_simulations_as_they_were_made():
    fits = []
    for k, (p_stay, p_skip) in enumerate(((0.15, 0.02), (0.02, 0.20))):
        _, rec = _simulated(p_stay, p_skip, 8930 + k).MoveStats()
        fits.append(util.fit_transitions(rec, [0] * len(rec), P))
        print("simulated stay %.2f skip %.2f: fitted stay_t %.4f skip_t %.4f" % (p_stay, p_skip, fits[-1].params["stay_t"], fits[-1].params["skip_t"]))
    assert fits[0].params["stay_t"] > fits[1].params["stay_t"] and fits[0].params["skip_t"] < fits[1].params["skip_t"]


# ---- the drivers on the oracle, through the fallback ------------------------------------------------------------------------------------
def _state(events):
    return [(ev.mean.tobytes(), ev.ref_align.tobytes(), ev.ref_like.tobytes(), ev.model.level_mean.tobytes(), ev.model.level_stdv.tobytes(),
             ev.model.sd_mean.tobytes(), ev.model.sd_stdv.tobytes()) for ev in events]


def _rates(events):
    return [tuple(float(getattr(ev.model, "prob_" + r)) for r in util.TRANSITION_RATES) for ev in events]


@pytest.mark.parametrize("name", ("narrow", "all_unaligned", "empty_read", "poor"))
def test_move_stats_through_the_fallback(name):
    draft, events, par = M.case(name)
    pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
    assert "ps_move_stats" in B.oracle_api().missing
    scores, rec, step, col = pa.MoveStats(levels=True)
    walk = M.oracle_walk(name)
    M.check_records(rec, [w[0] for w in walk], name)
    assert M.same(step, [w[1] for w in walk]) and M.same(col, [w[2] for w in walk])
    assert scores.tobytes() == M.oracle_scored(name)[0].tobytes() == np.asarray(pa.ScoreEvents(), dtype=np.float64).tobytes()
    assert _state(pa.events) == _state(events) and pa.sequence == draft
    s2, r2 = pa.MoveStats()
    assert s2.tobytes() == scores.tobytes() and r2.tobytes() == rec.tobytes()
    with RegionBatch([pa, B.make_pa(B.OraclePSAlign, *M.case(M.NO_EVENTS))], resident=False) as rb:
        both = rb.MoveStats(levels=True)
    assert both[0][1].tobytes() == rec.tobytes() and M.same(both[0][2], step) and both[1][1].shape == (0,) and both[1][2] == []


def test_refit_transitions_changes_the_rates_and_nothing_else():
    draft, events, par = M.case("wide")
    pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
    _, rec = pa.MoveStats()
    want = util.fit_transitions(rec, util.strand_groups(events), par)
    fit = pa.RefitTransitions()
    assert fit.params == want.params and fit.flags == want.flags and fit.ok
    assert _state(pa.events) == _state(events) and pa.sequence == draft and pa.params == par
    assert _rates(pa.events) != _rates(events)
    for ev in pa.events:
        suf = "_c" if ev.model.complement else "_t"
        assert _rates([ev])[0] == tuple(fit.params[r + suf] for r in util.TRANSITION_RATES)
    # lock-step, pooled over two regions and region by region
    regs = [M.case("wide"), M.case("narrow")]
    pas = [B.make_pa(B.OraclePSAlign, d, copy.deepcopy(ev), p) for d, ev, p in regs]
    with RegionBatch(pas) as rb:
        recs = [r for _, r in rb.MoveStats()]
        fits = rb.RefitTransitions(pool=True, params=P)
    pooled = util.fit_transitions(np.concatenate(recs), [g for _, ev, _ in regs for g in util.strand_groups(ev)], P)
    assert fits[0] is fits[1] and fits[0].params == pooled.params
    assert all(_state(pa.events) == _state(ev) for pa, (_, ev, _) in zip(pas, regs))
    pas = [B.make_pa(B.OraclePSAlign, d, copy.deepcopy(ev), p) for d, ev, p in regs]
    with RegionBatch(pas) as rb:
        own = rb.RefitTransitions(pool=False)
    assert own[0].params == fit.params and own[1].params != own[0].params


def test_consensus_region_with_and_without_the_refit():
    draft, events, _ = synth.make_region(220, 5, 8940, B.oracle_swalign, P)
    runs = {}
    for key, kw in (("plain", {}), ("off", dict(refit_transitions=False)), ("on", dict(refit_transitions=True)),
                    ("kw", dict(refit_transitions=dict(prior=0.0)))):
        B.reset_rand()
        pa, log = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P), []
        res = consensus.consensus_region(pa, reps=1, log=log, **kw)
        runs[key] = (res, log, _rates(pa.events))
    assert runs["off"] == runs["plain"] and runs["plain"][2] == _rates(events)
    assert runs["on"][1][0] == ("RefitTransitions", 8, draft) and [c for c, _, _ in runs["on"][1][1:]] == [c for c, _, _ in runs["plain"][1]]
    assert runs["on"][2] != runs["plain"][2] and runs["kw"][2] != runs["on"][2]
    fit = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P).RefitTransitions()
    assert runs["on"][2][0] == tuple(fit.params[r + "_t"] for r in util.TRANSITION_RATES)
    B.reset_rand()
    pas, logs = [B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P)], [[]]
    res = consensus.consensus_regions(pas, reps=1, logs=logs, refit_transitions=True)
    assert res[0] == runs["on"][0] and logs[0] == runs["on"][1] and _rates(pas[0].events) == runs["on"][2]


def test_train_starts_from_the_estimate(monkeypatch):
    draft, events, truth = synth.make_region(220, 5, 8941, B.oracle_swalign, P)
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
    best, _ = consensus.train(make_pa, dict(P), truth, iters=1, reps=1)
    B.reset_rand()
    best_e, _ = consensus.train(make_pa, dict(P), truth, iters=1, reps=1, estimate=True)
    fit = make_pa(P).RefitTransitions(params=P)
    assert seen[0] == P and best == P
    assert seen[1] == fit.params and best_e == fit.params and fit.ok
    assert all(seen[1][k] != P[k] for k in RATE_KEYS) and {k: v for k, v in seen[1].items() if k not in RATE_KEYS} == {k: v for k, v in P.items() if k not in RATE_KEYS}
