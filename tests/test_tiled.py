"""Partial-span reads on the CPU (tests/tiled_cases.py): the preconditions that keep the crafted cases from going stale, the oracle
against the live reference build on every case and representation, the oracle against itself and the reference's recorded outputs (tests/golden/tiled.npz).  Equality is exact throughout."""
import numpy as np
import pytest

import backends as B
import tiled_cases as TC

need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs /root/reference)")
RANDOM_SEEDS = list(range(1, 14))


def oracle_log(kind, key, mode):
    make = TC.crafted if kind == "crafted" else TC.random_tiled
    return TC.oracle_once(("log", kind, key, mode), lambda: TC.full_log(B.OraclePSAlign, *make(key, mode)))


# ---- preconditions -------------------------------------------------------------------------------------------------------------
def test_pinned_bands_stay_on_the_first_and_last_rows_for_1024_columns():
    """`pinned`, truncated: event 1 (covers the right third) keeps its band's first row at 1, event 2 (the left third) its last row
    at n0, on at least 1 024 consecutive columns — twice the four-wave model-row ring, more than either column-maxima ring"""
    draft, events, par = TC.crafted("pinned", "truncated")
    for e, at_top in ((1, True), (2, False)):
        n0 = events[e].mean.size
        assert n0 > par["realign_width"]                                   # not full-frame: the band is narrower than the event
        first, last = TC.band_rows(TC.fill_tables(B.oracle_api(), draft, events, par, e, 0)[0])
        run = TC.longest_run(first == 1) if at_top else TC.longest_run(last == n0)
        assert run >= 1024, (e, run)


@pytest.mark.parametrize("mode", TC.MODES)
def test_short_events_are_full_frame(mode):
    """`short`: events 1-3 have fewer levels than realign_width, and every level is in band on every column"""
    draft, events, par = TC.crafted("short", mode)
    for e in (1, 2, 3):
        n0 = events[e].mean.size
        assert n0 < par["realign_width"]
        first, last = TC.band_rows(TC.fill_tables(B.oracle_api(), draft, events, par, e, 0)[0])
        assert np.all(first == 1) and np.all(last == n0), e


@pytest.mark.parametrize("mode", TC.MODES)
def test_gap_stops_viterbi_in_mid_region(mode):
    draft, events, par = TC.crafted("gap", mode)
    L = TC.CRAFTED["gap"][0]
    T = TC.viterbi_tables(B.oracle_api(), draft, events, par, 0)["T"]
    assert 0 < T < L // 2, T
    starts = sorted(int(e.ref_align[e.ref_align > 0][0]) for e in events)
    assert starts[2] < L // 4 and starts[3] > L // 2                        # two groups of refstart


@pytest.mark.parametrize("mode", TC.MODES)
def test_single_coverage_takes_the_skip_branch(mode):
    """fewer positions kept than lie between the smallest refstart and the largest refend: positions were skipped"""
    draft, events, par = TC.crafted("single", mode)
    on = [e.ref_align[e.ref_align > 0] for e in events]
    span = int(max(a[-1] for a in on)) - int(min(a[0] for a in on)) + 1
    T = TC.viterbi_tables(B.oracle_api(), draft, events, par, 0)["T"]
    assert TC.CRAFTED["single"][0] // 2 < T < span, (T, span)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_cases_have_bare_and_deep_coverage(seed):
    for mode in TC.MODES:
        draft, events, par = TC.random_tiled(seed, mode)
        cov = B.make_pa(B.OraclePSAlign, draft, events, par).Coverage()
        assert cov.min() == 0 and cov.max() >= 3, (mode, cov.min(), cov.max())
        assert 4 <= len(events) <= 8
    assert (par["realign_width"] == 40.0) == (seed % 3 == 0)


def test_representations_differ_where_they_should():
    """zeroed keeps whole arrays with 0 outside, truncated cuts them to TRIM levels around the aligned ones, loader carries negative
    and past-the-end coordinates"""
    z, t, l = (TC.crafted("gap", m) for m in TC.MODES)
    n = len(z[0])
    assert z[0] == t[0] == l[0]
    for a, b, c in zip(z[1], t[1], l[1]):
        assert a.mean.size == c.mean.size >= b.mean.size
        assert a.ref_align.min() >= 0 and a.ref_align.max() <= n
        on = np.flatnonzero(b.ref_align > 0)
        assert on[0] <= TC.TRIM and b.mean.size - 1 - on[-1] <= TC.TRIM
    assert min(e.ref_align.min() for e in l[1]) < 0 and max(e.ref_align.max() for e in l[1]) > n
    assert any(b.mean.size < a.mean.size for a, b in zip(z[1], t[1]))


# ---- the oracle against the live reference -------------------------------------------------------------------------------------
@need_ref
@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("name", TC.NAMES)
def test_oracle_matches_live_reference_crafted(name, mode):
    draft, events, par = TC.crafted(name, mode)
    assert TC.full_log(B.RefPSAlign, draft, events, par) == oracle_log("crafted", name, mode)
    e = TC.PARTIAL[name]
    for d in (0, 1):
        got, want = (TC.fill_tables(api, draft, events, par, e, d) for api in (B.oracle_api(), B.ref_api()))
        for x, y in zip(got, want):
            assert np.array_equal(x, y, equal_nan=True), (d, e)


@need_ref
@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_oracle_matches_live_reference_random(seed, mode):
    draft, events, par = TC.random_tiled(seed, mode)
    assert TC.full_log(B.RefPSAlign, draft, events, par) == oracle_log("random", seed, mode)


# ---- the oracle against itself -------------------------------------------------------------------------------------------------
TWICE = [("crafted", n, m) for n in ("gap", "single") for m in TC.MODES] + [("crafted", "pinned", "truncated"), ("crafted", "short", "loader")] \
    + [("random", s, m) for s in (1, 2, 3) for m in TC.MODES]


@pytest.mark.parametrize("kind,key,mode", TWICE)
def test_oracle_is_defined_on_partial_span_reads(kind, key, mode):
    """same answer twice (the L = 1500 cases in one representation each: 7 s a run)"""
    make = TC.crafted if kind == "crafted" else TC.random_tiled
    draft, events, par = make(key, mode)
    first = oracle_log(kind, key, mode)
    assert TC.full_log(B.OraclePSAlign, draft, events, par) == first
    tabs = [TC.viterbi_tables(B.oracle_api(), draft, events, par, 16) for _ in range(2)]
    assert tabs[0]["T"] == tabs[1]["T"] and all(np.array_equal(tabs[0][k], tabs[1][k]) for k in ("obs", "bp", "lik_final", "fwd", "paths"))


# ---- the reference's recorded outputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.GOLDEN_CASES)
def test_oracle_replays_the_recorded_reference(name):
    TC.check_golden(B.OraclePSAlign, name)
