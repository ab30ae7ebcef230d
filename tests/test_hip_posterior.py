"""ps_posterior_stats on the GPU: k_post_fwd / k_post_bwd (csrc/ps_post.hip) against util.posterior_from_emissions — the definition,
pinned on the CPU by test_posterior.py — on the cases of post_cases; the footprint edges; the widest supported footprint; the
structure of the call (repeatable bytes, lock-step batches, refusals, nothing left behind in the handles); the scratch contract;
the launch counters.

Error bounds.  Everything is compared with the definition evaluated in longdouble, with U = 2^-52 (n0 + C) max(1, |logz|):
    tables (M, S)   |dev - ld| <= K_TABLES U                  (absolute: a cell far off the best path is the small difference of
                                                               large terms, so the table's largest value, logz, sets the scale)
    logz            |dev - ld| <= K U
    counts, emit    |dev - ld| <= K U max(1, value)
    col             |dev - ld| / |ld| <= K U, over the levels whose longdouble emit is >= 1e-290 (below that the float64 weights
                    underflow and col is NaN or any column of the band)
K is not chosen from what the device gives.  The float64 restatement's own worst ratio against longdouble over these cases is
0.0284 for the records and per-level arrays (emit) and 0.0327 for the tables (measured on the CPU; printed again by the tests); K is
4 x that, rounded up to a power of two — the margin DESIGN.md section 2 gives device exp / log and a different order of the sums
over serial float64 sums: K = 0.125, K_TABLES = 0.25.  The device's worst ratios are printed by every test and recorded in
DESIGN.md section 4."""
import copy
import ctypes as C

import numpy as np
import pytest

import backends as B
import move_cases as M
import poison_cases as PZ
import post_cases as PC
import ref_cases
from poreseq_amd import _capi, synth, util
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu
LD = np.longdouble
K = 0.125
K_TABLES = 0.25
COL_MIN_EMIT = 1e-290
BATCH = ("empty_read", "untouched", M.NO_EVENTS, "all_unaligned", "wide")


def levels_of(events):
    return [ev.mean.size for ev in events]


def launches(api):
    return api.prof_get("post_fwd")[1], api.prof_get("post_bwd")[1]


def unit(n0, C, logz):
    return PC.EPS * max(1, n0 + C) * max(1.0, abs(float(logz)))


def table_ratio(got, want_ld, n0, C):
    """worst |got - ld| / U over the two tables; the NaN patterns and the infinities must agree"""
    u, worst = unit(n0, C, want_ld.logz), 0.0
    for g, w in ((got[0], want_ld.main), (got[1], want_ld.stay)):
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isneginf(g), np.isneginf(w))
        fin = np.isfinite(w)
        if np.any(fin):
            worst = max(worst, float(np.max(np.abs(g[fin].astype(LD) - w[fin]))) / u)
    return worst


def record_ratio(rec, emit, col, want_ld, n0, C):
    """worst ratio of one event's record (and per-level arrays) to its bound / K"""
    u = unit(n0, C, want_ld.logz)
    worst = abs(float(LD(rec["logz"]) - want_ld.logz)) / u
    for k in PC.COUNTS:
        worst = max(worst, abs(float(LD(rec[k]) - want_ld.counts[k])) / (u * max(1.0, float(want_ld.counts[k]))))
    if emit is not None and n0:
        worst = max(worst, float(np.max(np.abs(emit.astype(LD) - want_ld.emit) / np.maximum(LD(1), want_ld.emit))) / u)
        on = want_ld.emit >= COL_MIN_EMIT
        assert not np.any(np.isnan(col[on]))
        if np.any(on):
            worst = max(worst, float(np.max(np.abs(col[on].astype(LD) - want_ld.col[on]) / np.abs(want_ld.col[on]))) / u)
        with np.errstate(invalid="ignore"):
            assert np.all(np.isnan(col[~on]) | ((col[~on] >= 1) & (col[~on] <= C)))
    return worst


def check_region(name, recs, emit, col, what):
    """one region's records (and per-level arrays, or None) against the longdouble restatement -> (device ratio, float64 ratio)"""
    dev = f64 = 0.0
    _, events, _ = PC.case(name) if name != M.NO_EVENTS else (None, [], None)
    assert recs.shape == (len(events),) and recs.dtype == _capi.EVENT_POSTERIOR, what
    for e, ev in enumerate(events):
        ld, dbl = PC.restated(name, e, "sum", LD), PC.restated(name, e, "sum")
        n0, Cn = PC.lattice(name, e)[4:]
        r = recs[e]
        assert int(r["n_levels"]) == n0 and int(r["inert"]) == int(PC.inert(name, e)) and int(r["pad"]) == 0, (what, e)
        if PC.inert(name, e):
            assert r.tobytes()[8:] == bytes(72), (what, e)
            if emit is not None:
                assert not np.any(emit[e]) and np.all(np.isnan(col[e]))
            continue
        assert int(r["n_cells"]) == ld.n_cells and int(r["n_cols"]) == ld.n_cols, (what, e)
        dev = max(dev, record_ratio(r, None if emit is None else emit[e], None if col is None else col[e], ld, n0, Cn))
        f64 = max(f64, record_ratio(dbl.record(n0), np.asarray(dbl.emit), np.asarray(dbl.col), ld, n0, Cn))
    return dev, f64


def device_tables(draft, events, par, e):
    api = _capi.load_hip()
    h = api.align_create(draft, copy.deepcopy(events), par)
    try:
        return api.debug_posterior(h, e, events[e].mean.size, len(draft) - 4)
    finally:
        api.align_destroy(h)


# ---- 1. the forward tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.NAMES)
def test_forward_tables(name):
    draft, events, par = PC.case(name)
    dev = f64 = 0.0
    for e in range(len(events)):
        got = device_tables(draft, events, par, e)
        main, stay = PC.oracle_tables(name, e)
        assert np.array_equal(np.isnan(got[0]), np.isnan(main)) and np.array_equal(np.isnan(got[1]), np.isnan(stay)), (name, e)
        ld, dbl = PC.restated(name, e, "sum", LD), PC.restated(name, e, "sum")
        n0, Cn = PC.lattice(name, e)[4:]
        dev = max(dev, table_ratio(got, ld, n0, Cn))
        f64 = max(f64, table_ratio((dbl.main, dbl.stay), ld, n0, Cn))
    print("%s tables: device %.4f, float64 restatement %.4f of 2^-52 (n0 + C) max(1, logz)" % (name, dev, f64))
    assert dev <= K_TABLES


@pytest.mark.parametrize("width", (31, 32, 127, 128))
def test_footprint_edges(width):
    """narrow's region with 2 W + 1 = 63 / 65 / 255 / 257 band rows: either side of a wavefront and of four"""
    draft, events, par = PC.case("narrow")
    par = ref_cases.with_width(par, width)
    states = B.oracle_api().seq_to_states(draft)
    valid = np.concatenate([[False], np.asarray(states) >= 0])
    api = _capi.load_hip()
    h = api.align_create(draft, copy.deepcopy(events), par)
    try:
        recs, emit, col = api.posterior_stats(h, levels_of(events), True)
    finally:
        api.align_destroy(h)
    dev = devt = 0.0
    for e in (0, 3):
        ev = events[e]
        mask = ~np.isnan(ref_cases.fill_tables(B.oracle_api(), draft, events, par, e, 0)[0])
        assert mask[:, 1:].sum(axis=0).max() == min(2 * width + 1, ev.mean.size)
        ld = util.posterior_from_emissions(util.fill_emissions(ev, states, par), mask, valid, *PC.liks(ev), dtype=LD, levels=True)
        got = device_tables(draft, events, par, e)
        devt = max(devt, table_ratio(got, ld, ev.mean.size, len(states)))
        assert int(recs["n_cells"][e]) == ld.n_cells
        dev = max(dev, record_ratio(recs[e], emit[e], col[e], ld, ev.mean.size, len(states)))
    print("width %d: device tables %.4f, records %.4f" % (width, devt, dev))
    assert devt <= K_TABLES and dev <= K


# ---- 2. records and per-level arrays ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.NAMES)
def test_records_and_levels(name):
    draft, events, par = PC.case(name)
    api = _capi.load_hip()
    h = api.align_create(draft, copy.deepcopy(events), par)
    try:
        recs, emit, col = api.posterior_stats(h, levels_of(events), True)
        plain = api.posterior_stats(h, levels_of(events))
    finally:
        api.align_destroy(h)
    assert plain.tobytes() == recs.tobytes()                                    # without the per-level arrays: the same records
    dev, f64 = check_region(name, recs, emit, col, name)
    print("%s records: device %.4f, float64 restatement %.4f of the bound at K = 1" % (name, dev, f64))
    assert dev <= K


# ---- 3. the widest footprint one workgroup holds ---------------------------------------------------------------------------------------
def _widest():
    """one read of about 1 100 levels whose alignment jumps over 1 200 columns at its middle level: the band's centre stands still
    there, half a read away from either end, and all 2 W + 1 rows of the band lie on one anti-diagonal"""
    P = dict(M.P0, realign_width=511.0)
    draft, events, _ = synth.make_region(1150, 1, 8960, B.oracle_swalign, P)
    ev = events[0]
    t = ev.mean.size // 2
    while not ev.ref_align[t] > 0:
        t += 1
    at = int(ev.ref_align[t])
    gap = synth.random_sequence(np.random.default_rng(8961), 1200)
    draft = draft[:at] + gap + draft[at:]
    ev.ref_align = np.where(ev.ref_align > at, ev.ref_align + 1200, ev.ref_align)
    return draft, events, P


def test_widest_footprint_and_the_first_refused_one():
    import math
    draft, events, par = ref_cases.once(("post_widest",), _widest)
    n0, Cn = events[0].mean.size, len(draft) - 4
    assert 1060 <= n0 <= 1250
    main, stay, _, _ = ref_cases.fill_tables(B.oracle_api(), draft, events, par, 0, 0)
    live = ~np.isnan(main)
    diag = np.add.outer(np.arange(n0 + 1), np.arange(Cn + 1))
    assert np.bincount(diag[:, 1:][live[:, 1:]]).max() == 1023                  # the footprint: every row of the band on one anti-diagonal
    got = device_tables(draft, events, par, 0)
    assert np.array_equal(np.isnan(got[0]), ~live) and np.array_equal(np.isnan(got[1]), np.isnan(stay))
    slack = 4 * PC.EPS * (n0 + Cn)
    for g, w in ((got[0], main), (got[1], stay)):
        fin = live & (w > -1e299)
        assert np.all(g[fin] >= w[fin] - slack * np.maximum(1.0, np.abs(w[fin])))
    assert np.array_equal(np.isneginf(got[1]), stay == -1e300)
    api = _capi.load_hip()
    h = api.align_create(draft, copy.deepcopy(events), par)
    try:
        rec = api.posterior_stats(h, [n0])[0]
    finally:
        api.align_destroy(h)
    score = max(0.0, float(np.max(main[:, 1:][live[:, 1:]])))
    assert int(rec["n_cells"]) == int(live[:, 1:].sum()) and int(rec["n_cols"]) == Cn and not rec["inert"]
    assert score <= float(rec["logz"]) <= score + (n0 + Cn) * math.log(7.0) + math.log(int(rec["n_cells"]))
    with np.errstate(invalid="ignore"):
        assert float(rec["logz"]) >= float(np.nanmax(got[0]))
    wide = ref_cases.with_width(par, 512)
    h = api.align_create(draft, copy.deepcopy(events), wide)
    try:
        with pytest.raises(_capi.PoreseqError, match=r"\(-4\).*footprint of 1025 rows"):                # PS_ERR_UNSUPPORTED
            api.posterior_stats(h, [n0])
        scores = api.score_alignments(h, 1)
    finally:
        api.align_destroy(h)
    assert scores.tolist() == B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), wide).ScoreEvents()


# ---- 4. structure -------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes():
    for name in ("poor", PC.N_RUN):
        pa = B.make_pa(PSAlign, *PC.case(name))
        a, b = pa.PosteriorStats(levels=True), pa.PosteriorStats(levels=True)
        assert PZ.same_bytes(list(a), list(b))
        assert pa.PosteriorStats().tobytes() == a[0].tobytes()


@pytest.mark.parametrize("resident", [True, False])
def test_ragged_lock_step_batch(resident):
    pas = [B.make_pa(PSAlign, *M.case(n)) for n in BATCH]
    api = _capi.load_hip()
    rb = RegionBatch(pas, resident=resident)
    try:
        rb.load()
        api.prof_enable(1)
        api.prof_reset()
        try:
            res = rb.PosteriorStats(levels=True)
            n = launches(api)
        finally:
            api.prof_enable(0)
        back = rb.PosteriorStats(idx=[4, 1])
        rb.drop()
    finally:
        rb.close()
    assert n == (1, 1)                                                          # 3 + 3 + 0 + 3 + 5 events: one launch of each kernel
    for name, r in zip(BATCH, res):
        dev, _ = check_region(name, r[0], r[1], r[2], "lock-step " + name)
        assert dev <= K
        one = B.make_pa(PSAlign, *M.case(name)).PosteriorStats(levels=True)
        assert PZ.same_bytes(list(r), list(one)), name
    assert back[0].tobytes() == res[4][0].tobytes() and back[1].tobytes() == res[1][0].tobytes()
    for pa, name in zip(pas, BATCH):
        assert all(np.array_equal(a.ref_align, b.ref_align, equal_nan=True) and np.array_equal(a.ref_like, b.ref_like, equal_nan=True)
                   for a, b in zip(pa.events, M.case(name)[1]))


def test_inert_events_get_the_zero_record():
    draft, events, par = M.case("wide")
    still = B.make_pa(PSAlign, draft, copy.deepcopy(events), ref_cases.with_width(par, 0)).PosteriorStats(levels=True)
    assert still[0]["inert"].tolist() == [1] * len(events) and still[0]["n_levels"].tolist() == levels_of(events)
    assert all(r.tobytes()[8:] == bytes(72) for r in still[0]) and not any(np.any(a) for a in still[1]) and all(np.all(np.isnan(c)) for c in still[2])
    rec = B.make_pa(PSAlign, draft, copy.deepcopy(events), par).PosteriorStats()
    assert rec["inert"].tolist() == [0, 0, 0, 0, 1] and rec[4].tobytes()[8:] == bytes(72)
    none = B.make_pa(PSAlign, *M.case(M.NO_EVENTS)).PosteriorStats(levels=True)
    assert none[0].shape == (0,) and none[1] == [] and none[2] == []


def test_a_non_finite_aligndata_is_refused_and_stays_usable():
    draft, events, par = M.case("mean_nan")
    api = _capi.load_hip()
    h = api.align_create(draft, copy.deepcopy(events), par)
    try:
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*ps_batch_posterior_stats"):              # PS_ERR_BAD_ARG
            api.posterior_stats(h, levels_of(events))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*ps_debug_posterior"):
            api.debug_posterior(h, 0, events[0].mean.size, len(draft) - 4)
        scores = api.score_alignments(h, len(events))
    finally:
        api.align_destroy(h)
    assert scores.tobytes() == M.oracle_scored("mean_nan")[0].tobytes()


def test_bad_arguments_of_the_c_abi():
    api = _capi.load_hip()
    draft, events, par = M.case("narrow")
    E = len(events)
    h = api.align_create(draft, copy.deepcopy(events), par)
    h0 = api.align_create(draft, [], par)
    try:
        rec = np.zeros(E, dtype=_capi.EVENT_POSTERIOR)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null stats"):
            api.check(api.lib.ps_posterior_stats(h, None, None, None))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\)"):
            api.check(api.lib.ps_posterior_stats(None, vp(rec), None, None))
        arr = (_capi.c_dp * E)()                                                                        # an array of null pointers
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*emit and col go together"):
            api.check(api.lib.ps_posterior_stats(h, vp(rec), arr, None))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null per-level array of event 0"):
            api.check(api.lib.ps_posterior_stats(h, vp(rec), arr, arr))
        api.prof_enable(1)
        api.prof_reset()
        try:
            api.check(api.lib.ps_posterior_stats(h0, vp(rec), None, None))      # no events: PS_OK, nothing launched
            assert launches(api) == (0, 0)
            api.check(api.lib.ps_posterior_stats(h, vp(rec), None, None))
            assert launches(api) == (1, 1)
        finally:
            api.prof_enable(0)
        assert check_region("narrow", rec, None, None, "per-level arrays NULL")[0] <= K
    finally:
        api.align_destroy(h)
        api.align_destroy(h0)


def _state(pas):
    return [(pa.sequence, [(ev.ref_align.tobytes(), ev.ref_like.tobytes()) for ev in pa.events]) for pa in pas]


def test_the_call_leaves_nothing_behind_in_the_handles():
    api = _capi.load_hip()
    for name in ("poor", "narrow"):
        draft, events, par = M.case(name)
        out = []
        for first in (False, True):
            h = api.align_create(draft, copy.deepcopy(events), par)
            try:
                if first:
                    api.posterior_stats(h, levels_of(events), True)
                before = copy.deepcopy(events)
                api.align_update_events(h, before)
                scores = api.score_alignments(h, len(events))
                after = copy.deepcopy(events)
                api.align_update_events(h, after)
            finally:
                api.align_destroy(h)
            out.append((scores.tobytes(), [(ev.ref_align.tobytes(), ev.ref_like.tobytes()) for ev in before],
                        [(ev.ref_align.tobytes(), ev.ref_like.tobytes()) for ev in after]))
        assert out[0] == out[1], name
        assert out[0][1] == [(ev.ref_align.tobytes(), ev.ref_like.tobytes()) for ev in events]
    names = ("wide", "narrow")
    mk = lambda: [B.make_pa(PSAlign, *M.case(n)) for n in names]
    alone = mk()
    with RegionBatch(alone, resident=True) as rb:
        sc_alone = rb.ScoreEvents()
        nb_alone = rb.Refine()
    pas = mk()
    with RegionBatch(pas, resident=True) as rb:
        first = rb.PosteriorStats()
        sc = rb.ScoreEvents()
        again = rb.PosteriorStats(levels=True)
        nb = rb.Refine()
    assert sc == sc_alone and nb == nb_alone and _state(pas) == _state(alone)
    assert all(a.tobytes() == b[0].tobytes() for a, b in zip(first, again))     # (ScoreEvents' realignment was dropped, as the reference drops it)
    for name, r in zip(names, first):
        assert r.tobytes() == B.make_pa(PSAlign, *M.case(name)).PosteriorStats().tobytes()


def test_posterior_refit_on_the_device_follows_the_fallback():
    """the drivers on the HIP backend: the same fit as on the oracle through the definition, up to the device's rounding of the
    expected counts (the rates are quotients of sums of them: 64 K U covers the quotient of two sums of five)"""
    draft, events, par = M.case("narrow")
    fit = B.make_pa(PSAlign, draft, copy.deepcopy(events), par).RefitTransitions(posterior=True, iters=2)
    want = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par).RefitTransitions(posterior=True, iters=2)
    assert fit.flags == want.flags and len(fit.logz) == 2
    u = 64 * K * PC.EPS * 600 * max(1.0, max(want.logz))
    assert all(abs(fit.params[k] - want.params[k]) <= u for k in want.rates) and all(abs(a - b) <= u * 8 for a, b in zip(fit.logz, want.logz))
    pas = [B.make_pa(PSAlign, *M.case(n)) for n in ("narrow", "poor")]
    with RegionBatch(pas) as rb:
        rb.load()
        fits = rb.RefitTransitions(pool=False, posterior=True)
        scores = rb.ScoreEvents()
    assert all(abs(fits[0].params[k] - B.make_pa(B.OraclePSAlign, *M.case("narrow")).RefitTransitions(posterior=True).params[k]) <= u for k in want.rates)
    assert scores[0] != B.make_pa(PSAlign, *M.case("narrow")).ScoreEvents()     # the handles were rebuilt with the new rates


# ---- 5. the scratch contract ----------------------------------------------------------------------------------------------------------
def test_poisoned_scratch_changes_nothing():
    """index word 1 and the bits of +1e300 over everything the call could find left over, in front of every native call"""
    for name in ("untouched", "all_unaligned", "poor", PC.N_RUN):
        want = B.make_pa(PSAlign, *PC.case(name)).PosteriorStats(levels=True)
        before = PZ.api("1e300").calls
        got = B.make_pa(PZ.CLASSES["1e300"], *PC.case(name)).PosteriorStats(levels=True)
        assert PZ.api("1e300").calls > before
        assert PZ.same_bytes(list(got), list(want)), name
    want = [B.make_pa(PSAlign, *M.case(n)).PosteriorStats(levels=True) for n in BATCH]
    pas = [B.make_pa(PZ.CLASSES["1e300"], *M.case(n)) for n in BATCH]
    with RegionBatch(pas, resident=False) as rb:
        res = rb.PosteriorStats(levels=True)
    assert all(PZ.same_bytes(list(a), list(b)) for a, b in zip(res, want))
    draft, events, par = PC.case("narrow")
    api, plain = PZ.api("1e300"), _capi.load_hip()
    tabs = []
    for lib in (plain, api):
        h = lib.align_create(draft, copy.deepcopy(events), par)
        try:
            tabs.append(lib.debug_posterior(h, 2, events[2].mean.size, len(draft) - 4))
        finally:
            lib.align_destroy(h)
    assert PZ.same_bytes(list(tabs[0]), list(tabs[1]))


def test_a_small_narrow_region_right_after_a_large_wide_one():
    """real leftovers: a 420-base, 6-event, width-300 ScoreEvents immediately before the call on the same thread"""
    P0 = M.P0
    big = dict(P0, realign_width=300.0)
    bd, be, _ = synth.make_region(420, 6, 8801, B.oracle_swalign, big)
    for name in ("narrow", "column0"):
        want = B.make_pa(PSAlign, *PC.case(name)).PosteriorStats(levels=True)
        B.make_pa(PSAlign, bd, copy.deepcopy(be), big).ScoreEvents()
        got = B.make_pa(PSAlign, *PC.case(name)).PosteriorStats(levels=True)
        assert PZ.same_bytes(list(got), list(want)), name


# ---- 6. launch counters ----------------------------------------------------------------------------------------------------------------
def test_launch_counts():
    """k_post_fwd and k_post_bwd run once per chain of a PosteriorStats call and in no other call; no fill and no backtrace runs"""
    api = _capi.load_hip()
    pas = [B.make_pa(PSAlign, *M.case(n)) for n in ("narrow", "wide")]
    api.prof_enable(1)
    api.prof_reset()
    try:
        counts = []
        for pa in pas:
            for call in (pa.ScoreEvents, pa.MoveStats, pa.PosteriorStats, lambda: pa.PosteriorStats(levels=True)):
                n0 = launches(api)
                call()
                counts.append(tuple(b - a for a, b in zip(n0, launches(api))))
        fills = api.prof_get("fill")[1] + api.prof_get("sweep")[1]
        pas[0].PosteriorStats()
        assert api.prof_get("fill")[1] + api.prof_get("sweep")[1] == fills
        with RegionBatch([B.make_pa(PSAlign, *M.case(n)) for n in ("narrow", "wide")]) as rb:
            for call in (rb.ScoreEvents, rb.PosteriorStats, rb.Refine):
                n0 = launches(api)
                call()
                counts.append(tuple(b - a for a, b in zip(n0, launches(api))))
    finally:
        api.prof_enable(0)
    assert counts == [(0, 0), (0, 0), (1, 1), (1, 1)] * 2 + [(0, 0), (1, 1), (0, 0)]
