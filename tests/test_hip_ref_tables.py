"""Caller-written ref_align arrays on the HIP path (tests/ref_cases.py): k_updaterefs, k_lb / lower_bound_d, band_of / k_lo and the
strip sweeps' band tables, and vit_gather, each on arrays that synth's alignments never hold — holes laid on the thread chunks of
k_updaterefs, the un-interpolated hole behind an aligned level 0, one aligned level (ref_index is NaN), back steps (ref_index
unsorted), markers, fractions, columns 0 and past the end, reads without an aligned level or without levels — at 0, 1, 2, 255, 256,
257, 513 and 1025 levels and at realign_width 3, 20 and 300.

Every comparison is exact: against the oracle, and for the bands and the number of kept Viterbi positions also against the plain restatement of
cpp/EventData.h:110-204, so that a wrong band is not excused by an oracle that happened to agree.  The oracle's results are
computed once per case and width and shared between the fill families.  conftest.py fans only test_hip_parity and
test_hip_variant over the families, so this module asks for them itself."""
import copy

import numpy as np
import pytest

import backends as B
import ref_cases as RC
import support_cases as SC
import viterbi_cases as K
import viterbi_ref as V
from poreseq_amd import _capi
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]
families = pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)      # topmost decorator: the family varies fastest
cases = pytest.mark.parametrize("name", RC.GPU_CASES, ids=RC.case_id)
widths = pytest.mark.parametrize("W", RC.WIDTHS)


def scores(lst):
    return np.array([s.score for s in lst])


# ---- DP tables ------------------------------------------------------------------------------------------------------------------
_tables = {}


def oracle_fill(name, W, e, d):
    """the oracle's debug_fill tables; only the current (case, width) is kept"""
    if _tables.get("key") != (name, W):
        _tables.clear()
        _tables["key"] = (name, W)
    if (e, d) not in _tables:
        draft, events, par = RC.case(name)
        _tables[(e, d)] = RC.fill_tables(B.oracle_api(), draft, events, RC.with_width(par, W), e, d)
    return _tables[(e, d)]


@families
@widths
@cases
def test_dp_matrices_and_bands(name, W, fwd_kernel):
    """forward and backward main / stay matrices and the forward step codes of every event; the NaN pattern is the restated band"""
    draft, events, par = RC.case(name)
    par = RC.with_width(par, W)
    hip = _capi.load_hip()
    C = len(draft) - 4
    for e, ev in enumerate(events):
        t = RC.ref_tables(ev.ref_align)
        for d in (0, 1):
            got = RC.fill_tables(hip, draft, events, par, e, d)
            band = ~np.isnan(got[0])
            want_band = RC.band_mask(t, ev.mean.size, C, W, d)
            if not np.array_equal(band, want_band):
                cols = np.flatnonzero((band != want_band).any(axis=0))
                raise AssertionError("event %d, direction %d: the band differs from the restatement, first at column %d" % (e, d, cols[0]))
            for k, (x, y) in enumerate(zip(got, oracle_fill(name, W, e, d))):
                if d == 1 and k >= 2:
                    continue   # backward step codes are not kept (nothing reads them)
                if not np.array_equal(x, y, equal_nan=True):
                    differs = ~((x == y) | (np.isnan(x.astype(np.float64)) & np.isnan(y.astype(np.float64))))
                    cols = np.flatnonzero(differs.any(axis=0))
                    raise AssertionError("event %d, direction %d, table %d: first differing column %d (rows %s), %d cells differ"
                                         % (e, d, k, cols[0], np.flatnonzero(differs[:, cols[0]])[:8].tolist(), int(differs.sum())))


# ---- API ------------------------------------------------------------------------------------------------------------------------
def api_results(cls, draft, events, par):
    """ScoreEvents, ScorePoints, ScoreMutations (edits at both ends), Refine and AlignStats(realign=True) with what they leave"""
    mk = lambda: B.make_pa(cls, draft, copy.deepcopy(events), par)
    out = {"ScoreEvents": mk().ScoreEvents(), "ScorePoints": scores(mk().ScorePoints()), "ScoreMutations": scores(mk().ScoreMutations(RC.edits(draft)))}
    pa = mk()
    out["Refine"] = (pa.Refine(), pa.sequence, RC.refs(pa))
    sc, st = mk().AlignStats(realign=True)
    out["AlignStats"] = (np.asarray(sc, dtype=np.float64).tobytes(), np.ascontiguousarray(st).tobytes())
    B.reset_rand()
    pa = mk()
    out["Mutate"] = (pa.Mutate(seqs="viterbi", reps=2), pa.sequence, RC.refs(pa))
    return out


@families
@widths
@cases
def test_api_parity_with_oracle(name, W, fwd_kernel):
    draft, events, par = RC.case(name)
    par = RC.with_width(par, W)
    want = RC.once(("api", name, W), lambda: api_results(B.OraclePSAlign, draft, events, par))
    got = api_results(PSAlign, draft, events, par)
    assert got["ScoreEvents"] == want["ScoreEvents"]
    for k in ("ScorePoints", "ScoreMutations"):
        bad = np.flatnonzero(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))
        assert bad.size == 0, (k, bad[:6].tolist(), got[k][bad[:6]].tolist(), want[k][bad[:6]].tolist())
    for k in ("Refine", "Mutate"):
        assert got[k][:2] == want[k][:2] and RC.same_arrays(got[k][2], want[k][2]), k
    assert got["AlignStats"] == want["AlignStats"]


# ---- Viterbi --------------------------------------------------------------------------------------------------------------------
@cases
def test_viterbi_tables_under_every_emission_build(name):
    """T (the oracle's and the restatement's), the trimmed-mean emissions, back-pointers, final scores and state paths, nkeep 16 and 0"""
    draft, events, par = RC.case(name)
    T = len(RC.once(("positions", name), lambda: RC.viterbi_positions(RC.case(name)[1])))
    cap = T + 4
    want = RC.once(("vit", name, 16), lambda: RC.viterbi_tables(B.oracle_api(), draft, events, par, 16, cap))
    builds = K.admitted_builds(len(events))
    assert builds == [1, 2, 3] and want["T"] == T
    for b in [0] + builds:
        got = RC.viterbi_tables(_capi.load_hip(), draft, events, par, 16, cap, b)
        assert got["T"] == T, (b, got["T"], T)
        if T == 0:
            continue
        assert np.array_equal(got["obs"], want["obs"]), b
        bp, lik = V.run64(want["obs"], K.SKIP, K.STAY)
        assert np.array_equal(got["bp"], bp) and np.array_equal(want["bp"], bp), b
        assert np.array_equal(got["lik_final"], lik) and np.array_equal(want["lik_final"], lik), b
        assert np.array_equal(got["paths"], want["paths"]), b
    want0 = RC.once(("vit", name, 0), lambda: RC.viterbi_tables(B.oracle_api(), draft, events, par, 0, cap))
    got = RC.viterbi_tables(_capi.load_hip(), draft, events, par, 0, cap)
    assert got["T"] == want0["T"] == T and got["fwd"] is None
    assert np.array_equal(got["paths"], want0["paths"]) and np.array_equal(got["bp"], want0["bp"]) and np.array_equal(got["obs"], want0["obs"])


# ---- read support: refstart / refend of the call's re-alignment --------------------------------------------------------------------
@families
@pytest.mark.parametrize("name", ["back_steps", "markers"])
def test_support_cover_counts(name, fwd_kernel):
    draft, events, par = RC.case(name)
    par = RC.with_width(par, 20)
    muts, grp = RC.edits(draft), SC.strands(events)
    want = RC.once(("support", name), lambda: SC.loop(draft, events, par, muts, grp, 2))
    got = B.make_pa(PSAlign, draft, copy.deepcopy(events), par).ScoreMutationSupport(muts, groups=grp, n_groups=2)
    assert np.array_equal(got[1]["cover"], want[1]["cover"]) and SC.same(got, want)


# ---- lock-step ------------------------------------------------------------------------------------------------------------------
LOCK_STEP = ("sic_hole", "back_steps", "single_mid")


def alone(cls, draft, events, par):
    pa = B.make_pa(cls, draft, copy.deepcopy(events), par)
    out = [pa.ScoreEvents(), pa.Refine(), pa.sequence]
    B.reset_rand()
    out += [pa.Mutate(seqs="viterbi"), pa.sequence]
    return out, RC.refs(pa)


@families
def test_lock_step_batch_equals_regions_alone_and_the_oracle(fwd_kernel):
    regs = [(d, e, RC.with_width(p, 20)) for d, e, p in (RC.case(n) for n in LOCK_STEP)]
    want = RC.once(("lock_step",), lambda: [alone(B.OraclePSAlign, *r) for r in regs])
    single = [alone(PSAlign, *r) for r in regs]
    pas = [B.make_pa(PSAlign, d, copy.deepcopy(e), p) for d, e, p in regs]
    with RegionBatch(pas) as rb:
        se = rb.ScoreEvents()
        nb = rb.Refine()
        s1 = [pa.sequence for pa in pas]
        nv = rb.Mutate(seqs="viterbi")
        s2 = [pa.sequence for pa in pas]
        rb.sync()
        rf = [RC.refs(pa) for pa in pas]
    for r in range(len(pas)):
        got = [se[r], nb[r], s1[r], nv[r], s2[r]]
        for other in (single[r], want[r]):
            assert got == other[0], r
            assert RC.same_arrays(rf[r], other[1]), r


# ---- out-of-range entries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [2147483648.0, 1e12, float("inf")])
def test_viterbi_refuses_entries_not_below_2_31(v):
    """refused on the host copy before any kernel of the call, naming event and level; the DP takes the same array and equals the
    oracle; the library is usable afterwards"""
    draft, events, par = RC.case("untouched")
    events[1].ref_align[17] = v
    for api in (_capi.load_hip(), B.oracle_api()):
        h = api.align_create(draft, copy.deepcopy(events), par)
        try:
            for call, who in ((lambda: api.viterbi_mutate(h, 16, *RC.VIT, 0), "ps_viterbi_mutate: event 1, level 17"),
                              (lambda: api.viterbi_mutate(h, 0, *RC.VIT, 0), "ps_viterbi_mutate: event 1, level 17"),
                              (lambda: api.batch_viterbi_mutate([h], [None], 16, *RC.VIT), "ps_batch_viterbi_mutate: region 0: event 1, level 17"),
                              (lambda: api.debug_viterbi([h], 64, 16, *RC.VIT), "ps_debug_viterbi: region 0: event 1, level 17")):
                with pytest.raises(_capi.PoreseqError) as err:
                    call()
                assert who in str(err.value) and "2^31" in str(err.value), str(err.value)
        finally:
            api.align_destroy(h)
    mk = lambda cls: B.make_pa(cls, draft, copy.deepcopy(events), par)
    assert mk(PSAlign).ScoreEvents() == mk(B.OraclePSAlign).ScoreEvents()
    with pytest.raises(_capi.PoreseqError):
        mk(PSAlign).Mutate(seqs="viterbi")
    draft, events, par = RC.case("untouched")
    B.reset_rand()
    x = B.make_pa(PSAlign, draft, copy.deepcopy(events), par)
    nx = x.Mutate(seqs="viterbi", reps=1)
    B.reset_rand()
    y = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
    assert nx == y.Mutate(seqs="viterbi", reps=1) and x.sequence == y.sequence
