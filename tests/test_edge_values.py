"""Outlier and non-finite event data on the CPU (tests/edge_cases.py): the preconditions that keep the cases what their names say,
the host's range predicate (poreseq_amd/csrc/ps_sane.h) judged by a native program that compiles the same header, the tabulated
build of the emission against IEEE division over everything that predicate accepts (tests/native/emission_check.cpp), and the
oracle against the live reference build on every case.  Equality is exact throughout; NaN is matched as a mask."""
import subprocess

import numpy as np
import pytest

import backends as B
import edge_cases as EC

need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs /root/reference)")


# ---- the emission, both builds, over the accepted range --------------------------------------------------------------------------
def test_tabulated_emission_equals_ieee_division_over_the_accepted_range():
    """zero mismatches over the grid and the random significands; the program's exit status says the same"""
    out = subprocess.run([EC.emission_check_exe()], stdout=subprocess.PIPE, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0 and text.strip().endswith("mismatches=0"), text
    assert "predicate=ps_sane.h" in text and "nonfinite=0" in text, text
    accepted = int(text.split("accepted=")[1].split()[0])
    assert accepted > 8000000, text


def test_the_earlier_range_fails_the_same_grid():
    """finite divisors in (1e-100, 1e100) let e e lambda overflow: mdiv(inf, b, y) is NaN where inf / b is inf.  The grid must see
    that, or it proves nothing about the range that replaced it."""
    out = subprocess.run([EC.emission_check_exe(), "old"], stdout=subprocess.PIPE, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 1 and "predicate=old" in text, text
    assert int(text.split("mismatches=")[1].split()[0]) > 0, text


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.FINITE)
def test_finite_tiers_score_finite(name):
    assert np.all(np.isfinite(EC.oracle_calls(name)["ScoreEvents"])), EC.oracle_calls(name)["ScoreEvents"]


@pytest.mark.parametrize("name", ("base",) + EC.TIER_A + EC.TIER_B)
def test_tiers_a_and_b_pass_the_host_predicate(name):
    _draft, events, par = EC.region(name)
    assert EC.host_verdict(events, par) == ("unmarked", "fast")


@pytest.mark.parametrize("name", EC.TIER_C + EC.TIER_E)
def test_tier_c_takes_the_ieee_builds(name):
    _draft, events, par = EC.region(name)
    assert EC.host_verdict(events, par) == ("unmarked", "ieee")


@pytest.mark.parametrize("name", EC.TIER_D)
def test_tier_d_is_marked_or_refused(name):
    """a +infinity emission is refused, every other value outside the reference's domain marked; the tables among them fail the range predicate"""
    _draft, events, par = EC.region(name)
    verdict = EC.host_verdict(events, par)
    assert verdict[0] == ("refused" if name in EC.TIER_D_REFUSED else "marked")
    assert verdict[1] == "ieee" or name == "off_inf"             # (lik_offset is no operand of a division)


@pytest.mark.parametrize("name", EC.TIER_D)
def test_tier_d_emissions_are_what_the_tier_says(name):
    """the emission of every (level, 5-mer) pair of the altered events, restated from cpp/AlignUtil.h:34-53 in numpy: the refused
    cases hold a +infinity (or, lik_offset, nothing finite), the marked ones NaN or -infinity and no +infinity"""
    _draft, events, par = EC.region(name)
    seen_pinf = seen_other = False
    with np.errstate(all="ignore"):
        for e in EC.altered_events(name):
            ev, md = events[e], events[e].model
            lam = md.sd_mean ** 3 / md.sd_stdv ** 2
            x, sd, lsd = ev.mean[:, None], ev.stdv[:, None], np.log(ev.stdv[::-1])[:, None]
            d = (x - md.level_mean) / md.level_stdv
            ee = (sd - md.sd_mean) / md.sd_mean
            em = -0.5 * (d * d + np.log(2 * np.pi)) - np.log(md.level_stdv) + 0.5 * (np.log(lam) - 3 * lsd - np.log(2 * np.pi) - ee * ee * lam / sd) + par["lik_offset"]
            seen_pinf |= bool(np.isposinf(em).any())
            seen_other |= bool((np.isnan(em) | np.isneginf(em)).any())
    if name in EC.TIER_D_REFUSED:
        assert seen_pinf or name in ("model_sd_zero", "lam_inf")     # (these two: +inf terms that meet a -inf or NaN of the same row)
    else:
        assert seen_other and not seen_pinf


def test_corner_tuples_sit_on_the_ends_of_the_range():
    """one step further and the predicate says no"""
    for name, e, field, at, value in (("corner_hi", 1, "stdv", 40, np.nextafter(EC.HI, np.inf)), ("corner_lo", 1, "stdv", 40, np.nextafter(EC.LO, 0)),
                                      ("corner_mean", 1, "mean", 40, np.nextafter(EC.HI, np.inf)), ("corner_lo", 2, "mean", 100, np.nextafter(EC.LO, 0))):
        events = EC.region(name)[1]
        getattr(events[e], field)[at] = value
        assert EC.host_verdict(events) == ("unmarked", "ieee"), (name, field)
    for name, field, value in (("corner_hi", "sd_stdv", np.nextafter(2.0 ** -292, 0)), ("corner_lo", "sd_stdv", 2.0 ** -91)):
        events = EC.region(name)[1]
        getattr(events[1].model, field)[0] = value          # lambda one step past 2^200 / below 2^-200
        assert EC.host_verdict(events) == ("unmarked", "ieee"), (name, field)
    md = EC.region("corner_hi")[1][1].model
    assert md.sd_mean[0] ** 3 / md.sd_stdv[0] ** 2 == EC.LAM_HI
    md = EC.region("corner_lo")[1][1].model
    assert EC.LAM_LO <= md.sd_mean[0] ** 3 / md.sd_stdv[0] ** 2 < EC.LAM_LO * 1.0000001


def test_sd_zero_gives_plus_infinity_and_nan_emissions():
    """event 1: a zero in mid-event, +inf scores from the row that reads its logarithm.  Event 2: zeros at both ends, which mirror onto
    each other — the first and last row divide by 0 next to log 0, and their emission is NaN for every 5-mer.  The reference's
    `if (liks[k] > cur)` chains never take a NaN candidate, so event 2's matrices hold no NaN beyond the band mask: the NaN shows
    in the emission, restated here from cpp/AlignUtil.h:34-53, and in what the matrices do not contain."""
    m1 = EC.oracle_fill("sd_zero", 1, 0)[0]
    assert np.any(np.isposinf(m1)) and not np.any(np.isinf(EC.oracle_fill("base", 1, 0)[0]))
    ev = EC.region("sd_zero")[1][2]
    md = ev.model
    with np.errstate(all="ignore"):
        lam = md.sd_mean ** 3 / md.sd_stdv ** 2
        for row in (1, ev.mean.size):
            sd, lsd = ev.stdv[row - 1], np.log(ev.stdv[ev.mean.size - row])
            e = (sd - md.sd_mean) / md.sd_mean
            assert np.all(np.isnan(0.5 * (np.log(lam) - 3 * lsd - np.log(2 * np.pi) - e * e * lam / sd)))
    for d in (0, 1):
        for k in (0, 1):
            assert np.array_equal(np.isnan(EC.oracle_fill("sd_zero", 2, d)[k]), np.isnan(EC.oracle_fill("base", 2, d)[k]))
    nonfinite = int(np.count_nonzero(~np.isfinite(EC.oracle_calls("sd_zero")["ScorePoints"])))
    assert nonfinite == 1992, nonfinite
    assert EC.oracle_calls("sd_zero")["Refine"][0] == 1952


def test_skip0_and_ins0_give_minus_infinity_in_the_transition_logs():
    for name, field in (("skip0", "prob_skip"), ("ins0", "prob_insert")):
        events = EC.region(name)[1]
        with np.errstate(divide="ignore"):
            assert all(np.log(getattr(ev.model, field)) == -np.inf for ev in events)
    assert [ev.model.prob_stay == 0.0 for ev in EC.region("ins0")[1]] == [not ev.model.complement for ev in EC.region("ins0")[1]]


def test_corner_overflow_has_minus_infinity_emissions_from_finite_inputs():
    _draft, events, _ = EC.region("corner_overflow")
    assert all(np.all(np.isfinite(getattr(ev, f))) for ev in events for f in ("mean", "stdv"))
    assert np.all(np.isfinite(events[1].model.sd_mean))
    md, sd = events[1].model, events[1].stdv[40]
    with np.errstate(over="ignore"):
        e = (sd - md.sd_mean[0]) / md.sd_mean[0]
        assert np.isfinite(e) and np.isposinf(e * e * (md.sd_mean[0] ** 3 / md.sd_stdv[0] ** 2) / sd)      # q = +inf: the emission is -inf
    # (scores are maxima against 0: a -inf candidate never wins, the matrices stay finite)
    assert not np.any(np.isinf(EC.oracle_fill("corner_overflow", 1, 0)[0]))


def test_edits_sit_on_the_altered_levels():
    draft, events, _ = EC.region("spike")
    muts = EC.edits(draft, events, "spike")
    at = set(m.start for m in muts[20:])
    for e, i in EC.altered_levels("spike"):
        assert int(events[e].ref_align[i]) - 1 in at or events[e].ref_align[i] <= 0
    assert {len(m.mut) - len(m.orig) for m in muts[20:]} == {-1, 0, 1, 2, 3}
    assert len(muts) >= 35


def test_outliers_kill_the_references_forward_vector():
    """ViterbiMutate's forward vector: where every state's trimmed-mean emission is below -745 nats the reference normalises 0 / 0 and
    carries NaN from there on (row 96 of `spike`, row 7 of `sd_small`); the max-plus tables stay finite.  The GPU test applies the
    forward rule to the rows before that and requires a dead vector after."""
    import tiled_cases as TC
    for name, first in (("spike", 96), ("sd_small", 7), ("base", 245)):
        t = TC.viterbi_tables(B.oracle_api(), *EC.region(name), 16)
        assert EC.live_forward_rows(t["fwd"]) == first and t["T"] == 245, name
        assert np.all(np.isnan(t["fwd"][first:].sum(axis=1)))
        assert np.all(np.isfinite(t["obs"])) and np.all(np.isfinite(t["lik_final"]))
        if first < 245:
            assert t["obs"][first].max() < -745


# ---- tier E: finite, unmarked data that kills ViterbiMutate's max-plus vector ------------------------------------------------------
def oracle_viterbi_tables(name):
    import tiled_cases as TC
    return EC.oracle_once(("vit", name), lambda: TC.viterbi_tables(B.oracle_api(), *EC.region(name), 16))


@pytest.mark.parametrize("name", EC.TIER_E_DEAD)
def test_tier_e_kills_the_max_plus_vector_where_pinned(name):
    """finite levels; the kept position named in edge_cases.VIT_FIRST_DEAD and every later one have back-pointer -1 in all 1024
    states and the final scores are all -1e300.  The dying row's emissions are all -inf (d d or e e overflows), all finite and
    below -1e300 (vit_below_big), or — vit_accum — no emission of the table is below -1e300: the running score passes it, over five
    partly dead rows.  The forward vector dies at row 100 in every case (exp = 0)."""
    import viterbi_cases as K
    import viterbi_ref as V
    _draft, events, _par = EC.region(name)
    assert len(events) == 3 and all(np.all(np.isfinite(getattr(ev, f))) for ev in events for f in ("mean", "stdv"))
    t = oracle_viterbi_tables(name)
    first = EC.VIT_FIRST_DEAD[name]
    assert t["T"] == 245
    counts = np.count_nonzero(t["bp"] == -1, axis=1)
    assert np.all(counts[first:] == 1024) and np.all(t["lik_final"] == -1e300)
    assert not np.any(np.isnan(t["obs"])) and t["obs"].max() < 1e300
    if name == "vit_accum":
        assert t["obs"].min() > -1e300
        assert np.all(counts[:104] == 0) and np.all((counts[104:first] > 0) & (counts[104:first] < 1024)), counts[98:112]
    else:
        assert np.all(counts[:first] == 0)
        row = t["obs"][first]
        assert np.all(row < -1e300) and (np.all(np.isfinite(row)) if name == "vit_below_big" else np.all(np.isneginf(row)))
        assert np.all(np.isfinite(np.delete(t["obs"], first, axis=0)))
    bp, lik = V.run64(t["obs"], K.SKIP, K.STAY)
    assert np.array_equal(t["bp"], bp) and np.array_equal(t["lik_final"], lik)
    assert EC.live_forward_rows(t["fwd"]) == 100 and np.all(np.isnan(t["fwd"][100:].sum(axis=1)))


def test_tier_e_control_trims_its_minus_infinity():
    """four events with a level on position 100: the -inf is the lowest quarter of every state's list and is dropped.  No
    back-pointer is -1, every emission row is finite, and row 100 alone differs from the base region's"""
    base, t = oracle_viterbi_tables("base"), oracle_viterbi_tables("vit_trimmed")
    assert t["T"] == base["T"] == 245 and np.all(t["bp"] >= 0) and np.all(np.isfinite(t["obs"])) and np.all(np.isfinite(t["lik_final"]))
    assert np.flatnonzero(np.any(t["obs"] != base["obs"], axis=1)).tolist() == [100]
    assert EC.live_forward_rows(t["fwd"]) == 245
    # the same level on the three-event region is vit_mean_overflow
    assert EC.CASES["vit_trimmed"] == EC.CASES["vit_mean_overflow"]


@pytest.mark.parametrize("name", EC.TIER_E_DEAD)
def test_tier_e_deterministic_decode_is_refused_by_the_oracle(name):
    """ps_viterbi_mutate, ps_batch_viterbi_mutate and ps_debug_viterbi with nkeep = 0 answer PS_ERR_BAD_ARG naming the entry point,
    the region of a lock-step call and the first dead position; the same handle then runs the stochastic call"""
    import tiled_cases as TC
    from poreseq_amd._capi import PoreseqError
    orc = B.oracle_api()
    draft, events, par = EC.region(name)
    where = EC.UNREACHABLE % EC.VIT_FIRST_DEAD[name]
    h, hb, rngs = orc.align_create(draft, events, par), orc.align_create(*EC.region("base")), [orc.rng_create(1), orc.rng_create(1)]
    try:
        for call, who in ((lambda: orc.viterbi_mutate(h, 0, *TC.VIT, 0), "ps_viterbi_mutate: no state"),
                          (lambda: orc.batch_viterbi_mutate([hb, h], rngs, 0, *TC.VIT), "ps_batch_viterbi_mutate: region 1: "),
                          (lambda: orc.debug_viterbi([hb, h], 400, 0, *TC.VIT), "ps_debug_viterbi: region 1: ")):
            with pytest.raises(PoreseqError) as err:
                call()
            assert "(-1)" in str(err.value) and who in str(err.value) and where in str(err.value), str(err.value)
        B.reset_rand()
        seqs = orc.viterbi_mutate(h, 16, *TC.VIT, 0)
        assert len(seqs) == 16 and orc.score_alignments(h, len(events)).tolist() == list(EC.oracle_calls(name)["ScoreEvents"])
    finally:
        for r in rngs:
            orc.rng_destroy(r)
        orc.align_destroy(h)
        orc.align_destroy(hb)


def test_off0_finds_nothing_and_off_big_scores_high():
    assert max(EC.oracle_calls("off0")["ScoreEvents"]) < 50 and EC.oracle_calls("off0")["Mutate"][0] == 0
    assert min(EC.oracle_calls("off_big")["ScoreEvents"]) > 5000


@pytest.mark.parametrize("name", tuple(EC.FORM_OF))
def test_shapes_reach_the_form_they_are_meant_for(name):
    """the widest anti-diagonal footprint over every event and direction, through the host's rule for P (edge_cases.slots)"""
    draft, events, par = EC.shape(name)
    widths = [EC.footprint(EC.shape_tables(B.oracle_api(), name, e, d)[0]) for e in range(len(events)) for d in (0, 1)]
    lo, hi = EC.FORM_OF[name]
    P = EC.slots(max(widths), par["realign_width"])
    print(name, widths, P)
    assert lo <= P <= hi, (widths, P)
    if name == "wide":
        assert min(widths) >= 1023, widths


# ---- the oracle against the live reference ---------------------------------------------------------------------------------------
@need_ref
@pytest.mark.parametrize("name", tuple(EC.CASES))
def test_oracle_matches_live_reference(name):
    """ScoreEvents, ScorePoints, ScoreMutations on edits(), Refine, Mutate(list), Mutate('viterbi') and PointTable, and the DP tables
    of every altered event: bit for bit, the non-finite cases included.  The reference build has no per-event terms to give
    ScoreMutationSupport; its ScoreMutations scores pin the scores of the oracle's."""
    got = EC.call_set(B.RefPSAlign, name, support=False)
    want = EC.oracle_calls(name)
    assert EC.differences(got, want, keys=list(got)) == []
    assert EC.same_floats(want["Support"][0], got["ScoreMutations"])
    for e in EC.altered_events(name):
        for d in (0, 1):
            for x, y in zip(EC.fill_tables(B.ref_api(), name, e, d), EC.oracle_fill(name, e, d)):
                assert np.array_equal(x, y, equal_nan=True), (e, d)
