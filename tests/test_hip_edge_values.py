"""Outlier event data on the HIP path (tests/edge_cases.py) against the oracle: values that `synth.make_region` never draws, and the
parts of the library that exist only for them.

  tier A  finite data the host calls sane (tabulated reciprocals), under all four fill families
  tier B  the corners of the accepted range (poreseq_amd/csrc/ps_sane.h), under the strip sweeps and k_fill
  tier C  the IEEE-division builds: (i) data outside the range, with the step-down from two / four wavefronts to one;
          (ii) ordinary data under PORESEQ_EXACT_DIV=1 at the smallest shapes that reach each instance
  tier D  tables whose emissions are infinite or NaN: -infinity and NaN run through the DP and the edit scoring and are refused by
          ViterbiMutate; a +infinity emission is refused by ps_align_create (PS_ERR_BAD_ARG, the message names the offender)
  tier E  finite, unmarked data whose trimmed-mean emissions kill ViterbiMutate's max-plus vector (back-pointer -1 in every state
          from one kept position on): tables and stochastic paths exact under every emission build, the deterministic back-trace
          refused by the rule of DESIGN.md section 2

Every comparison is at tolerance 0 with NaN matched as a mask, except the forward probabilities of ViterbiMutate, which keep the rule
and the helper of test_hip_viterbi_tables.py.  The oracle's results are computed once per case (edge_cases.oracle_once); the oracle
itself is held to the live reference build on the same cases by test_edge_values.py.  conftest.py fans only test_hip_parity and
test_hip_variant over the families, so this module asks for them itself."""
import copy

import numpy as np
import pytest

import backends as B
import edge_cases as EC
import tiled_cases as TC
import viterbi_cases as K
import viterbi_ref as V
from test_hip_tiled import Profiled
from test_hip_viterbi_tables import check_forward, check_region
from poreseq_amd import _capi
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu
families = pytest.mark.parametrize("fwd_kernel", ["sweep", "sweep_w2", "sweep_w4", "fill"], indirect=True)
two_families = pytest.mark.parametrize("fwd_kernel", ["sweep", "fill"], indirect=True)
stepped_down = pytest.mark.parametrize("fwd_kernel", ["sweep_w2", "sweep_w4"], indirect=True)
need_ld = pytest.mark.skipif(not V.HAVE_LD, reason="np.longdouble has no 64-bit mantissa on this machine")


def hip(draft, events, par):
    return B.make_pa(PSAlign, draft, copy.deepcopy(events), par)


IEEE = EC.TIER_C + EC.TIER_D_MARKED + EC.TIER_E      # cases whose tables fail the range predicate: every launch divides
FILL_FORMS = ("fill_pair", "fill_pair_fwd", "fill_cmp", "fill_512", "fill_1024", "fill_wide")
SCORE_CLASSES = ("score_g7", "score_g8", "score_g16", "score_g32", "score_g64")


class Forms(Profiled):
    """Profiled, with the host-side counts of which form each launch took: k_fill's forms, k_score's size classes, and the launches
    of each kernel class that divided (fill_ieee, sweep_ieee, score_ieee) instead of using tabulated reciprocals"""

    def __exit__(self, *exc):
        self.n = {k: self.api.prof_get(k)[1] for k in FILL_FORMS + SCORE_CLASSES + ("fill_ieee", "sweep_ieee", "score_ieee", "sweep_kept", "score")}
        return super().__exit__(*exc)

    def divided(self, yes):
        """every fill / sweep launch and every k_score launch took the IEEE build (yes) or none did"""
        fills = sum(self.n[k] for k in FILL_FORMS)
        assert fills == self.fills, (fills, self.fills, self.n)
        scored = sum(self.n[k] for k in SCORE_CLASSES)
        want = (self.fills, self.sweeps, scored) if yes else (0, 0, 0)
        return (self.n["fill_ieee"], self.n["sweep_ieee"], self.n["score_ieee"]) == want

    def only_fill_forms(self, forms, also=()):
        """each of `forms` ran, and nothing outside `forms` and `also`"""
        return all(self.n[k] > 0 for k in forms) and all(self.n[k] == 0 for k in FILL_FORMS if k not in forms + also)


def compare_tables(got, want, what):
    """main and stay matrices and (forward) the step codes; names the first differing column"""
    e, d = what[-2:]
    for k, (x, y) in enumerate(zip(got, want)):
        if d == 1 and k >= 2:
            continue   # backward step codes are not kept (nothing reads them)
        if not np.array_equal(x, y, equal_nan=True):
            differs = ~((x == y) | (np.isnan(x.astype(np.float64)) & np.isnan(y.astype(np.float64))))
            cols = np.flatnonzero(differs.any(axis=0))
            raise AssertionError("%s: event %d, direction %d, table %d: first differing column %d (rows %s), %d cells differ"
                                 % (what[0], e, d, k, cols[0], np.flatnonzero(differs[:, cols[0]])[:8].tolist(), int(differs.sum())))


def check_dp(name, family):
    for e in EC.altered_events(name):
        for d in (0, 1):
            with Forms() as prof:
                got = EC.fill_tables(_capi.load_hip(), name, e, d)
            assert prof.ran(family), (family, prof.sweeps, prof.fills, prof.waves)
            assert prof.divided(name in IEEE), prof.n
            compare_tables(got, EC.oracle_fill(name, e, d), (name, e, d))


def check_calls(name, family, keys=None):
    """the call set of edge_cases.call_set against the oracle's; the family asked for ran"""
    draft, events, par = EC.region(name)
    want = EC.oracle_calls(name)
    with Forms() as prof:
        assert EC.same_floats(hip(draft, events, par).ScoreEvents(), want["ScoreEvents"])
        assert EC.same_floats(EC.scores(hip(draft, events, par).ScoreMutations(EC.edits(draft, events, name))), want["ScoreMutations"])
    assert prof.ran(family), (family, prof.sweeps, prof.fills, prof.waves)
    assert prof.divided(name in IEEE) and prof.n["score"] > 0, prof.n
    if keys is None:
        got = EC.call_set(PSAlign, name, viterbi=name not in EC.TIER_D_MARKED)
        keys = list(got)
    else:
        got = {"ScoreEvents": hip(draft, events, par).ScoreEvents(),
               "ScoreMutations": EC.scores(hip(draft, events, par).ScoreMutations(EC.edits(draft, events, name)))}
        if "ScorePoints" in keys:
            got["ScorePoints"] = EC.scores(hip(draft, events, par).ScorePoints())
    assert EC.differences(got, want, keys=keys) == []


# ---- tier A ---------------------------------------------------------------------------------------------------------------------
@families
@pytest.mark.parametrize("name", EC.TIER_A)
def test_tier_a_dp_matrices_bit_exact(name, fwd_kernel):
    check_dp(name, fwd_kernel)


@families
@pytest.mark.parametrize("name", EC.TIER_A)
def test_tier_a_calls_match_oracle(name, fwd_kernel):
    """ScoreEvents, ScorePoints, ScoreMutations(edits), Refine with refs, Mutate(list), Mutate('viterbi') after reset_rand, PointTable
    and ScoreMutationSupport"""
    check_calls(name, fwd_kernel)


def alone(cls, draft, events, par):
    pa = B.make_pa(cls, draft, copy.deepcopy(events), par)
    out = [pa.ScoreEvents(), pa.Refine(), pa.sequence]
    B.reset_rand()
    out += [pa.Mutate(seqs="viterbi"), pa.sequence]
    rf = EC.refs(pa)
    return out, pa.PointTable(), rf


@families
def test_lock_step_batch_of_base_spike_skip0(fwd_kernel):
    """three regions whose parameters and value ranges differ in one lock-step batch equal the three run alone, and the oracle"""
    from point_cases import same
    regs = [EC.region(n) for n in ("base", "spike", "skip0")]
    want = EC.oracle_once(("lock_step",), lambda: [alone(B.OraclePSAlign, *r) for r in regs])
    single = [alone(PSAlign, *r) for r in regs]
    pas = [hip(*r) for r in regs]
    with RegionBatch(pas) as rb:
        se = rb.ScoreEvents()
        nb = rb.Refine()
        s1 = [pa.sequence for pa in pas]
        nv = rb.Mutate(seqs="viterbi")             # (every region of a batch owns a generator seeded like a fresh process)
        s2 = [pa.sequence for pa in pas]
        rb.sync()
        rf = [EC.refs(pa) for pa in pas]
        tables = rb.PointTable()
    for r, pa in enumerate(pas):
        got = [se[r], nb[r], s1[r], nv[r], s2[r]]
        for other in (single[r], want[r]):
            assert got == other[0], r
            assert same(tables[r], other[1]), r
            assert EC.same_arrays(rf[r], other[2]), r


@need_ld
@pytest.mark.parametrize("name", ("spike", "sd_small") + EC.TIER_E)
def test_viterbi_tables_under_every_emission_build(name):
    """T, the trimmed-mean emissions, back-pointers, final scores and state paths exact on every row; forward vectors by the rule of
    test_hip_viterbi_tables.py on the rows where the reference has one.  From the first position whose emissions are all below
    -745 nats (exp = 0 for every state: row 96 of `spike`, row 7 of `sd_small`, row 100 of tier E) the reference normalises 0 / 0 and
    carries NaN to the end; its back-steps then fall through to the last state (`r < cs` is never true).  The device's vector must
    be dead there too — every row total 0 or NaN, which makes k_vit_trace fall through the same way — and the paths, compared
    exactly, say that it is.  Tier E: the insertion sort and the trimmed mean of all three emission kernels meet -inf entries
    (dropped in `vit_trimmed`, summed in the others), and k_vit_steps rows that are dead or dying (edge_cases.VIT_FIRST_DEAD)."""
    draft, events, par = EC.region(name)
    want = EC.oracle_once(("vit", name), lambda: TC.viterbi_tables(B.oracle_api(), draft, events, par, 16))
    alive = EC.live_forward_rows(want["fwd"])
    assert alive == want["T"] if name == "vit_trimmed" else 5 <= alive < want["T"]
    builds = K.admitted_builds(len(events))
    assert builds == [1, 2, 3]
    for b in [0] + builds:
        got = TC.viterbi_tables(_capi.load_hip(), draft, events, par, 16, b)
        what = "%s, build %d" % (name, b)
        check_region(got, want, what, forward=False)
        if name in EC.VIT_FIRST_DEAD:
            assert np.all(got["bp"][EC.VIT_FIRST_DEAD[name]:] == -1) and np.all(got["lik_final"] == -1e300)
        if b in (0, builds[-1]):
            check_forward({"fwd": got["fwd"][:alive]}, {"fwd": want["fwd"][:alive]}, want["obs"][:alive], what)
            tot = got["fwd"][alive:].sum(axis=1)
            assert np.all((tot == 0) | np.isnan(tot)), (what, tot[:8])


# ---- tier B ---------------------------------------------------------------------------------------------------------------------
@two_families
@pytest.mark.parametrize("name", EC.TIER_B)
def test_tier_b_corners_of_the_accepted_range(name, fwd_kernel):
    """the extreme tuples the tabulated build still takes: DP tables of the altered events, ScoreEvents, ScoreMutations"""
    check_dp(name, fwd_kernel)
    check_calls(name, fwd_kernel, keys=["ScoreEvents", "ScoreMutations"])


# ---- tier C (i): data outside the range ------------------------------------------------------------------------------------------
@two_families
@pytest.mark.parametrize("name", EC.TIER_C)
def test_tier_c_data_outside_the_range(name, fwd_kernel):
    """k_sweep / k_sweep2 / k_sweeps / k_score (sweep) and k_fill (fill) with IEEE division, chosen by ps_align_create itself.
    corner_overflow is the tuple that overflowed inside the earlier range: -inf emissions from finite inputs."""
    check_dp(name, fwd_kernel)
    check_calls(name, fwd_kernel)


@stepped_down
@pytest.mark.parametrize("name", EC.TIER_C + EC.TIER_E)
def test_tier_c_steps_down_to_one_wavefront(name, fwd_kernel):
    """two or four wavefronts per sweep are asked for; the multi-wavefront builds exist with tabulated reciprocals only, so pick_form
    answers with one: strip sweeps ran, none of them on two or four wavefronts, same results"""
    draft, events, par = EC.region(name)
    want = EC.oracle_calls(name)
    with Forms() as prof:
        got = {"ScoreEvents": hip(draft, events, par).ScoreEvents(), "ScorePoints": EC.scores(hip(draft, events, par).ScorePoints()),
               "ScoreMutations": EC.scores(hip(draft, events, par).ScoreMutations(EC.edits(draft, events, name)))}
    assert prof.sweeps > 0 and prof.fills == 0 and prof.waves == {"sweep_w2": 0, "sweep_w4": 0}, (prof.sweeps, prof.fills, prof.waves)
    assert prof.divided(True), prof.n
    assert EC.differences(got, want, keys=list(got)) == []


@stepped_down
def test_sane_data_does_run_on_the_wavefronts_asked_for(fwd_kernel):
    """the counterpart: the same calls on the base region do take the multi-wavefront build (the step-down above is the division's)"""
    draft, events, par = EC.region("base")
    with Forms() as prof:
        got = hip(draft, events, par).ScoreEvents()
    assert prof.sweeps > 0 and prof.waves[fwd_kernel] > 0 and prof.divided(False)
    assert got == EC.oracle_calls("base")["ScoreEvents"]


# ---- tier C (ii): ordinary data under PORESEQ_EXACT_DIV --------------------------------------------------------------------------
def shape_oracle(name, what):
    draft, events, par = EC.shape(name)
    mk = lambda: B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
    make = {"ScoreEvents": lambda: mk().ScoreEvents(), "ScorePoints": lambda: EC.scores(mk().ScorePoints()),
            "ScoreMutations": lambda: EC.scores(mk().ScoreMutations(EC.shape_edits(draft))),
            "Mutate": lambda: (lambda pa: (pa.Mutate(seqs=[ev.sequence for ev in events[:3]], reps=2), pa.sequence, EC.refs(pa)))(mk())}
    return EC.oracle_once(("shape", name, what), make[what])


def shape_dp(name, e=1):
    for d in (0, 1):
        got = EC.shape_tables(_capi.load_hip(), name, e, d)
        compare_tables(got, EC.oracle_once(("shape_fill", name, e, d), lambda: EC.shape_tables(B.oracle_api(), name, e, d)), (name, e, d))


@pytest.fixture
def exact_div(monkeypatch):
    """read at every ps_align_create; monkeypatch clears it"""
    monkeypatch.setenv("PORESEQ_EXACT_DIV", "1")


@pytest.mark.parametrize("fwd_kernel", ["sweep_w2"], indirect=True)
def test_exact_div_is_what_the_variable_selects(exact_div, fwd_kernel):
    """two wavefronts asked for, one taken, and the sweep counted as dividing"""
    draft, events, par = EC.shape("base")
    with Forms() as prof:
        assert hip(draft, events, par).ScoreEvents() == shape_oracle("base", "ScoreEvents")
    assert prof.sweeps > 0 and prof.waves == {"sweep_w2": 0, "sweep_w4": 0} and prof.divided(True)


@pytest.mark.parametrize("fwd_kernel", ["sweep"], indirect=True)
def test_exact_div_dense_sweeps(exact_div, fwd_kernel):
    """k_sweep<K, false> (ScoreEvents: forward only) and k_sweep2<K, false> (debug_fill, ScorePoints: forward and backward records of
    every column — sweep2_min = 0 and a list that reads more than a quarter of the columns)"""
    draft, events, par = EC.shape("base")
    with Forms() as prof:
        shape_dp("base")
        assert hip(draft, events, par).ScoreEvents() == shape_oracle("base", "ScoreEvents")
        assert EC.same_floats(EC.scores(hip(draft, events, par).ScorePoints()), shape_oracle("base", "ScorePoints"))
    assert prof.sweeps > 0 and prof.fills == 0 and prof.n["sweep_kept"] == 0 and prof.divided(True), prof.n


@pytest.mark.parametrize("fwd_kernel", ["sweep"], indirect=True)
def test_exact_div_sparse_column_sweep_and_score_groups(exact_div, fwd_kernel):
    """k_sweeps<K, false> and k_score<7 / 8 / 16 / 32 / 64, false> on kept columns: 24 edits on L = 400 read at most 2 columns each per
    direction, under a quarter of the 396 (choose_columns, ps_score.cpp), sparse_min = 0; the insertions of 2, 5, 20 and 40 bases fill
    the four wider size classes of k_score beside the point edits' seven columns"""
    draft, events, par = EC.shape("sparse")
    muts = EC.shape_edits(draft)
    assert sorted(set(min(len(m.mut) + 6, 64) for m in muts)) == [6, 7, 8, 11, 26, 46]
    with Forms() as prof:
        got = EC.scores(hip(draft, events, par).ScoreMutations(muts))
    assert prof.sweeps > 0 and prof.fills == 0 and prof.n["sweep_kept"] == prof.sweeps and prof.divided(True), prof.n
    assert all(prof.n[k] > 0 for k in SCORE_CLASSES), prof.n
    assert EC.same_floats(got, shape_oracle("sparse", "ScoreMutations"))


@pytest.mark.parametrize("fwd_kernel", ["sweep"], indirect=True)
def test_exact_div_backtrace_only_sweep(exact_div, fwd_kernel):
    """k_sweep<K, false> on FindMutations' candidate alignments (forward only, nothing kept but the step codes): Mutate(list)"""
    draft, events, par = EC.shape("base")
    pa = hip(draft, events, par)
    with Forms() as prof:
        nb = pa.Mutate(seqs=[ev.sequence for ev in events[:3]], reps=2)
    assert prof.sweeps > 0 and prof.fills == 0 and prof.divided(True), prof.n
    want = shape_oracle("base", "Mutate")
    assert (nb, pa.sequence) == want[:2] and EC.same_arrays(EC.refs(pa), want[2])


def fill_calls(name, forms, mutate=False, also=()):
    """ScoreEvents, ScoreMutations, Mutate(list) and the DP tables of event 1 against the oracle; every fill launch took one of
    `forms`, each of them at least once, and divided"""
    draft, events, par = EC.shape(name)
    with Forms() as prof:
        assert hip(draft, events, par).ScoreEvents() == shape_oracle(name, "ScoreEvents")
        assert EC.same_floats(EC.scores(hip(draft, events, par).ScoreMutations(EC.shape_edits(draft))), shape_oracle(name, "ScoreMutations"))
        if mutate:
            pa = hip(draft, events, par)
            nb = pa.Mutate(seqs=[ev.sequence for ev in events[:3]], reps=2)
            want = shape_oracle(name, "Mutate")
            assert (nb, pa.sequence) == want[:2] and EC.same_arrays(EC.refs(pa), want[2])
        shape_dp(name)
    assert prof.fills > 0 and prof.sweeps == 0, (prof.fills, prof.sweeps)
    assert prof.only_fill_forms(forms, also) and prof.divided(True), prof.n


@pytest.mark.parametrize("fwd_kernel", ["fill"], indirect=True)
def test_exact_div_fill_pairs(exact_div, fwd_kernel, monkeypatch):
    """k_fill<768, PAIR, false, false>: PORESEQ_DEBUG_PAIR_MIN=0 pairs every launch with 2 P <= 768 (P = 320 here) — the forward and
    backward sweep of a job in one workgroup (ScoreMutations, debug_fill: ndir = 2), and two forward-only jobs of one event
    (FindMutations' candidates in Mutate(list): three candidates per event)"""
    monkeypatch.setenv("PORESEQ_DEBUG_PAIR_MIN", "0")
    fill_calls("base", ("fill_pair", "fill_pair_fwd"), mutate=True, also=("fill_512",))   # (ScoreEvents: every event once, nothing to pair)


@pytest.mark.parametrize("fwd_kernel", ["fill"], indirect=True)
def test_exact_div_fill_compact_layout(exact_div, fwd_kernel):
    """k_fill<512, lone, false, CMP>: 8 sweeps are under the pairing threshold of 160 and P = 64 <= 256 (realign_width 45)"""
    fill_calls("cmp", ("fill_cmp",))


@pytest.mark.parametrize("fwd_kernel", ["fill"], indirect=True)
@pytest.mark.parametrize("name", ["base", "w430"])
def test_exact_div_fill_lone_sweep(name, exact_div, fwd_kernel):
    """k_fill<512, lone, false, plain layout>: P > 256 rules out the compact layout — 320 on the base region (forward-only candidate
    jobs of Mutate(list) included), 512 at realign_width 430 (the widest 512-thread launch)"""
    fill_calls(name, ("fill_512",), mutate=name == "base", also=("fill_cmp",) if name == "base" else ())   # (a shorter candidate may fit 256 slots)


@pytest.mark.parametrize("fwd_kernel", ["fill"], indirect=True)
def test_exact_div_fill_1024_thread_form(exact_div, fwd_kernel):
    """k_fill<1024, lone, false, plain>: realign_width 600 on 640 bases, P = 640 > 512"""
    fill_calls("t1024", ("fill_1024",))


@pytest.mark.parametrize("fwd_kernel", ["fill"], indirect=True)
def test_exact_div_fill_wide(exact_div, fwd_kernel):
    """k_fill_wide<false>: realign_width 1000 on 1 090 bases, footprints of 1 025 and 1 030 rows, P = 1 152 > 1 024"""
    fill_calls("wide", ("fill_wide",))


# ---- tier E: finite, unmarked data that kills ViterbiMutate's max-plus vector ----------------------------------------------------
@two_families
@pytest.mark.parametrize("name", EC.TIER_E)
def test_tier_e_dp_and_calls_match_oracle(name, fwd_kernel):
    """the DP matrices carry a level row whose emission is -inf (or below -1e300) for every state, from finite input; the call set
    includes Mutate('viterbi'), whose 16 stochastic back-traces run over the dead tables.  The two- and four-wavefront sweeps are
    asked for in test_tier_c_steps_down_to_one_wavefront: these tables divide, so they step down"""
    check_dp(name, fwd_kernel)
    check_calls(name, fwd_kernel)


def test_tier_e_lock_step_batch_and_the_refused_decode():
    """(base, vit_mean_overflow, vit_trimmed) in one lock-step batch: Mutate('viterbi') equals the three run alone and the oracle.
    With nkeep = 0 the dead region is refused by ps_viterbi_mutate, ps_batch_viterbi_mutate and ps_debug_viterbi — PS_ERR_BAD_ARG
    naming the entry point, region 1 of the lock-step calls and kept position 100 — the batch as a whole; the same handles then
    answer ScoreEvents as before, and the live regions decode"""
    names = ("base", "vit_mean_overflow", "vit_trimmed")
    regs = [EC.region(n) for n in names]

    def viterbi_alone(cls, r):
        B.reset_rand()
        pa = B.make_pa(cls, r[0], copy.deepcopy(r[1]), r[2])
        return pa.Mutate(seqs="viterbi"), pa.sequence, EC.refs(pa)

    want = EC.oracle_once(("tier_e_batch",), lambda: [viterbi_alone(B.OraclePSAlign, r) for r in regs])
    single = [viterbi_alone(PSAlign, r) for r in regs]
    pas = [hip(*r) for r in regs]
    with RegionBatch(pas) as rb:
        nv = rb.Mutate(seqs="viterbi")
        rb.sync()
    for r, pa in enumerate(pas):
        for other in (single[r], want[r]):
            assert (nv[r], pa.sequence) == other[:2] and EC.same_arrays(EC.refs(pa), other[2]), names[r]
    api, orc = _capi.load_hip(), B.oracle_api()
    where = EC.UNREACHABLE % EC.VIT_FIRST_DEAD["vit_mean_overflow"]
    hs = [api.align_create(r[0], copy.deepcopy(r[1]), r[2]) for r in regs]
    rngs = [api.rng_create(1) for _ in regs]
    try:
        for call, who in ((lambda: api.viterbi_mutate(hs[1], 0, *TC.VIT, 0), "ps_viterbi_mutate: no state"),
                          (lambda: api.batch_viterbi_mutate(hs, rngs, 0, *TC.VIT), "ps_batch_viterbi_mutate: region 1: "),
                          (lambda: api.debug_viterbi(hs, 400, 0, *TC.VIT), "ps_debug_viterbi: region 1: ")):
            with pytest.raises(_capi.PoreseqError) as err:
                call()
            assert "(-1)" in str(err.value) and who in str(err.value) and where in str(err.value), str(err.value)
        for k in (0, 2):
            ho = orc.align_create(regs[k][0], copy.deepcopy(regs[k][1]), regs[k][2])
            try:
                assert api.viterbi_mutate(hs[k], 0, *TC.VIT, 0) == orc.viterbi_mutate(ho, 0, *TC.VIT, 0)
            finally:
                orc.align_destroy(ho)
        assert api.batch_viterbi_mutate([hs[0], hs[2]], [rngs[0], rngs[2]], 0, *TC.VIT) == [api.viterbi_mutate(hs[k], 0, *TC.VIT, 0) for k in (0, 2)]
        for h, r, name in zip(hs, regs, names):      # (last: scoring writes the alignments back, which the walk reads)
            assert api.score_alignments(h, len(r[1])).tolist() == list(EC.oracle_calls(name)["ScoreEvents"]), name
    finally:
        for g in rngs:
            api.rng_destroy(g)
        for h in hs:
            api.align_destroy(h)


# ---- tier D ---------------------------------------------------------------------------------------------------------------------
@two_families
@pytest.mark.parametrize("name", EC.TIER_D_MARKED)
def test_tier_d_marked_dp_and_scoring_match_oracle(name, fwd_kernel):
    """emissions of -infinity and NaN (a NaN or infinite mean, a negative or infinite stdv, NaN / negative / infinite model entries):
    such candidates never win a maximum in the reference nor in the kernels, so the matrices stay finite and every call but
    ViterbiMutate returns the oracle's bits, NaN scores in the same places"""
    check_dp(name, fwd_kernel)
    check_calls(name, fwd_kernel)


@pytest.mark.parametrize("name", EC.TIER_D_MARKED)
def test_tier_d_marked_is_refused_by_viterbi_mutate(name):
    """PS_ERR_BAD_ARG naming the first offending level or model row, from the single call, the lock-step call and the debug hook; the
    objects are left as they were and the AlignData stays usable"""
    draft, events, par = EC.region(name)
    pa = hip(draft, events, par)
    with pytest.raises(_capi.PoreseqError) as err:
        pa.Mutate(seqs="viterbi")
    assert "(-1)" in str(err.value) and EC.NAMED[name] in str(err.value) and "ps_viterbi_mutate" in str(err.value), str(err.value)
    assert pa.sequence == draft and EC.same_arrays(EC.refs(pa), EC.refs(hip(draft, events, par)))
    pas = [hip(*EC.region("base")), hip(draft, events, par)]
    with RegionBatch(pas) as rb:
        with pytest.raises(_capi.PoreseqError) as err:
            rb.Mutate(seqs="viterbi")
        assert EC.NAMED[name] in str(err.value)
        assert rb.ScoreEvents()[1] == EC.oracle_calls(name)["ScoreEvents"]
    assert [p.sequence for p in pas] == [draft, draft]
    api = _capi.load_hip()
    h = api.align_create(draft, copy.deepcopy(events), par)
    try:
        with pytest.raises(_capi.PoreseqError) as err:
            api.debug_viterbi([h], 400, 16, *TC.VIT)
        assert EC.NAMED[name] in str(err.value)
    finally:
        api.align_destroy(h)


@pytest.mark.parametrize("name", EC.TIER_D_REFUSED)
def test_tier_d_plus_infinity_is_refused_by_every_call(name):
    """a +infinity emission (a level with stdv == 0, a model row with level_stdv == 0 or an infinite lambda, an infinite lik_offset):
    ps_align_create fails with PS_ERR_BAD_ARG and names the first offender; every public call creates its AlignData first"""
    draft, events, par = EC.region(name)
    with pytest.raises(_capi.PoreseqError) as err:
        _capi.load_hip().align_create(draft, copy.deepcopy(events), par)
    assert "(-1)" in str(err.value) and EC.NAMED[name] in str(err.value), str(err.value)
    muts = EC.edits(draft, events, name)
    calls = [lambda pa: pa.ScoreEvents(), lambda pa: pa.ScorePoints(), lambda pa: pa.ScoreMutations(muts), lambda pa: pa.Refine(),
             lambda pa: pa.Mutate(seqs=[ev.sequence for ev in events[:3]], reps=2), lambda pa: pa.Mutate(seqs="viterbi"),
             lambda pa: pa.Mutate(), lambda pa: pa.PointTable(), lambda pa: pa.ScoreMutationSupport(muts),
             lambda pa: pa.ScoreMutationDeltas(muts), lambda pa: pa.ScoreSequences([draft]), lambda pa: pa.ApplyMuts([])]
    for call in calls:
        pa = hip(draft, events, par)
        with pytest.raises(_capi.PoreseqError) as err:
            call(pa)
        assert EC.NAMED[name] in str(err.value)
        assert pa.sequence == draft
    with pytest.raises(_capi.PoreseqError):
        with RegionBatch([hip(*EC.region("base")), hip(draft, events, par)]) as rb:
            rb.ScoreEvents()
    # the library is as usable as before
    assert hip(*EC.region("base")).ScoreEvents() == EC.oracle_calls("base")["ScoreEvents"]
