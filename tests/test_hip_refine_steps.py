"""GPU tests of the steps between the ends of Mutate / Refine (refine_cases.py): the HIP library against the ORACLE, exactly —
ps_score_alignments' `likes` vector and its accumulation, every list and the state after every step of three rounds of
find -> score -> make on one handle (single handles and lock-step batches, crafted seeds and ViterbiMutate's), k_likes against the
host loop on either side of its 12 284-state table, ps_make_mutations / ps_batch_make_mutations / ApplyMuts on crafted and random
scored lists with the `score` launch count as witness of the recursion, and ps_find_point_mutations' list.  test_refine_steps.py
holds the oracle to the live reference build on the same cases."""
import copy
import os

import numpy as np
import pytest

import backends as B
import refine_cases as R
from poreseq_amd import _capi, synth
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu

families = pytest.mark.parametrize("fwd_kernel", ["sweep", "sweep_w2", "sweep_w4", "fill"], indirect=True)
VIT = (16, 0.05, 0.01, 0.33, 0.75)        # Mutate(seqs="viterbi")'s ViterbiMutate arguments (poreseqcpp.Mutate)
KNOB = "PORESEQ_DEBUG_LIKES_HOST"


def hip():
    return _capi.load_hip()


class counted:
    """ps_prof_enable(1) around a block; .n(name) = launches (or host-side counts) of a kernel class since it began"""

    def __enter__(self):
        hip().prof_enable(1)
        hip().prof_reset()
        return self

    def __exit__(self, *exc):
        hip().prof_enable(0)
        return False

    def n(self, name):
        return hip().prof_get(name)[1]


class knob:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get(KNOB)
        os.environ[KNOB] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[KNOB]
        else:
            os.environ[KNOB] = self.old
        return False


def oracle_rounds(key, draft, events, par, seeds):
    return R.oracle_once(("rounds", key), lambda: R.rounds(B.oracle_api(), draft, events, par, seeds))


# ------------------------------------------------------------------------------------------------ likes
@families
@pytest.mark.parametrize("name", R.REGIONS)
def test_likes_vector_and_its_accumulation(name, fwd_kernel):
    draft, events, par, _ = R.region(name)
    want = R.oracle_once(("likes", name), lambda: R.likes_twice(B.oracle_api(), draft, events, par))
    got = R.likes_twice(hip(), draft, events, par)
    assert got[:4] == want[:4]


# ------------------------------------------------------------------------------------------------ three rounds, step by step
@families
@pytest.mark.parametrize("name", sorted(R.seed_sets()))
def test_three_rounds_step_by_step(name, fwd_kernel):
    draft, events, par, _ = R.region("work")
    seeds = R.seed_sets()[name]
    want = oracle_rounds(("work", name), draft, events, par, seeds)
    assert R.first_difference(R.rounds(hip(), draft, events, par, seeds), want) is None


@families
@pytest.mark.parametrize("name", ["wide420", "tiled", "inert", "barely"])
def test_three_rounds_on_the_other_regions(name, fwd_kernel):
    draft, events, par, truth = R.region(name)
    seeds = [truth, truth[30:150]]
    want = oracle_rounds((name, "truth+slice"), draft, events, par, seeds)
    assert R.first_difference(R.rounds(hip(), draft, events, par, seeds), want) is None


@families
def test_list_stops_at_the_cap(fwd_kernel):
    draft, events, par, _ = R.region("cap60")
    want = oracle_rounds(("cap60", "cap"), draft, events, par, R.cap_seeds())
    assert len(want[0][1][0]) == len(draft) // 3
    assert R.first_difference(R.rounds(hip(), draft, events, par, R.cap_seeds()), want) is None


def viterbi_seeds():
    """the 16 seeds Mutate(seqs="viterbi") would draw on the `work` region, from the oracle after reset_rand"""
    def make():
        draft, events, par, _ = R.region("work")
        api = B.oracle_api()
        B.reset_rand()
        h = api.align_create(draft, events, par)
        try:
            return api.viterbi_mutate(h, *VIT, 0)
        finally:
            api.align_destroy(h)
    return R.oracle_once("viterbi_seeds", make)


@families
def test_three_rounds_with_viterbi_seeds(fwd_kernel):
    draft, events, par, _ = R.region("work")
    seeds = viterbi_seeds()
    assert len(seeds) == 16
    want = oracle_rounds(("work", "viterbi"), draft, events, par, seeds)
    assert R.first_difference(R.rounds(hip(), draft, events, par, seeds), want) is None


def batch_rounds(api, regions, seed_lists, n_rounds=3):
    """refine_cases.rounds for several regions in lock-step through the batch entry points -> one log per region"""
    hs = [api.align_create(d, copy.deepcopy(ev), par) for d, ev, par in regions]
    sq = [api.seqs_create(s) for s in seed_lists]
    Es = [len(ev) for _, ev, _ in regions]
    logs = [[] for _ in regions]

    def note(label, results):
        for k, res in enumerate(results):
            logs[k].append((label, res, R.state(api, hs[k], Es[k])))

    try:
        for r in range(n_rounds):
            hm = api.batch_find_mutations(hs, sq)
            try:
                note("find %d" % r, [R.listing(api, m) for m in hm])
                hsc = api.batch_score_mutations(hs, hm)
            finally:
                for m in hm:
                    api.muts_destroy(m)
            try:
                note("score %d" % r, [R.listing(api, m) for m in hsc])
                nb = api.batch_make_mutations(hs, hsc)
            finally:
                for m in hsc:
                    api.muts_destroy(m)
            note("make %d" % r, nb)
        for h, (_, _, par) in zip(hs, regions):
            api.check(api.lib.ps_align_new_call(h, int(par["scoring_width"])))
        hm = api.batch_find_mutations(hs, sq)
        try:
            note("find after new_call", [R.listing(api, m) for m in hm])
        finally:
            for m in hm:
                api.muts_destroy(m)
    finally:
        for s in sq:
            api.seqs_destroy(s)
        for h in hs:
            api.align_destroy(h)
    return logs


@families
def test_lock_step_batch_equals_the_single_handles(fwd_kernel):
    """three regions with 7, 2 and 0 seeds through ps_batch_find_mutations / ps_batch_score_mutations / ps_batch_make_mutations"""
    regs, seeds = [], []
    for name, pick in (("work", lambda t: R.seed_sets()["mixed7"]), ("wide420", lambda t: [t, t[30:150]]), ("tiled", lambda t: [])):
        draft, events, par, truth = R.region(name)
        regs.append((draft, events, par))
        seeds.append(pick(truth))
    logs = batch_rounds(hip(), regs, seeds)
    for (draft, events, par), sd, log in zip(regs, seeds, logs):
        assert R.first_difference(log, R.rounds(hip(), draft, events, par, sd)) is None
        assert R.first_difference(log, oracle_rounds(("batch", draft, len(sd)), draft, events, par, sd)) is None
    assert logs[2][0][1][0] == [] and logs[0][0][1][0]        # no seeds: no edits; the first region has some


# ------------------------------------------------------------------------------------------------ k_likes against the host loop
def test_device_and_host_likes_agree():
    draft, events, par, _ = R.region("work")
    seeds = R.seed_sets()["mixed7"]
    want = oracle_rounds(("work", "mixed7"), draft, events, par, seeds)
    with counted() as c:
        dev = R.rounds(hip(), draft, events, par, seeds)
        assert c.n("likes_dev") >= 1 and c.n("likes_host") == 0
    with knob("1"), counted() as c:
        host = R.rounds(hip(), draft, events, par, seeds)
        assert c.n("likes_host") >= 1 and c.n("likes_dev") == 0
    with knob("0"), counted() as c:
        assert R.first_difference(R.rounds(hip(), draft, events, par, seeds), want) is None
        assert c.n("likes_dev") >= 1 and c.n("likes_host") == 0
    assert R.first_difference(dev, host) is None
    assert R.first_difference(dev, want) is None


def find_once(api, draft, events, par, seeds):
    h = api.align_create(draft, copy.deepcopy(events), par)
    try:
        hm = api.find_mutations(h, seeds)
        try:
            return R.listing(api, hm), R.state(api, h, len(events))
        finally:
            api.muts_destroy(hm)
    finally:
        api.align_destroy(h)


def test_likes_table_boundary():
    """a seed of 12 288 bases — 12 284 states, k_likes' table exactly full — stays on the device; one of 12 289 takes the host
    loop, and the short seed of the same call with it.  The smallest shape at which that edge exists: the oracle's two
    Smith-Waterman matrices are about 0.75 GB each."""
    par = dict(R.P0)
    draft, events, truth = synth.make_region(12288, 2, 9330, B.oracle_swalign, par)
    full, over = truth, truth + "A"
    assert len(full) == 12288
    with counted() as c:
        got = find_once(hip(), draft, events, par, [full])
        assert (c.n("likes_dev"), c.n("likes_host")) == (1, 0)
    assert got == find_once(B.oracle_api(), draft, events, par, [full])
    assert len(got[0][0]) > 100
    with counted() as c:
        got = find_once(hip(), draft, events, par, [over, truth[100:400]])
        assert c.n("likes_dev") == 0 and c.n("likes_host") >= 1
    assert got == find_once(B.oracle_api(), draft, events, par, [over, truth[100:400]])


# ------------------------------------------------------------------------------------------------ greedy pass
def _big(name):
    return name.split("_")[-1] in ("700", "refine") and not name.startswith("all_neg")


@pytest.mark.parametrize("name", sorted(R.greedy_lists()))
def test_greedy_pass_with_events(name):
    draft, events, par, _ = R.region("work")
    muts = R.greedy_lists()[name]
    want = R.oracle_once(("apply", name), lambda: R.apply_list(B.oracle_api(), draft, events, par, muts))
    with counted() as c:
        got = R.apply_list(hip(), draft, events, par, muts)
        launches = c.n("score")
    assert got == want
    # the `score` launches witness the recursion: more than ten deferred edits are re-scored, ten or fewer are dropped
    if name in R.RECURSING or _big(name):
        assert launches >= 1
    if name in R.NO_DEFERRAL or name in ("deferred_10", "spacing_9") or name.startswith("all_neg") or name.endswith(("_0", "_1")):
        assert launches == 0


def test_greedy_pass_as_list_logic():
    """no events: nothing is launched, and every list ends as the oracle's does"""
    big = {}
    with counted() as c:
        for seq, prof, muts, is_big in R.sweep_cases(320, 9501):
            got = R.apply_list(hip(), seq, [], R.P0, muts)
            assert got == R.apply_list(B.oracle_api(), seq, [], R.P0, muts), (seq, prof, len(muts))
            R.big_applied(big, prof, is_big, got[0])
        assert [c.n(k) for k in ("score", "fill", "sweep", "sw")] == [0, 0, 0, 0]
    assert R.every_live_profile_applied_big_lists(big), big


def test_batch_make_mutations_equals_the_singles():
    """one region that recurses, one that does not, one with an empty list"""
    api = hip()
    draft, events, par, _ = R.region("work")
    names = ("deferred_11", "deferred_10", "distinct_neg_0")
    hs = [api.align_create(draft, copy.deepcopy(events), par) for _ in names]
    hm = [api.muts_create(R.greedy_lists()[n], with_scores=True) for n in names]
    try:
        with counted() as c:
            nb = api.batch_make_mutations(hs, hm)
            assert c.n("score") >= 1
        got = [(n, R.state(api, h, len(events))) for n, h in zip(nb, hs)]
    finally:
        for m in hm:
            api.muts_destroy(m)
        for h in hs:
            api.align_destroy(h)
    for name, g in zip(names, got):
        assert g == R.apply_list(api, draft, events, par, R.greedy_lists()[name]), name
        assert g == R.apply_list(B.oracle_api(), draft, events, par, R.greedy_lists()[name]), name
    assert got[0][0] > 0 and got[1][0] > 0 and got[2][0] == 0


def test_apply_muts():
    draft, events, par, _ = R.region("work")
    muts = R.greedy_lists()["distinct_neg_100"]
    a, b = B.make_pa(PSAlign, draft, events, par), B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
    a.ApplyMuts(muts)
    b.ApplyMuts(muts)
    assert a.sequence == b.sequence and a.sequence != draft
    for x, y in zip(a.events, b.events):
        assert x.ref_align.tobytes() == y.ref_align.tobytes() and x.ref_like.tobytes() == y.ref_like.tobytes()


@pytest.mark.parametrize("seq", ["ACGT", "ACGTA", "GATTACAGATNACAGGATTACA"])
def test_point_list(seq):
    assert R.point_listing(hip(), seq) == R.point_listing(B.oracle_api(), seq)
