"""Results do not depend on what the device scratch held before a call.

Every pool, dense slab, cached AlignData slab and pinned staging buffer of the library is grow-only and reused without being
cleared; DESIGN.md section 3 calls them scratch between API calls.  `ps_debug_poison` (poison_cases.PoisonApi puts it in front of
every native call) overwrites all of them: 1 in every 32-bit word of the buffers that may hold indices, counts or flags, and in the
value-only pools (csrc/ps_poison.h) either 1-words again or +1e300 — finite, so that no max ignores it, larger than any score and
the ruin of every sum.  A kernel or host loop that reads a cell its own call did not write then returns a wrong result here, where a
fresh process would have handed it a zero.

Every comparison is the one the module of the same cases makes — exact against the oracle, or phase_cases.check / genotype_cases
with their derived bounds — and every result also equals, by bytes, the same call made without poison.  Oracle results come from
the once-per-session caches those modules use, so a full run computes them once.  The last group makes real leftovers instead: a
larger, wider region immediately before a smaller, narrower one on the same thread.

What each removed clear does to these tests is recorded in README.md (status, "Scratch memory")."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import backends as B
import deep_cases as D
import genotype_cases as GC
import phase_cases as PC
import poison_cases as P
import refine_cases as R
import support_cases as SC
import sweep_cases as S
import test_hip_deep_stacks as HD
import test_hip_sw_band as HB
import test_hip_sweep as HS
import test_hip_tiled as HT
import test_hip_viterbi_tables as HV
import tiled_cases as T
import viterbi_cases as K
from poreseq_amd import _capi, synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign
from poreseq_amd.util import DEFAULT_PARAMS

pytestmark = pytest.mark.gpu
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]
families = pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)      # topmost decorator: the family varies fastest
patterns = pytest.mark.parametrize("pattern", P.PATTERN_IDS)
P0 = dict(DEFAULT_PARAMS, verbose=0)
# sweep_cases seeds whose first event has a hole and a forward jump and whose last event never aligned: 222 bases, 5 events,
# realign_width 129, scoring_width 9, point_width 60; 114 bases, 8 events, realign_width 20, scoring_width 0, point_width 1
SEEDS = (117, 106)
_plain = {}


def plain_once(key, make):
    """the unpoisoned HIP result of a case, computed once per key (the fill family is part of the key where it matters)"""
    if key not in _plain:
        _plain[key] = make()
    return _plain[key]


def hip():
    return _capi.load_hip()


def same_by_key(got, want):
    """P.same_bytes entry by entry of two dicts, naming the entry that differs"""
    assert list(got) == list(want)
    for k in want:
        try:
            P.same_bytes(got[k], want[k])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (k, e)) from None


def test_the_seeds_are_what_the_groups_need():
    for seed in SEEDS:
        draft, holed, clean, par, muts = S.case(seed)
        assert np.any((holed[0].ref_align == 0) & (clean[0].ref_align > 0)) and np.any(holed[0].ref_align > clean[0].ref_align)
        assert not np.any(holed[-1].ref_align > 0) and len(holed) > 1
    assert max(len(m.mut) for m in S.case(SEEDS[0])[4]) >= 59          # k_score<64>


# ---- DP tables --------------------------------------------------------------------------------------------------------------------
def dp_region(name):
    """(draft, events, params, events whose tables are compared)"""
    if name == "single":
        draft, events, par = T.crafted("single", "loader")
        return draft, events, par, (T.PARTIAL["single"],)
    draft, holed, clean, par, muts = S.case(int(name))
    return draft, holed, par, (0, len(holed) - 1)


@families
@patterns
@pytest.mark.parametrize("W", [3, 300])
@pytest.mark.parametrize("name", ["117", "106", "single"])
def test_dp_tables(name, W, pattern, fwd_kernel):
    """debug_fill's forward and backward main and stay matrices and the forward step codes, poison before every call"""
    draft, events, par, which = dp_region(name)
    par = dict(par, realign_width=float(W))
    for e in which:
        for d in (0, 1):
            want = T.oracle_once(("poison_dp", name, W, e, d), lambda: T.fill_tables(B.oracle_api(), draft, events, par, e, d))
            plain = T.fill_tables(hip(), draft, events, par, e, d)
            got = T.fill_tables(P.api(pattern), draft, events, par, e, d)
            for k in range(4 if d == 0 else 2):      # backward step codes are not kept (nothing reads them)
                assert np.array_equal(got[k], want[k], equal_nan=True), (e, d, k, int((~((got[k] == want[k]) | (np.isnan(got[k].astype(float)) & np.isnan(want[k].astype(float))))).sum()))
            P.same_bytes(got, plain)


# ---- calls on one object ----------------------------------------------------------------------------------------------------------
def end_edits(draft, seed):
    """multi-base edits at both ends, one past the end, one of 60 inserted bases (k_score<64>), a few points"""
    rng = np.random.default_rng(6000 + seed)
    n = len(draft)
    ins = lambda m: "".join(rng.choice(list("ACGT"), m))
    return [S.edit(0, "", "TT"), S.edit(0, draft[0:3], "G"), S.edit(1, draft[1:2], ""), S.edit(n - 5, draft[n - 5:n - 2], "CA"),
            S.edit(n - 1, draft[n - 1:], "A"), S.edit(n, "", "AC"), S.edit(n + 1, "", "A"), S.edit(n // 2, "", ins(60)),
            S.edit(n // 3, draft[n // 3:n // 3 + 2], ins(3))] + synth.random_point_mutations(rng, draft, 12)


def extra_log(cls, seed):
    """what sweep_cases' logs leave out: the explicit edit list, AlignStats(realign=True), Mutate on a seed list with an
    unalignable and a duplicate seed"""
    draft, holed, clean, par, muts = S.case(seed)
    mk = lambda ev: B.make_pa(cls, draft, copy.deepcopy(ev), par)
    pa = mk(holed)
    log = {"ScoreMutations": S.listing(pa.ScoreMutations(end_edits(draft, seed)))}
    sc, st = pa.AlignStats(realign=True)
    log["AlignStats"] = (np.asarray(sc, dtype=np.float64), np.ascontiguousarray(st))
    cands = S.candidates(draft, seed)
    log["Mutate"] = (pa.Mutate(seqs=[cands[0], "ACGT" * 6, cands[0], cands[2]], reps=2), pa.sequence, S.refs(pa))
    return log


@families
@patterns
@pytest.mark.parametrize("seed", SEEDS)
def test_every_call_on_one_object(seed, pattern, fwd_kernel):
    """ScoreEvents, ScorePoints, ScoreMutations, Mutate('self'), Refine on one object, Mutate('viterbi') after reset_rand"""
    want = T.oracle_once(("sweep", seed), lambda: S.full_log(B.OraclePSAlign, seed))
    plain = plain_once(("full", seed, fwd_kernel), lambda: S.full_log(PSAlign, seed))
    got = S.full_log(P.CLASSES[pattern], seed)
    for k in want:
        assert got[k] == want[k], k
    P.same_bytes(got, plain)


@families
@patterns
@pytest.mark.parametrize("seed", SEEDS)
def test_edit_lists_align_stats_and_seed_lists(seed, pattern, fwd_kernel):
    want = T.oracle_once(("poison_extra", seed), lambda: extra_log(B.OraclePSAlign, seed))
    plain = plain_once(("extra", seed, fwd_kernel), lambda: extra_log(PSAlign, seed))
    got = extra_log(P.CLASSES[pattern], seed)
    P.same_bytes(got, want)
    P.same_bytes(got, plain)


@patterns
@pytest.mark.parametrize("seed", SEEDS)
def test_point_table_support_and_score_sequences(seed, pattern):
    want = T.oracle_once(("sweep_own", seed), lambda: S.own_choice_log(B.OraclePSAlign, seed))
    plain = plain_once(("own", seed), lambda: S.own_choice_log(PSAlign, seed))
    got = S.own_choice_log(P.CLASSES[pattern], seed)
    assert S.same_own_choice(got, want)
    P.same_bytes(got, plain)


def single_log(cls):
    """test_hip_tiled's calls on the crafted `single` region (400 bases, partial-span reads in loader coordinates): long enough for
    the column-pair maxima of all columns (k_oldall) behind ScorePoints and Refine"""
    draft, events, par = T.crafted("single", "loader")
    mk = lambda: B.make_pa(cls, draft, copy.deepcopy(events), par)
    out = {"ScoreEvents": mk().ScoreEvents(), "ScorePoints": HT.scores(mk().ScorePoints()), "ScoreMutations": HT.scores(mk().ScoreMutations(T.edits(draft, events, 17)))}
    pa = mk()
    out["Refine"] = (pa.Refine(), pa.sequence, HT.refs(pa))
    pa = mk()
    out["Mutate"] = (pa.Mutate(seqs=[ev.sequence for ev in events[:3]], reps=3), pa.sequence, HT.refs(pa))
    return out


def single_rest(cls):
    """the calls test_hip_tiled's list leaves out, each on an object of its own: PointTable, AlignStats(realign=True),
    ScoreSequences, Mutate('self'), Mutate on a seed list with an unalignable and a duplicate seed, Mutate('viterbi')"""
    draft, events, par = T.crafted("single", "loader")
    mk = lambda: B.make_pa(cls, draft, copy.deepcopy(events), par)
    sc, st = mk().AlignStats(realign=True)
    out = {"PointTable": tuple(mk().PointTable()), "AlignStats": (np.asarray(sc, dtype=np.float64), np.ascontiguousarray(st)),
           "ScoreSequences": mk().ScoreSequences(HT.candidates(draft))}
    pa = mk()
    out["Mutate:self"] = (pa.Mutate(reps=2), pa.sequence, HT.refs(pa))
    pa = mk()
    out["Mutate:seeds"] = (pa.Mutate(seqs=[events[0].sequence, "ACGT" * 6, events[0].sequence, events[1].sequence], reps=2), pa.sequence, HT.refs(pa))
    B.reset_rand()
    pa = mk()
    out["Mutate:viterbi"] = (pa.Mutate(seqs="viterbi", reps=1), pa.sequence, HT.refs(pa))
    return out


@families
@patterns
def test_every_call_on_the_partial_span_region(pattern, fwd_kernel):
    want = HT.oracle_api_results("single", "loader")
    got = single_log(P.CLASSES[pattern])
    assert got["ScoreEvents"] == want["ScoreEvents"]
    for k in ("ScorePoints", "ScoreMutations"):
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:6].tolist())
    for k in ("Refine", "Mutate"):
        assert got[k][:2] == want[k][:2] and HT.same_arrays(got[k][2], want[k][2]), k
    P.same_bytes(got, plain_once(("single", fwd_kernel), lambda: single_log(PSAlign)))


@families
@patterns
def test_the_other_calls_on_the_partial_span_region(pattern, fwd_kernel):
    want = T.oracle_once(("poison_single_rest",), lambda: single_rest(B.OraclePSAlign))
    got = single_rest(P.CLASSES[pattern])
    same_by_key(got, want)
    P.same_bytes(got, plain_once(("single_rest", fwd_kernel), lambda: single_rest(PSAlign)))


def tiny(L):
    """test_hip_parity's sequences of 5 and 12 bases: 1 and 8 states"""
    draft, events, truth = synth.make_region(30, 3, 400 + {5: 1, 12: 4}[L], B.oracle_swalign, P0, draft_error=0.0)
    ev = copy.deepcopy(events)
    for e in ev:
        e.ref_align[e.ref_align > L - 4] = 0
    return draft[:L], ev


def tiny_log(cls, L):
    draft, ev = tiny(L)
    mk = lambda: B.make_pa(cls, draft, copy.deepcopy(ev), P0)
    pa = mk()
    log = [pa.ScoreEvents(), S.listing(pa.ScorePoints()), tuple(pa.PointTable()),
           S.listing(pa.ScoreMutations([S.edit(0, "", "AC"), S.edit(L, "", "G"), S.edit(L + 1, "", "G"), S.edit(1, draft[1:2], "")]))]
    sc, st = pa.AlignStats(realign=True)
    log += [np.asarray(sc, dtype=np.float64), np.ascontiguousarray(st), pa.Refine(), pa.sequence, S.refs(pa)]
    # each of the rest on an object of its own: candidates and seeds are the first event's own sequence of about 30 bases, the short
    # sequence with a substitution, an unalignable and a duplicate seed.  (The short sequence has no error, so no Mutate changes it:
    # find, score and make run and apply nothing.)
    swap = draft[:2] + ("A" if draft[2] != "A" else "C") + draft[3:]
    log.append(mk().ScoreSequences([draft, swap, ev[0].sequence]))
    for seqs in ("self", [ev[0].sequence, "ACGT" * 6, ev[0].sequence, swap], "viterbi"):
        B.reset_rand()
        pa = mk()
        log += [pa.Mutate(seqs=seqs, reps=2), pa.sequence, S.refs(pa)]
    return log


@families
@patterns
@pytest.mark.parametrize("L", [5, 12])
def test_sequences_of_5_and_12_bases(L, pattern, fwd_kernel):
    want = T.oracle_once(("poison_tiny", L), lambda: tiny_log(B.OraclePSAlign, L))
    got = tiny_log(P.CLASSES[pattern], L)
    P.same_bytes(got, want)
    P.same_bytes(got, plain_once(("tiny", L, fwd_kernel), lambda: tiny_log(PSAlign, L)))


PHASE_SHAPES = ("skipped_site", "M257_W8", "E257")


@patterns
@pytest.mark.parametrize("case", PHASE_SHAPES)
def test_support_genotypes_and_phase(case, pattern):
    """the three reductions behind k_score on the shapes of phase_cases: sums and counts by bytes, cis / trans and the genotype
    likelihoods under their derived bounds (phase_cases.check, genotype_cases.same)"""
    draft, events, par, sites, W, lim, S_ = PC.shapes()[case]
    cls = P.CLASSES[pattern]
    mk = lambda c: B.make_pa(c, draft, copy.deepcopy(events), par)
    grp, fr = SC.strands(events), (1 / 3, 0.5)
    want, scores = PC.want_of(("shape", case), draft, events, par, sites, W, lim, S_)
    got = mk(cls).ScoreMutationPhase(sites, window=W, min_link=lim, max_sets=S_)
    PC.check(got, want, scores, "%s, poison %s" % (case, pattern))
    P.same_bytes(got[:5], plain_once(("phase", case), lambda: mk(PSAlign).ScoreMutationPhase(sites, window=W, min_link=lim, max_sets=S_))[:5])

    def geno_want():
        terms = SC.oracle_terms(draft, events, par, sites)
        return SC.loop(draft, events, par, sites, grp, 2, terms=terms), GC.yardstick(terms, len(draft), list(fr))
    sup, geno = T.oracle_once(("poison_geno", case), geno_want)
    sc, rec, scored, lik, nc = mk(cls).ScoreMutationGenotypes(sites, alt_frac=fr)
    print("%s, poison %s: worst |lik - loopld| / bound = %.4f" % (case, pattern, GC.worst(lik, geno)))
    assert SC.same((sc, rec), sup) and SC.score_bytes(scored) == np.asarray(sc).tobytes()
    assert GC.same(lik, nc, geno) and np.array_equal(nc, rec["cover"].sum(axis=1))
    P.same_bytes((sc, rec, lik, nc), (lambda g: (g[0], g[1], g[3], g[4]))(plain_once(("geno", case), lambda: mk(PSAlign).ScoreMutationGenotypes(sites, alt_frac=fr))))
    got = mk(cls).ScoreMutationSupport(sites)
    assert SC.same(got, sup) and SC.score_bytes(got[2]) == np.asarray(got[0]).tobytes()


# ---- the steps inside a round -----------------------------------------------------------------------------------------------------
def round_case(name):
    if name == "work":
        draft, events, par, _ = R.region("work")
        return draft, events, par, R.seed_sets()["mixed7"], ("work", "mixed7")
    draft, events, par, truth = R.region(name)
    return draft, events, par, [truth, truth[30:150]], (name, "truth+slice")


@families
@patterns
@pytest.mark.parametrize("name", ["work", "tiled"])
def test_three_rounds_step_by_step(name, pattern, fwd_kernel):
    """ps_find_mutations, ps_score_mutations, ps_make_mutations, three rounds on one handle, poison between every two C calls: the
    exported lists, the sequence and every event's refs after each step"""
    draft, events, par, seeds, key = round_case(name)
    want = R.oracle_once(("rounds", key), lambda: R.rounds(B.oracle_api(), draft, events, par, seeds))
    api = P.api(pattern)
    n0 = api.calls
    got = R.rounds(api, draft, events, par, seeds)
    assert api.calls - n0 >= 3 * 3 + 2
    assert R.first_difference(got, want) is None
    P.same_bytes(got, plain_once(("rounds", name, fwd_kernel), lambda: R.rounds(hip(), draft, events, par, seeds)))


# ---- Viterbi tables ---------------------------------------------------------------------------------------------------------------
STEP_ROWS = {"T9": lambda: K.random_rows(9, 109), "T33": lambda: K.random_rows(33, 133), "half_neginf": lambda: K.dead_rows("half_neginf")}


@patterns
@pytest.mark.parametrize("nkeep", [16, 0])
@pytest.mark.parametrize("name", list(STEP_ROWS))
def test_viterbi_steps(name, nkeep, pattern):
    """debug_viterbi_steps: back-pointers and final scores equal the ordered scan, the paths the oracle's, the forward table within
    test_hip_viterbi_tables' bound of the long-double recursion, and everything the unpoisoned call's by bytes"""
    rows = STEP_ROWS[name]()
    T_ = len(rows)
    rnd = K.deviates(16, T_, K.DEAD_SEED.get(name, T_))
    run = lambda api: api.debug_viterbi_steps([rows], [rnd] if nkeep else None, nkeep, *HV.ARGS)[0]
    orc = T.oracle_once(("poison_steps", name, nkeep), lambda: run(B.oracle_api()))
    got = run(P.api(pattern))
    HV.check_exact(got, orc, rows)
    assert np.array_equal(got["paths"], orc["paths"]) and (got["fwd"] is None) == (nkeep == 0)
    if name == "half_neginf":
        assert K.dead_counts(got["bp"]) == K.DEAD_CASES[name][2]
    if nkeep:
        (HV.check_forward_until_dead if name == "half_neginf" else HV.check_forward)(got, orc, rows, "%s, poison %s" % (name, pattern))
    P.same_bytes(got, plain_once(("steps", name, nkeep), lambda: run(hip())))


def region_tables(api, reg, nkeep, build):
    B.reset_rand()
    h = api.align_create(reg[0], reg[1], K.P0)
    try:
        return api.debug_viterbi([h], D.batch_cap([reg]), nkeep, *HD.ARGS, obs_build=build)[0]
    finally:
        api.align_destroy(h)


@patterns
@pytest.mark.parametrize("nkeep", [16, 0])
@pytest.mark.parametrize("name,build", [("E9", 0), ("E9", 2), ("E73", 0)])
def test_viterbi_tables_of_deep_stacks(name, build, nkeep, pattern):
    """debug_viterbi on stacks of 9 events (the LDS build and k_vit_obs<64> forced) and 73 (k_vit_obs<256>), the build taken shown
    by the launch counters: emissions against the restatement, every table as test_hip_deep_stacks demands"""
    reg = D.stack(name)
    with HD.counted() as c:
        got = region_tables(P.api(pattern), reg, nkeep, build)
    assert c.builds == HD.only(build or D.expected_build(D.STACKS[name][0])), (name, build, c.builds)      # one launch, of the build named
    HD.check_stack(got, name, nkeep, "%s, build %d, nkeep %d, poison %s" % (name, build, nkeep, pattern), forward=(build == 0 and nkeep == 16))
    P.same_bytes(got, plain_once(("stack", name, build, nkeep), lambda: region_tables(hip(), reg, nkeep, build)))


# ---- Smith-Waterman ---------------------------------------------------------------------------------------------------------------
def sw_cases():
    """(pairs, the oracle's lists, its summaries): the strip-edge lengths of test_hip_sw_band, the byte alphabets of test_hip_sweep
    and one pair of equal lengths whose best alignment lies 300 columns off the diagonal (no band of 128 holds it: the certificate
    fails and the redo batch runs on the buffers of the first)"""
    def make():
        pairs, lists, sums = (list(x) for x in HB._edge_cases())
        for alphabet in HS.ALPHABETS:
            pairs += HS.sw_pairs(alphabet)
            wl, ws = HS.sw_oracle(alphabet)
            lists += list(wl)
            sums += list(ws)
        rng = np.random.default_rng(77)
        x, y, z = (synth.random_sequence(rng, n) for n in (400, 300, 300))
        off = (x + y, z + x)
        w = B.oracle_api().swfull(*off)
        return pairs + [off], lists + [w], sums + [_capi.summary_from_lists(off[0], off[1], *w)]
    return T.oracle_once(("poison_sw",), make)


def sw_run(api, pairs):
    return [api.swfull(a, b) for a, b in pairs], api.sw_summaries(pairs)


@patterns
@pytest.mark.parametrize("fill", list(HS.SW_FILLS))
def test_smith_waterman_lists_and_summaries(fill, pattern):
    pairs, want_lists, want_sums = sw_cases()
    env, must_run, must_not = HS.SW_FILLS[fill]
    with HS.sw_env(env):
        c0 = hip().debug_sw_band()
        with HS.Counters("sw_pk8", "sw_band", "sw_lists", "sw_summary") as c:
            got = sw_run(P.api(pattern), pairs)
        c1 = hip().debug_sw_band()
        plain = plain_once(("sw", fill), lambda: sw_run(hip(), pairs))
    assert c.n["sw_lists"] >= len(pairs) and c.n["sw_summary"] >= 1, c.n
    assert (not must_run or c.n[must_run] > 0) and (not must_not or c.n[must_not] == 0), c.n      # the named fill ran, under poison
    if fill == "band":
        assert c1["banded"] - c0["banded"] >= 2 * len(HB.EDGE_LENGTHS) and c1["fell_back"] - c0["fell_back"] >= 2
    for k, (g, w) in enumerate(zip(got[0], want_lists)):
        assert g[0] == w[0] and HS.same_float(g[1], w[1]), (k, g[:2], w[:2])
        assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]), k
    for k, (g, w) in enumerate(zip(got[1], want_sums)):
        assert tuple(g)[:-1] == tuple(w)[:-1] and HS.same_float(g.accuracy, w.accuracy), (k, g, w)
    P.same_bytes([list(x) for x in got[0]] + [tuple(x) for x in got[1]], [list(x) for x in plain[0]] + [tuple(x) for x in plain[1]])


def map_case():
    draft, events, _ = synth.make_region(333, 3, 4711, B.oracle_swalign, P0)
    rng = np.random.default_rng(4711)
    cands = []
    for rate in (0.02, 0.05):
        s = np.array(list(synth.corrupt(rng, draft, rate, rate, rate)))
        k = rng.choice(s.size, 12, replace=False)
        s[k[:6]] = "N"
        s[k[6:]] = np.char.lower(s[k[6:]])
        cands.append("".join(s))
    return draft, events, cands + [draft[140:] + draft[:140]]      # the last: the draft rotated by 140, its best alignment outside a band of 128


@patterns
@pytest.mark.parametrize("fill", list(HS.SW_FILLS))
def test_score_sequences_map_form(fill, pattern):
    draft, events, cands = T.oracle_once(("poison_map_case",), map_case)
    mk = lambda cls: B.make_pa(cls, draft, copy.deepcopy(events), P0)
    want = T.oracle_once(("poison_sw_map",), lambda: mk(B.OraclePSAlign).ScoreSequences(cands))
    env, must_run, must_not = HS.SW_FILLS[fill]
    with HS.sw_env(env):
        c0 = hip().debug_sw_band()
        with HS.Counters("sw_pk8", "sw_band", "sw_map") as c:
            got = mk(P.CLASSES[pattern]).ScoreSequences(cands)
        c1 = hip().debug_sw_band()
        plain = plain_once(("map", fill), lambda: mk(PSAlign).ScoreSequences(cands))
    assert c.n["sw_map"] > 0 and (not must_run or c.n[must_run] > 0) and (not must_not or c.n[must_not] == 0), c.n
    if fill == "band":
        assert c1["banded"] - c0["banded"] == len(cands) and c1["fell_back"] - c0["fell_back"] >= 1      # sw_map_redo
    assert got.shape == (len(cands), len(events)) and np.array_equal(got, want)
    P.same_bytes(got, plain)


# ---- lock-step --------------------------------------------------------------------------------------------------------------------
def ragged():
    """regions of different L, E, widths and parameters, and one without events: (draft, events, params, edits)"""
    out = []
    for seed in SEEDS:
        draft, holed, clean, par, muts = S.case(seed)
        out.append((draft, holed, par, muts))
    draft, events, par, _ = R.region("work")
    out.append((draft, [], par, end_edits(draft, 1)))
    out.append((draft, events, par, end_edits(draft, 2)))
    return out


def region_alone(cls, reg):
    draft, events, par, muts = reg
    pa = B.make_pa(cls, draft, copy.deepcopy(events), par)
    out = [pa.ScoreEvents(), tuple(pa.PointTable()), S.listing(pa.ScoreMutations(muts))]
    if events:
        out += [pa.Mutate(reps=1), pa.sequence, pa.Refine(), pa.sequence, S.refs(pa)]
    return out


@patterns
@pytest.mark.parametrize("resident", [True, False])
def test_lock_step_batch(resident, pattern):
    """ScoreEvents, PointTable, ScoreMutations, Mutate, Refine on a ragged RegionBatch with poison between the calls: every region
    equals its own unpoisoned PSAlign and the oracle"""
    regs = ragged()
    want = [T.oracle_once(("poison_lock", k), lambda reg=reg: region_alone(B.OraclePSAlign, reg)) for k, reg in enumerate(regs)]
    alone = [plain_once(("lock", k), lambda reg=reg: region_alone(PSAlign, reg)) for k, reg in enumerate(regs)]
    live = [k for k, reg in enumerate(regs) if reg[1]]
    pas = [B.make_pa(PSAlign, d, copy.deepcopy(e), p) for d, e, p, _ in regs]
    with RegionBatch(pas, api=P.api(pattern), resident=resident) as rb:
        se = rb.ScoreEvents()
        pt = rb.PointTable()
        sm = rb.ScoreMutations([reg[3] for reg in regs])
        nm = rb.Mutate(idx=live, reps=1)
        s1 = [pa.sequence for pa in pas]
        nr = rb.Refine(idx=live)
        s2 = [pa.sequence for pa in pas]
        rb.sync()
    for k, reg in enumerate(regs):
        got = [se[k], tuple(pt[k]), S.listing(sm[k])]
        if reg[1]:
            got += [nm[k], s1[k], nr[k], s2[k], S.refs(pas[k])]
        P.same_bytes(got, want[k])
        P.same_bytes(got, alone[k])


# ---- a recycled AlignData slab ----------------------------------------------------------------------------------------------------
@patterns
def test_recycled_align_slab(pattern):
    """a larger handle goes, its slab is poisoned in the cache, a smaller handle takes it over (the cache shrinks by a slab that the
    larger one fitted) and computes what the oracle computes"""
    api, plain = P.api(pattern), hip()
    big_d, big_e, _ = synth.make_region(520, 4, 33, B.oracle_swalign, P0)
    draft, events, par, _ = R.region("work")
    h = plain.align_create(big_d, big_e, P0)
    cached0 = api.poison()["align_cache"].bytes
    plain.align_destroy(h)
    cached1 = api.poison()["align_cache"].bytes
    assert cached1 > cached0
    h = plain.align_create(draft, copy.deepcopy(events), par)
    try:
        taken = cached1 - api.poison()["align_cache"].bytes
        assert 0 < taken <= cached1 - cached0      # the smallest cached slab that fits: the big one's or a smaller one
        hm = api.find_point_mutations(h)
        try:
            hs = api.score_mutations(h, hm)
        finally:
            api.muts_destroy(hm)
        try:
            got = [api.score_alignments(h, len(events)).tolist(), R.listing(api, hs)]
        finally:
            api.muts_destroy(hs)
    finally:
        plain.align_destroy(h)

    def oracle():
        o = B.oracle_api()
        h = o.align_create(draft, copy.deepcopy(events), par)
        try:
            hm = o.find_point_mutations(h)
            hs = o.score_mutations(h, hm)
            o.muts_destroy(hm)
            out = [o.score_alignments(h, len(events)).tolist(), R.listing(o, hs)]
            o.muts_destroy(hs)
            return out
        finally:
            o.align_destroy(h)
    P.same_bytes(got, T.oracle_once(("poison_recycled",), oracle))


# ---- real leftovers, no hook ------------------------------------------------------------------------------------------------------
def leftover_regions():
    big = dict(P0, realign_width=300.0)
    small = dict(P0, realign_width=3.0)
    return synth.make_region(420, 6, 8801, B.oracle_swalign, big)[:2] + (big,), synth.make_region(260, 3, 8802, B.oracle_swalign, small)[:2] + (small,)


CALLS = {
    "ScoreEvents": lambda pa, d: pa.ScoreEvents(),
    "ScorePoints": lambda pa, d: S.listing(pa.ScorePoints()),
    "PointTable": lambda pa, d: tuple(pa.PointTable()),
    "ScoreMutations": lambda pa, d: S.listing(pa.ScoreMutations(end_edits(d, len(d)))),
    "Support": lambda pa, d: pa.ScoreMutationSupport(end_edits(d, len(d)))[:2],
    "AlignStats": lambda pa, d: tuple(np.ascontiguousarray(x) for x in pa.AlignStats(realign=True)),
    "ScoreSequences": lambda pa, d: pa.ScoreSequences(S.candidates(d, len(d))),
    "Refine": lambda pa, d: (pa.Refine(), pa.sequence, S.refs(pa)),
    "Mutate": lambda pa, d: (pa.Mutate(reps=1), pa.sequence, S.refs(pa)),
    "viterbi": lambda pa, d: (B.reset_rand(), pa.Mutate(seqs="viterbi", reps=1), pa.sequence, S.refs(pa))[1:],
}


@families
@pytest.mark.parametrize("call", list(CALLS))
def test_a_small_narrow_region_right_after_a_large_wide_one(call, fwd_kernel):
    """leftovers of the same layout look like plausible scores, which a constant pattern does not: the 260-base, 3-event, width-3
    region run immediately after the 420-base, 6-event, width-300 one on the same thread equals the oracle"""
    (bd, be, bp), (sd, se, sp) = T.oracle_once(("poison_leftover_regions",), leftover_regions)
    want = T.oracle_once(("poison_leftover", call), lambda: CALLS[call](B.make_pa(B.OraclePSAlign, sd, copy.deepcopy(se), sp), sd))
    CALLS[call](B.make_pa(PSAlign, bd, copy.deepcopy(be), bp), bd)
    got = CALLS[call](B.make_pa(PSAlign, sd, copy.deepcopy(se), sp), sd)
    P.same_bytes(got, want)


# ---- the hook itself --------------------------------------------------------------------------------------------------------------
def test_report_names_every_allocated_pool():
    """after calls that touch every subsystem the report names every pool of the table, a class each; what is allocated was
    overwritten over its whole capacity; nothing is exempt today; poisoning twice in a row is fine"""
    import test_poison_table as TT
    table = TT.table()
    api = hip()
    S.full_log(PSAlign, SEEDS[0])                  # the library's own choice of fills (k_fill at this size), then strip sweeps
    try:
        for f in (api.set_sweep_min, api.set_sweep2_min, api.set_sparse_min):
            f(0)
        S.full_log(PSAlign, SEEDS[0])
    finally:
        for f in (api.set_sweep_min, api.set_sweep2_min, api.set_sparse_min):
            f(-1)
    S.own_choice_log(PSAlign, SEEDS[0])
    extra_log(PSAlign, SEEDS[0])
    draft, events, par, sites, W, lim, S_ = PC.shapes()["skipped_site"]
    B.make_pa(PSAlign, draft, copy.deepcopy(events), par).ScoreMutationPhase(sites, window=W, min_link=lim, max_sets=S_)
    with HS.sw_env(HS.SW_FILLS["band"][0]):
        sw_run(hip(), sw_cases()[0][-1:])
        draft, events, cands = T.oracle_once(("poison_map_case",), map_case)
        B.make_pa(PSAlign, draft, copy.deepcopy(events), P0).ScoreSequences(cands[-1:])      # a redone map pair
    rep = P.poison("1e300")
    again = P.poison("ones")
    assert rep == again
    pools = {k: v for k, v in rep.items() if not k.startswith("host:") and k not in ("slab", "align_cache", "stage")}
    assert set(pools) <= set(table), sorted(set(pools) - set(table))
    for name, r in pools.items():
        assert r.cls == table[name][0] and r.skipped == 0, (name, r)
    filled = {k for k, r in pools.items() if r.bytes > 0}
    print("pools overwritten: %d of %d in the table, %.1f MB; slab %.1f MB, align_cache %.1f MB, stage %.1f MB, host %s" %
          (len(filled), len(table), sum(r.bytes for r in pools.values()) / 1e6, rep["slab"].bytes / 1e6, rep["align_cache"].bytes / 1e6,
           rep["stage"].bytes / 1e6, sorted(k for k in rep if k.startswith("host:"))))
    # these calls grow every pool of the table, in a process of their own as well (k_fill's list of workgroups and its step words
    # from the library's own choice of fills, the kept columns from the sparse edit scoring forced above, sw_map_redo from the map pair)
    print("not overwritten (never allocated): %s" % sorted(set(table) - filled))
    assert filled == set(table), sorted(set(table) - filled)
    assert rep["stage"].bytes > 0 and rep["host:sw_res"].bytes > 0 and rep["slab"].skipped == 0 and rep["align_cache"].bytes > 0
    assert not [k for k, r in rep.items() if r.cls == "EXEMPT"]


def test_poison_with_nothing_allocated():
    """a fresh process: the hook is the first call into the library"""
    code = ("import sys; sys.path.insert(0, %r); from poreseq_amd import _capi; r = _capi.load_hip().debug_poison(); "
            "assert r['slab'].bytes == 0 and r['align_cache'].bytes == 0 and r['stage'].bytes == 0, r; "
            "assert not [k for k in r if k not in ('slab', 'align_cache', 'stage')], r; print('PS_OK')" % B.ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ))
    assert out.returncode == 0 and out.stdout.strip().endswith("PS_OK"), out.stderr[-2000:]
