"""CPU: the oracle against the live reference build (oracle/_ref) on the cases of sweep_cases.py — the random lattice sweep and the
three long directed cases that test_hip_sweep.py holds the HIP path to.  Every comparison is exact.  Not a replacement for
test_oracle.py's own sweep, which keeps its seeds and lattice."""
import copy

import numpy as np
import pytest

import backends as B
import sweep_cases as S

need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs the reference sources)")


@need_ref
@pytest.mark.parametrize("seed", S.SEEDS)
def test_oracle_matches_live_reference_on_the_lattice(seed):
    """ScoreEvents, ScorePoints, ScoreMutations, Mutate, Refine, the realigned events, ViterbiMutate on the events as generated
    (the reference's own ViterbiMutate reads out of bounds on alignments with holes), PointTable and ScoreSequences (the
    reference build has neither entry point: both sides run the literal definitions).  ScoreMutationSupport needs per-event terms,
    which the reference build cannot give; test_support.py holds the oracle's to their definition."""
    ref = S.full_log(B.RefPSAlign, seed, B.ref_swalign, holed_viterbi=False)
    orc = S.full_log(B.OraclePSAlign, seed, B.ref_swalign, holed_viterbi=False)
    for k in ref:
        assert ref[k] == orc[k], k
    assert S.same_own_choice(S.own_choice_log(B.RefPSAlign, seed, B.ref_swalign, support=False),
                             S.own_choice_log(B.OraclePSAlign, seed, B.ref_swalign, support=False))


@need_ref
@pytest.mark.parametrize("k", range(len(S.DIRECTED_WIDTHS)))
def test_oracle_matches_live_reference_on_the_directed_cases(k):
    draft, events, P, muts = S.directed(k, B.ref_swalign)
    got = [S.listing(B.make_pa(cls, draft, copy.deepcopy(events), P).ScoreMutations(muts)) for cls in (B.RefPSAlign, B.OraclePSAlign)]
    assert got[0] == got[1]


def test_the_oracle_is_repeatable_on_the_holed_viterbi_leg():
    """the leg the reference cannot run: the same answer twice (the oracle is defined there, test_oracle.py)"""
    for seed in S.SEEDS[:4]:
        a = S.full_log(B.OraclePSAlign, seed)["viterbi_holed"]
        b = S.full_log(B.OraclePSAlign, seed)["viterbi_holed"]
        assert a == b


def test_the_cases_reach_every_value_and_every_size_class():
    """preconditions that keep the sweep from going stale: every lattice value of the four width / offset parameters is drawn by
    some seed, every size class of the edit-scoring kernel is met by some seed's edit list (a scoring band of 0 scores nothing),
    and the directed cases hold edits of more than 64 columns with about 1100 levels per event"""
    seen = {k: set() for k in ("realign_width", "scoring_width", "point_width", "lik_offset")}
    classes = set()
    for seed in S.SEEDS:
        draft, holed, clean, P, muts = S.case(seed)
        for k in seen:
            seen[k].add(P[k])
        classes |= {S.score_class(len(draft), P["scoring_width"], m) for m in muts}
        assert 60 <= len(clean[0].sequence) + 40 and 1 <= len(clean) <= 8
    assert seen["realign_width"] == set(map(float, S.REALIGN)) and seen["scoring_width"] == set(map(float, S.SCORING))
    assert seen["point_width"] == set(map(float, S.POINT)) and seen["lik_offset"] == set(S.OFFSET)
    assert classes >= set(S.SCORE_CLASSES)
    for k in range(len(S.DIRECTED_WIDTHS)):
        draft, events, P, muts = S.directed(k)
        assert all(900 <= ev.mean.size <= 1500 for ev in events)
        assert sum(S.score_class(len(draft), P["scoring_width"], m) == "score_g64" for m in muts) >= 6
