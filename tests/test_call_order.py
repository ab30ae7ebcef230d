"""Call order on resident handles.  A `RegionBatch(resident=True)` keeps one native AlignData per region across calls; the
reference builds a fresh one per PSAlign call and writes ref_align / ref_like back only from ApplyMuts, Mutate and Refine
(_poreseqcpp.pyx:375, 434, 471) — ScoreEvents, ScorePoints and ScoreMutations realign a scratch copy and drop it.  So whatever the
order of the calls, three things must be equal after every one of them, in return values, sequences and every event's refs after
`sync()`: the resident batch, the batch that rebuilds its AlignData per call, and the same calls on each region's own PSAlign.

With the default realign_width of 300 a realignment lands where it started, which is why the parameter sets here are different
per region and mostly narrow.  CPU: the oracle library (and the live reference build, where it has the entry points) behind
RegionBatch.  GPU: the HIP library, against itself three ways and against OraclePSAlign."""
import copy

import numpy as np
import pytest

import backends as B
import sweep_cases as S
import tiled_cases as TC
from poreseq_amd import synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign
from poreseq_amd.util import DEFAULT_PARAMS

# (realign_width, scoring_width, point_width, lik_offset) of the four regions on which ScoreEvents -> Refine went wrong
FOUR = ((7, 0, 1, 0.0), (300, 511, 60, 12.0), (45, 9, 5, 4.5), (129, 100, 20, 0.5))
SCORING = ("ScoreEvents", "ScorePoints", "ScoreMutations", "PointTable", "ScoreMutationSupport")   # realign, write nothing back
MUTATING = ("Refine", "Mutate:list", "Mutate:viterbi")
CALLS = SCORING + ("ScoreSequences",) + MUTATING

_regions = {}


def regions():
    """six regions with different parameter sets: the four above and two of the lattice sweep (one with holes and jumps); per
    region (draft, events, params, edits, candidate sequences, seed sequences)"""
    if not _regions:
        out = []
        for k, (W, SW, PW, LO) in enumerate(FOUR):
            P = dict(DEFAULT_PARAMS, verbose=0, realign_width=float(W), scoring_width=float(SW), point_width=float(PW), lik_offset=LO)
            draft, events, _ = synth.make_region(150 + 40 * k, 3 + k, 50 + k, B.oracle_swalign, P)
            rng = np.random.default_rng(50 + k)
            out.append((draft, events, P, synth.random_point_mutations(rng, draft, 12) + [S.edit(20, draft[20:22], "ACGTTGCA"), S.edit(len(draft) - 3, "", "GG")]))
        for seed, holed in ((116, True), (123, False)):
            draft, hv, clean, P, muts = S.case(seed)
            out.append((draft, hv if holed else clean, P, muts))
        _regions["r"] = [(d, e, P, m, S.candidates(d, 70 + k)[:2], [ev.sequence for ev in e[:3]]) for k, (d, e, P, m) in enumerate(out)]
    return _regions["r"]


def sequences():
    """seeded random call sequences of length 5, each with a scoring call directly before a mutating one and at most one
    Mutate('viterbi') (a batch draws every region's deviates from a generator of its own, seeded like a fresh process: the region
    alone is given a fresh generator before that call).  The generator's seed is the first whose six sequences hold all nine calls."""
    rng = np.random.default_rng(901)
    out = []
    while len(out) < 6:
        seq = [str(c) for c in rng.choice(CALLS, 5)]
        if seq.count("Mutate:viterbi") <= 1 and any(a in SCORING and b in MUTATING for a, b in zip(seq, seq[1:])):
            out.append(tuple(seq))
    assert set(sum(out, ())) == set(CALLS)
    return out


def _table(t):
    return [None if t[0] is None else np.nan_to_num(t[0], nan=-12345.0).tolist()] + [x.tolist() for x in t[1:]]


def _support(r):
    return (r[0].tolist(), r[1].tolist(), S.listing(r[2]))


def on_batch(rb, call, regs):
    """one call on every region of the batch: the return values per region, in a form that compares with =="""
    if call == "ScoreEvents":
        return rb.ScoreEvents()
    if call == "ScorePoints":
        return [S.listing(x) for x in rb.ScorePoints()]
    if call == "ScoreMutations":
        return [S.listing(x) for x in rb.ScoreMutations([r[3] for r in regs])]
    if call == "PointTable":
        return [_table(t) for t in rb.PointTable()]
    if call == "ScoreMutationSupport":
        return [_support(x) for x in rb.ScoreMutationSupport([r[3] for r in regs])]
    if call == "ScoreSequences":
        return [x.tolist() for x in rb.ScoreSequences([r[4] for r in regs])]
    if call == "Refine":
        nb = rb.Refine()
        return [nb[i] for i in range(len(regs))]
    if call == "Mutate:list":
        return [rb.Mutate(idx=[i], seqs=r[5], reps=2)[i] for i, r in enumerate(regs)]   # (every region has seed sequences of its own)
    assert call == "Mutate:viterbi"
    nb = rb.Mutate(seqs="viterbi", reps=1)
    return [nb[i] for i in range(len(regs))]


def on_one(pa, call, r):
    if call == "ScoreEvents":
        return pa.ScoreEvents()
    if call == "ScorePoints":
        return S.listing(pa.ScorePoints())
    if call == "ScoreMutations":
        return S.listing(pa.ScoreMutations(r[3]))
    if call == "PointTable":
        return _table(pa.PointTable())
    if call == "ScoreMutationSupport":
        return _support(pa.ScoreMutationSupport(r[3]))
    if call == "ScoreSequences":
        return pa.ScoreSequences(r[4]).tolist()
    if call == "Refine":
        return pa.Refine()
    if call == "Mutate:list":
        return pa.Mutate(seqs=r[5], reps=2)
    assert call == "Mutate:viterbi"
    B.reset_rand()
    return pa.Mutate(seqs="viterbi", reps=1)


def state(pas):
    return [(pa.sequence,) + S.refs(pa) for pa in pas]


def run_batch(cls, regs, seq, resident):
    """[(return values, (sequence, ref_align, ref_like) per region after sync())] after every call of the sequence"""
    pas = [B.make_pa(cls, r[0], copy.deepcopy(r[1]), r[2]) for r in regs]
    log = []
    with RegionBatch(pas, resident=resident) as rb:
        for call in seq:
            ret = on_batch(rb, call, regs)
            rb.sync()
            log.append((ret, state(pas)))
    return log


def run_alone(cls, regs, seq):
    pas = [B.make_pa(cls, r[0], copy.deepcopy(r[1]), r[2]) for r in regs]
    log = []
    for call in seq:
        ret = [on_one(pa, call, r) for pa, r in zip(pas, regs)]
        log.append((ret, state(pas)))
    return log


def first_difference(a, b, seq):
    for k, ((ra, sa), (rb_, sb)) in enumerate(zip(a, b)):
        for r in range(len(ra)):
            if ra[r] != rb_[r]:
                return "call %d (%s), region %d: return values differ" % (k, seq[k], r)
            if sa[r][0] != sb[r][0]:
                return "call %d (%s), region %d: sequences differ" % (k, seq[k], r)
            if sa[r][1:] != sb[r][1:]:
                return "call %d (%s), region %d: ref_align / ref_like differ" % (k, seq[k], r)
    return None


def oracle_alone(regs, seq):
    return TC.oracle_once(("call_order", seq), lambda: run_alone(B.OraclePSAlign, regs, seq))


FIXED = ("ScoreEvents", "Refine")


def check_three_ways(cls, regs, seq):
    alone = run_alone(cls, regs, seq)
    for resident in (True, False):
        got = run_batch(cls, regs, seq, resident)
        assert first_difference(got, alone, seq) is None, ("resident" if resident else "rebuilt per call", first_difference(got, alone, seq))
    return alone


# ---- CPU: the oracle library (and the live reference build) behind RegionBatch ---------------------------------------------------
def test_score_events_then_refine_on_a_resident_batch_oracle():
    """the fixed sequence on the four regions: before ps_align_keep_refs the resident batch applied 1 base in region 0 where the
    region alone applies none, and 18 in region 3 where the region alone applies 20"""
    check_three_ways(B.OraclePSAlign, regions()[:4], FIXED)


@pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs the reference sources)")
def test_score_events_then_refine_on_a_resident_batch_reference():
    regs = regions()[:4]
    alone = check_three_ways(B.RefPSAlign, regs, FIXED)
    assert first_difference(alone, oracle_alone(regs, FIXED), FIXED) is None


@pytest.mark.parametrize("seq", sequences(), ids="-".join)
def test_random_call_sequences_agree_three_ways_oracle(seq):
    regs = regions()
    alone = check_three_ways(B.OraclePSAlign, regs, seq)
    assert first_difference(alone, oracle_alone(regs, seq), seq) is None


def keep_refs_through_the_c_abi(api):
    """ps_align_keep_refs / ps_align_new_call on one handle: keep, score, new_call gives the refs back; keeping twice in a row keeps
    the first; ps_make_mutations forgets the kept refs (the next new_call leaves the realigned ones)"""
    d, e, P = regions()[3][:3]
    E = len(e)
    h = api.align_create(d, copy.deepcopy(e), P)
    try:
        before = api.align_event_refs(h, E)
        for _ in range(2):
            api.check(api.lib.ps_align_new_call(h, int(P["scoring_width"])))
            api.check(api.lib.ps_align_keep_refs(h))
            api.score_alignments(h, E)
        moved = api.align_event_refs(h, E)
        assert not same_arrays(before, moved)
        api.check(api.lib.ps_align_new_call(h, int(P["point_width"])))
        assert same_arrays(before, api.align_event_refs(h, E))
        hm = api.find_point_mutations(h)
        hs = api.score_mutations(h, hm)
        api.make_mutations(h, hs)
        api.muts_destroy(hm); api.muts_destroy(hs)
        after = api.align_event_refs(h, E)
        api.check(api.lib.ps_align_new_call(h, int(P["scoring_width"])))
        assert same_arrays(after, api.align_event_refs(h, E)) and not same_arrays(after, before)
    finally:
        api.align_destroy(h)


def same_arrays(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_library_without_keep_refs_gets_a_scratch_align_data(monkeypatch):
    """ps_align_keep_refs is optional in the binding (checkers built before it existed): RegionBatch then builds a scratch
    AlignData per scoring call from the resident one's written-back state, with the same results"""
    from poreseq_amd import _capi
    B.oracle_api()                      # (builds the library if need be)
    old = _capi.CApi(B.ORACLE_SO)
    old.missing.add("ps_align_keep_refs")
    monkeypatch.setitem(B._cache, "oracle", old)
    check_three_ways(B.OraclePSAlign, regions()[:4], FIXED)
    seq = sequences()[1]
    alone = check_three_ways(B.OraclePSAlign, regions(), seq)
    assert first_difference(alone, oracle_alone(regions(), seq), seq) is None


def test_keep_refs_through_the_c_abi_oracle():
    keep_refs_through_the_c_abi(B.oracle_api())


# ---- GPU: the HIP library ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_keep_refs_through_the_c_abi_hip():
    from poreseq_amd import _capi
    keep_refs_through_the_c_abi(_capi.load_hip())


@pytest.mark.gpu
def test_score_events_then_refine_on_a_resident_batch_hip():
    regs = regions()[:4]
    alone = check_three_ways(PSAlign, regs, FIXED)
    assert first_difference(alone, oracle_alone(regs, FIXED), FIXED) is None


@pytest.mark.gpu
@pytest.mark.parametrize("seq", sequences(), ids="-".join)
def test_random_call_sequences_agree_three_ways_hip(seq):
    regs = regions()
    alone = check_three_ways(PSAlign, regs, seq)
    assert first_difference(alone, oracle_alone(regs, seq), seq) is None
