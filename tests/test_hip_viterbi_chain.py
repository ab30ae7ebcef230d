"""ViterbiMutate through the cut of a lock-step call into sub-batches: the concatenation of the sub-batches' paths, the region index
a refusal names, and the regions' own generators across the cut.  No other test makes that cut happen: the cap of one sub-batch is
max(1e9, 0.9 x share) bytes of tables, and every other Viterbi test stays far below 1 GB.

Where the cut occurs.  PORESEQ_MAX_BATCH_GB=1 (read at every call, as test_batch.py sets its budgets) makes the cap
max(1e9, 0.9e9) = 1e9 bytes.  The library's estimate per region is 26 * 1024 * T + 32 * T * E bytes for T kept positions and E events:
26 688 bytes per position at E = 2.  The four regions are synth.make_region(L, 2, seed, draft_error=0): the truth is the draft, no
Smith-Waterman is needed.  ref_cases.viterbi_positions counts T on the CPU (the test asserts the figures):

    region   L       T        bytes by the estimate
    0        12560   12449    332 238 912
    1        12560   12445    332 132 160
    2        12560   12430    331 731 840      regions 0-2: 37 324 positions, 996 102 912 bytes  <= 1e9: one sub-batch
    3         3000    2972     79 316 736      with region 3: 1 075 419 648 bytes > 1e9: it goes alone

Without the budget the share is tens of GB and the call is one launch group; with it, two (the profile's "viterbi" entry counts one
per sub-batch).  The dead region of the refusal test (edge_cases, tier E: three events, 245 positions, 6 546 400 bytes) is cut off
too: 996 102 912 + 6 546 400 = 1 002 649 312 > 1e9.  The region that keeps no position (ref_cases' all_unaligned) takes 0 bytes, so
regions 0, 2 and 3 fit the cap beside it and that call is not cut with or without the budget; it is run both ways all the same.

Each call runs about 12 500 sequential steps per region, the regions side by side, over about 1 GB of tables."""
import copy

import pytest

import edge_cases as EC
import ref_cases as RC
from poreseq_amd import _capi, synth

pytestmark = pytest.mark.gpu

VIT = RC.VIT
REGIONS = ((12560, 8801), (12560, 8802), (12560, 8803), (3000, 8804))      # (length, seed), two events each
POSITIONS = (12449, 12445, 12430, 2972)
DEAD, DEAD_POSITIONS = "vit_mean_overflow", 245
CAP = 1e9
BUDGET_GB = "1"
BAD_ARG = "(-1)"


def need(T, E):
    """the library's estimate of a region's tables, in bytes"""
    return 26.0 * 1024.0 * T + 32.0 * T * E


def regions():
    """[(draft, events, params)] of the four regions; made once, handed out as copies"""
    made = RC.once(("viterbi_chain", "regions"), lambda: [synth.make_region(L, 2, seed, None, RC.P0, draft_error=0)[:2] for L, seed in REGIONS])
    return [(d, copy.deepcopy(ev), dict(RC.P0)) for d, ev in made]


def refs_bytes(events):
    return [(ev.ref_align.tobytes(), ev.ref_like.tobytes()) for ev in events]


class handles:
    """AlignData of the regions, and a way to make fresh generators (seed 1: rand() of a fresh process) for every call"""

    def __init__(self, regs):
        self.api, self.regs = _capi.load_hip(), regs
        self.hs, self.rngs = [], []

    def __enter__(self):
        for d, ev, p in self.regs:
            self.hs.append(self.api.align_create(d, copy.deepcopy(ev), p))
        return self

    def fresh_rngs(self):
        new = [self.api.rng_create(1) for _ in self.hs]
        self.rngs += new
        return new

    def batch(self, nkeep):
        return self.api.batch_viterbi_mutate(self.hs, self.fresh_rngs(), nkeep, *VIT)

    def refs(self):
        """(ref_align, ref_like) bytes of every event of every region, as the handles hold them now"""
        out = []
        for h, (d, ev, p) in zip(self.hs, self.regs):
            mine = copy.deepcopy(ev)
            self.api.align_update_events(h, mine)
            out.append(refs_bytes(mine))
        return out

    def __exit__(self, *exc):
        for g in self.rngs:
            self.api.rng_destroy(g)
        for h in self.hs:
            self.api.align_destroy(h)


def alone(reg, nkeep):
    """ps_viterbi_mutate of one region with the generator of a fresh process"""
    api = _capi.load_hip()
    h = api.align_create(reg[0], copy.deepcopy(reg[1]), reg[2])
    try:
        api.srand(1)
        return api.viterbi_mutate(h, nkeep, *VIT, 0)
    finally:
        api.align_destroy(h)


def alone_all(nkeep):
    """the four regions one by one; computed once per session and left unchanged"""
    return RC.once(("viterbi_chain", "alone", nkeep), lambda: [alone(r, nkeep) for r in regions()])


def counted(api, call):
    """(the call's result, launch groups the profile counted as "viterbi" during it)"""
    api.prof_enable(1)
    try:
        api.prof_reset()
        out = call()
        return out, api.prof_get("viterbi")[1]
    finally:
        api.prof_enable(0)


def test_the_sizes_put_the_cut_where_the_docstring_says():
    """(CPU arithmetic: the positions the walk keeps, and what the greedy cut makes of the library's estimate)"""
    T = [len(RC.viterbi_positions(ev)) for _, ev, _ in regions()]
    assert tuple(T) == POSITIONS
    first3 = sum(need(t, 2) for t in T[:3])
    assert first3 <= CAP < first3 + need(T[3], 2) and need(T[3], 2) < 0.25 * need(T[0], 2)
    dead = EC.region(DEAD)[1]
    assert len(dead) == 3 and len(RC.viterbi_positions(dead)) == DEAD_POSITIONS and first3 + need(DEAD_POSITIONS, 3) > CAP
    assert RC.viterbi_positions(RC.case("all_unaligned")[1]) == []


@pytest.mark.parametrize("nkeep", [16, 0])
def test_cut_batch_equals_uncut_batch_equals_regions_alone(nkeep, monkeypatch):
    regs = regions()
    before = [refs_bytes(ev) for _, ev, _ in regs]
    with handles(regs) as H:
        uncut, n_uncut = counted(H.api, lambda: H.batch(nkeep))
        monkeypatch.setenv("PORESEQ_MAX_BATCH_GB", BUDGET_GB)
        cut, n_cut = counted(H.api, lambda: H.batch(nkeep))
        monkeypatch.delenv("PORESEQ_MAX_BATCH_GB")
        after = H.refs()
    print("nkeep %d: launch groups uncut %d, cut %d; sequences per region %s" % (nkeep, n_uncut, n_cut, [len(s) for s in cut]))
    assert (n_uncut, n_cut) == (1, 2)
    assert [len(s) for s in uncut] == [max(nkeep, 1)] * 4
    assert cut == uncut
    assert uncut == alone_all(nkeep)
    assert after == before


@pytest.mark.parametrize("nkeep", [16, 0])
def test_a_region_that_keeps_no_position_returns_no_sequences(nkeep, monkeypatch):
    regs = regions()
    regs[1] = RC.case("all_unaligned")
    want = alone_all(nkeep)
    with handles(regs) as H:
        uncut = H.batch(nkeep)
        monkeypatch.setenv("PORESEQ_MAX_BATCH_GB", BUDGET_GB)
        under_budget = H.batch(nkeep)
        monkeypatch.delenv("PORESEQ_MAX_BATCH_GB")
    for got in (uncut, under_budget):
        assert got[1] == []
        assert [got[k] for k in (0, 2, 3)] == [want[k] for k in (0, 2, 3)]


def test_a_refusal_names_the_callers_region_index_across_the_cut(monkeypatch):
    regs = regions()
    regs[3] = EC.region(DEAD)
    api = _capi.load_hip()
    fresh = api.align_create(regs[0][0], copy.deepcopy(regs[0][1]), regs[0][2])
    try:
        score_before = api.score_alignments(fresh, 2).tolist()
    finally:
        api.align_destroy(fresh)
    with handles(regs) as H:
        monkeypatch.setenv("PORESEQ_MAX_BATCH_GB", BUDGET_GB)
        api.prof_enable(1)
        try:
            api.prof_reset()
            with pytest.raises(_capi.PoreseqError) as err:
                H.batch(0)
            groups = api.prof_get("viterbi")[1]
        finally:
            api.prof_enable(0)
        monkeypatch.delenv("PORESEQ_MAX_BATCH_GB")
        msg = str(err.value)
        print(msg, "| launch groups", groups)
        assert BAD_ARG in msg and "ps_batch_viterbi_mutate: region 3: " in msg and "region 0" not in msg, msg
        assert EC.UNREACHABLE % EC.VIT_FIRST_DEAD[DEAD] in msg, msg
        assert groups == 2
        # the other AlignData stay usable: the decode of the three, and one ScoreEvents as a fresh handle answers it
        assert api.batch_viterbi_mutate(H.hs[:3], H.fresh_rngs()[:3], 0, *VIT) == alone_all(0)[:3]
        assert api.score_alignments(H.hs[0], 2).tolist() == score_before
