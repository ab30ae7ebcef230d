"""Deep event stacks through the emission builds of ps_viterbi.hip (tests/deep_cases.py): k_vit_obs_lds (up to 72 events),
k_vit_obs<64> and k_vit_obs<256>, each asked for every number of contributing events it takes, on either side of 64 / 65, 72 / 73
and 256 / 257, alone and in lock-step batches of very unequal depths.  Tolerance 0 throughout: T and the emission rows are the
oracle's and the plain restatement's (deep_cases.trimmed_row) bit for bit, back-pointers and final scores viterbi_ref's, state
paths the oracle's; the forward vectors are held by the rule of test_hip_viterbi_tables.check_forward.  The launch counters
vit_obs_lds / vit_obs_64 / vit_obs_256 (prof_get) say which build a call took; every test prints them.

test_deep_stacks.py holds the same inputs to their preconditions and the oracle to the restatement on the CPU."""
import copy

import numpy as np
import pytest

import backends as B
import deep_cases as D
import ref_cases as RC
import test_hip_viterbi_tables as HV
import viterbi_cases as K
import viterbi_ref as V
from poreseq_amd import _capi
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu
ARGS = (K.SKIP, K.STAY, K.MMIN, K.MMAX)
TABLES = ("obs", "bp", "lik_final", "fwd", "paths")
UNSUPPORTED, BAD_ARG = "(-4)", "(-1)"


class counted:
    """the emission builds launched inside the block: {build: launches}"""

    def __enter__(self):
        self.api = _capi.load_hip()
        self.api.prof_enable(1)
        self.api.prof_reset()
        self.builds = {}
        return self

    def __exit__(self, *exc):
        try:
            self.builds = {b: self.api.prof_get(name)[1] for b, name in D.COUNTERS.items()}
        finally:
            self.api.prof_enable(0)
        return False


def only(build, n=1):
    return {b: (n if b == build else 0) for b in D.COUNTERS}


def hip_tables(regs, nkeep, build=0):
    """debug_viterbi of the HIP library over the regions [(draft, events)] in one call"""
    hip = _capi.load_hip()
    hs = []
    try:
        for draft, events in regs:
            hs.append(hip.align_create(draft, events, K.P0))
        return hip.debug_viterbi(hs, D.batch_cap(regs), nkeep, *ARGS, obs_build=build)
    finally:
        for h in hs:
            hip.align_destroy(h)


def check_stack(got, name, nkeep, what, forward=False):
    walk, obs = D.restated(name)
    want = D.oracle_tables(name, nkeep)
    bp, lik = D.steps_ref(name)
    assert got["T"] == want["T"] == len(walk) > 0, what
    if not np.array_equal(got["obs"], obs):
        t = int(np.flatnonzero((got["obs"] != obs).any(axis=1))[0])
        raise AssertionError("%s: emissions differ from the restatement first at position %d (%d contributors)" % (what, t, len(walk[t][1])))
    assert np.array_equal(got["obs"], want["obs"]), what
    assert np.array_equal(got["bp"], bp) and np.array_equal(got["lik_final"], lik), what
    assert np.array_equal(got["paths"], want["paths"]), what
    assert (got["fwd"] is None) == (nkeep == 0)
    if forward and V.HAVE_LD:
        HV.check_forward(got, want, obs, what)


@pytest.mark.parametrize("name", D.NAMES)
def test_stack_tables_under_every_emission_build(name):
    """the default call and every build that admits E: all tables at nkeep 16 and 0, the build taken shown by the counters; the
    builds that do not admit E refuse"""
    E = D.STACKS[name][0]
    reg = [D.stack(name)]
    admitted = K.admitted_builds(E)
    for b in [0] + admitted:
        took = b or D.expected_build(E)
        for nkeep in (16, 0):
            B.reset_rand()
            with counted() as c:
                got = hip_tables(reg, nkeep, b)[0]
            print("%s (E = %d), build asked %d, nkeep %d: launches %s" % (name, E, b, nkeep, {D.COUNTERS[k]: v for k, v in c.builds.items()}))
            assert c.builds == only(took), (name, b, c.builds)
            check_stack(got, name, nkeep, "%s, build %d, nkeep %d" % (name, b, nkeep), forward=(b == 0 and nkeep == 16))
    for b in sorted({1, 2, 3} - set(admitted)):
        with counted() as c:
            with pytest.raises(_capi.PoreseqError):
                hip_tables(reg, 16, b)
        assert c.builds == only(0, 0)


# ---- 256 / 257 ------------------------------------------------------------------------------------------------------------------------
def test_257_events_are_refused_and_the_library_lives_on():
    hip, orc = _capi.load_hip(), B.oracle_api()
    draft, events = D.stack257()
    B.reset_rand()
    before = hip_tables([D.stack("E9")], 16)[0]

    def refused(call):
        with counted() as c:
            with pytest.raises(_capi.PoreseqError) as err:
                call()
        assert UNSUPPORTED in str(err.value) and D.TOO_MANY in str(err.value), str(err.value)
        assert c.builds == only(0, 0)

    h = hip.align_create(draft, copy.deepcopy(events), K.P0)
    try:
        for nkeep in (16, 0):
            refused(lambda: hip.debug_viterbi([h], len(draft) + 64, nkeep, *ARGS))
        refused(lambda: hip.debug_viterbi([h], len(draft) + 64, 16, *ARGS, obs_build=3))
        refused(lambda: hip.viterbi_mutate(h, 16, *ARGS, 0))
        # the same handle still scores
        want = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), K.P0).ScoreEvents()
        assert hip.score_alignments(h, len(events)).tolist() == want
    finally:
        hip.align_destroy(h)
    # a lock-step Mutate('viterbi'), next to a region that any build takes
    d9, e9 = D.stack("E9")
    pas = [B.make_pa(PSAlign, d9, e9, K.P0), B.make_pa(PSAlign, draft, copy.deepcopy(events), K.P0)]
    with RegionBatch(pas) as rb:
        refused(lambda: rb.Mutate(seqs="viterbi", reps=1))
    assert pas[0].sequence == d9 and pas[1].sequence == draft
    with pytest.raises(_capi.PoreseqError) as err:
        B.make_pa(PSAlign, draft, copy.deepcopy(events), K.P0).Mutate(seqs="viterbi", reps=1)
    assert D.TOO_MANY in str(err.value)
    # the oracle takes it
    got = RC.viterbi_tables(orc, draft, events, K.P0, 0, len(draft) + 64)
    assert got["T"] == D.oracle_tables("E256", 0)["T"] > 0 and np.all(np.isfinite(got["obs"]))
    # and the library is as usable as before
    B.reset_rand()
    after = hip_tables([D.stack("E9")], 16)[0]
    assert after["T"] == before["T"]
    for k in TABLES:
        assert after[k].tobytes() == before[k].tobytes(), k
    check_stack(after, "E9", 16, "E9 after the refusals")


# ---- batches of very unequal depths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with73", (True, False), ids=("E1_73_T0_9_72", "E1_T0_9_72"))
def test_mixed_batch_tables_equal_the_regions_alone(with73):
    """one debug_viterbi call over regions of 1, 73, (no position), 9 and 72 events: each region's tables are those of the region
    run alone, by bytes, and the oracle's; one build serves all of them: k_vit_obs<256> with the 73-event member, k_vit_obs_lds
    (at the LDS size of 72 events) without it.  The deviates come from one generator in region order either way."""
    regs = D.mixed_batch(with73, middle="no positions")
    names = ["E73", None, "E9", "E72"] if with73 else [None, "E9", "E72"]
    B.reset_rand()
    with counted() as c:
        got = hip_tables(regs, 16)
    print("batch of E = %s: launches %s" % ([len(ev) for _, ev in regs], {D.COUNTERS[k]: v for k, v in c.builds.items()}))
    assert c.builds == only(3 if with73 else 1)
    B.reset_rand()
    alone = [hip_tables([reg], 16)[0] for reg in regs]
    orc, hs = B.oracle_api(), []
    B.reset_rand()
    try:
        for draft, events in regs:
            hs.append(orc.align_create(draft, copy.deepcopy(events), K.P0))
        want = orc.debug_viterbi(hs, D.batch_cap(regs), 16, *ARGS)
    finally:
        for h in hs:
            orc.align_destroy(h)
    middle = 2 if with73 else 1
    assert [g["T"] > 0 for g in got] == [r != middle for r in range(len(regs))]
    assert len(set(g["T"] for g in got)) >= len(regs) - 1
    for r, (g, a, w) in enumerate(zip(got, alone, want)):
        assert g["T"] == a["T"] == w["T"], r
        for k in TABLES:
            assert g[k].tobytes() == a[k].tobytes(), (r, k)
        for k in ("obs", "bp", "lik_final", "paths"):
            assert np.array_equal(g[k], w[k]), (r, k)
    for g, name in zip(got[1:], names):
        if name:
            assert np.array_equal(g["obs"], D.restated(name)[1]) and np.array_equal(g["bp"], D.steps_ref(name)[0]), name
    B.reset_rand()
    got0 = hip_tables(regs, 0)
    for g, w in zip(got0, want):
        assert np.array_equal(g["bp"], w["bp"]) and g["fwd"] is None
    for g, name in zip(got0[1:], names):
        if name:
            assert np.array_equal(g["paths"], D.oracle_tables(name, 0)["paths"]), name


def test_viterbi_calls_refuse_a_region_without_events():
    """alone and inside a batch, as the oracle does (test_deep_stacks.py): nothing is launched"""
    hip = _capi.load_hip()
    regs = D.mixed_batch(True)
    hs = [hip.align_create(d, e, K.P0) for d, e in regs]
    try:
        for batch in (hs, hs[2:3]):
            with counted() as c:
                with pytest.raises(_capi.PoreseqError) as err:
                    hip.debug_viterbi(batch, D.batch_cap(regs), 16, *ARGS)
            assert "no events" in str(err.value) and c.builds == only(0, 0)
    finally:
        for h in hs:
            hip.align_destroy(h)


def _scored(lst):
    return [(s.start, s.orig, s.mut, s.score) for s in lst]


def _same(a, b):
    """equal results of a PSAlign call: numbers, strings, None, arrays (by bytes), lists and tuples of those"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) == type(b) and a == b


def region_calls(cls, reg, seed):
    """what one PSAlign of the class answers for the region: ScoreEvents, ScoreMutations, PointTable, AlignStats"""
    draft, events = reg
    mk = lambda: B.make_pa(cls, draft, copy.deepcopy(events), K.P0)
    scores, stats = mk().AlignStats()
    return [mk().ScoreEvents(), _scored(mk().ScoreMutations(D.short_edits(draft, seed))), tuple(mk().PointTable()),
            (None if scores is None else np.asarray(scores, dtype=np.float64), stats)]


def region_mutate(cls, reg):
    draft, events = reg
    B.reset_rand()
    pa = B.make_pa(cls, draft, copy.deepcopy(events), K.P0)
    return [pa.Mutate(seqs="viterbi", reps=1), pa.sequence] + RC.refs(pa)


@pytest.mark.parametrize("with73", (True, False), ids=("E1_73_0_9_72", "E1_0_9_72"))
def test_mixed_batch_through_region_batch(with73):
    """RegionBatch over E = (1, 73, 0, 9, 72) and over (1, 0, 9, 72): every call answers per region what the region's own PSAlign
    answers and what the oracle's does; the region without events answers as it does alone (empty results; Mutate('viterbi')
    refuses it either way)"""
    regs = D.mixed_batch(with73)
    R = len(regs)
    empty = 2 if with73 else 1
    seeds = [7800 + len(ev) for _, ev in regs]
    alone = [region_calls(PSAlign, reg, s) for reg, s in zip(regs, seeds)]
    want = [RC.once(("deep calls", len(reg[1])), lambda reg=reg, s=s: region_calls(B.OraclePSAlign, reg, s)) for reg, s in zip(regs, seeds)]
    pas = [B.make_pa(PSAlign, d, copy.deepcopy(e), K.P0) for d, e in regs]
    with RegionBatch(pas) as rb:
        stats = rb.AlignStats()
        got = [rb.ScoreEvents(), [_scored(x) for x in rb.ScoreMutations([D.short_edits(d, s) for (d, _), s in zip(regs, seeds)])],
               [tuple(x) for x in rb.PointTable()], [(None if sc is None else np.asarray(sc, dtype=np.float64), st) for sc, st in stats]]
        for r in range(R):
            for k, what in enumerate(("ScoreEvents", "ScoreMutations", "PointTable", "AlignStats")):
                assert _same(got[k][r], alone[r][k]), (what, r, "batch against the region alone")
                assert _same(got[k][r], want[r][k]), (what, r, "batch against the oracle")
        assert got[0][empty] == [] and got[3][empty][1].shape == (0,)
        # Mutate('viterbi'): refused with the region without events in it, as that region is alone
        with counted() as c:
            with pytest.raises(_capi.PoreseqError) as err:
                rb.Mutate(seqs="viterbi", reps=1)
        assert BAD_ARG in str(err.value) and "ps_batch_viterbi_mutate" in str(err.value) and c.builds == only(0, 0)
        with pytest.raises(_capi.PoreseqError) as err:
            B.make_pa(PSAlign, *regs[empty], K.P0).Mutate(seqs="viterbi", reps=1)
        assert BAD_ARG in str(err.value) and "ps_viterbi_mutate" in str(err.value)
        live = [r for r in range(R) if r != empty]
        with counted() as c:
            nb = rb.Mutate(idx=live, seqs="viterbi", reps=1)
        print("Mutate('viterbi') over E = %s: launches %s" % ([len(regs[r][1]) for r in live], {D.COUNTERS[k]: v for k, v in c.builds.items()}))
        assert c.builds == only(3 if with73 else 1)
    for r in live:
        got_r = [nb[r], pas[r].sequence] + RC.refs(pas[r])
        for cls in (PSAlign, B.OraclePSAlign):
            ref = RC.once(("deep mutate", cls.__name__, "E%d" % len(regs[r][1])), lambda: region_mutate(cls, regs[r]))
            assert got_r[:2] == ref[:2] and RC.same_arrays(got_r[2:], ref[2:]), (r, cls.__name__)
    assert pas[empty].sequence == regs[empty][0]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.END_TO_END)
def test_mutate_viterbi_end_to_end(name):
    """Mutate('viterbi', reps = 1) on the stacks at the builds' limits: the returned base count, the sequence and every event's
    final refs are the oracle's"""
    reg = D.stack(name)
    with counted() as c:
        got = region_mutate(PSAlign, reg)
    want = RC.once(("deep mutate", "OraclePSAlign", name), lambda: region_mutate(B.OraclePSAlign, reg))
    print("%s: %d bases changed; launches %s" % (name, got[0], {D.COUNTERS[k]: v for k, v in c.builds.items()}))
    assert c.builds == only(D.expected_build(D.STACKS[name][0]))
    assert got[0] == want[0] > 0 and got[1] == want[1] != reg[0]
    assert RC.same_arrays(got[2:], want[2:])
