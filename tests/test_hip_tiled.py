"""Partial-span reads on the HIP path (tests/tiled_cases.py) against the oracle, under all four fill families: reads that start or
stop inside the region, in the three representations a caller can hand them over in.  What full-span events never reach: a band
pinned to the first or last rows for longer than the strip sweeps' LDS rings (`pinned`), full-frame events whose every strip is in
band on every column (`short`), k_updaterefs extrapolating over long heads and tails, ViterbiMutate's stop (`gap`) and skip
(`single`) branches with refstart differing between events, edits scored where no read or one read lies.

Every comparison is exact, except the forward probabilities of ViterbiMutate, which keep the rule and the helper of
test_hip_viterbi_tables.py.  The oracle's results are computed once per case and shared between the families (tiled_cases.oracle_once).
conftest.py fans only test_hip_parity and test_hip_variant over the families, so this module asks for them itself.

No mismatch was found on an MI355X when the module was written.  A failure here is either a product bug in the band, ring,
feeder, k_updaterefs, vit_gather or sparse-column code — the DP test names the first differing column — or a limit of the library
on these inputs, and is to be treated as a finding."""
import copy

import numpy as np
import pytest

import backends as B
import tiled_cases as TC
import viterbi_cases as K
import viterbi_ref as V
from point_cases import same
from test_hip_viterbi_tables import check_region
from poreseq_amd import _capi, synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]
families = pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)      # topmost decorator: the family varies fastest
need_ld = pytest.mark.skipif(not V.HAVE_LD, reason="np.longdouble has no 64-bit mantissa on this machine")


def scores(lst):
    return np.array([s.score for s in lst])


def refs(pa):
    return [ev.ref_align.copy() for ev in pa.events] + [ev.ref_like.copy() for ev in pa.events]


def same_arrays(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def partial_events(name):
    """events whose span is not the whole genome piece (event 0 of every case but `gap` covers everything)"""
    L, M, _, spans, _ = TC.CRAFTED[name]
    return [e for e, (s, t) in enumerate(spans) if s > -M or t < L + M]


class Profiled:
    """the launches of the two fill families while the block runs"""

    def __enter__(self):
        self.api = _capi.load_hip()
        self.api.prof_enable(1)
        self.api.prof_reset()
        return self

    def __exit__(self, *exc):
        self.sweeps, self.fills = self.api.prof_get("sweep")[1], self.api.prof_get("fill")[1]
        self.waves = {k: self.api.prof_get(k)[1] for k in ("sweep_w2", "sweep_w4")}
        self.api.prof_enable(0)
        return False

    def ran(self, family):
        """the family's kernel ran and the other's did not; for the two- and four-wavefront sweeps, sweeps on that many wavefronts
        did run (the library steps down to fewer wavefronts when no form of the asked width fits an alignment)"""
        if family == "fill":
            return self.fills > 0 and self.sweeps == 0
        return self.sweeps > 0 and self.fills == 0 and self.waves.get(family, 1) > 0


# ---- DP tables ------------------------------------------------------------------------------------------------------------------
_tables = {}


def oracle_fill(name, mode, e, d):
    """the oracle's debug_fill tables; only the current (case, representation) is kept (the L = 1500 matrices are 6 MB each)"""
    if _tables.get("key") != (name, mode):
        _tables.clear()
        _tables["key"] = (name, mode)
    if (e, d) not in _tables:
        draft, events, par = TC.crafted(name, mode)
        _tables[(e, d)] = TC.fill_tables(B.oracle_api(), draft, events, par, e, d)
    return _tables[(e, d)]


@families
@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("name", TC.NAMES)
def test_dp_matrices_bit_exact(name, mode, fwd_kernel):
    """forward and backward main / stay matrices and the forward step codes of every partial event"""
    draft, events, par = TC.crafted(name, mode)
    hip = _capi.load_hip()
    for e in partial_events(name):
        for d in (0, 1):
            with Profiled() as prof:
                got = TC.fill_tables(hip, draft, events, par, e, d)
            assert prof.ran(fwd_kernel), (fwd_kernel, prof.sweeps, prof.fills, prof.waves)
            for k, (x, y) in enumerate(zip(got, oracle_fill(name, mode, e, d))):
                if d == 1 and k >= 2:
                    continue   # backward step codes are not kept (nothing reads them)
                if not np.array_equal(x, y, equal_nan=True):
                    differs = ~((x == y) | (np.isnan(x.astype(np.float64)) & np.isnan(y.astype(np.float64))))
                    cols = np.flatnonzero(differs.any(axis=0))
                    raise AssertionError("event %d, direction %d, table %d: first differing column %d (rows %s), %d cells differ"
                                         % (e, d, k, cols[0], np.flatnonzero(differs[:, cols[0]])[:8].tolist(), int(differs.sum())))


# ---- API ------------------------------------------------------------------------------------------------------------------------
def oracle_api_results(name, mode):
    def make():
        draft, events, par = TC.crafted(name, mode)
        mk = lambda: B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)
        out = {"ScoreEvents": mk().ScoreEvents(), "Coverage": mk().Coverage(), "ScorePoints": scores(mk().ScorePoints()),
               "ScoreMutations": scores(mk().ScoreMutations(TC.edits(draft, events, 17)))}
        pa = mk()
        out["Refine"] = (pa.Refine(), pa.sequence, refs(pa))
        pa = mk()
        out["Mutate"] = (pa.Mutate(seqs=[ev.sequence for ev in events[:3]], reps=3), pa.sequence, refs(pa))
        return out
    return TC.oracle_once(("api", name, mode), make)


@families
@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("name", TC.NAMES)
def test_api_parity_with_oracle(name, mode, fwd_kernel):
    draft, events, par = TC.crafted(name, mode)
    want = oracle_api_results(name, mode)
    api = _capi.load_hip()
    mk = lambda: B.make_pa(PSAlign, draft, copy.deepcopy(events), par)
    with Profiled() as prof:
        assert mk().ScoreEvents() == want["ScoreEvents"]
    assert prof.ran(fwd_kernel), (fwd_kernel, prof.sweeps, prof.fills, prof.waves)
    assert np.array_equal(mk().Coverage(), want["Coverage"])
    assert np.array_equal(scores(mk().ScorePoints()), want["ScorePoints"])
    muts = TC.edits(draft, events, 17)
    try:
        for sparse_min in (0, 1 << 30):          # kept columns, then whole matrices
            api.set_sparse_min(sparse_min)
            got = scores(mk().ScoreMutations(muts))
            bad = np.flatnonzero(got != want["ScoreMutations"])
            assert bad.size == 0, (sparse_min, [(int(k), muts[k].start, muts[k].orig, muts[k].mut, got[k], want["ScoreMutations"][k]) for k in bad[:6]])
    finally:
        api.set_sparse_min(0 if fwd_kernel != "fill" else 1 << 30)
    pa = mk()
    nb, seq, rf = want["Refine"]
    assert pa.Refine() == nb and pa.sequence == seq and same_arrays(refs(pa), rf)
    pa = mk()
    nb, seq, rf = want["Mutate"]
    assert pa.Mutate(seqs=[ev.sequence for ev in events[:3]], reps=3) == nb and pa.sequence == seq and same_arrays(refs(pa), rf)


# ---- Viterbi --------------------------------------------------------------------------------------------------------------------
VITERBI = [("crafted", n, m) for n in ("gap", "single") for m in TC.MODES] + [("random", s, m) for s in range(1, 7) for m in TC.MODES]


def make_case(kind, key, mode):
    return TC.crafted(key, mode) if kind == "crafted" else TC.random_tiled(key, mode)


@need_ld
@pytest.mark.parametrize("kind,key,mode", VITERBI)
def test_viterbi_tables_under_every_emission_build(kind, key, mode):
    """T, the trimmed-mean emissions, back-pointers, final scores and state paths exact; forward vectors by the rule of
    test_hip_viterbi_tables.py (error against the long-double recursion within 4x the oracle's own)"""
    draft, events, par = make_case(kind, key, mode)
    want = TC.oracle_once(("vit", kind, key, mode, 16), lambda: TC.viterbi_tables(B.oracle_api(), draft, events, par, 16))
    builds = K.admitted_builds(len(events))
    assert builds == [1, 2, 3]
    for b in [0] + builds:
        got = TC.viterbi_tables(_capi.load_hip(), draft, events, par, 16, b)
        check_region(got, want, "%s %s %s, build %d" % (kind, key, mode, b), forward=b in (0, builds[-1]))
    want0 = TC.oracle_once(("vit", kind, key, mode, 0), lambda: TC.viterbi_tables(B.oracle_api(), draft, events, par, 0))
    got = TC.viterbi_tables(_capi.load_hip(), draft, events, par, 0)
    assert got["T"] == want0["T"] and got["fwd"] is None
    assert np.array_equal(got["paths"], want0["paths"]) and np.array_equal(got["bp"], want0["bp"]) and np.array_equal(got["obs"], want0["obs"])


def seed_lists(api, draft, events, par, k):
    """ps_viterbi_mutate's sequences for nkeep 0 and 16 after a realign, the generators seeded as test_viterbi_stochastic_seeds_sweep does"""
    import ctypes
    out = []
    for nkeep in (0, 16):
        ctypes.CDLL(None).srand(100 + k)
        _capi.load_hip().srand(100 + k)
        h = api.align_create(draft, copy.deepcopy(events), par)
        try:
            api.score_alignments(h, len(events))
            out.append(api.viterbi_mutate(h, nkeep, *TC.VIT, 0))
        finally:
            api.align_destroy(h)
    return out


@families
@pytest.mark.parametrize("kind,key,mode", VITERBI)
def test_viterbi_seed_lists(kind, key, mode, fwd_kernel):
    draft, events, par = make_case(kind, key, mode)
    k = VITERBI.index((kind, key, mode))
    want = TC.oracle_once(("seeds", kind, key, mode), lambda: seed_lists(B.oracle_api(), draft, events, par, k))
    got = seed_lists(_capi.load_hip(), draft, events, par, k)
    assert len(got[0]) == 1 and len(got[1]) == 16
    assert got == want


# ---- the consensus schedule -----------------------------------------------------------------------------------------------------
def schedule(cls, draft, events, par):
    """Mutate('self'), then {Mutate('viterbi'), Refine} until unchanged: calls, returns and sequences"""
    B.reset_rand()
    pa = B.make_pa(cls, draft, copy.deepcopy(events), par)
    log = [("Mutate:self", pa.Mutate(reps=4), pa.sequence)]
    for _ in range(4):
        log.append(("Mutate:viterbi", pa.Mutate(seqs="viterbi"), pa.sequence))
        nb = pa.Refine()
        log.append(("Refine", nb, pa.sequence))
        if nb == 0:
            break
    return log, refs(pa)


@families
@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("kind,key", [("crafted", "single"), ("random", 7)])
def test_consensus_schedule_matches_oracle(kind, key, mode, fwd_kernel):
    draft, events, par = make_case(kind, key, mode)
    want = TC.oracle_once(("schedule", kind, key, mode), lambda: schedule(B.OraclePSAlign, draft, events, par))
    got = schedule(PSAlign, draft, events, par)
    assert got[0] == want[0]
    assert same_arrays(got[1], want[1])


# ---- lock-step ------------------------------------------------------------------------------------------------------------------
def lock_step_regions():
    d, e, _ = synth.make_region(300, 5, 7105, B.oracle_swalign, TC.P0)
    return [TC.crafted("gap", "zeroed"), TC.crafted("pinned", "truncated"), TC.crafted("short", "loader"), (d, copy.deepcopy(e), dict(TC.P0))]


def alone(cls, draft, events, par):
    """ScoreEvents, Refine, Mutate('viterbi') and PointTable of one region on its own"""
    pa = B.make_pa(cls, draft, copy.deepcopy(events), par)
    out = [pa.ScoreEvents(), pa.Refine(), pa.sequence]
    B.reset_rand()
    out += [pa.Mutate(seqs="viterbi"), pa.sequence]
    rf = refs(pa)
    return out, pa.PointTable(), rf


@families
def test_lock_step_batch_equals_regions_alone_and_the_oracle(fwd_kernel):
    regs = lock_step_regions()
    want = TC.oracle_once(("lock_step",), lambda: [alone(B.OraclePSAlign, *r) for r in regs])
    single = [alone(PSAlign, *r) for r in regs]
    pas = [B.make_pa(PSAlign, d, copy.deepcopy(e), p) for d, e, p in regs]
    with RegionBatch(pas) as rb:
        se = rb.ScoreEvents()
        nb = rb.Refine()
        s1 = [pa.sequence for pa in pas]
        nv = rb.Mutate(seqs="viterbi")
        s2 = [pa.sequence for pa in pas]
        rb.sync()
        rf = [refs(pa) for pa in pas]            # (PointTable leaves a resident handle's refs as it found them: tests/test_call_order.py)
        tables = rb.PointTable()
    for r, pa in enumerate(pas):
        got = [se[r], nb[r], s1[r], nv[r], s2[r]]
        for other in (single[r], want[r]):
            assert got == other[0], r
            assert same(tables[r], other[1]), r
            assert same_arrays(rf[r], other[2]), r


# ---- the reference's recorded outputs --------------------------------------------------------------------------------------------
@families
@pytest.mark.parametrize("name", TC.GOLDEN_CASES)
def test_golden_replay(name, fwd_kernel):
    """tests/golden/tiled.npz, recorded from the reference build: the replay does not need that build (the inputs of `pinned` are
    regenerated from the seed, which takes the oracle library's aligner; the stored cases need neither)"""
    TC.check_golden(PSAlign, name)


# ---- newer entry points ---------------------------------------------------------------------------------------------------------
def candidates(draft):
    rng = np.random.default_rng(23)
    return [synth.corrupt(rng, draft, 0.02, 0.02, 0.02), synth.corrupt(rng, draft, 0.05, 0.05, 0.05), synth.corrupt(rng, draft[30:-30], 0.01, 0.01, 0.01)]


@families
@pytest.mark.parametrize("mode", TC.MODES)
def test_point_table_and_score_sequences_on_single_coverage(mode, fwd_kernel):
    draft, events, par = TC.crafted("single", mode)
    mk = lambda cls: B.make_pa(cls, draft, copy.deepcopy(events), par)
    want = TC.oracle_once(("newer", mode), lambda: (mk(B.OraclePSAlign).PointTable(), mk(B.OraclePSAlign).ScoreSequences(candidates(draft))))
    assert same(mk(PSAlign).PointTable(), want[0])
    got = mk(PSAlign).ScoreSequences(candidates(draft))
    assert got.shape == (3, len(events)) and np.array_equal(got, want[1])
