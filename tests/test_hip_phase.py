"""Phase of het edits on the GPU (k_link, k_phase, k_haptag; ps_score_mutation_phase / ps_batch_score_mutation_phase):
`PSAlign.ScoreMutationPhase`, `RegionBatch.ScoreMutationPhase` and `consensus.variant_support(phase=True)` against the definition's
plain loops over the oracle's terms and re-aligned refs (phase_cases).  Scores, counts, sets, haplotypes and the per-event sums by
bytes / equality; cis / trans against the long double loop under the derived bound 2^-52 (16 + n_both) sum (1 + |da| + |db|); the
phase records also as the float64 replay of the rule on the links the call itself returned — see phase_cases for all three."""
import copy
import ctypes as C
import io
import os
import pickle
import subprocess
import sys
import threading

import numpy as np
import pytest

import backends as B
import phase_cases as PC
import support_cases as S
from poreseq_amd import _capi
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import variant_support
from poreseq_amd.poreseqcpp import PSAlign
from test_batch import SPLIT_DENSE_GB, SPLIT_KEPT_GB, _split_case

pytestmark = pytest.mark.gpu
P0 = PC.P0
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]      # conftest's fwd_kernel fixture: the spans come from different backtrace kernels
SHAPES = ["M1", "M2", "M3_W2", "M9_W8", "M255_W1", "M256_W2", "M257_W8", "M0", "E1", "E257", "inert_event", "skipped_site",
          "every_site_alone", "M63_S1", "M64_S8", "M65_S1", "M129_S8", "sets14_S8", "sets14_S1", "no_events", "tiled_single"]


def hpa(draft, events, par=P0):
    return B.make_pa(PSAlign, draft, copy.deepcopy(events), par)


def _bytes(got):
    return [np.ascontiguousarray(got[i]).tobytes() for i in (0, 1, 2, 3)] + [got[4]]


@pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)
@pytest.mark.parametrize("name", list(PC.DIPLOID))
def test_diploid_regions_are_phased_under_every_fill(name, fwd_kernel):
    draft, events, ev_hap, edits, _carrier = PC.diploid(name)
    want, scores = PC.want_of(("diploid", name), draft, events, P0, edits, 2, 0.0, 4)
    pa = hpa(draft, events)
    got = pa.ScoreMutationPhase(edits)
    PC.check(got, want, scores, "diploid %s %s" % (name, fwd_kernel))
    assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))
    _sc, _link, phase, hap, n_sets, _scored = got
    assert n_sets == 1 and phase["hap"].tolist() == [1, -1, 1, -1]
    assert (hap["lik1"][:, 0] > hap["lik2"][:, 0]).tolist() == [h == 1 for h in ev_hap]


def test_shapes_cover_the_cases_shared_with_the_cpu_tests():
    assert sorted(SHAPES) == sorted(PC.shapes())


@pytest.mark.parametrize("case", SHAPES)
def test_shapes_at_which_the_kernels_can_go_wrong(case):
    draft, events, par, sites, W, lim, S_ = PC.shapes()[case]
    want, scores = PC.want_of(("shape", case), draft, events, par, sites, W, lim, S_)
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        got = hpa(draft, events, par).ScoreMutationPhase(sites, window=W, min_link=lim, max_sets=S_)
        prof = {k: api.prof_get(k)[1:] for k in ("link", "phase", "haptag", "genotype", "support")}
    finally:
        api.prof_enable(0)
    PC.check(got, want, scores, case)
    E, M = len(events), len(sites)
    assert got[0].shape == (M,) and got[1].shape == (M, W) and got[2].shape == (M,) and got[3].shape == (E, S_) and len(got[5]) == M
    assert not got[1]["reserved"].any() and prof["genotype"][0] == 0 and prof["support"][0] == 0
    if M == 0 or E == 0:
        assert [prof[k][0] for k in ("link", "phase", "haptag")] == [0, 0, 0]
    else:
        assert prof["link"] == (1, 8.0 * E * M + 32.0 * W * M)
        assert prof["phase"] == (1, (32.0 * W + 16.0) * M)
        assert prof["haptag"] == (1, 8.0 * E * M + 16.0 * M + 24.0 * S_ * E)
    if case == "E257":
        assert got[1]["n_both"].max() > 256                                 # pairs shared by events of both staging passes
    if case == "every_site_alone":
        assert got[4] == M > S_ and got[2]["set"].tolist() == list(range(M)) and (np.abs(got[2]["vote"][1:]) > 1).all()
    if case == "no_events":
        assert got[4] == M and (got[0] == -1e-6).all() and not got[1]["n_both"].any()
    if case == "tiled_single":
        assert set(np.unique(got[1]["n_both"]).tolist()) >= {1, 2, 3, 4} and got[1]["n_both"].max() < E


def test_null_outputs_through_the_raw_c_call():
    draft, events, par, sites, W, lim, S_ = PC.shapes()["sets14_S8"]
    api = _capi.load_hip()
    M, E = len(sites), len(events)
    full = hpa(draft, events, par).ScoreMutationPhase(sites, window=W, min_link=lim, max_sets=S_)

    def fresh(run):
        """`run` on an AlignData of its own (a call re-aligns the events of its handle) -> its result, the three launch counts"""
        h = api.align_create(draft, copy.deepcopy(events), par)
        hm = api.muts_create(sites)
        api.prof_enable(1)
        api.prof_reset()
        try:
            return run(h, hm), [api.prof_get(k)[1] for k in ("link", "phase", "haptag")]
        finally:
            api.prof_enable(0)
            api.muts_destroy(hm)
            api.align_destroy(h)

    link, phase = np.zeros((M, W), dtype=_capi.EDIT_LINK), np.zeros(M, dtype=_capi.EDIT_PHASE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _, n1 = fresh(lambda h, hm: api.check(api.lib.ps_score_mutation_phase(h, hm, W, lim, S_, None, vp(link), vp(phase), None, None)))
    lean, n2 = fresh(lambda h, hm: api.score_mutation_phase(h, hm, M, E, W, lim, S_, want_hap=False))
    assert n1 == [1, 1, 0] and n2 == [1, 1, 0]                              # nobody wants the events tagged: k_haptag is not launched
    assert link.tobytes() == full[1].tobytes() == lean[1].tobytes() and phase.tobytes() == full[2].tobytes() == lean[2].tobytes()
    assert lean[0].tobytes() == full[0].tobytes() and lean[3] is None and lean[4] == full[4] == 14


RAGGED = [("M9_W8", "M65_S1", "skipped_site"), ("tiled_single", "M0", "no_events", "M257_W8")]      # different M, E, window, max_sets


@pytest.mark.parametrize("resident", [True, False])
def test_lock_step_equals_the_single_calls_and_the_loops(resident):
    names = RAGGED[0] if resident else RAGGED[1]
    cs = [PC.shapes()[n] for n in names]
    kw = lambda c: dict(window=c[4], min_link=c[5], max_sets=c[6])
    singles = [hpa(c[0], c[1], c[2]).ScoreMutationPhase(c[3], **kw(c)) for c in cs]
    pas = [hpa(c[0], c[1], c[2]) for c in cs]
    rb = RegionBatch(pas, resident=resident)
    try:
        got = rb.ScoreMutationPhase([c[3] for c in cs], window=[c[4] for c in cs], min_link=[c[5] for c in cs], max_sets=[c[6] for c in cs])
        back = rb.ScoreMutationPhase([cs[2][3], cs[0][3]], idx=[2, 0], window=[cs[2][4], cs[0][4]], min_link=0.0, max_sets=[cs[2][6], cs[0][6]])
        for pa, c in zip(pas, cs):                                          # sequences and Python events are untouched
            assert pa.sequence == c[0]
            assert all(np.array_equal(a.ref_align, b.ref_align) and np.array_equal(a.ref_like, b.ref_like) for a, b in zip(pa.events, c[1]))
        rb.drop()       # (closing a resident batch would write its re-aligned events back)
    finally:
        rb.close()
    for n, c, g, one in zip(names, cs, got, singles):
        want, scores = PC.want_of(("shape", n), *c)
        PC.check(g, want, scores, "lock-step " + n)
        PC.check(one, want, scores, "single " + n)
        assert _bytes(g) == _bytes(one)
    assert _bytes(back[0]) == _bytes(singles[2]) and _bytes(back[1]) == _bytes(singles[0])


def test_other_calls_on_a_resident_batch_are_the_same_before_and_after():
    cs = [PC.shapes()[n] for n in ("M9_W8", "skipped_site")]
    lists = [c[3] for c in cs]
    digest = lambda tables, scored: [np.ascontiguousarray(a).tobytes() for t in tables for a in t] + [S.score_bytes(s) for s in scored]
    with RegionBatch([hpa(c[0], c[1]) for c in cs]) as rb:
        before = digest(rb.PointTable(), rb.ScoreMutations(lists))
        rb.ScoreMutationPhase(lists, window=3)
        after = digest(rb.PointTable(), rb.ScoreMutations(lists))
        rb.drop()
    assert before == after


def test_two_host_threads_equal_the_calls_alone():
    cs = [PC.shapes()[n] for n in ("sets14_S8", "tiled_single")]
    call = lambda k: hpa(cs[k][0], cs[k][1], cs[k][2]).ScoreMutationPhase(cs[k][3], window=cs[k][4], min_link=cs[k][5], max_sets=cs[k][6])
    alone = [call(0), call(1)]
    got = [None, None]

    def work(k):
        for _ in range(3):
            got[k] = call(k)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert all(_bytes(g) == _bytes(a) for g, a in zip(got, alone))
    for k, n in enumerate(("sets14_S8", "tiled_single")):
        PC.check(alone[k], *PC.want_of(("shape", n), *cs[k]), "alone " + n)


_HERE = os.path.dirname(os.path.abspath(__file__))
SPLIT_KW = PC.SPLIT_KW
# the child process of the test below: the phase call on the three regions of test_batch._split_case, pickled to argv[2]
_SPLIT_CHILD = (
    "import copy, pickle, sys\n"
    "sys.path[:0] = [%r, %r]\n"
    "import backends as B\n"
    "from test_batch import _split_case, P\n"
    "from test_hip_phase import SPLIT_KW\n"
    "from poreseq_amd import _capi\n"
    "from poreseq_amd.batch import RegionBatch\n"
    "from poreseq_amd.poreseqcpp import PSAlign\n"
    "api = _capi.load_hip()\n"
    "if sys.argv[1] == 'kept': api.set_sparse_min(0)\n"
    "regs, sup_lists, sm_lists, groups = _split_case()\n"
    "rb = RegionBatch([B.make_pa(PSAlign, d, copy.deepcopy(ev), P) for d, ev in regs])\n"
    "out = [r[:5] for r in rb.ScoreMutationPhase(sup_lists, **SPLIT_KW)] + [r[:5] for r in rb.ScoreMutationPhase(sm_lists, **SPLIT_KW)]\n"
    "rb.drop(); rb.close()\n"
    "pickle.dump(out, open(sys.argv[2], 'wb'))\n"
) % (os.path.dirname(_HERE), _HERE)


def test_phase_calls_survive_being_cut_into_sub_batches(tmp_path):
    """Both split paths of the edit-scoring chain, forced as tests/test_batch.py forces them for the other kinds: three regions (the
    middle one without events), once with an empty list among them and once with none empty.  A batch is cut between regions, never
    inside a list: byte for byte the outputs of the call that was not cut (made in this process), and those equal the loops.  Two
    child processes, as the knobs are read once per process."""
    def run(mode, extra):
        path = str(tmp_path / (mode + ".pkl"))
        env = dict(os.environ, PORESEQ_TRACE="1", **extra)
        r = subprocess.run([sys.executable, "-c", _SPLIT_CHILD, mode, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        with open(path, "rb") as f:
            return pickle.load(f), r.stderr

    regs, sup_lists, sm_lists, _groups = _split_case()
    from test_batch import P
    with RegionBatch([B.make_pa(PSAlign, d, copy.deepcopy(ev), P) for d, ev in regs], resident=False) as rb:
        plain = [r[:5] for r in rb.ScoreMutationPhase(sup_lists, **SPLIT_KW)] + [r[:5] for r in rb.ScoreMutationPhase(sm_lists, **SPLIT_KW)]
    dense, err1 = run("dense", {"PORESEQ_DEBUG_GUESS_P": "64", "PORESEQ_NO_SWEEP": "1", "PORESEQ_MAX_BATCH_GB": SPLIT_DENSE_GB})
    kept, err2 = run("kept", {"PORESEQ_MAX_BATCH_GB": SPLIT_KEPT_GB})
    assert "over the share: split" in err1 and "[ps] score_mutations: 1 regions" in err1 and "kept columns\n" not in err1
    assert any("[ps] score_mutations: 1 regions" in l and l.endswith(": kept columns") for l in err2.splitlines())
    assert any("[ps] score_mutations: 2 regions" in l and l.endswith(": kept columns") for l in err2.splitlines())
    assert [_bytes(r) for r in dense] == [_bytes(r) for r in plain] and [_bytes(r) for r in kept] == [_bytes(r) for r in plain]
    lists = sup_lists + sm_lists
    for (k, i), want, scores in PC.split_wants():
        scored = [S.edit(m.start, m.orig, m.mut) for m in lists[3 * k + i]]
        for m, s in zip(scored, plain[3 * k + i][0]):
            m.score = float(s)
        PC.check(plain[3 * k + i] + (scored,), want, scores, "split lists %d region %d" % (k, i))


def test_bad_arguments_of_the_c_abi():
    api = _capi.load_hip()
    draft, events = PC.region(120, 5, 7401)
    h = api.align_create(draft, copy.deepcopy(events), P0)
    hm = api.muts_create(S.point_list(draft)[300:310])
    try:
        sc, link, phase = np.empty(10), np.zeros((10, 8), dtype=_capi.EDIT_LINK), np.zeros(10, dtype=_capi.EDIT_PHASE)
        hap, ns = np.zeros((5, 8), dtype=_capi.EVENT_HAP), np.zeros(1, dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        call = lambda W=2, lim=0.0, S_=4, l=vp(link), p=vp(phase): api.check(api.lib.ps_score_mutation_phase(
            h, hm, W, lim, S_, _capi._dp(sc), l, p, vp(hap), ns.ctypes.data_as(_capi.c_i32p)))
        for W in (0, 9, -1):
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*window = %d, allowed are 1 \.\. 8" % W):     # PS_ERR_BAD_ARG
                call(W=W)
        for S_ in (0, 9):
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*max_sets = %d, allowed are 1 \.\. 8" % S_):
                call(S_=S_)
        for lim, text in ((-1.0, "-1"), (float("nan"), "-?nan"), (float("inf"), "inf"), (-0.5, "-0.5")):
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*min_link = %s, allowed is a finite value >= 0" % text):
                call(lim=lim)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null link"):
            call(l=None)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null phase"):
            call(p=None)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\)"):
            api.check(api.lib.ps_score_mutation_phase(None, hm, 2, 0.0, 4, None, vp(link), vp(phase), None, None))
        bad = api.muts_create([S.edit(-1, "A", "C")])                       # what ps_score_mutations rejects
        try:
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*negative mutation start"):
                api.check(api.lib.ps_score_mutation_phase(h, bad, 2, 0.0, 4, None, vp(link), vp(phase), None, None))
        finally:
            api.muts_destroy(bad)
        call()                                                              # the same arrays with arguments that fit: the handle still works
        call(W=8, S_=8, lim=1.7976931348623157e308)
        assert ns[0] == 10 and np.isfinite(sc).all()
        none = api.muts_create([])
        try:
            ns[0], hap["n1"] = 7, 7
            api.check(api.lib.ps_score_mutation_phase(h, none, 2, 0.0, 8, None, vp(link), vp(phase), vp(hap), ns.ctypes.data_as(_capi.c_i32p)))
            assert ns[0] == 0 and not hap["n1"].any()                       # an empty list: PS_OK, no set, no event tagged
        finally:
            api.muts_destroy(none)
    finally:
        api.muts_destroy(hm)
        api.align_destroy(h)
    lib = C.CDLL(_capi.HIP_LIB)
    assert hasattr(lib, "ps_score_mutation_phase") and hasattr(lib, "ps_batch_score_mutation_phase") and api.missing == set()


def test_variant_support_phases_the_diploid_regions_as_on_the_cpu():
    regs = [PC.diploid("400"), PC.diploid("260")]
    pas = [hpa(r[0], r[1]) for r in regs]
    out = io.StringIO()
    res = variant_support(pas, PC.variant_lists(), out=out, phase=True, **PC.VARIANT_KW)
    text = out.getvalue().splitlines()
    assert PC.VARIANT_PS_LINE in text
    assert "".join(l + "\n" for l in text if not l.startswith("#")) == PC.VARIANT_BODY          # the CPU test's text
    for r, reg in zip(res, regs):
        assert r[5].tolist() == [1 if h == 1 else 2 for h in reg[2]] and r[6][0] == [1, 2, 4, 5] and r[6][4] == 1
    for pa, reg in zip(pas, regs):
        assert pa.sequence == reg[0] and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, reg[1]))
