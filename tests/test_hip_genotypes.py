"""Genotype likelihoods per edit on the GPU (k_genotype, ps_score_mutation_genotypes / ps_batch_score_mutation_genotypes):
`PSAlign.ScoreMutationGenotypes`, `RegionBatch.ScoreMutationGenotypes` and `consensus.variant_support(ploidy=...)` against the
definition's plain loops over the oracle's terms and re-aligned refs (genotype_cases, support_cases).  Scores, support records,
n_cover and the hom-alt column by bytes / equality; the mixture columns against the long double loop under the derived bound
2^-52 (16 + n_cover) sum (1 + |d|) — see genotype_cases for where it comes from."""
import copy
import ctypes as C
import io
import threading

import numpy as np
import pytest

import backends as B
import genotype_cases as GC
import support_cases as S
import tiled_cases as T
from poreseq_amd import _capi, synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import variant_support
from poreseq_amd.poreseqcpp import PSAlign
from poreseq_amd.util import DEFAULT_PARAMS, alt_fractions, call_genotypes

pytestmark = pytest.mark.gpu
P0 = dict(DEFAULT_PARAMS, verbose=0)
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]      # conftest's fwd_kernel fixture: the spans come from different backtrace kernels
ENDS = (1e-6, 1.0 - 1e-6)                              # both ends of the allowed range
K8 = (1e-6, 0.01, 0.2, 1 / 3, 0.5, 2 / 3, 0.9, 1.0 - 1e-6)

_MADE = {}


def region(L, E, seed):
    """(draft, events) of a synthetic region, made once"""
    if (L, E, seed) not in _MADE:
        _MADE[(L, E, seed)] = synth.make_region(L, E, seed, B.oracle_swalign, P0)[:2]
    return _MADE[(L, E, seed)]


def hpa(draft, events, par=P0):
    return B.make_pa(PSAlign, draft, copy.deepcopy(events), par)


def want_of(key, draft, events, par, muts, grp, G, fracs):
    """(support_cases.loop's (scores, records), genotype_cases.yardstick) of one case, computed once"""
    def make():
        terms = S.oracle_terms(draft, events, par, muts)
        return S.loop(draft, events, par, muts, grp, G), GC.yardstick(terms, len(draft), list(fracs))
    return T.oracle_once(("hip-genotype",) + key, make)


def check(got, want, tag):
    """every output of one call against the yardsticks; the figure is printed before anything is asserted"""
    scores, rec, scored, lik, nc = got
    sup, geno = want
    print("%s: worst |lik - loopld| / bound = %.4f" % (tag, GC.worst(lik, geno)))
    assert S.same((scores, rec), sup) and S.score_bytes(scored) == np.asarray(scores).tobytes()
    assert GC.same(lik, nc, geno)
    assert np.array_equal(nc, rec["cover"].sum(axis=1))


def long_list(draft):
    """the point list, six multi-base edits, one edit at start == L and one that ScoreMutations skips (start > L)"""
    n = len(draft)
    return S.point_list(draft) + [S.edit(7, draft[7:10], "AC"), S.edit(60, "", "GTTA"), S.edit(150, draft[150:152], ""),
                                  S.edit(0, draft[0:3], "G"), S.edit(n - 6, draft[n - 6:n - 2], ""), S.edit(230, draft[230:234], "TGCAT"),
                                  S.edit(n, "", "AC"), S.edit(n + 3, "A", "C")]


@pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)
@pytest.mark.parametrize("name,mode", [("gap", "zeroed"), ("single", "loader")])
def test_crafted_cases_equal_the_loops_under_every_fill(name, mode, fwd_kernel):
    draft, events, par = T.crafted(name, mode)
    grp, muts, fr = S.strands(events), long_list(draft), (1 / 3, 2 / 3)
    want = want_of((name, mode), draft, events, par, muts, grp, 2, fr)
    pa = hpa(draft, events, par)
    got = pa.ScoreMutationGenotypes(muts, alt_frac=fr)
    check(got, want, "%s/%s %s" % (name, mode, fwd_kernel))
    assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))
    assert got[3].shape == (len(muts), 3) and got[4][-1] == 0 and not got[3][-1].any() and got[0][-1] == -1e-6      # the skipped edit
    assert got[4].max() > 1 and np.count_nonzero(got[3][:, 0]) > 0


def _shapes():
    d, e5 = region(120, 5, 7401)
    pts = S.point_list(d)
    inert = copy.deepcopy(e5)
    inert[2].ref_align[:] = 0                   # an event without alignment: no span, its Alignment is a no-op
    e257 = [copy.deepcopy(e5[i % 5]) for i in range(257)]      # the second SUP_EV staging pass, with the barrier between the passes
    g5 = [0, 1, 0, 1, 0]
    return {
        "M1": (d, e5, P0, pts[400:401], g5, 2, (0.5,)),
        "M256": (d, e5, P0, pts[:256], g5, 2, (0.5,)),
        "M257": (d, e5, P0, pts[:257], g5, 2, (0.25, 0.75)),
        "M0": (d, e5, P0, [], g5, 2, (0.5,)),
        "E1": (d, e5[:1], P0, pts[:300], [1], 2, (0.5,)),
        "E257": (d, e257, P0, pts[230:300], [i % 3 for i in range(257)], 3, (1 / 3, 2 / 3)),
        "inert_event": (d, inert, P0, pts[:300], g5, 2, (0.5,)),
        "K0": (d, e5, P0, pts[:300], g5, 2, ()),
        "K1_low_end": (d, e5, P0, pts[:300], [0] * 5, 1, ENDS[:1]),
        "K1_high_end": (d, e5, P0, pts[:300], [0] * 5, 1, ENDS[1:]),
        "K8": (d, e5, P0, pts[:300], [7, 0, 3, 7, 5], 8, K8),
        "point_width_0": (d, e5, dict(P0, point_width=0.0), None, g5, 2, (0.5,)),
    }


@pytest.mark.parametrize("case", ["M1", "M256", "M257", "M0", "E1", "E257", "inert_event", "K0", "K1_low_end", "K1_high_end", "K8", "point_width_0"])
def test_shapes_at_which_the_kernel_can_go_wrong(case):
    draft, events, par, muts, grp, G, fr = _shapes()[case]
    want = want_of(("shape", case), draft, events, par, muts, grp, G, fr)
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        got = hpa(draft, events, par).ScoreMutationGenotypes(muts, alt_frac=fr, groups=grp, n_groups=G)
        _ms, launches, nbytes = api.prof_get("genotype")
        _ms, sup_launches, sup_bytes = api.prof_get("support")
    finally:
        api.prof_enable(0)
    check(got, want, case)
    E, M, K = len(events), len(want[0][0]), len(fr)
    assert got[3].shape == (M, K + 1) and got[4].shape == (M,) and got[1].shape == (M, G) and len(got[2]) == M
    if M == 0:
        assert launches == 0 and sup_launches == 0
    else:
        assert launches == 1 and nbytes == 8.0 * E * M + (8.0 * (K + 1) + 4.0) * M
        assert sup_launches == 1 and sup_bytes == 8.0 * E * M + (8.0 + 24.0 * G) * M          # the support kernel's own
    if case == "E257":
        assert got[4].max() > 256                                   # edits covered by events of both staging passes
    if case == "inert_event":
        lone = hpa(draft, events, par).ScoreMutationGenotypes(muts, alt_frac=fr, groups=[0, 0, 1, 0, 0], n_groups=2)
        assert not lone[1]["cover"][:, 1].any() and np.array_equal(lone[4], lone[1]["cover"][:, 0]) and lone[3].tobytes() == got[3].tobytes()


def test_null_outputs_through_the_raw_c_call():
    draft, events, par, muts, grp, G, fr = _shapes()["M257"]
    api = _capi.load_hip()
    M, K = len(muts), len(fr)
    full = hpa(draft, events, par).ScoreMutationGenotypes(muts, alt_frac=fr, groups=grp, n_groups=G)
    g = np.array(grp, dtype=np.int32)
    f = np.array(fr, dtype=np.float64)
    gp, fp = g.ctypes.data_as(_capi.c_i32p), _capi._dp(f)

    def fresh(run):
        """`run` on an AlignData of its own (a call re-aligns the events of its handle) -> its result, prof_get of both kernels"""
        h = api.align_create(draft, copy.deepcopy(events), par)
        hm = api.muts_create(muts)
        api.prof_enable(1)
        api.prof_reset()
        try:
            return run(h, hm), api.prof_get("support")[1], api.prof_get("genotype")[1]
        finally:
            api.prof_enable(0)
            api.muts_destroy(hm)
            api.align_destroy(h)

    lik, lik2 = np.full((M, K + 1), 7.0), np.full((M, K + 1), 7.0)
    sc, nc = np.full(M, 7.0), np.full(M, 7, dtype=np.int32)
    _, sup1, gen1 = fresh(lambda h, hm: api.check(api.lib.ps_score_mutation_genotypes(h, hm, G, gp, K, fp, None, None, _capi._dp(lik), None)))   # lik alone
    _, sup2, gen2 = fresh(lambda h, hm: api.check(api.lib.ps_score_mutation_genotypes(h, hm, G, gp, K, fp, _capi._dp(sc), None, _capi._dp(lik2),
                                                                                      nc.ctypes.data_as(_capi.c_i32p))))
    lean, sup3, gen3 = fresh(lambda h, hm: api.score_mutation_genotypes(h, hm, M, g, G, f, want_support=False))
    assert (sup1, sup2, sup3) == (0, 0, 0) and (gen1, gen2, gen3) == (1, 1, 1)     # no records wanted: the support kernel has nothing to write
    assert lik.tobytes() == full[3].tobytes() == lik2.tobytes() == lean[2].tobytes()
    assert sc.tobytes() == full[0].tobytes() == lean[0].tobytes()   # the score then comes from k_genotype: the same bits
    assert np.array_equal(nc, full[4]) and np.array_equal(lean[3], full[4]) and lean[1] is None


RAGGED = [(120, 1, 7410, 1, ()), (250, 4, 7411, 2, (0.5,)), (400, 6, 7412, 3, K8)]     # L, E, seed, G, fractions


def _ragged():
    out = []
    for k, (L, E, seed, G, fr) in enumerate(RAGGED):
        d, e = region(L, E, seed)
        muts = S.point_list(d)[k * 11:k * 11 + 150 + 190 * k] + [S.edit(20, d[20:23], "A"), S.edit(len(d), "", "T")]
        out.append((d, e, muts, [i % G for i in range(E)], G, fr))
    return out


def _want_ragged(k, reg):
    d, e, m, g, G, fr = reg
    return want_of(("ragged", k), d, e, P0, m, g, G, fr)


def _bytes(got):
    return [np.ascontiguousarray(got[i]).tobytes() for i in (0, 1, 3, 4)]


@pytest.mark.parametrize("resident", [True, False])
def test_lock_step_equals_the_single_calls_and_the_loops(resident):
    regs = _ragged()
    singles = [hpa(d, e).ScoreMutationGenotypes(m, alt_frac=fr, groups=g, n_groups=G) for d, e, m, g, G, fr in regs]
    pas = [hpa(r[0], r[1]) for r in regs]
    rb = RegionBatch(pas, resident=resident)
    try:
        got = rb.ScoreMutationGenotypes([r[2] for r in regs], alt_frac=[r[5] for r in regs], groups=[r[3] for r in regs], n_groups=[r[4] for r in regs])
        back = rb.ScoreMutationGenotypes([regs[2][2], regs[0][2]], idx=[2, 0], alt_frac=[regs[2][5], regs[0][5]],
                                         groups=[regs[2][3], regs[0][3]], n_groups=[3, 1])
        for pa, r in zip(pas, regs):                                       # sequences and Python events are untouched
            assert pa.sequence == r[0]
            assert all(np.array_equal(a.ref_align, b.ref_align) and np.array_equal(a.ref_like, b.ref_like) for a, b in zip(pa.events, r[1]))
        rb.drop()       # (closing a resident batch would write its re-aligned events back)
    finally:
        rb.close()
    for k, reg in enumerate(regs):
        want = _want_ragged(k, reg)
        check(got[k], want, "lock-step region %d" % k)
        check(singles[k], want, "single region %d" % k)
        assert _bytes(got[k]) == _bytes(singles[k])
    assert _bytes(back[0]) == _bytes(singles[2]) and _bytes(back[1]) == _bytes(singles[0])


def test_other_calls_on_a_resident_batch_are_the_same_before_and_after():
    regs = _ragged()[1:]
    lists = [r[2] for r in regs]
    kw = dict(groups=[r[3] for r in regs], n_groups=[r[4] for r in regs])

    def digest(tables, scored, support):
        return ([np.ascontiguousarray(a).tobytes() for t in tables for a in t] + [S.score_bytes(s) for s in scored] +
                [np.ascontiguousarray(a).tobytes() for s in support for a in s[:2]])

    with RegionBatch([hpa(r[0], r[1]) for r in regs]) as rb:
        before = digest(rb.PointTable(), rb.ScoreMutations(lists), rb.ScoreMutationSupport(lists, **kw))
        rb.ScoreMutationGenotypes(lists, alt_frac=[r[5] for r in regs], **kw)
        rb.ScoreMutationGenotypes(None)
        after = digest(rb.PointTable(), rb.ScoreMutations(lists), rb.ScoreMutationSupport(lists, **kw))
        rb.drop()
    assert before == after


def test_two_host_threads_equal_the_calls_alone():
    regs = _ragged()[1:]
    call = lambda k: hpa(regs[k][0], regs[k][1]).ScoreMutationGenotypes(regs[k][2], alt_frac=regs[k][5], groups=regs[k][3], n_groups=regs[k][4])
    alone = [call(0), call(1)]
    got = [None, None]

    def work(k):
        for _ in range(3):
            got[k] = call(k)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert all(_bytes(g) == _bytes(a) for g, a in zip(got, alone))
    for k in range(2):
        check(alone[k], _want_ragged(k + 1, regs[k]), "alone %d" % k)


def test_bad_arguments_of_the_c_abi():
    api = _capi.load_hip()
    draft, events = region(120, 5, 7401)
    h = api.align_create(draft, copy.deepcopy(events), P0)
    hm = api.muts_create(S.point_list(draft)[:10])
    try:
        grp = np.array([0, 1, 0, 1, 2], dtype=np.int32)
        fr = np.array([0.5, 0.25, 0.0, 1.0, np.nan, 2e-7, 0.5, 0.5, 0.5], dtype=np.float64)
        sc, lik, nc = np.empty(10), np.empty((10, 9)), np.empty(10, dtype=np.int32)
        rec = np.empty((10, 8), dtype=_capi.EDIT_SUPPORT)
        gp, fp, sp, lp = grp.ctypes.data_as(_capi.c_i32p), _capi._dp(fr), _capi._dp(sc), _capi._dp(lik)
        rp, cp = rec.ctypes.data_as(C.POINTER(_capi.PsEditSupport)), nc.ctypes.data_as(_capi.c_i32p)
        call = lambda G=3, g=gp, K=2, f=fp, l=lp: api.check(api.lib.ps_score_mutation_genotypes(h, hm, G, g, K, f, sp, rp, l, cp))
        for K in (-1, 9):
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*n_frac = %d, allowed are 0 \.\. 8" % K):     # PS_ERR_BAD_ARG, both numbers
                call(K=K)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*alt_frac\[2\] = 0, allowed is 1e-06 \.\. 1 - 1e-06"):     # the first that does not fit
            call(K=5)
        at = lambda i: _capi._dp(fr[i:])
        for i, text in ((3, "1"), (4, "-?nan"), (5, "2e-07")):
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*alt_frac\[0\] = %s, allowed is 1e-06 \.\. 1 - 1e-06" % text):
                call(K=1, f=at(i))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null lik"):
            call(l=None)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null alt_frac with n_frac = 2"):
            call(f=None)
        for G in (0, 9):                                                    # the group arguments: validated as the support call does
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*n_groups = %d, allowed are 1 \.\. 8" % G):
                call(G=G)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*event 4 has group 2, n_groups = 2"):
            call(G=2)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null group"):
            call(g=None)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\)"):
            api.check(api.lib.ps_score_mutation_genotypes(None, hm, 3, gp, 2, fp, sp, rp, lp, cp))
        call()                                                              # the same arrays with arguments that fit: the handle still works
        call(K=0, f=None)                                                   # no fractions: alt_frac may be NULL
        f8 = np.full(8, 0.5)
        call(K=8, f=_capi._dp(f8))
        assert np.isfinite(lik).all() and np.isfinite(sc).all()
    finally:
        api.muts_destroy(hm)
        api.align_destroy(h)
    lib = C.CDLL(_capi.HIP_LIB)
    assert hasattr(lib, "ps_score_mutation_genotypes") and hasattr(lib, "ps_batch_score_mutation_genotypes") and api.missing == set()


def test_variant_support_with_a_ploidy_over_two_regions_with_absolute_starts():
    regs = _ragged()[1:]
    starts = [100, 9000]
    absolute = lambda: [[S.edit(s0 + x.start, x.orig, x.mut) for x in r[2]] for r, s0 in zip(regs, starts)]
    pas = [hpa(r[0], r[1]) for r in regs]
    plain, vcf = io.StringIO(), io.StringIO()
    variant_support(pas, absolute(), region_starts=starts, out=plain, fmt="vcf", chrom=["ctgA", "ctgB"])
    res = variant_support(pas, absolute(), region_starts=starts, out=vcf, fmt="vcf", chrom=["ctgA", "ctgB"], ploidy=2, sample="s1")
    old = [l for l in plain.getvalue().splitlines() if not l.startswith("#")]
    head = [l for l in vcf.getvalue().splitlines() if l.startswith("#")]
    new = [l for l in vcf.getvalue().splitlines() if not l.startswith("#")]
    assert [l for l in head if l.startswith("##FORMAT")] == [l for l in head if "ID=GT," in l or "ID=GQ," in l or "ID=PL," in l] and len(head) == 12
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1"
    assert len(old) > 0 and ["\t".join(l.split("\t")[:8]) for l in new] == old                 # the same records in the same order
    cols = []
    for k, (reg, r) in enumerate(zip(regs, res)):
        d, e, m, _, _, _ = reg
        want = want_of(("variant", k), d, e, P0, m, S.strands(e), 2, alt_fractions(2))
        check(r, want, "variant region %d" % k)
        gt, gq, pl = call_genotypes(want[1][0], want[1][1], 2)
        cols += ["{}:{}:{}".format(gt[i], gq[i], ",".join(str(p) for p in pl[i])) for i in range(len(m)) if r[0][i] > 0]
        assert [s.start for s in r[2]] == [starts[k] + x.start for x in m]
    assert [l.split("\t")[8] for l in new] == ["GT:GQ:PL"] * len(new) and [l.split("\t")[9] for l in new] == cols
    assert len({c.split(":")[0] for c in cols}) > 1
    for pa, r in zip(pas, regs):
        assert pa.sequence == r[0] and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, r[1]))
