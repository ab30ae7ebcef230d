"""Per-edit read support by event group on the GPU (k_support, ps_score_mutation_support / ps_batch_score_mutation_support):
`PSAlign.ScoreMutationSupport`, `RegionBatch.ScoreMutations` / `ScoreMutationSupport` and `consensus.variant_support` against the
definition's plain loops over the oracle's terms and re-aligned refs (support_cases.loop).  Integer fields equal, doubles by bytes."""
import copy
import ctypes as C
import io
import threading

import numpy as np
import pytest

import backends as B
import support_cases as S
import tiled_cases as T
from poreseq_amd import _capi, synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import variant_region, variant_support
from poreseq_amd.poreseqcpp import PSAlign
from poreseq_amd.util import DEFAULT_PARAMS

pytestmark = pytest.mark.gpu
P0 = dict(DEFAULT_PARAMS, verbose=0)
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]      # conftest's fwd_kernel fixture: the spans come from different backtrace kernels

_MADE = {}


def region(L, E, seed):
    """(draft, events) of a synthetic region, made once"""
    if (L, E, seed) not in _MADE:
        _MADE[(L, E, seed)] = synth.make_region(L, E, seed, B.oracle_swalign, P0)[:2]
    return _MADE[(L, E, seed)]


def hpa(draft, events, par=P0):
    return B.make_pa(PSAlign, draft, copy.deepcopy(events), par)


def want_of(key, draft, events, par, muts, grp, G):
    return T.oracle_once(("hip-support",) + key, lambda: S.loop(draft, events, par, muts, grp, G))


def long_list(draft):
    """the point list, six multi-base edits, one edit at start == L and one that ScoreMutations skips (start > L)"""
    n = len(draft)
    return S.point_list(draft) + [S.edit(7, draft[7:10], "AC"), S.edit(60, "", "GTTA"), S.edit(150, draft[150:152], ""),
                                  S.edit(0, draft[0:3], "G"), S.edit(n - 6, draft[n - 6:n - 2], ""), S.edit(230, draft[230:234], "TGCAT"),
                                  S.edit(n, "", "AC"), S.edit(n + 3, "A", "C")]


@pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)
@pytest.mark.parametrize("name,mode", [("gap", "zeroed"), ("single", "loader")])
def test_crafted_cases_equal_the_loop_under_every_fill(name, mode, fwd_kernel):
    draft, events, par = T.crafted(name, mode)
    grp, muts = S.strands(events), long_list(draft)
    want = want_of((name, mode), draft, events, par, muts, grp, 2)
    pa = hpa(draft, events, par)
    got = pa.ScoreMutationSupport(muts)
    assert S.same(got, want)
    assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))
    assert got[0][-1] == -1e-6 and not got[1][-1]["sum"].any() and not got[1][-1]["cover"].any()           # the skipped edit
    assert got[0].tobytes() == S.score_bytes(hpa(draft, events, par).ScoreMutations(muts))
    assert got[0].tobytes() == T.oracle_once(("hip-support-scores", name, mode), lambda: S.score_bytes(
        B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par).ScoreMutations(muts)))


def _shapes():
    d, e5 = region(120, 5, 7401)
    pts = S.point_list(d)
    inert = copy.deepcopy(e5)
    inert[2].ref_align[:] = 0                   # an event without alignment: no span, its Alignment is a no-op
    return {
        "G1": (d, e5, P0, pts[:300], [0] * 5, 1),
        "G3_empty_middle": (d, e5, P0, pts[:300], [0, 2, 2, 0, 2], 3),
        "G8_E5": (d, e5, P0, pts[:300], [7, 0, 3, 7, 5], 8),
        "E1": (d, e5[:1], P0, pts[:300], [1], 2),
        "M1": (d, e5, P0, pts[400:401], [0, 1, 0, 1, 0], 2),
        "M256": (d, e5, P0, pts[:256], [0, 1, 0, 1, 0], 2),
        "M257": (d, e5, P0, pts[:257], [0, 1, 0, 1, 0], 2),
        "M0": (d, e5, P0, [], [0, 1, 0, 1, 0], 2),
        "inert_event": (d, inert, P0, pts[:300], [0, 1, 0, 1, 0], 2),
        "point_width_0": (d, e5, dict(P0, point_width=0.0), None, [0, 1, 0, 1, 0], 2),
    }


@pytest.mark.parametrize("case", ["G1", "G3_empty_middle", "G8_E5", "E1", "M1", "M256", "M257", "M0", "inert_event", "point_width_0"])
def test_shapes_at_which_the_kernel_can_go_wrong(case):
    draft, events, par, muts, grp, G = _shapes()[case]
    want = want_of(("shape", case), draft, events, par, muts, grp, G)
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        got = hpa(draft, events, par).ScoreMutationSupport(muts, groups=grp, n_groups=G)
        _ms, launches, nbytes = api.prof_get("support")
    finally:
        api.prof_enable(0)
    assert S.same(got, want)
    E, M = len(events), len(want[0])
    assert got[1].shape == (M, G) and len(got[2]) == M
    if M == 0:
        assert launches == 0
    else:
        assert launches == 1 and nbytes == 8.0 * E * M + (8.0 + 24.0 * G) * M
    if case == "G3_empty_middle":
        assert not got[1]["sum"][:, 1].any() and not got[1]["cover"][:, 1].any() and got[1]["cover"][:, 0].any()
    if case == "inert_event":
        lone = hpa(draft, events, par).ScoreMutationSupport(muts, groups=[0, 0, 1, 0, 0], n_groups=2)[1]
        assert not lone["cover"][:, 1].any() and not lone["sum"][:, 1].any()      # cover 0, sum 0.0 in its group


RAGGED = [(120, 1, 7410, 1), (250, 4, 7411, 2), (400, 6, 7412, 3)]     # L, E, seed, G


def _ragged():
    out = []
    for k, (L, E, seed, G) in enumerate(RAGGED):
        d, e = region(L, E, seed)
        muts = S.point_list(d)[k * 11:k * 11 + 150 + 190 * k] + [S.edit(20, d[20:23], "A"), S.edit(len(d), "", "T")]
        out.append((d, e, muts, [i % G for i in range(E)], G))
    return out


@pytest.mark.parametrize("resident", [True, False])
def test_lock_step_equals_the_single_calls_and_the_loop(resident):
    regs = _ragged()
    singles = [hpa(d, e).ScoreMutationSupport(m, groups=g, n_groups=G) for d, e, m, g, G in regs]
    pas = [hpa(d, e) for d, e, _, _, _ in regs]
    rb = RegionBatch(pas, resident=resident)
    try:
        got = rb.ScoreMutationSupport([m for _, _, m, _, _ in regs], groups=[g for _, _, _, g, _ in regs], n_groups=[G for *_, G in regs])
        scored = rb.ScoreMutations([m for _, _, m, _, _ in regs])
        back = rb.ScoreMutationSupport([regs[2][2], regs[0][2]], idx=[2, 0], groups=[regs[2][3], regs[0][3]], n_groups=[3, 1])
        for pa, (d, e, _, _, _) in zip(pas, regs):                        # sequences and Python events are untouched
            assert pa.sequence == d
            assert all(np.array_equal(a.ref_align, b.ref_align) and np.array_equal(a.ref_like, b.ref_like) for a, b in zip(pa.events, e))
        rb.drop()       # (closing a resident batch would write its re-aligned events back)
    finally:
        rb.close()
    for k, (d, e, m, g, G) in enumerate(regs):
        want = want_of(("ragged", k), d, e, P0, m, g, G)
        assert S.same(got[k], want) and S.same(singles[k], want)
        assert S.score_bytes(scored[k]) == want[0].tobytes() == S.score_bytes(got[k][2])
        assert [(s.start, s.orig, s.mut) for s in scored[k]] == [(x.start, x.orig, x.mut) for x in m]
    assert S.same(back[0], singles[2]) and S.same(back[1], singles[0])


def test_other_calls_on_a_resident_batch_are_the_same_before_and_after():
    regs = _ragged()[1:]
    lists = [m for _, _, m, _, _ in regs]

    def digest(tables, scored):
        return [np.ascontiguousarray(a).tobytes() for t in tables for a in t] + [S.score_bytes(s) for s in scored]

    with RegionBatch([hpa(d, e) for d, e, _, _, _ in regs]) as rb:
        before = digest(rb.PointTable(), rb.ScoreMutations(lists))
        rb.ScoreMutationSupport(lists, groups=[g for _, _, _, g, _ in regs], n_groups=[G for *_, G in regs])
        rb.ScoreMutationSupport(None)
        after = digest(rb.PointTable(), rb.ScoreMutations(lists))
        rb.drop()
    assert before == after


def test_two_host_threads_equal_the_calls_alone():
    regs = _ragged()[1:]
    call = lambda k: hpa(regs[k][0], regs[k][1]).ScoreMutationSupport(regs[k][2], groups=regs[k][3], n_groups=regs[k][4])
    alone = [call(0), call(1)]
    got = [None, None]

    def work(k):
        for _ in range(3):
            got[k] = call(k)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert all(S.same(g, a) for g, a in zip(got, alone))


def test_bad_arguments_of_the_c_abi():
    api = _capi.load_hip()
    draft, events = region(120, 5, 7401)
    h = api.align_create(draft, copy.deepcopy(events), P0)
    hm = api.muts_create(S.point_list(draft)[:10])
    try:
        grp = np.array([0, 1, 0, 1, 2], dtype=np.int32)
        sc = np.empty(10)
        rec = np.empty((10, 8), dtype=_capi.EDIT_SUPPORT)
        gp, sp, rp = grp.ctypes.data_as(_capi.c_i32p), _capi._dp(sc), rec.ctypes.data_as(C.POINTER(_capi.PsEditSupport))
        call = lambda G, g=gp, r=rp: api.check(api.lib.ps_score_mutation_support(h, hm, G, g, sp, r))
        for G in (0, 9, -1):
            with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*n_groups = %d, allowed are 1 \.\. 8" % G):   # PS_ERR_BAD_ARG, both numbers
                call(G)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*event 4 has group 2, n_groups = 2"):
            call(2)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null group"):
            call(3, None)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null support"):
            call(3, gp, None)
        call(3)                                                             # the same arrays with a G that fits
        api.check(api.lib.ps_score_mutation_support(h, hm, 3, gp, None, rp))   # scores may be NULL
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\)"):
            api.check(api.lib.ps_score_mutation_support(None, hm, 3, gp, sp, rp))
    finally:
        api.muts_destroy(hm)
        api.align_destroy(h)
    lib = C.CDLL(_capi.HIP_LIB)
    assert hasattr(lib, "ps_score_mutation_support") and hasattr(lib, "ps_batch_score_mutation_support") and api.missing == set()


def test_variant_support_over_two_regions_with_absolute_starts():
    regs = _ragged()[1:]
    starts = [100, 9000]
    absolute = lambda: [[S.edit(s0 + x.start, x.orig, x.mut) for x in m] for (_, _, m, _, _), s0 in zip(regs, starts)]
    ref = io.StringIO()
    for (d, e, _, _, _), ml, s0 in zip(regs, absolute(), starts):
        variant_region(hpa(d, e), ml, region_start=s0, out=ref)
    pas = [hpa(d, e) for d, e, _, _, _ in regs]
    tsv, vcf = io.StringIO(), io.StringIO()
    res = variant_support(pas, absolute(), region_starts=starts, out=tsv)
    variant_support(pas, absolute(), region_starts=starts, out=vcf, fmt="vcf", chrom=["ctgA", "ctgB"])
    lines = tsv.getvalue().splitlines()
    assert lines[0].startswith("#start") and ["\t".join(l.split("\t")[:4]) for l in lines[1:]] == ref.getvalue().splitlines()
    k = 1
    for (d, e, m, _, _), r in zip(regs, res):
        want = want_of(("variant", len(d)), d, e, P0, m, S.strands(e), 2)
        assert S.same(r, want)
        for rec in want[1].tolist():
            assert lines[k].split("\t")[4:] == [str(v) for x in rec for v in (x[1], x[2], x[3], x[0])]
            k += 1
    recs = [l for l in vcf.getvalue().splitlines() if not l.startswith("#")]
    positive = [(ch, s) for ch, r in zip(("ctgA", "ctgB"), res) for s in r[0].tolist() if s > 0]
    assert len(positive) > 0 and len(recs) == len(positive) < len(lines) - 1
    assert [(l.split("\t")[0], l.split("\t")[7].split(";")[0]) for l in recs] == [(ch, "LLR={}".format(s)) for ch, s in positive]
    for pa, (d, e, _, _, _) in zip(pas, regs):
        assert pa.sequence == d and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, e))
