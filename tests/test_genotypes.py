"""Genotype likelihoods per edit on the CPU checkers: the path of a library without ps_score_mutation_genotypes
(PSAlign.ScoreMutationGenotypes / RegionBatch.ScoreMutationGenotypes over util.genotypes_from_deltas) against the definition's plain
loops (genotype_cases), identities of the definition, util.call_genotypes on canned values, the VCF / TSV writers of
consensus.variant_support with a ploidy, the preconditions that keep the crafted cases from going stale, and the symbols."""
import copy
import ctypes
import io
import math
import os
import re

import numpy as np
import pytest

import backends as B
import genotype_cases as GC
import support_cases as S
import tiled_cases as T
from poreseq_amd import _capi, batch
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import variant_support
from poreseq_amd.util import MutationScore, alt_fractions, call_genotypes, genotypes_from_deltas
from test_support import EDITS, RECS, SEQ, TSV, VCF, VCF_HEAD

CASES = [("gap", "zeroed"), ("single", "loader")]
NEW = ("ps_score_mutation_genotypes", "ps_batch_score_mutation_genotypes")


def case(name, mode, ploidy):
    """(draft, events, params, groups, support_cases.loop's result, the genotype yardstick) on the point list at point_width, made once"""
    draft, events, par = T.crafted(name, mode)
    grp = S.strands(events)
    sup = T.oracle_once(("support", name, mode), lambda: S.loop(draft, events, par, None, grp, 2))
    terms = T.oracle_once(("support-terms", name, mode), lambda: S.oracle_terms(draft, events, par, None))
    want = T.oracle_once(("genotype", name, mode, ploidy), lambda: GC.yardstick(terms, len(draft), alt_fractions(ploidy)))
    return draft, events, par, grp, sup, want


def opa(draft, events, par):
    return B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)


def check(got, sup, want, tag):
    """one ScoreMutationGenotypes result against both yardsticks; on the fallback path the float64 loop must match by bytes"""
    scores, rec, scored, lik, nc = got
    print("%s: worst |lik - loopld| / bound = %.4f" % (tag, GC.worst(lik, want)))
    assert S.same((scores, rec), sup) and S.score_bytes(scored) == np.asarray(scores).tobytes()
    assert lik.tobytes() == want[0].tobytes()
    assert GC.same(lik, nc, want)
    assert np.array_equal(nc, rec["cover"].sum(axis=1))


@pytest.mark.parametrize("ploidy", [2, 3])
@pytest.mark.parametrize("name,mode", CASES)
def test_fallback_equals_the_loops(name, mode, ploidy):
    draft, events, par, grp, sup, want = case(name, mode, ploidy)
    assert "ps_score_mutation_genotypes" in B.oracle_api().missing
    pa = opa(draft, events, par)
    got = pa.ScoreMutationGenotypes(alt_frac=alt_fractions(ploidy))
    check(got, sup, want, "%s/%s P=%d" % (name, mode, ploidy))
    assert got[3].shape == (len(sup[0]), ploidy) and got[4].dtype == np.int32
    assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))   # self is not modified
    if ploidy == 2:                                                      # the default is one fraction, 0.5
        assert opa(draft, events, par).ScoreMutationGenotypes()[3].tobytes() == got[3].tobytes()


@pytest.mark.parametrize("resident", [True, False])
def test_region_batch_over_oracle_regions_equals_the_loops(resident):
    made = [case(n, m, p) for (n, m), p in zip(CASES, (2, 3))]
    pas = [opa(d, e, p) for d, e, p, _, _, _ in made]
    with RegionBatch(pas, resident=resident) as rb:
        got = rb.ScoreMutationGenotypes(None, alt_frac=[alt_fractions(2), alt_fractions(3)])
        one = rb.ScoreMutationGenotypes(None, idx=[1], alt_frac=alt_fractions(3))
        for pa, (d, e, _, _, _, _) in zip(pas, made):
            assert pa.sequence == d and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, e))
        if resident:
            rb.drop()       # (closing a resident batch writes the re-aligned events back: not this test's subject)
    for k, (g, (_, _, _, _, sup, want)) in enumerate(zip(got, made)):
        check(g, sup, want, "batch region %d" % k)
    check(one[0], made[1][4], made[1][5], "batch idx=[1]")


def _random(seed, E, M):
    rng = np.random.default_rng(seed)
    d = rng.choice([-1.0, 1.0], size=(E, M)) * 10.0 ** rng.uniform(-6, 3, size=(E, M))
    return d, np.tile([1, M + 5], (E, 1)), np.arange(M)


def _bound(d):
    return 2.0 ** -52 * (16 + d.shape[0]) * (1.0 + np.abs(d)).sum(axis=0)


def test_identities_of_the_definition():
    d, spans, starts = _random(5, 40, 60)
    fr = [1e-6, 0.02, 0.25, 0.5, 0.98]
    lik, nc = genotypes_from_deltas(d, spans, starts, 1000, fr)
    assert lik.shape == (60, 6) and nc.tolist() == [40] * 60
    # L(f; d) - L(1 - f; -d) = sum d: (1 - f) + f e^d = e^d (f + (1 - f) e^-d).  Dyadic fractions, so that 1 - (1 - f) is f again
    # in FP64 and both sides see the same pair (f, g): with f = 1e-6 the mirrored g is off by 1e-10 relative, which is the inputs'
    # error and not the formula's.
    dy = [2.0 ** -19, 0.03125, 0.25, 0.5, 0.96875]
    assert all(1.0 - (1.0 - f) == f for f in dy)
    fore, _ = genotypes_from_deltas(d, spans, starts, 1000, dy)
    back, _ = genotypes_from_deltas(-d, spans, starts, 1000, [1.0 - f for f in dy])
    tot = d.astype(np.longdouble).sum(axis=0)
    gap = np.abs(fore[:, :5].astype(np.longdouble) - back[:, :5] - tot[:, None])
    print("mirror identity: worst / bound = %.4f" % float((gap / _bound(d)[:, None]).max()))
    assert np.all(gap <= _bound(d)[:, None])
    # the hom-alt column is the in-order sum, and the float64 formula sits inside the bound of the long double one
    hom = np.zeros(60)
    for e in range(40):
        hom = hom + d[e]
    assert lik[:, 5].tobytes() == hom.tobytes()
    terms = (starts.tolist(), d.tolist(), [(1, 65)] * 40)
    assert GC.same(lik, nc, GC.yardstick(terms, 1000, fr)) and lik.tobytes() == GC.loop64(terms, 1000, fr)[0].tobytes()
    # K = 0: one column
    l0, n0 = genotypes_from_deltas(d, spans, starts, 1000, [])
    assert l0.shape == (60, 1) and l0[:, 0].tobytes() == hom.tobytes() and np.array_equal(n0, nc)
    # an all-zero column: log(g + f) per read, within n_cover 2^-52 of 0
    z = d.copy()
    z[:, 7] = 0.0
    lz, _ = genotypes_from_deltas(z, spans, starts, 1000, fr)
    assert np.all(np.abs(lz[7]) <= 40 * 2.0 ** -52) and lz[7, 5] == 0.0
    # -inf for one read contributes log(1 - f); +inf gives +inf; NaN propagates — each in its own column only
    w = d.copy()
    w[3, 0], w[3, 1], w[3, 2] = -np.inf, np.inf, np.nan
    lw, nw = genotypes_from_deltas(w, spans, starts, 1000, [0.25])
    rest, _ = genotypes_from_deltas(np.delete(d, 3, axis=0), spans[1:], starts, 1000, [0.25])
    print("-inf term: |got - (rest + log g)| / (2 bound) = %.4f" % (abs(lw[0, 0] - (rest[0, 0] + math.log(0.75))) / (2 * _bound(d)[0])))
    assert abs(lw[0, 0] - (rest[0, 0] + math.log(0.75))) <= 2 * _bound(d)[0] and lw[0, 1] == -np.inf      # (two evaluations: a bound each)
    assert lw[1, 0] == np.inf and lw[1, 1] == np.inf and np.isnan(lw[2]).all()
    assert lw[3:].tobytes() == genotypes_from_deltas(d, spans, starts, 1000, [0.25])[0][3:].tobytes() and nw.tolist() == [40] * 60
    # events outside the span and skipped edits do not enter
    sp = spans.copy()
    sp[0] = (1, 0)
    sp[1] = (1, 10)
    lo, no = genotypes_from_deltas(d, sp, starts, 30, [0.5])
    assert no[:10].tolist() == [39] * 10 and no[10:31].tolist() == [38] * 21 and not no[31:].any() and not lo[31:].any()
    for bad in ([0.0], [1.0], [float("nan")], [0.5] * 9, [1e-7], [-0.5]):
        with pytest.raises(ValueError):
            genotypes_from_deltas(d, spans, starts, 1000, bad)


def test_call_genotypes_on_canned_values():
    assert alt_fractions(1) == [] and alt_fractions(2) == [0.5] and alt_fractions(3) == [1 / 3, 2 / 3] and len(alt_fractions(9)) == 8
    for bad in (0, 10, -1, 2.5):
        with pytest.raises(ValueError):
            alt_fractions(bad)
    ln10 = math.log(10.0)
    lik = np.array([[-3.0, -20.0],                   # hom-ref wins
                    [2.0, -5.0],                     # het
                    [1.0, 30.0],                     # hom-alt
                    [0.0, 0.0],                      # a three-way tie: the first genotype
                    [5.0, 5.0],                      # het ties hom-alt: het comes first
                    [-0.1 * ln10, -5000.0],          # PL 1 and the cap 9999
                    [np.nan, 1.0],                   # NaN: no call
                    [4.0, 8.0],                      # n_cover 0: no call
                    [-2000.0, -np.inf]])
    nc = np.array([5, 5, 5, 5, 5, 5, 5, 0, 5], dtype=np.int32)
    gt, gq, pl = call_genotypes(lik, nc, 2)
    assert gt == ["0/0", "0/1", "1/1", "0/0", "0/1", "0/0", "./.", "./.", "0/0"]
    assert pl[0] == [0, 13, 87] and gq[0] == 13
    assert pl[1] == [9, 0, 30] and gq[1] == 9
    assert pl[2] == [130, 126, 0] and gq[2] == 99                   # GQ capped at 99
    assert pl[3] == [0, 0, 0] and gq[3] == 0
    assert pl[4] == [22, 0, 0] and gq[4] == 0
    assert pl[5] == [0, 1, 9999] and gq[5] == 1                     # PL capped at 9999
    assert pl[6] == [0, 0, 0] and gq[6] == 0 and pl[7] == [0, 0, 0] and gq[7] == 0
    assert pl[8] == [0, 8686, 9999] and gq[8] == 99
    gt1, gq1, pl1 = call_genotypes(np.array([[-4.0], [0.5], [0.0], [np.nan]]), np.array([3, 3, 3, 3]), 1)
    assert gt1 == ["0", "1", "0", "."] and pl1 == [[0, 17], [2, 0], [0, 0], [0, 0]] and gq1 == [17, 2, 0, 0]
    gt3, gq3, pl3 = call_genotypes(np.array([[1.0, 3.0, -2.0], [-1.0, -1.5, -9.0], [0.5, 0.5, 0.5], [1.0, 2.0, 2.0]]), np.array([4, 4, 4, 0]), 3)
    assert gt3 == ["0/1/1", "0/0/0", "0/0/1", "././."]
    assert pl3 == [[13, 9, 0, 22], [0, 4, 7, 39], [2, 0, 0, 0], [0, 0, 0, 0]] and gq3 == [9, 4, 0, 0]
    with pytest.raises(ValueError):
        call_genotypes(lik, nc, 3)                                  # two columns are ploidy 2
    for P in (1, 2, 3):                                             # an empty list: nothing to call, and nothing raised
        assert call_genotypes(np.empty((0, P)), np.empty(0, dtype=np.int32), P) == ([], [], [])
    with pytest.raises(ValueError):
        call_genotypes(np.empty((0, 2)), np.empty(0, dtype=np.int32), 3)


# ---- writers --------------------------------------------------------------------------------------------------------------------
LIK = [[1.25, -3.0], [0.5, 0.75], [-0.5, -2.25], [12.0, 40.0], [0.0, 0.001]]
NCOV = [5, 1, 3, 7, 0]

TSV2 = ("#start\torig\tmut\tscore\tcover_t\tpos_t\tneg_t\tsum_t\tcover_c\tpos_c\tneg_c\tsum_c\tn_cover\tgt\tgq\tgl_0\tgl_1\tgl_2\n"
        "1003\tT\tG\t2.5\t3\t2\t1\t1.5\t2\t1\t0\t1.0\t5\t0/1\t5\t0.0\t1.25\t-3.0\n"
        "1005\t.\tCC\t0.75\t1\t1\t0\t0.5\t0\t0\t0\t0.25\t1\t1/1\t1\t0.0\t0.5\t0.75\n"
        "1006\tCA\t.\t-1.25\t2\t0\t2\t-1.0\t1\t0\t1\t-0.25\t3\t0/0\t2\t0.0\t-0.5\t-2.25\n"
        "1000\tAC\t.\t40.0\t4\t4\t0\t30.0\t3\t3\t0\t10.0\t7\t1/1\t99\t0.0\t12.0\t40.0\n"
        "1002\tGTT\tCA\t0.001\t1\t0\t0\t0.0\t1\t1\t0\t0.001\t0\t./.\t0\t0.0\t0.0\t0.001\n")
VCF2 = (VCF_HEAD.replace('#CHROM', '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype: the alt-copy count with the largest likelihood over the spanning reads (uncalibrated)">\n'
                                   '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the second smallest PL, at most 99 (uncalibrated)">\n'
                                   '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods over the spanning reads, 0 .. ploidy alt copies (uncalibrated)">\n'
                                   '#CHROM').replace('\tINFO\n', '\tINFO\tFORMAT\tNA12878\n') +
        "chr7\t1004\t.\tT\tG\t11\t.\tLLR=2.5;DP=5;GDP=3,2;GSUP=2,1;GOPP=1,0;GLLR=1.5,1.0\tGT:GQ:PL\t0/1:5:5,0,18\n"
        "chr7\t1005\t.\tT\tTCC\t3\t.\tLLR=0.75;DP=1;GDP=1,0;GSUP=1,0;GOPP=0,0;GLLR=0.5,0.25\tGT:GQ:PL\t1/1:1:3,1,0\n"
        "chr7\t1001\t.\tACG\tG\t174\t.\tLLR=40.0;DP=7;GDP=4,3;GSUP=4,3;GOPP=0,0;GLLR=30.0,10.0\tGT:GQ:PL\t1/1:99:174,122,0\n"
        "chr7\t1002\t.\tCGTT\tCCA\t0\t.\tLLR=0.001;DP=2;GDP=1,1;GSUP=0,1;GOPP=0,0;GLLR=0.0,0.001\tGT:GQ:PL\t./.:0:0,0,0\n")


def _canned(monkeypatch):
    seen = {"support": 0, "genotypes": 0}

    def base():
        scored = []
        for (st, o, m, sc) in EDITS:
            ms = MutationScore()
            ms.start, ms.orig, ms.mut, ms.score = st, o, m, sc
            scored.append(ms)
        return np.array([e[3] for e in EDITS]), np.array(RECS, dtype=_capi.EDIT_SUPPORT), scored

    def fake_support(self, muts_per_region, idx=None, groups=None, n_groups=None):
        seen["support"] += 1
        return [base()]

    def fake_genotypes(self, muts_per_region, idx=None, alt_frac=(0.5,), groups=None, n_groups=None):
        seen["genotypes"] += 1
        seen["starts"], seen["n_groups"], seen["alt_frac"] = [[m.start for m in ml] for ml in muts_per_region], n_groups, list(alt_frac)
        return [base() + (np.array(LIK), np.array(NCOV, dtype=np.int32))]

    monkeypatch.setattr(batch.RegionBatch, "ScoreMutationSupport", fake_support)
    monkeypatch.setattr(batch.RegionBatch, "ScoreMutationGenotypes", fake_genotypes)
    return seen


@pytest.mark.parametrize("fmt,ploidy,want", [("tsv", 2, TSV2), ("vcf", 2, VCF2), ("tsv", None, TSV), ("vcf", None, VCF)])
def test_writer_goldens(monkeypatch, fmt, ploidy, want):
    seen = _canned(monkeypatch)
    muts = [S.edit(1000 + st, o, m) for st, o, m, _ in EDITS]
    out = io.StringIO()
    res = variant_support([opa(SEQ, [], T.P0)], [muts], region_starts=[1000], out=out, fmt=fmt, chrom="chr7", ploidy=ploidy, sample="NA12878")
    assert out.getvalue() == want
    assert [m.start for m in muts] == [1003, 1005, 1006, 1000, 1002]                # the caller's list is not changed
    assert [s.start for s in res[0][2]] == [1003, 1005, 1006, 1000, 1002]           # absolute outside
    if ploidy is None:
        assert (seen["support"], seen["genotypes"]) == (1, 0) and len(res[0]) == 3  # today's path, today's bytes
    else:
        assert (seen["support"], seen["genotypes"]) == (0, 1) and len(res[0]) == 5  # ONE genotype call, (lik, n_cover) on top
        assert seen["starts"] == [[3, 5, 6, 0, 2]] and seen["n_groups"] == 2 and seen["alt_frac"] == [0.5]
        assert res[0][3].tolist() == LIK and res[0][4].tolist() == NCOV
    with pytest.raises(ValueError):
        variant_support([opa(SEQ, [], T.P0)], [muts], ploidy=10)


@pytest.mark.parametrize("fmt", ["tsv", "vcf"])
def test_a_region_without_edits_writes_no_lines(fmt):
    """one region without candidate edits among others is the normal input of `variant -m`: with a ploidy as without"""
    draft, events, par, _, _, _ = case("gap", "zeroed", 2)
    muts = lambda: [[], [S.edit(5000 + m.start, m.orig, m.mut) for m in T.edits(draft, events, 5)[:12]], []]
    pas = [opa(draft, events, par) for _ in range(3)]
    plain, out = io.StringIO(), io.StringIO()
    variant_support(pas, muts(), region_starts=[100, 5000, 9000], out=plain, fmt=fmt, min_score=-1e9)
    res = variant_support(pas, muts(), region_starts=[100, 5000, 9000], out=out, fmt=fmt, min_score=-1e9, ploidy=2)
    body = lambda text: [l for l in text.getvalue().splitlines() if not l.startswith("#")]
    assert len(body(out)) == 12 and ["\t".join(l.split("\t")[:len(p.split("\t"))]) for l, p in zip(body(out), body(plain))] == body(plain)
    for k in (0, 2):
        assert res[k][3].shape == (0, 2) and res[k][4].shape == (0,) and len(res[k][0]) == 0 and res[k][2] == []
    assert res[1][3].shape == (12, 2) and res[1][4].max() > 0
    alone = variant_support(opa(draft, events, par), [], out=io.StringIO(), fmt=fmt, ploidy=3)          # and a single empty region
    assert alone[3].shape == (0, 3) and alone[4].shape == (0,)


def test_crafted_case_still_exercises_the_definition():
    """preconditions on "gap": without them a sum over all events, a dropped branch or a missing genotype would go unnoticed"""
    draft, events, par, grp, sup, want = case("gap", "zeroed", 2)
    starts, delta, spans = T.oracle_once(("support-terms", "gap", "zeroed"), lambda: S.oracle_terms(draft, events, par, None))
    E, M, L = len(events), len(starts), len(draft)
    d = np.array(delta)
    assert np.isfinite(d).all()
    cov = np.array([[S.covers(spans, starts, L, e, m) for m in range(M)] for e in range(E)])
    assert np.count_nonzero((d > 0) & cov) > 0 and np.count_nonzero((d < 0) & cov) > 0      # both branches of x
    assert np.count_nonzero((d != 0) & ~cov) > 0                                            # summing over all events would be caught
    assert np.any(want[0][:, -1] != sup[1]["sum"].sum(axis=1))                              # hom-alt is not the score's sum
    gts = set(call_genotypes(want[0], want[1], 2)[0])
    print("genotypes on the point list:", sorted(gts))
    assert {"0/0", "0/1", "1/1"} <= gts


def test_new_symbols_are_declared_optional_and_exported_by_the_product():
    hdr = open(os.path.join(B.ROOT, "include", "poreseq_hip.h")).read()
    declared = set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _capi.SYMBOLS and name in _capi.OPTIONAL
    api = B.oracle_api()                             # the checker lacks them and still loads
    assert set(NEW) <= api.missing and api.missing <= _capi.OPTIONAL
    lib = ctypes.CDLL(_capi.HIP_LIB)                 # the product exports them
    for name in NEW:
        assert hasattr(lib, name), name
    assert _capi.load_hip().missing == set()
