"""Per-edit read support by event group on the CPU checkers: the path of a library without ps_score_mutation_support
(PSAlign.ScoreMutationSupport / RegionBatch.ScoreMutationSupport over util.support_from_deltas) against the definition's plain loops
(support_cases.loop), the preconditions that keep the crafted cases from going stale, and the TSV / VCF writers of
consensus.variant_support."""
import copy
import io

import numpy as np
import pytest

import backends as B
import support_cases as S
import tiled_cases as T
from poreseq_amd import _capi, batch, consensus
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import variant_region, variant_support, vcf_fields, vcf_qual
from poreseq_amd.util import MutationScore

CASES = [("gap", "zeroed"), ("single", "loader")]


def case(name, mode):
    """(draft, events, params, groups, the loop's result on the point list at point_width), made once"""
    draft, events, par = T.crafted(name, mode)
    grp = S.strands(events)
    want = T.oracle_once(("support", name, mode), lambda: S.loop(draft, events, par, None, grp, 2))
    return draft, events, par, grp, want


def opa(draft, events, par):
    return B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)


@pytest.mark.parametrize("name,mode", CASES)
def test_fallback_equals_the_loop_and_scores_are_scorepoints(name, mode):
    draft, events, par, grp, want = case(name, mode)
    assert "ps_score_mutation_support" in B.oracle_api().missing
    pa = opa(draft, events, par)
    got = pa.ScoreMutationSupport()
    assert S.same(got, want)
    assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))   # self is not modified
    points = opa(draft, events, par).ScorePoints()
    assert S.score_bytes(points) == got[0].tobytes() == S.score_bytes(got[2])
    assert [(s.start, s.orig, s.mut) for s in got[2]] == [(s.start, s.orig, s.mut) for s in points]
    # the strand default is what explicit groups give; one group holds every event
    assert S.same(opa(draft, events, par).ScoreMutationSupport(groups=grp, n_groups=2), want)
    one = opa(draft, events, par).ScoreMutationSupport(groups=[0] * len(events))
    assert one[1].shape == (len(want[0]), 1) and np.array_equal(one[1]["cover"][:, 0], want[1]["cover"].sum(axis=1))


@pytest.mark.parametrize("resident", [True, False])
def test_region_batch_over_oracle_regions_equals_the_loop(resident):
    made = [case(*c) for c in CASES]
    pas = [opa(d, e, p) for d, e, p, _, _ in made]
    with RegionBatch(pas, resident=resident) as rb:
        got = rb.ScoreMutationSupport(None)
        lists = [S.point_list(d)[:40] for d, _, _, _, _ in made]
        sub = rb.ScoreMutationSupport(lists, groups=[g for _, _, _, g, _ in made], n_groups=2)
        scored = rb.ScoreMutations(lists)
        for pa, (d, e, _, _, _) in zip(pas, made):
            assert pa.sequence == d and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, e))
        if resident:
            rb.drop()       # (closing a resident batch writes the re-aligned events back: not this test's subject)
    assert all(S.same(g, w) for g, (_, _, _, _, w) in zip(got, made))
    for (d, e, p, g, _), ml, s, sc in zip(made, lists, sub, scored):
        assert S.same(s, S.loop(d, e, p, ml, g, 2))                      # (a given list is scored at scoring_width)
        assert S.score_bytes(sc) == s[0].tobytes() == S.score_bytes(opa(d, e, p).ScoreMutations(ml))


def test_crafted_cases_still_exercise_the_definition():
    """preconditions: without them `cover` could be replaced by `delta != 0` (or by all events) and the tests above would not notice"""
    for (name, mode), levels in zip(CASES, ((0, 1, 2, 3), (0, 1, 2, 3, 4))):
        draft, events, par, grp, want = case(name, mode)
        starts, delta, spans = T.oracle_once(("support-terms", name, mode), lambda: S.oracle_terms(draft, events, par, None))
        E, M, L = len(events), len(starts), len(draft)
        if name == "gap":
            assert (L, E, M) == (399, 6, 3160)
        per_edit = want[1]["cover"].sum(axis=1)
        assert set(np.unique(per_edit).tolist()) == set(levels)
        cov = np.array([[S.covers(spans, starts, L, e, m) for m in range(M)] for e in range(E)])
        d = np.array(delta)
        assert np.count_nonzero((d != 0) & ~cov) > 0 and np.count_nonzero((d == 0) & cov) > 0
        assert np.count_nonzero(d > 0) > 0 and np.count_nonzero(d < 0) > 0
        assert want[1]["pos"].sum() > 0 and want[1]["neg"].sum() > 0 and set(grp) == {0, 1}


# ---- writers --------------------------------------------------------------------------------------------------------------------
SEQ = "ACGTTGCAAC"
EDITS = [(3, "T", "G", 2.5), (5, "", "CC", 0.75), (6, "CA", "", -1.25), (0, "AC", "", 40.0), (2, "GTT", "CA", 1e-3)]
RECS = [[(1.5, 3, 2, 1, 0), (1.0, 2, 1, 0, 0)], [(0.5, 1, 1, 0, 0), (0.25, 0, 0, 0, 0)], [(-1.0, 2, 0, 2, 0), (-0.25, 1, 0, 1, 0)],
        [(30.0, 4, 4, 0, 0), (10.0, 3, 3, 0, 0)], [(0.0, 1, 0, 0, 0), (1e-3, 1, 1, 0, 0)]]

TSV = ("#start\torig\tmut\tscore\tcover_t\tpos_t\tneg_t\tsum_t\tcover_c\tpos_c\tneg_c\tsum_c\n"
       "1003\tT\tG\t2.5\t3\t2\t1\t1.5\t2\t1\t0\t1.0\n"
       "1005\t.\tCC\t0.75\t1\t1\t0\t0.5\t0\t0\t0\t0.25\n"
       "1006\tCA\t.\t-1.25\t2\t0\t2\t-1.0\t1\t0\t1\t-0.25\n"
       "1000\tAC\t.\t40.0\t4\t4\t0\t30.0\t3\t3\t0\t10.0\n"
       "1002\tGTT\tCA\t0.001\t1\t0\t0\t0.0\t1\t1\t0\t0.001\n")
VCF_HEAD = ('##fileformat=VCFv4.2\n##source=poreseq_amd.variant_support\n'
            '##INFO=<ID=LLR,Number=1,Type=Float,Description="Log-likelihood change of the edit summed over all reads (natural log)">\n'
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads whose re-aligned span holds the edit (a span test, not a likelihood test)">\n'
            '##INFO=<ID=GDP,Number=.,Type=Integer,Description="Spanning reads per group (groups: t,c)">\n'
            '##INFO=<ID=GSUP,Number=.,Type=Integer,Description="Spanning reads per group that favour the edit (term > 0) (groups: t,c)">\n'
            '##INFO=<ID=GOPP,Number=.,Type=Integer,Description="Spanning reads per group that oppose the edit (term < 0) (groups: t,c)">\n'
            '##INFO=<ID=GLLR,Number=.,Type=Float,Description="Log-likelihood change per group, over all reads of the group (groups: t,c)">\n'
            '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')
VCF = (VCF_HEAD +
       "chr7\t1004\t.\tT\tG\t11\t.\tLLR=2.5;DP=5;GDP=3,2;GSUP=2,1;GOPP=1,0;GLLR=1.5,1.0\n"           # substitution: POS = start + 1
       "chr7\t1005\t.\tT\tTCC\t3\t.\tLLR=0.75;DP=1;GDP=1,0;GSUP=1,0;GOPP=0,0;GLLR=0.5,0.25\n"        # insertion behind base 4 (T)
       "chr7\t1001\t.\tACG\tG\t174\t.\tLLR=40.0;DP=7;GDP=4,3;GSUP=4,3;GOPP=0,0;GLLR=30.0,10.0\n"     # deletion at start 0: the base after it
       "chr7\t1002\t.\tCGTT\tCCA\t0\t.\tLLR=0.001;DP=2;GDP=1,1;GSUP=0,1;GOPP=0,0;GLLR=0.0,0.001\n")  # GTT -> CA, anchored on base 1 (C)


def _canned(monkeypatch):
    seen = {}

    def fake(self, muts_per_region, idx=None, groups=None, n_groups=None):
        seen["starts"], seen["n_groups"] = [[m.start for m in ml] for ml in muts_per_region], n_groups
        scored = []
        for (st, o, m, sc) in EDITS:
            ms = MutationScore()
            ms.start, ms.orig, ms.mut, ms.score = st, o, m, sc
            scored.append(ms)
        return [(np.array([e[3] for e in EDITS]), np.array(RECS, dtype=_capi.EDIT_SUPPORT), scored)]

    monkeypatch.setattr(batch.RegionBatch, "ScoreMutationSupport", fake)
    return seen


@pytest.mark.parametrize("fmt,want", [("tsv", TSV), ("vcf", VCF)])
def test_writer_goldens(monkeypatch, fmt, want):
    seen = _canned(monkeypatch)
    muts = [S.edit(1000 + st, o, m) for st, o, m, _ in EDITS]
    out = io.StringIO()
    res = variant_support([opa(SEQ, [], T.P0)], [muts], region_starts=[1000], out=out, fmt=fmt, chrom="chr7")
    assert out.getvalue() == want
    assert seen["starts"] == [[3, 5, 6, 0, 2]] and seen["n_groups"] == 2            # region-relative inside the call
    assert [m.start for m in muts] == [1003, 1005, 1006, 1000, 1002]                # the caller's list is not changed
    assert [s.start for s in res[0][2]] == [1003, 1005, 1006, 1000, 1002]           # absolute outside


def test_vcf_fields_and_qual():
    assert vcf_fields(SEQ, 3, "T", "G") == (4, "T", "G")
    assert vcf_fields(SEQ, 5, "", "CC") == (5, "T", "TCC")
    assert vcf_fields(SEQ, 6, "CA", "") == (6, "GCA", "G")
    assert vcf_fields(SEQ, 0, "AC", "") == (1, "ACG", "G")
    assert vcf_fields(SEQ, 0, "", "T") == (1, "A", "TA")
    assert vcf_fields(SEQ, 2, "GTT", "CA", 100) == (102, "CGTT", "CCA")
    assert vcf_fields(SEQ, 2, "GT", "CA") == (3, "GT", "CA")
    assert [vcf_qual(s) for s in (-3.0, 0.0, 0.1, 1.0, 2.5, 1e9, float("nan"))] == [0, 0, 0, 4, 11, 9999, 0]
    with pytest.raises(ValueError):
        variant_support([], [], fmt="bcf")


def test_tsv_columns_are_variant_regions_lines():
    draft, events, par, grp, want = case("gap", "zeroed")
    muts = lambda: [S.edit(5000 + m.start, m.orig, m.mut) for m in T.edits(draft, events, 5)]
    ref = io.StringIO()
    variant_region(opa(draft, events, par), muts(), region_start=5000, out=ref)
    out = io.StringIO()
    res = variant_support(opa(draft, events, par), muts(), region_starts=5000, out=out)
    lines, ref_lines = out.getvalue().splitlines(), ref.getvalue().splitlines()
    assert lines[0].startswith("#") and len(lines) == len(ref_lines) + 1
    assert ["\t".join(l.split("\t")[:4]) for l in lines[1:]] == ref_lines
    rel = T.edits(draft, events, 5)
    sc, sup = S.loop(draft, events, par, rel, grp, 2)
    assert S.same(res, (sc, sup))
    for l, rec in zip(lines[1:], sup.tolist()):
        assert l.split("\t")[4:] == [str(v) for r in rec for v in (r[1], r[2], r[3], r[0])]


def test_groups_that_do_not_fit_are_value_errors():
    draft, events, par, grp, _ = case("gap", "zeroed")
    pa = opa(draft, events, par)
    E = len(events)
    for kw in (dict(groups=[0] * E, n_groups=0), dict(groups=[0] * E, n_groups=9), dict(groups=[0] * (E - 1) + [2], n_groups=2),
               dict(groups=[0] * (E - 1)), dict(groups=[0] * (E + 1), n_groups=2), dict(groups=[-1] + [0] * (E - 1), n_groups=2)):
        with pytest.raises(ValueError):
            pa.ScoreMutationSupport([S.edit(10, "A", "C")], **kw)
    with RegionBatch([pa], resident=False) as rb:
        with pytest.raises(ValueError):
            rb.ScoreMutationSupport([[S.edit(10, "A", "C")]], groups=[[0] * E], n_groups=9)
        with pytest.raises(ValueError):
            rb.ScoreMutationSupport([[S.edit(10, "A", "C")], []])
